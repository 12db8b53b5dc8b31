// bsm_internal.hpp -- shared internals of libbsm_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bsm.h"

namespace bsm {

// ---------------------------------------------------------------------------
// errors: thread-local message + status codes
// ---------------------------------------------------------------------------
void set_error(const char* fmt, ...);
const char* last_error();
// stage timer of the solver (bsm_stage_times): reset, then mark the end of each stage
void stage_reset(hipStream_t s);
void stage_mark(const char* name, hipStream_t s);

#define BSM_HIP_TRY(expr)                                                                   \
    do {                                                                                    \
        hipError_t bsm_e_ = (expr);                                                         \
        if (bsm_e_ != hipSuccess) {                                                         \
            ::bsm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(bsm_e_),     \
                             __FILE__, __LINE__);                                           \
            return bsm_e_ == hipErrorOutOfMemory ? BSM_ERR_OOM : BSM_ERR_HIP;               \
        }                                                                                   \
    } while (0)

#define BSM_TRY(expr)                 \
    do {                              \
        int bsm_rc_ = (expr);         \
        if (bsm_rc_ != BSM_OK) return bsm_rc_; \
    } while (0)

#define BSM_REQUIRE(cond, code, ...)           \
    do {                                       \
        if (!(cond)) {                         \
            ::bsm::set_error(__VA_ARGS__);     \
            return (code);                     \
        }                                      \
    } while (0)

// ---------------------------------------------------------------------------
// arithmetic with the reference's semantics: IEEE, no contraction, integers
// wrap (Cargo.toml:18). Signed integers are computed in the same-width
// unsigned type so device code never hits C++ signed-overflow UB.
// ---------------------------------------------------------------------------
template <typename T> struct Arith;
template <> struct Arith<double> {
    __device__ __forceinline__ static double add(double a, double b) { return __dadd_rn(a, b); }
    __device__ __forceinline__ static double sub(double a, double b) { return __dsub_rn(a, b); }
    __device__ __forceinline__ static double mul(double a, double b) { return __dmul_rn(a, b); }
    __device__ __forceinline__ static bool nz(double v) { return !(v == 0.0); }
    __device__ __forceinline__ static double zero() { return 0.0; }
    __device__ __forceinline__ static double neg_zero() { return -0.0; }
};
template <> struct Arith<float> {
    __device__ __forceinline__ static float add(float a, float b) { return __fadd_rn(a, b); }
    __device__ __forceinline__ static float sub(float a, float b) { return __fsub_rn(a, b); }
    __device__ __forceinline__ static float mul(float a, float b) { return __fmul_rn(a, b); }
    __device__ __forceinline__ static bool nz(float v) { return !(v == 0.0f); }
    __device__ __forceinline__ static float zero() { return 0.0f; }
    __device__ __forceinline__ static float neg_zero() { return -0.0f; }
};
template <typename T, typename U> struct ArithInt {
    __device__ __forceinline__ static T add(T a, T b) { return (T)((U)a + (U)b); }
    __device__ __forceinline__ static T sub(T a, T b) { return (T)((U)a - (U)b); }
    __device__ __forceinline__ static T mul(T a, T b) { return (T)((U)a * (U)b); }
    __device__ __forceinline__ static bool nz(T v) { return v != 0; }
    __device__ __forceinline__ static T zero() { return 0; }
    __device__ __forceinline__ static T neg_zero() { return 0; }
};
template <> struct Arith<int32_t> : ArithInt<int32_t, uint32_t> {};
template <> struct Arith<uint32_t> : ArithInt<uint32_t, uint32_t> {};
template <> struct Arith<int64_t> : ArithInt<int64_t, uint64_t> {};
template <> struct Arith<uint64_t> : ArithInt<uint64_t, uint64_t> {};

template <typename T> struct IsFloat { static constexpr bool value = false; };
template <> struct IsFloat<double> { static constexpr bool value = true; };
template <> struct IsFloat<float> { static constexpr bool value = true; };

inline size_t dtype_size(int dt) {
    switch (dt) {
        case BSM_F64: case BSM_I64: case BSM_U64: return 8;
        case BSM_F32: case BSM_I32: case BSM_U32: return 4;
        default: return 0;
    }
}

// Invoke F.template operator()<T>() for the runtime dtype.
template <typename F> int dispatch_dtype(int dt, F&& f) {
    switch (dt) {
        case BSM_F64: return f.template operator()<double>();
        case BSM_F32: return f.template operator()<float>();
        case BSM_I32: return f.template operator()<int32_t>();
        case BSM_U32: return f.template operator()<uint32_t>();
        case BSM_I64: return f.template operator()<int64_t>();
        case BSM_U64: return f.template operator()<uint64_t>();
        default: set_error("unknown dtype %d", dt); return BSM_ERR_INVALID;
    }
}

// ---------------------------------------------------------------------------
// device context: one non-blocking stream per device, created lazily.
// ---------------------------------------------------------------------------
int current_device(int* dev);
int ctx_stream(hipStream_t* s);  // stream of the calling thread's device
// Small device -> host read through a pinned bounce buffer, synchronous on s
// (a pageable hipMemcpyAsync costs ~19 us; this is a few).
hipError_t read_dev(void* host, const void* dev, size_t bytes, hipStream_t s);

// Per-thread cache of device temporaries (tmp_get / tmp_put): a hipFree
// waits for the whole device, and a call such as add_sparse makes ~25 of
// them (1.3-2 ms per call at the reference bench's e = 300k,
// profiles/r03_u_*). A cached block is only handed out again to the same
// thread for the same device and stream, so stream order separates its uses
// (the device is part of the key: the null stream names a different queue on
// every device). Every block is a plain hipMalloc allocation.
void* tmp_get(size_t n, int device, hipStream_t s, size_t* cap);
void tmp_put(void* p, size_t cap, int device, hipStream_t s);

// RAII device buffer for host-path temporaries. alloc(n) is hipMalloc /
// hipFree; alloc(n, s) takes the block from the calling thread's cache for
// stream s and gives it back there, for the many small temporaries of a call.
struct DBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipStream_t st = nullptr;
    int dev = -1;
    size_t cap = 0;  // > 0: a cached temporary of this capacity
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { reset(); }
    void reset() {
        if (p) {
            if (cap) tmp_put(p, cap, dev, st);
            else (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
        cap = 0;
    }
    int alloc(size_t n, hipStream_t s) {
        reset();
        if (n == 0) n = 16;
        if (hipGetDevice(&dev) != hipSuccess) {
            set_error("device temporary: no current device");
            return BSM_ERR_HIP;
        }
        p = tmp_get(n, dev, s, &cap);
        if (!p) {
            cap = 0;
            set_error("device temporary of %zu bytes: out of memory", n);
            return BSM_ERR_OOM;
        }
        bytes = n;
        st = s;
        return BSM_OK;
    }
    int alloc(size_t n) {
        reset();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            set_error("hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? BSM_ERR_OOM : BSM_ERR_HIP;
        }
        bytes = n;
        return BSM_OK;
    }
    // The caller takes the block and frees it with hipFree. A cached
    // temporary is a hipMalloc block too: it simply leaves the cache's care.
    void* release() {
        void* q = p;
        p = nullptr;
        bytes = 0;
        cap = 0;
        return q;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace bsm

// Row-block x column-panel copy of a matrix (kernels_tiled.hip).
struct bsm_tiled {
    int device = 0;
    int dtype = BSM_F64;         // BSM_F64 or BSM_F32 (the value stream's type)
    uint64_t k = 32;             // right-hand columns the copy serves (32 or 1)
    uint32_t overread = 4;       // chunks of dummy padding past the last task
    uint32_t stage = 4;          // k = 1: chunks per pipeline stage
    uint32_t passes = 1;         // 2: half-width rows, two sweeps per batch (meta = col << 8 | row >> 1)
    uint64_t rows = 0, n_cols = 0, nnz = 0;
    uint32_t nw = 0, rpw = 0, nb = 0, rw = 0, pshift = 0;
    uint64_t chunks = 0;         // total, without the over-read padding
    int64_t* offs = nullptr;     // nw*nb + 1 chunk offsets
    void* meta = nullptr;        // (chunks + overread) * 64 meta words (col << 8 | row, or col << 11 | row at k = 1)
    uint32_t meta_bytes = 4;     // 8: k = 32 on 2^24 columns or more
    void* val = nullptr;         // (chunks + overread) * 64 values of dtype
    unsigned* bar = nullptr;     // batch arrival counters of the SpMM (one launch at a time per copy)
};

// The symmetric copy of a handle (bsm_csr::sym), which the refined and the
// pcg solves read (kernels_refine.hip builds it).
struct bsm_sym {
    int64_t* rp = nullptr;   // n + 1
    int32_t* col = nullptr;  // nnz, ascending inside a row whenever a's rows are
    void* vals = nullptr;    // nnz values of a's dtype
    uint64_t nnz = 0;
    double norm_inf = 0.0;  // ||S||inf: the largest row sum of |values|
    uint64_t max_len = 0;   // m: the longest row
};

// Device-resident finalised Csr<T>.
struct bsm_csr {
    int dtype = BSM_F64;
    int device = 0;
    uint64_t rows = 0, cols = 0, nnz = 0;
    int64_t* row_ptr = nullptr;  // rows+1
    int32_t* col = nullptr;      // nnz
    void* vals = nullptr;        // nnz * sizeof(T)
    // lazily computed analysis (see bsm_analyse)
    // analysis (csr_analyse) is cached on the handle: computed when the handle
    // is made from host data, lazily for device-built results (add / sub /
    // mul_sparse) the first time a kernel choice needs it
    mutable bool analysed = false;
    mutable bool rows_sorted = true;  // col non-decreasing inside every row
    mutable uint64_t max_row_len = 0;
    // cached column-panel plan of mul_dense (spmm_plan), keyed by panel width;
    // plan_mu serialises its (re)build and use across threads sharing the handle
    mutable std::mutex plan_mu;
    mutable int32_t* plan_seg = nullptr;
    mutable uint64_t plan_cols = 0;
    mutable bool plan_usable = false;
    // cached row-block x column-panel copy (kernels_tiled.hip), same mutex
    mutable bsm_tiled* tiled = nullptr;
    mutable bool tiled_tried = false;
    // solve(order="nd")'s plan (kernels_nd_plan.hip): the pattern's ordering, tree
    // and device index arrays, built on first use (the pattern is immutable),
    // same mutex; released with the handle
    mutable std::shared_ptr<void> nd_plan;
    // the refined solve's matrix (kernels_refine.hip): the stored entries with
    // column <= row, mirrored; built on first use, same mutex; released with
    // the handle
    mutable bsm_sym* sym = nullptr;
    // row_ptr / col / vals from the result cache (csr_alloc): their block
    // capacities, 0 = plain hipMalloc (bsm_csr_free hipFrees those)
    size_t cache_cap[3] = {0, 0, 0};
    // small mul_dense results: a host copy written by the same kernel as the
    // device arrays (row_ptr int64 [rows + 1], cols int32 [nnz], values
    // [nnz]); bsm_csr_download serves it without touching the device. The
    // device arrays never change after creation, so it cannot go stale.
    std::unique_ptr<char[]> host_copy;
};


// A kept nested-dissection Cholesky factor of P A P^T (kernels_nd.hip). The
// plan (ordering, tree, device index arrays) is shared with the handles and
// the cache that hold it; the numeric storage is the factor's own.
struct bsm_nd_factor {
    int dtype = BSM_F64;      // the factor's own
    int src_dtype = BSM_F64;  // the factored matrix's (bsm_nd_factor_create_as: it may differ); a refactorisation's must equal it
    int device = 0;
    uint64_t n = 0;
    std::shared_ptr<void> plan;  // NdCached; null for n == 0
    bsm::DBuf fr, dv;            // the fronts (L in their pivot panels) and the inverse diagonal tiles
    mutable std::mutex mu;       // one solve, export, logdet or refactorisation at a time
    mutable uint64_t nnz_l = 0;  // L's stored entries, once an export has counted them (under mu)
    // The pattern the factor was made from, which a refactorisation's matrix
    // is compared against: row_ptr (n + 1 int64, padded to 256 bytes), then
    // col (nnz int32), on the device. Shared with the plan cache's entry and
    // with the other factors of the same plan while any of them lives.
    std::shared_ptr<bsm::DBuf> pattern;
    uint64_t nnz = 0;   // that pattern's entries
    bool valid = true;  // false after a refactorisation that failed past its checks: fr / dv hold no factor (under mu)
    // an update / downdate has rewritten pivot panels since the last numeric factorisation: the children's update
    // blocks left in the trailing tiles no longer belong to them, so a partial refactor must not pull them (under mu)
    bool stale_blocks = false;
    // The Schur set (bsm_nd_factor_create_schur): the vertices the plan's root owns, in the
    // caller's order (empty: none; fixed for the handle's life), and on the device, as int32, each one's place among
    // the root's columns followed by the inverse map (the caller's index of each root column)
    std::vector<uint64_t> schur_idx;
    bsm::DBuf schur_map;
};

namespace bsm {
// Host-side phase times of a schedule build (bsm_mcsr_prepare's plan_ms).
struct PlanTimes {
    double total_ms = 0, count_ms = 0, scan_ms = 0, alloc_ms = 0, write_ms = 0, panel_ms = 0, buffers_ms = 0;
};
inline std::chrono::steady_clock::time_point host_now() { return std::chrono::steady_clock::now(); }
inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int csr_alloc(bsm_csr** out, int dtype, uint64_t rows, uint64_t cols, uint64_t nnz);
int csr_analyse(const bsm_csr* m, hipStream_t s);
// mul_dense's schedule (capi.hip): build once per handle and k (synchronous;
// schedule 0 auto, 1 the tiled copy whenever possible, 2 never), then launch.
// The caller holds a->plan_mu for both.
int spmm_prepare_locked(const bsm_csr* a, uint64_t k, int schedule, uint64_t reserve, hipStream_t s,
                        PlanTimes* pt);
int spmm_launch_locked(const bsm_csr* a, uint64_t k, bool allow_tiled, const void* x, void* y, int32_t* nz,
                       hipStream_t s);
// pinned host staging / per-thread device arena (capi.hip)
void* pinned(size_t bytes);
// host columns (Dense::get_col) -> a device ROW-major n x k array in `out`
// (synchronous) (capi.hip)
int upload_dense_cols(int dtype, uint64_t n, uint64_t k, const void* const* cols, DBuf& out, hipStream_t s);
// staged pinned pipelines (transfer.hip); all synchronous
int h2d_staged(void* dst, const void* src, size_t bytes, hipStream_t s);
int d2h_staged(void* dst, const void* src, size_t bytes, hipStream_t s);
int h2d_cols_narrow(int32_t* dst, const uint64_t* src, uint64_t n, uint64_t cols, uint64_t* bad, hipStream_t s);
int h2d_row_ptr(int64_t* dst, const uint64_t* src, uint64_t n, uint64_t base, hipStream_t s);
bool host_registered(const void* p);
int d2h_csr_direct(const int64_t* rp, const int32_t* col, const void* vals, uint64_t rows, uint64_t nnz, size_t es,
                   uint64_t* row_ptr, uint64_t* col_idx, void* vals_out, hipStream_t s);
int d2h_cols_widen(uint64_t* dst, const int32_t* src, uint64_t n, hipStream_t s);
void xfer_count_small_pinned();  // bsm_xfer_counters: a download through the one pinned buffer

// kernels (kernels_*.hip), all async on stream s
uint64_t scan_workspace_bytes(uint64_t n);
int exclusive_scan_i32_to_i64(const int32_t* in, int64_t* out, uint64_t n, void* ws,
                              uint64_t ws_bytes, hipStream_t s);  // out has n+1 entries
int spmm_dispatch(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, const int64_t* rp,
                  const int32_t* col, const void* vals, uint64_t k, const void* x, void* y,
                  int32_t* row_nnz, bool neg_zero_init, hipStream_t s,
                  uint64_t max_row_len = UINT64_MAX);  // the longest row, when known (kernel choice)
// the kernel spmm_dispatch launches for these arguments under the environment
// as it is now (spmm_rule.hpp; launch_spmm switches on this very call)
enum class SpmmKernel : int;
SpmmKernel spmm_kernel_choice(int dtype, uint64_t rows, uint64_t nnz, uint64_t k, uint64_t max_row_len,
                              const void* x, const void* y);
// nnz-balanced integer SpMM for skewed rows (zeroes y; row_nnz may be null)
bool spmm_wants_split(int dtype, uint64_t k, uint64_t max_row_len);
int spmm_split_dispatch(int dtype, uint64_t rows, uint64_t nnz, const int64_t* rp, const int32_t* col,
                        const void* vals, uint64_t k, const void* x, void* y, int32_t* row_nnz, hipStream_t s);
// device construction from an insert sequence (kernels_build.hip)
int csr_from_inserts_device(int dtype, uint64_t rows, uint64_t cols, uint64_t n, const uint64_t* row,
                            const uint64_t* col, const void* vals, bsm_csr** out, hipStream_t s);
// sparse x sparse (kernels_sparse.hip); synchronous
int sparse_addsub_dispatch(const bsm_csr* a, const bsm_csr* b, bool sub, bsm_csr** out, hipStream_t s);
int sparse_mul_dispatch(const bsm_csr* a, const bsm_csr* b, bsm_csr** out, hipStream_t s);
int csr_from_coo_device(int dtype, uint64_t rows, uint64_t cols, uint64_t n, const uint64_t* row,
                        const uint64_t* col, const void* vals, bsm_csr** out, hipStream_t s);
int gen_insert_stream(int dtype, uint64_t seed, uint64_t i0, uint64_t n, uint64_t rows, uint64_t cols,
                      uint64_t vmod, uint64_t* row, uint64_t* col, void* vals, hipStream_t s);
uint64_t spmm_panel_cols(int dtype, uint64_t n_cols, uint64_t k);  // 0 = single pass
uint64_t spmm_plan_bytes(uint64_t rows, uint64_t n_cols, uint64_t panel_cols);
int spmm_plan(uint64_t rows, uint64_t n_cols, const int64_t* rp, const int32_t* col,
              uint64_t panel_cols, int32_t* seg, int* usable, hipStream_t s);  // synchronous
int spmm_panelled(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, const int64_t* rp,
                  const int32_t* col, const void* vals, uint64_t k, const void* x, void* y,
                  int32_t* row_nnz, uint64_t panel_cols, const int32_t* seg, hipStream_t s);
// row-block x column-panel schedule (kernels_tiled.hip)
bool tiled_wanted(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, uint64_t k, uint64_t max_row_len);
// whether the model picks the two-pass kernel for this shape on `cus` CUs (BSM_TILED_HALF aside)
bool tiled_half_wanted(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, uint64_t k, uint32_t cus);
// synchronous; the copy must leave `reserve` device bytes free; pt (may be
// null) receives host times of its phases
int tiled_create(int dtype, uint64_t rows, uint64_t n_cols, uint64_t nnz, const int64_t* rp, const int32_t* col,
                 const void* vals, uint64_t k, int flags, bsm_tiled** out, hipStream_t s, uint64_t reserve = 0,
                 PlanTimes* pt = nullptr);
int tiled_spmm(const bsm_tiled* t, const void* x, void* y, int32_t* row_nnz, bool neg_init, hipStream_t s);
void tiled_destroy(bsm_tiled* t);
int compact_dispatch(int dtype, uint64_t rows, uint64_t k, const void* y, const int64_t* out_rp,
                     int32_t* out_col, void* out_vals, hipStream_t s);
// Small results (rows <= SMALL_OUT_ROWS, rows x k <= SMALL_OUT_CAP): the
// row-count scan and the compaction in one workgroup, which also writes the
// result into `host` (page-locked: row_ptr int64 [rows + 1], then cols int32
// [cap] at small_col_bytes alignment, then values [cap]); kernels_spmm.hip.
constexpr uint64_t SMALL_OUT_ROWS = 8192;
constexpr uint64_t SMALL_OUT_CAP = 131072;
inline size_t small_col_bytes(uint64_t cap) { return (cap * sizeof(int32_t) + 15) / 16 * 16; }
int compact_small_dispatch(int dtype, uint64_t rows, uint64_t k, const int32_t* nz, const void* y, int64_t* out_rp,
                           int32_t* out_col, void* out_vals, void* host, uint64_t cap, hipStream_t s);
int pack_cols_to_rowmajor(int dtype, uint64_t n, uint64_t k, const void* colmajor, void* rowmajor,
                          hipStream_t s);
int unpack_rowmajor_to_cols(int dtype, uint64_t n, uint64_t k, const void* rowmajor,
                            void* colmajor, hipStream_t s);
int transpose_dispatch(const bsm_csr* a, bsm_csr** out, hipStream_t s);
int analyse_dispatch(const int64_t* rp, const int32_t* col, uint64_t rows, uint64_t cols,
                     uint64_t* d_out3, hipStream_t s);
int gen_row_ptr(uint64_t seed, uint64_t row0, uint64_t rows, uint32_t n_cols, int kind,
                uint32_t a, uint32_t b, int64_t* rp, void* ws, uint64_t ws_bytes, hipStream_t s);
int gen_entries(int dtype, uint64_t seed, uint64_t row0, uint64_t rows, uint32_t n_cols,
                int value_kind, const int64_t* rp, int32_t* col, void* vals, hipStream_t s);
int gen_dense(int dtype, uint64_t seed, uint64_t row0, uint64_t n, uint64_t k, int value_kind,
              void* x, hipStream_t s);
int solve_dispatch_cholesky(const bsm_csr* a, bsm_csr** out, hipStream_t s);
int solve_dispatch_trsv(const bsm_csr* m, bool lower, uint64_t k, uint64_t n, const void* b_dev,
                        void* x_dev, hipStream_t s);
int solve_dispatch_full(const bsm_csr* a, uint64_t k, uint64_t n, const void* b_dev, void* x_dev,
                        hipStream_t s);
int solve_dispatch_blocked(const bsm_csr* a, uint64_t k, uint64_t n, const void* b_dev, void* x_dev,
                           hipStream_t s);
int solve_dispatch_nd(const bsm_csr* a, uint64_t k, uint64_t n, const void* b_dev, void* x_dev, hipStream_t s);
// the kept nd factor (kernels_nd.hip and kernels_nd_*.hip); all synchronous on s. b_dev / x_dev:
// ROW-major n x k, as solve_dispatch_nd's
// factor_dtype: BSM_F64 or BSM_F32; where it is not a's, a's values are converted first
// idx (m distinct vertices < n, checked by the caller; m == 0: none): the Schur set, the root front's own columns
int nd_factor_create(const bsm_csr* a, int factor_dtype, bsm_nd_factor** out, hipStream_t s,
                     const uint64_t* idx = nullptr, uint64_t m = 0);
// The Schur complement of a kept factor made with a set (kernels_nd_schur.hip); all synchronous
// on s. out_dev: m x m of f's dtype, column-major with leading dimension ld >= m, in the caller's order of the
// set. b_dev / x_dev: ROW-major n x k, g_dev / xg_dev: ROW-major m x k, all of f's dtype.
int nd_factor_schur(const bsm_nd_factor* f, const bsm_csr* a, void* out_dev, uint64_t ld, hipStream_t s);
int nd_factor_schur_condense(const bsm_nd_factor* f, uint64_t k, const void* b_dev, void* g_dev, hipStream_t s);
int nd_factor_schur_expand(const bsm_nd_factor* f, uint64_t k, const void* b_dev, const void* xg_dev, void* x_dev,
                           hipStream_t s);
// system: BSM_ND_SYS_A / _L / _LT (bsm.h)
int nd_factor_solve(const bsm_nd_factor* f, int system, uint64_t k, uint64_t n, const void* b_dev, void* x_dev,
                    hipStream_t s);
int nd_factor_refactor(bsm_nd_factor* f, const bsm_csr* a, hipStream_t s);
int nd_factor_logdet(const bsm_nd_factor* f, double* logdet, hipStream_t s);
int nd_factor_perm(const bsm_nd_factor* f, int64_t* perm, hipStream_t s);
int nd_factor_export(const bsm_nd_factor* f, bsm_csr** l, bsm_csr** l_star, hipStream_t s);
// Z = A^-1 on the pattern of L + L^T: the diagonal (A's order) into diag_dev
// (or null), Z[rows[e]][cols[e]] (A's order, indices < n, uint64 on the
// device) into vals_dev for e < nq. *n_miss pairs lie outside the pattern,
// the first of them at *first_miss (their vals are 0).
int nd_factor_selinv(const bsm_nd_factor* f, void* diag_dev, uint64_t nq, const uint64_t* rows_dev,
                     const uint64_t* cols_dev, void* vals_dev, uint64_t* n_miss, uint64_t* first_miss, hipStream_t s);
// The factor of P (S + sign W W^T) P^T in place (sign = +1 / -1, 1 <= k <= 16
// checked by the caller). W column-compressed on the device: colptr (k + 1),
// rows (A's order, < n, nnz_w of them), vals (f's src_dtype), no stored zeros.
// *n_miss columns lie outside the pattern, the first of them *first_miss:
// nothing was written then. Synchronous on s.
int nd_factor_updown(bsm_nd_factor* f, int sign, uint64_t k, uint64_t nnz_w, const int64_t* colptr_dev,
                     const uint64_t* rows_dev, const void* vals_dev, uint64_t* n_miss, uint64_t* first_miss,
                     hipStream_t s);
// A x = b for a sparse b, x at selected rows. b on the HOST,
// column-compressed as nd_factor_updown's W and checked by the caller (col_ptr
// ascending from 0, rows < n strictly ascending within a column), vals of f's
// dtype; xrows: nq host rows < n, or null for every row. x_dev: ROW-major
// nq x k (n x k) of f's dtype. info: 4 entries or null (bsm.h). The caller has
// found n, k and the number of output rows positive. Synchronous on s.
int nd_factor_solve_sparse(const bsm_nd_factor* f, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                           const void* vals, uint64_t nq, const uint64_t* xrows, void* x_dev, uint32_t* info,
                           hipStream_t s);
// New values at a few named places of the factored pattern:
// the fronts on the paths from those entries to the roots are factored again,
// with the bits of nd_factor_refactor(f, a). rows / cols: nc pairs on the HOST,
// any order, (j, i) as good as (i, j), repeats allowed. a_old != null (the
// `since` form, rows / cols ignored): the places are the stored entries with
// col <= row whose bits differ between a_old and a. info: 3 entries or null
// (active fronts, fronts in the plan, changed entries). Synchronous on s.
int nd_factor_refactor_partial(bsm_nd_factor* f, const bsm_csr* a_old, const bsm_csr* a, uint64_t nc,
                               const uint64_t* rows, const uint64_t* cols, uint64_t* info, hipStream_t s);
// The differentiable solve's pieces. The sampled dense-dense
// product on a CSR pattern (kernels_sddmm.hip; mode: BSM_SDDMM_*; async on s):
// the checks of dtype, mode, k and squareness are its own.
int sddmm_dispatch(int dtype, int mode, uint64_t rows, uint64_t cols, uint64_t nnz, const int64_t* rp,
                   const int32_t* col, uint64_t k, const void* u, const void* v, void* out, hipStream_t s);
// BSM_SDDMM_SYM_LOWER on the factor's kept pattern (async on s)
int nd_factor_sddmm(const bsm_nd_factor* f, int dtype, uint64_t k, const void* u, const void* v, void* out,
                    hipStream_t s);
// nd_factor_refactor on the kept pattern with nnz device values of `dtype` in
// its storage order: no upload, no pattern comparison. Synchronous on s.
int nd_factor_refactor_values(bsm_nd_factor* f, int dtype, uint64_t nnz, const void* vals_dev, hipStream_t s);
// nd_factor_selinv's Z read out at every stored entry of the kept pattern
// (f->nnz values of f's dtype on the device). Synchronous on s.
int nd_factor_inv_pattern(const bsm_nd_factor* f, void* out_dev, hipStream_t s);
// mixed precision on a kept factor (kernels_refine.hip)
// n float values into the other float dtype, round-to-nearest (async on s)
int convert_values(int src_dtype, int dst_dtype, uint64_t n, const void* src, void* dst, hipStream_t s);
void sym_destroy(bsm_sym* m);
// The refined solve; the caller has checked a against f (dtype, device,
// shape) and tol >= 0. b_dev / x_dev: ROW-major n x k of a's dtype (they may
// be the same array); iters / berr: k host entries or null. Synchronous on s.
int nd_refine_solve(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, const void* b_dev, void* x_dev,
                    uint32_t max_iter, double tol, uint32_t* iters, double* berr, hipStream_t s);

// What the refined solve shares with the pcg solve (kernels_pcg.hip).
using ull = unsigned long long;

// |v| as an integer: ordered as the values are, every NaN above +inf
__device__ __forceinline__ ull abs_bits(double v) { return (ull)__double_as_longlong(fabs(v)); }
__device__ __forceinline__ double bits_abs(ull b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ ull umax(ull a, ull b) { return a > b ? a : b; }

struct DrainOnError {  // cached temporaries go back only after the kernels that use them
    hipStream_t s;
    bool armed = true;
    ~DrainOnError() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

constexpr unsigned REFINE_MAX_BLOCKS = 1024;  // the partials one workgroup reduces

struct RefineCol;  // refine_rule.hpp
// the handle's symmetric copy, built on first use
int sym_obtain(const bsm_csr* a, hipStream_t s, const bsm_sym** out);
// lanes per row of refine_resid, and its workgroups (properties of S and n alone)
int resid_group(const bsm_sym* S, int64_t n);
unsigned resid_blocks(int g, int64_t n);
// The refined solve's first iterate, by its own kernels: B = (double)b, st =
// the columns' ||b||inf and scales, X = scale M^-1 cast(B / scale), R = B - S X,
// part = refine_resid's maxima of |r| and |x| ([block][2][k], *nb blocks). W:
// n k values of the factor's dtype. Async on s past the solve.
int refine_first_iterate(const bsm_nd_factor* f, const bsm_csr* a, const bsm_sym* S, int64_t n, int64_t k,
                         const void* b_dev, double* B, double* X, double* R, void* W, ull* part, RefineCol* st,
                         unsigned* nb, hipStream_t s);
// W = M^-1 cast(V / scale) on st's active columns, zeros on the others
// (refine_scale_cast, then the factor's A-system solve in place)
int refine_precondition(const bsm_nd_factor* f, int64_t n, int64_t k, const double* V, const RefineCol* st, void* W,
                        hipStream_t s);
// R = B - S X with its partial maxima (refine_resid)
int refine_residual(const bsm_csr* a, const bsm_sym* S, int64_t n, int64_t k, const double* X, const double* B,
                    double* R, ull* part, unsigned* nb, hipStream_t s);
// The pcg solve (kernels_pcg.hip); arguments and checks as nd_refine_solve's,
// flags: k host entries or null (bit 0: the column broke down).
int nd_pcg_solve(const bsm_nd_factor* f, const bsm_csr* a, uint64_t k, const void* b_dev, void* x_dev,
                 uint32_t max_iter, double tol, uint32_t* iters, double* berr, uint32_t* flags, hipStream_t s);
// The nev smallest eigenpairs of S by block shift-invert Lanczos
// (kernels_eig.hip); the caller has checked a against f and the arguments
// (eig_rule.hpp: ncv is the basis size in use, tol >= 0). v0_dev: ROW-major
// n x block of a's dtype or null; vec_dev: ROW-major n x nev of a's dtype or
// null; lam / resid: nev host entries; info: 4 host entries or null.
// Synchronous on s.
int nd_eigsh(const bsm_nd_factor* f, const bsm_csr* a, uint64_t nev, uint64_t block, uint64_t ncv, double tol,
             uint64_t seed, const void* v0_dev, double* lam, void* vec_dev, double* resid, uint32_t* info,
             hipStream_t s);
// The same for S y = lambda S_M y, S_M being m's lower triangle mirrored (m:
// n x n, a's dtype and device, checked by the caller): the loop in the S_M
// inner product. BSM_ERR_UNSUPPORTED when S_M proves not positive definite,
// with nothing written.
int nd_eigsh_gen(const bsm_nd_factor* f, const bsm_csr* a, const bsm_csr* m, uint64_t nev, uint64_t block, uint64_t ncv,
                 double tol, uint64_t seed, const void* v0_dev, double* lam, void* vec_dev, double* resid,
                 uint32_t* info, hipStream_t s);
}  // namespace bsm

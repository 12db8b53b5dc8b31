// nd_internal.hpp -- what the nested-dissection solver's files share: the plan's types and small
// helpers, and the host functions that cross a file boundary. kernels_nd_plan.hip builds and caches plans;
// kernels_nd.hip factors and solves on one; the kept factor's other answers each have a file (kernels_nd_selinv /
// _updown / _sparse / _partial / _schur.hip). Every kernel is defined in one file: another file reaches it through a
// host function declared here (NdHost: instantiated for float and double by kernels_nd.hip).
#pragma once

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "bsm_internal.hpp"
#include "reach_rule.hpp"

namespace bsm {

struct NdDev {
    int64_t foff;      // the front at F + foff
    int64_t dinv_off;  // npt inverse diagonal tiles (Dinv[q * 64 + l] = Linv[l][q])
    int64_t flag_off;  // nt x npt tile flags
    int64_t st_off;    // m front rows (st) and their places in the parent's front (ri)
    int64_t voff;      // f_pad solve-vector entries per right-hand column
    int64_t start;     // own columns [start, start + np)
    int32_t ld, np, np_pad, m, npt, nt, parent, kid0, kid1;
    int32_t tb_off;     // (child) nt + 1 bounds of the parent's tile rows in ri: tb[t] = first a, ri[a] >= 64 t
    int32_t pull_swap;  // (parent) kid1's update block is added before kid0's (kid1 on a lower level)
    int32_t tile_off;   // the front's lower tiles' index base (nd_lower_idx) in the plan's per-tile lists of A
};

// (I, K), I >= K, among a front's nt (nt + 1) / 2 lower tiles, column by column
__host__ __device__ inline int64_t nd_lower_idx(int32_t nt, int32_t I, int32_t K) {
    return (int64_t)K * nt - (int64_t)K * (K - 1) / 2 + (I - K);
}

__device__ __forceinline__ int32_t lower_bound_i32(const int32_t* a, int32_t len, int64_t x) {
    int32_t lo = 0, hi = len;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// per factor task: its children's blocks, first and second in nd_extend2's
// order (NdPull::ra = 0: none), so the tile reads them with its task instead
// of through node -> child -> bounds (tb); written by nd_task_pull
struct NdPull {
    int64_t uoff;   // the child's update block U at F + uoff (U[a][b] at uoff + b ld + a)
    int64_t uvoff;  // its update vector at V + uvoff (the folded forward solve)
    int32_t rcoff, ld, a0, ra, b0, rbn;
};

inline unsigned nd_blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// The layout's options: part of the plan's keys
struct NdLay {
    int32_t lag = 0;     // the tiles below a diagonal follow it by this many fronts' diagonals (0: by all of them)
    bool plain = false;  // the extend-add by nd_extend2 launches (their task lists are built only then)
    bool operator==(const NdLay& o) const { return lag == o.lag && plain == o.plain; }
};

// A pattern's plan, device side: one allocation holding the node
// descriptors, front rows, their places in the parents, pinv / owner, the
// level lists, tiles and extend tasks, and perm; plus the per-level offsets
// the launches need. Cached on the handle (bsm_csr::nd_plan) unless
// BSM_ND_CACHE=0: the pattern of a finalised Csr never changes.
struct NdCached {
    int64_t leaf = 0;
    int32_t nn = 0, n_levels = 0;
    std::vector<int64_t> tiles_off, lvl_off, ext2_off, ftask_off, btask_off;
    int64_t f_elems = 0, dinv_elems = 0, n_flags = 0, vtot = 0, max_front = 0;
    size_t o_dev = 0, o_st = 0, o_ri = 0, o_pinv = 0, o_owner = 0, o_lvl = 0, o_tiles = 0, o_ext2 = 0, o_ftask = 0,
           o_btask = 0, o_perm = 0, o_tb = 0;
    size_t n_tiles = 0, n_ext2 = 0;
    int64_t n_lower = 0, n_aent = 0;  // the fronts' lower tiles; A's lower entries
    std::vector<int32_t> lvl_nt, lvl_npt;  // per level: the largest nt and npt of its fronts (the selected inverse's grids)
    // each node's parent and level on the host: the update / downdate of a kept
    // factor builds its active fronts' per-level lists from them (§4.9j)
    std::vector<int32_t> h_parent, h_level;
    // and its two children: the sparse solve's forward set names the active ones (§4.9k)
    std::vector<int32_t> h_kid0, h_kid1;
    // and its tile rows, read back from the device by the first partial refactor (§4.9l), under part_mu
    std::mutex part_mu;
    std::vector<int32_t> h_nt;
    DBuf aent, tq;                    // the default pipeline: A's entries by tile (nd_aent_*), per task ranges
    DBuf pdesc;                       // and per task its children's blocks (nd_task_pull)
    NdLay lay;
    double ms_graph = 0, ms_order = 0, ms_symbolic = 0, ms_layout = 0, ms_pack = 0;
    DBuf plan;
    // The numeric storage (fronts, inverse diagonal tiles, flags) stays with
    // the cached plan for the handle's next solve: hipFree of the 5.6 GB of
    // fronts and hipMalloc again cost ~0.9 ms of a C5 solve's 11.4
    // (profiles/r05_q_*). One solve at a time uses them (num_mu; a concurrent
    // solve on the same handle allocates its own). BSM_ND_KEEP=0: freed after
    // every solve.
    std::mutex num_mu;
    DBuf fr, dv, fl;
    std::atomic<size_t> kept_bytes{0};  // fr + dv + fl, written under num_mu
    // The device copy of the pattern this plan was built from (row_ptr, then
    // col, as the cross-handle cache's entries keep it), for whoever still
    // holds it: the cache's entry and the kept factors of this plan, which
    // compare a refactorisation's matrix against it. Not owned by the plan.
    std::mutex pat_mu;
    std::weak_ptr<DBuf> pattern;
    // drop the kept numeric storage unless a solve holds it
    bool release_numeric() {
        std::unique_lock<std::mutex> l(num_mu, std::try_to_lock);
        if (!l.owns_lock()) return false;
        fr.reset();
        dv.reset();
        fl.reset();
        kept_bytes = 0;
        return true;
    }
};

// The environment's switches (README.md), read once per solve
struct NdOpts {
    int64_t leaf;  // C5 leaf sweep: 128 / 192 / 256 / 320 -> 11.9 / 11.4 / 12.3 / 12.5 ms
    NdLay lay;     // BSM_ND_LAG, BSM_ND_PLAIN
    int threads;   // the host analysis' workers
    bool cache, shared, keep;  // the plan on the handle; across handles; its numeric storage kept too
    size_t cache_entries, cache_mb;
    bool fold;                 // one right-hand side: the forward solve inside the factor
    int fwd_tiles, bwd_tiles;  // the solves by tiles: 0 never, 1 every level, 2 levels with fewer pairs than CUs
    bool poison, hash_zero, trace, stamps;  // tests and diagnostics
};

// the bytes of a pattern copy's row_ptr (n + 1 int64, padded to 256 bytes); col (nnz int32) follows
inline size_t nd_pattern_rp_bytes(int64_t n) { return ((size_t)(n + 1) * sizeof(int64_t) + 255) / 256 * 256; }

// Waits for the stream when an error return leaves kernels queued that
// write the kept numeric storage, so no other solve takes that storage
// (num_mu is released after this guard runs) while they still run.
struct NdDrainOnError {
    hipStream_t s;
    bool armed = false;
    ~NdDrainOnError() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

// the plan's device arrays
struct NdPtrs {
    const NdDev* nodes;
    const int32_t *st, *ri, *pinv, *owner, *lvl;
    const int4 *tiles, *ext2;
    const int2 *ftask, *btask;
    const int64_t* perm;
};
inline NdPtrs nd_ptrs(const NdCached& C) {
    const char* pb = C.plan.as<char>();
    NdPtrs p;
    p.nodes = (const NdDev*)(pb + C.o_dev);
    p.st = (const int32_t*)(pb + C.o_st);
    p.ri = (const int32_t*)(pb + C.o_ri);
    p.pinv = (const int32_t*)(pb + C.o_pinv);
    p.owner = (const int32_t*)(pb + C.o_owner);
    p.lvl = (const int32_t*)(pb + C.o_lvl);
    p.tiles = (const int4*)(pb + C.o_tiles);
    p.ext2 = (const int4*)(pb + C.o_ext2);
    p.ftask = (const int2*)(pb + C.o_ftask);
    p.btask = (const int2*)(pb + C.o_btask);
    p.perm = (const int64_t*)(pb + C.o_perm);
    return p;
}

// the device's CUs and the persistent kernels' workgroups per CU
struct NdGrid {
    int cus = 0, per_cu = 0, fper = 0, bper = 0;
};

// the state a failed refactorisation leaves behind (under f->mu)
#define ND_REQUIRE_VALUES(f) \
    BSM_REQUIRE((f)->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first")

// ---- kernels_nd_plan.hip ----
NdOpts nd_options();
int nd_obtain_plan(const bsm_csr* a, const NdOpts& opt, NdLay lay, size_t es, hipStream_t s,
                   std::shared_ptr<NdCached>& pc, const std::vector<int64_t>* last = nullptr);
void nd_trace(const NdOpts& opt, const NdCached& C, int64_t N, size_t es);
void nd_cache_trim(size_t budget, const NdCached* keep);
int nd_alloc_numeric(DBuf& b, size_t bytes, const NdCached* keep);
int nd_pattern_copy(const bsm_csr* a, hipStream_t s, std::shared_ptr<DBuf>& out);
int nd_pattern_same(const bsm_csr* a, const bsm_nd_factor& f, hipStream_t s);

// ---- kernels_nd.hip ----
// Its kernels for the other files, per dtype: the persistent kernels' occupancy, nd_factor on a list of tasks, one
// level of nd_forward_path / nd_backward_path, the dense forward and backward levels (up to a level), and the
// right-hand sides' permutation
template <typename T>
struct NdHost {
    static int grid(bool factor, bool solves, NdGrid& g);
    static int factor_launch(const NdPtrs& p, const NdGrid& g, const int4* tiles, int64_t nt, T* F, T* Dinv, int* flags,
                             int* ticket, int* status, T* fV, const T* fbp, const int64_t* aent, const T* av,
                             const int2* tq, const NdPull* pd, unsigned long long* stamps, hipStream_t s);
    static int path_launch(bool forward, const NdCached& C, const ReachFront* act, unsigned cnt, unsigned kc, int64_t N,
                           T* bp, T* V, const T* F, const T* Dinv, hipStream_t s);
    static int forward_levels(const NdCached& C, const NdOpts& opt, const NdGrid& g, int64_t N, uint64_t k, const T* F,
                              const T* Dinv, const T* bp, T* V, int* d_yf, int* d_ftk, int* d_status, hipStream_t s,
                              int32_t lv_end);
    static int backward_levels(const NdCached& C, const NdOpts& opt, const NdGrid& g, int64_t N, uint64_t k, const T* F,
                               const T* Dinv, T* bp, T* V, int* d_xf, int* d_btk, int* d_status, hipStream_t s,
                               int32_t lv_end);
    static int permute_launch(bool gather, const NdCached& C, int64_t N, uint64_t k, const T* src, T* dst,
                              hipStream_t s);
};
int nd_status_end(bool factor, const int* d_status, NdDrainOnError& drain, const char* stage, hipStream_t s);
int nd_factor_numeric(const bsm_csr* a, bsm_nd_factor& f, hipStream_t s);
int nd_refactor_matches(const bsm_nd_factor* f, const bsm_csr* a);

}  // namespace bsm

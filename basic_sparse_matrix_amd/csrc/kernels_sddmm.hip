// kernels_sddmm.hip -- the sampled dense-dense product on a CSR pattern
// (gfx950): out[p] for every stored entry p = (i, j),
//   BSM_SDDMM_ALL        out[p] = dot(U[i,:], V[j,:])
//   BSM_SDDMM_SYM_LOWER  j < i: dot(U[i,:], V[j,:]) + dot(U[j,:], V[i,:]);
//                        j == i: dot(U[i,:], V[i,:]); j > i: +0.0, nothing loaded
// The dot's order is sddmm_rule.hpp's and depends on k alone: W = sddmm_lanes(k)
// lanes share an entry, lane c loads U[i, c] and V[j, c] (a row piece is one
// coalesced read), and the tree is __shfl_down steps of width W. Entries are
// assigned flat over nnz, SDDMM_BLOCK_ENTRIES consecutive ones to a block: in
// each step the block's 256 / W groups take consecutive entries (col read and
// out written side by side), and an entry's row is found by bisection of
// row_ptr inside the block's own row span, which two threads bisect out of the
// whole row_ptr once per block. No atomics; nothing but out[0..nnz) is written.
#include <algorithm>

#include "bsm_internal.hpp"
#include "sddmm_rule.hpp"

namespace bsm {
namespace {

constexpr int SDDMM_BLOCK_ENTRIES = 512;

// the row of entry p: the smallest r in [lo, hi] with rp[r + 1] > p, else hi
// (reads rp[lo + 1 .. hi] only)
__device__ __forceinline__ int64_t sddmm_row_of(const int64_t* __restrict__ rp, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rp[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// sddmm_tree64 across the W lanes of a group: lane c holds t[c], `live` terms exist; lane 0 gets the sum
template <typename T, int W>
__device__ __forceinline__ T sddmm_lane_tree(T t, int c, int live) {
#pragma unroll
    for (int h = W / 2; h >= 1; h /= 2) {
        const T o = __shfl_down(t, (unsigned)h, W);
        if (c < h && c + h < live) t = Arith<T>::add(t, o);
        live = live < h ? live : h;
    }
    return t;
}

template <typename T, int W, bool SYM>
__global__ __launch_bounds__(256) void sddmm_kernel(int64_t rows, int64_t nnz, const int64_t* __restrict__ rp,
                                                    const int32_t* __restrict__ col, int64_t k,
                                                    const T* __restrict__ U, const T* __restrict__ V,
                                                    T* __restrict__ out) {
    constexpr int G = 256 / W;  // entries per step
    __shared__ int64_t span[2];
    const int64_t base = (int64_t)blockIdx.x * SDDMM_BLOCK_ENTRIES;
    const int64_t end = base + SDDMM_BLOCK_ENTRIES < nnz ? base + SDDMM_BLOCK_ENTRIES : nnz;
    if (threadIdx.x < 2) span[threadIdx.x] = sddmm_row_of(rp, 0, rows - 1, threadIdx.x ? end - 1 : base);
    __syncthreads();
    int64_t r_lo = span[0];
    const int64_t r_hi = span[1];
    const int g = (int)threadIdx.x / W, c = (int)threadIdx.x % W;
    for (int64_t p0 = base; p0 < end; p0 += G) {  // the same trip count for the whole block: every lane shuffles
        const int64_t p = p0 + g;
        const bool on = p < end;
        int64_t i = 0, j = 0;
        if (on) {
            i = r_lo = sddmm_row_of(rp, r_lo, r_hi, p);  // a group's entries ascend
            j = col[p];
        }
        const bool one = on && (!SYM || j <= i), two = SYM && on && j < i;
        T d1 = Arith<T>::zero(), d2 = Arith<T>::zero();
        for (int64_t c0 = 0; c0 < k; c0 += W) {  // one pass for k <= 64, else chunks of 64 in ascending order
            const int live = (int)(k - c0 < W ? k - c0 : W);
            T t1 = Arith<T>::zero(), t2 = Arith<T>::zero();
            if (c < live) {
                const int64_t cc = c0 + c;
                if (one) t1 = Arith<T>::mul(U[i * k + cc], V[j * k + cc]);
                if (two) t2 = Arith<T>::mul(U[j * k + cc], V[i * k + cc]);
            }
            t1 = sddmm_lane_tree<T, W>(t1, c, live);
            d1 = c0 ? Arith<T>::add(d1, t1) : t1;
            if constexpr (SYM) {
                t2 = sddmm_lane_tree<T, W>(t2, c, live);
                d2 = c0 ? Arith<T>::add(d2, t2) : t2;
            }
        }
        if (on && c == 0) out[p] = two ? Arith<T>::add(d1, d2) : one ? d1 : Arith<T>::zero();
    }
}

template <typename T, int W>
int sddmm_launch(int mode, int64_t rows, int64_t nnz, const int64_t* rp, const int32_t* col, int64_t k, const T* u,
                 const T* v, T* out, hipStream_t s) {
    const unsigned grid = (unsigned)((nnz + SDDMM_BLOCK_ENTRIES - 1) / SDDMM_BLOCK_ENTRIES);
    if (mode == BSM_SDDMM_SYM_LOWER) sddmm_kernel<T, W, true><<<grid, 256, 0, s>>>(rows, nnz, rp, col, k, u, v, out);
    else sddmm_kernel<T, W, false><<<grid, 256, 0, s>>>(rows, nnz, rp, col, k, u, v, out);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

template <typename T>
int sddmm_t(int mode, int64_t rows, int64_t nnz, const int64_t* rp, const int32_t* col, int64_t k, const void* u,
            const void* v, void* out, hipStream_t s) {
    const T* const uu = static_cast<const T*>(u);
    const T* const vv = static_cast<const T*>(v);
    T* const oo = static_cast<T*>(out);
    switch (sddmm_lanes((uint64_t)k)) {
        case 1: return sddmm_launch<T, 1>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
        case 2: return sddmm_launch<T, 2>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
        case 4: return sddmm_launch<T, 4>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
        case 8: return sddmm_launch<T, 8>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
        case 16: return sddmm_launch<T, 16>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
        case 32: return sddmm_launch<T, 32>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
        default: return sddmm_launch<T, 64>(mode, rows, nnz, rp, col, k, uu, vv, oo, s);
    }
}

}  // namespace

int sddmm_dispatch(int dtype, int mode, uint64_t rows, uint64_t cols, uint64_t nnz, const int64_t* rp,
                   const int32_t* col, uint64_t k, const void* u, const void* v, void* out, hipStream_t s) {
    BSM_REQUIRE(dtype == BSM_F64 || dtype == BSM_F32, BSM_ERR_INVALID, "sddmm: f32/f64 only, got dtype %d", dtype);
    BSM_REQUIRE(mode == BSM_SDDMM_ALL || mode == BSM_SDDMM_SYM_LOWER, BSM_ERR_INVALID,
                "sddmm: mode must be BSM_SDDMM_ALL or BSM_SDDMM_SYM_LOWER, got %d", mode);
    BSM_REQUIRE(k > 0, BSM_ERR_INVALID, "sddmm: k == 0 (a dot product of no terms)");
    BSM_REQUIRE(mode != BSM_SDDMM_SYM_LOWER || rows == cols, BSM_ERR_INVALID,
                "sddmm: BSM_SDDMM_SYM_LOWER needs a square pattern, got %llu x %llu", (unsigned long long)rows,
                (unsigned long long)cols);
    if (rows == 0 || nnz == 0) return BSM_OK;
    BSM_REQUIRE(rp && col && u && v && out, BSM_ERR_INVALID, "null argument");
    BSM_REQUIRE(nnz / SDDMM_BLOCK_ENTRIES < 0x7fffffffull, BSM_ERR_UNSUPPORTED,
                "sddmm: %llu entries exceed the grid", (unsigned long long)nnz);
    BSM_REQUIRE(std::max(rows, cols) < ((uint64_t)1 << 62) / k, BSM_ERR_UNSUPPORTED,
                "sddmm: an operand of %llu x %llu exceeds the 64-bit index", (unsigned long long)std::max(rows, cols),
                (unsigned long long)k);
    return dtype == BSM_F64
               ? sddmm_t<double>(mode, (int64_t)rows, (int64_t)nnz, rp, col, (int64_t)k, u, v, out, s)
               : sddmm_t<float>(mode, (int64_t)rows, (int64_t)nnz, rp, col, (int64_t)k, u, v, out, s);
}

}  // namespace bsm

// kernels_nd_selinv.hip -- the selected inverse of a kept nd factor (below)
#include <algorithm>

#include "nd_internal.hpp"

namespace bsm {
namespace {

#include "solve_tiles.hpp"

// Z = A^-1 on the pattern of L + L^T by the Takahashi / Erisman-Tinney
// recursion: the separator tree walked top-down, a Z front per front (F's
// layout, lower tiles, the diagonal tiles whole), with the 64-wide pivot tile
// columns as supernodes. Per level from the top: nd_selinv_pull brings each
// front's Z22 = Z[st, st] out of its parent's finished Z front (nd_extend2
// backwards), then for K = npt - 1 .. 0 three launches over the level's fronts:
//     nd_selinv_yhat   Y_IK = L_IK Dinv_K                       every I > K
//     nd_selinv_below  Z_IK = - sum_{J > K} Zsym(I, J) Y_JK     every I > K, J ascending
//     nd_selinv_diag   Z_KK = Dinv_K^T Dinv_K - sum_{I > K} Y_IK^T Z_IK, I ascending
// One workgroup per tile and a counted loop per sum: no flags, no atomics, and
// the bits do not depend on the grid. A padding pivot is an identity pivot
// coupled to nothing: its column of L, its row of L and its part of Dinv are
// masked to 0 / the identity as they are loaded (the factor leaves some of
// them undefined), so its row and column of Z come out exactly 0 and 1. The
// update block of F is never read.

// L_IK into LDS as the products' A operand: X[c][r] = L[64 I + r][64 K + c], 0
// in a padding pivot's column or row and in the rows past f
template <typename T>
__device__ __forceinline__ void nd_selinv_load_l(const NdDev& nd, const T* __restrict__ Fn, int I, int K,
                                                 T (*X)[TLD], int tid) {
    const int rem = nd.np - 64 * K;
    T v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u, r = e & 63, c = e >> 6, row = 64 * I + r;
        const bool live = c < rem && (row < nd.np || (row >= nd.np_pad && row < nd.np_pad + nd.m));
        v[u] = live ? Fn[(int64_t)(64 * K + c) * nd.ld + row] : (T)0;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u;
        X[e >> 6][e & 63] = v[u];
    }
}
// Dinv_K into LDS: X[k][c] = Linv[k][c] (Dinv[c * 64 + k]), the identity over the padding pivots
template <typename T>
__device__ __forceinline__ void nd_selinv_load_dinv(const NdDev& nd, const T* __restrict__ Dinv, int K, T (*X)[TLD],
                                                    int tid) {
    const int rem = nd.np - 64 * K;
    const T* const dk = Dinv + nd.dinv_off + (int64_t)K * 4096;
    T v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u, k = e & 63, c = e >> 6;
        v[u] = k < rem && c < rem ? dk[e] : (k == c ? (T)1 : (T)0);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u;
        X[e & 63][e >> 6] = v[u];
    }
}
// a 64 x 64 block at src (leading dimension ld) into LDS: X[e & 63][e >> 6] = src[(e >> 6) ld + (e & 63)]
// (TRANS: X[e >> 6][e & 63])
template <typename T, bool TRANS>
__device__ __forceinline__ void nd_selinv_load(const T* __restrict__ src, int64_t ld, T (*X)[TLD], int tid) {
    T v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u;
        v[u] = src[(int64_t)(e >> 6) * ld + (e & 63)];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u;
        if (TRANS) X[e >> 6][e & 63] = v[u];
        else X[e & 63][e >> 6] = v[u];
    }
}

// Z22 of every front of a level out of its parent's Z front: tile y of the
// front-row tiles' lower triangle (column by column), Z22[a][b] = Zp[ri[a]][ri[b]]
// read from the parent's lower triangle (ri ascends, so a >= b is; a diagonal
// tile is written whole, its upper part mirrored), 0 past the m front rows.
// grid: fronts x tmax
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_pull(const NdDev* __restrict__ nodes, const int32_t* __restrict__ lvl,
                                                      int tmax, const int32_t* __restrict__ ri, T* __restrict__ Z) {
    const NdDev& nd = nodes[lvl[blockIdx.x / tmax]];
    const int mt = nd.nt - nd.npt;
    int y = (int)(blockIdx.x % tmax);
    if (y >= mt * (mt + 1) / 2) return;
    int J = 0;
    while (y >= mt - J) {
        y -= mt - J;
        ++J;
    }
    const int I = J + y, tid = threadIdx.x;
    const bool has = nd.parent >= 0 && nd.m > 0;
    const NdDev& pd = nodes[has ? nd.parent : 0];
    const T* const Zp = Z + pd.foff;
    const int32_t* const rc = ri + nd.st_off;
    T* const dst = Z + nd.foff + (int64_t)(nd.np_pad + 64 * J) * nd.ld + nd.np_pad + 64 * I;
    const int mlast = nd.m > 0 ? nd.m - 1 : 0;
#pragma unroll 4
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u, r = e & 63, c = e >> 6;
        const int a = 64 * I + r, b = 64 * J + c;
        T v = (T)0;
        if (has && a < nd.m && b < nd.m) {
            const int32_t pa = rc[min(a, mlast)], pb = rc[min(b, mlast)];
            const int32_t hi = pa > pb ? pa : pb, lo = pa > pb ? pb : pa;
            v = Zp[(int64_t)lo * pd.ld + hi];
        }
        dst[(int64_t)c * nd.ld + r] = v;
    }
}

// phase 1 of step K: Y_IK = L_IK Dinv_K into the front's panel (Y + 64 voff,
// ld x 64, column-major). grid: fronts x ntmax, tile row I = block % ntmax
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_yhat(const NdDev* __restrict__ nodes, const int32_t* __restrict__ lvl,
                                                      int ntmax, int K, const T* __restrict__ F,
                                                      const T* __restrict__ Dinv, T* __restrict__ Y) {
    __shared__ T PT[64][TLD];
    __shared__ T QT[64][TLD];
    const NdDev& nd = nodes[lvl[blockIdx.x / ntmax]];
    const int I = (int)(blockIdx.x % ntmax);
    if (K >= nd.npt || I <= K || I >= nd.nt) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = 16 * w + (lane >> 4), cm = lane & 15;
    nd_selinv_load_l<T>(nd, F + nd.foff, I, K, PT, tid);
    nd_selinv_load_dinv<T>(nd, Dinv, K, QT, tid);
    __syncthreads();
    T acc[4][4] = {};
    mfma_tile<T, false>((lds_t<T>*)&PT[0][0], (lds_t<T>*)&QT[0][0], acc, w, lane);
    T* const yp = Y + 64 * nd.voff + 64 * I;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) yp[(int64_t)(16 * cb + cm) * nd.ld + rb + 4 * q] = acc[cb][q];
}

// phase 2 of step K: Z_IK = - sum_{J = K + 1}^{nt - 1} Zsym(I, J) Y_JK, J
// ascending; Zsym(I, J) is Z's tile (I, J) for I >= J and tile (J, I)
// transposed otherwise (all of them finished: later steps' columns, or
// pulled). grid: fronts x ntmax
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_below(const NdDev* __restrict__ nodes,
                                                       const int32_t* __restrict__ lvl, int ntmax, int K,
                                                       const T* __restrict__ Y, T* __restrict__ Z) {
    __shared__ T PT[64][TLD];
    __shared__ T QT[64][TLD];
    const NdDev& nd = nodes[lvl[blockIdx.x / ntmax]];
    const int I = (int)(blockIdx.x % ntmax);
    if (K >= nd.npt || I <= K || I >= nd.nt) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = 16 * w + (lane >> 4), cm = lane & 15;
    const int64_t ld = nd.ld;
    T* const Zn = Z + nd.foff;
    const T* const yp = Y + 64 * nd.voff;
    T acc[4][4] = {};
    for (int J = K + 1; J < nd.nt; ++J) {
        // PT[k][r] = Zsym(I, J)[r][k]
        if (I >= J) nd_selinv_load<T, true>(Zn + (int64_t)64 * J * ld + 64 * I, ld, PT, tid);
        else nd_selinv_load<T, false>(Zn + (int64_t)64 * I * ld + 64 * J, ld, PT, tid);
        nd_selinv_load<T, false>(yp + 64 * J, ld, QT, tid);  // QT[k][c] = Y_JK[k][c]
        __syncthreads();
        mfma_tile<T, true>((lds_t<T>*)&PT[0][0], (lds_t<T>*)&QT[0][0], acc, w, lane);
        __syncthreads();
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) Zn[(int64_t)(64 * K + 16 * cb + cm) * ld + 64 * I + rb + 4 * q] = acc[cb][q];
}

// phase 3 of step K: Z_KK = Dinv_K^T Dinv_K - sum_{I = K + 1}^{nt - 1} Y_IK^T
// Z_IK, I ascending; stored whole, the upper part the mirror of the lower
// (later steps and the children read either half as Zsym). grid: fronts
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_diag(const NdDev* __restrict__ nodes, const int32_t* __restrict__ lvl,
                                                      int K, const T* __restrict__ Dinv, const T* __restrict__ Y,
                                                      T* __restrict__ Z) {
    __shared__ T PT[64][TLD];
    __shared__ T QT[64][TLD];
    const NdDev& nd = nodes[lvl[blockIdx.x]];
    if (K >= nd.npt) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = 16 * w + (lane >> 4), cm = lane & 15;
    const int64_t ld = nd.ld;
    T* const Zn = Z + nd.foff;
    const T* const yp = Y + 64 * nd.voff;
    nd_selinv_load_dinv<T>(nd, Dinv, K, QT, tid);
    __syncthreads();
    T acc[4][4] = {};
    mfma_tile<T, false>((lds_t<T>*)&QT[0][0], (lds_t<T>*)&QT[0][0], acc, w, lane);
    __syncthreads();
    for (int I = K + 1; I < nd.nt; ++I) {
        nd_selinv_load<T, false>(yp + 64 * I, ld, PT, tid);                            // PT[k][r] = Y_IK[k][r]
        nd_selinv_load<T, false>(Zn + (int64_t)64 * K * ld + 64 * I, ld, QT, tid);  // QT[k][c] = Z_IK[k][c]
        __syncthreads();
        mfma_tile<T, true>((lds_t<T>*)&PT[0][0], (lds_t<T>*)&QT[0][0], acc, w, lane);
        __syncthreads();
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) PT[rb + 4 * q][16 * cb + cm] = acc[cb][q];
    __syncthreads();
    T* const dst = Zn + (int64_t)64 * K * ld + 64 * K;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u, r = e & 63, c = e >> 6;
        dst[(int64_t)c * ld + r] = r >= c ? PT[r][c] : PT[c][r];
    }
}

// diag[perm[q]] = Z[q][q] for the n real pivots (A's order)
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_diag_out(int64_t n, const int32_t* __restrict__ owner,
                                                          const NdDev* __restrict__ nodes,
                                                          const int64_t* __restrict__ perm, const T* __restrict__ Z,
                                                          T* __restrict__ diag) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const NdDev& nd = nodes[owner[q]];
    const int64_t c = q - nd.start;
    diag[perm[q]] = Z[nd.foff + c * nd.ld + c];
}

// Z at new indices (p, q), either triangle: the front owning the lower of the
// two, the higher one a pivot row of it or found among its front rows. *hit is
// false (and the value 0) for a pair outside the pattern of L + L^T.
template <typename T>
__device__ __forceinline__ T nd_selinv_at(int64_t p, int64_t q, const int32_t* __restrict__ owner,
                                          const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                          const T* __restrict__ Z, bool* hit) {
    const int64_t lo = p < q ? p : q, hi = p < q ? q : p;
    const NdDev& nd = nodes[owner[lo]];
    const int64_t c = lo - nd.start;
    int64_t r = hi - nd.start;
    *hit = true;
    if (hi >= nd.start + nd.np) {
        const int32_t* const fs = st + nd.st_off;
        const int32_t a = lower_bound_i32(fs, nd.m, hi);
        *hit = a < nd.m && fs[a] == hi;
        r = nd.np_pad + a;
    }
    return *hit ? Z[nd.foff + c * nd.ld + r] : (T)0;
}

// vals[e] = Z[rows[e]][cols[e]] (A's order, either triangle; both indices < n).
// A pair outside the pattern of L + L^T: counted in miss[0], the first such e
// in miss[1], vals[e] = 0.
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_lookup(int64_t nq, const uint64_t* __restrict__ rows,
                                                        const uint64_t* __restrict__ cols,
                                                        const int32_t* __restrict__ pinv,
                                                        const int32_t* __restrict__ owner,
                                                        const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                                        const T* __restrict__ Z, T* __restrict__ vals,
                                                        unsigned long long* __restrict__ miss) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nq) return;
    bool hit;
    const T z = nd_selinv_at<T>(pinv[rows[e]], pinv[cols[e]], owner, nodes, st, Z, &hit);
    if (!hit) {
        atomicAdd(&miss[0], 1ull);
        atomicMin(&miss[1], (unsigned long long)e);
    }
    vals[e] = z;
}

// The same read-out over a CSR pattern (bsm_dev_nd_factor_inv_pattern):
// vals[e] = Z[i][col[e]] with i the row of entry e, found by bisection of rp
// (n + 1 entries). Every stored entry of the factored pattern lies in the
// fronts, so there is no miss to count.
template <typename T>
__global__ __launch_bounds__(256) void nd_selinv_lookup_csr(int64_t n, int64_t nnz, const int64_t* __restrict__ rp,
                                                            const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ pinv,
                                                            const int32_t* __restrict__ owner,
                                                            const NdDev* __restrict__ nodes,
                                                            const int32_t* __restrict__ st, const T* __restrict__ Z,
                                                            T* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n - 1;  // the smallest row with rp[row + 1] > e
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rp[mid + 1] > e) hi = mid;
        else lo = mid + 1;
    }
    bool hit;
    vals[e] = nd_selinv_at<T>(pinv[lo], pinv[col[e]], owner, nodes, st, Z, &hit);
}

// The selected inverse of a kept factor: Z and the panels for the call (not
// the handle's bytes, not the cache's budget), the levels top-down, then the
// read-outs into diag_dev (n values, or null), vals_dev (nq pairs) and
// pattern_dev (f.nnz values in the kept pattern's storage order, or null). The
// caller holds f.mu; f's storage is only read.
template <typename T>
int nd_factor_selinv_t(const bsm_nd_factor& f, void* diag_dev, uint64_t nq, const uint64_t* rows_dev,
                       const uint64_t* cols_dev, void* vals_dev, uint64_t* n_miss, uint64_t* first_miss,
                       hipStream_t s, void* pattern_dev = nullptr) {
    stage_reset(s);
    const int64_t N = (int64_t)f.n;
    const NdOpts opt = nd_options();
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    DBuf zb, yb, ms;
    const size_t z_b = (size_t)C.f_elems * sizeof(T), y_b = (size_t)std::max<int64_t>(C.vtot, 1) * 64 * sizeof(T);
    BSM_TRY(nd_alloc_numeric(zb, z_b, nullptr));
    BSM_TRY(nd_alloc_numeric(yb, y_b, nullptr));
    BSM_TRY(ms.alloc(2 * sizeof(unsigned long long), s));
    stage_mark("nd_selinv_alloc", s);
    NdDrainOnError drain{s, true};  // Z and the panels are freed, and the handle's mutex released, after it runs
    if (opt.poison) {  // BSM_ND_POISON=1 (tests): nothing the recursion did not write may be read
        BSM_HIP_TRY(hipMemsetAsync(zb.p, 0xff, z_b, s));
        BSM_HIP_TRY(hipMemsetAsync(yb.p, 0xff, y_b, s));
    }
    T* const Z = zb.as<T>();
    T* const Y = yb.as<T>();
    const T* const F = f.fr.as<T>();
    const T* const Dinv = f.dv.as<T>();
    for (int32_t lv = C.n_levels - 1; lv >= 0; --lv) {
        const int64_t l0 = C.lvl_off[(size_t)lv], nf = C.lvl_off[(size_t)lv + 1] - l0;
        if (nf == 0) continue;
        const int32_t ntmax = C.lvl_nt[(size_t)lv], nptmax = C.lvl_npt[(size_t)lv];
        const int64_t tmax = (int64_t)ntmax * (ntmax + 1) / 2;  // bounds every front's front-row tiles
        BSM_REQUIRE(nf * std::max<int64_t>(tmax, 1) < ((int64_t)1 << 31), BSM_ERR_UNSUPPORTED,
                    "nd selected inverse: a level of %lld fronts of up to %d tile rows exceeds the grid", (long long)nf,
                    ntmax);
        const int32_t* const lvl = p.lvl + l0;
        if (tmax > 0) {
            nd_selinv_pull<T><<<(unsigned)(nf * tmax), 256, 0, s>>>(p.nodes, lvl, (int)tmax, p.ri, Z);
            BSM_HIP_TRY(hipGetLastError());
        }
        for (int32_t K = nptmax - 1; K >= 0; --K) {
            if (ntmax > K + 1) {
                nd_selinv_yhat<T><<<(unsigned)(nf * ntmax), 256, 0, s>>>(p.nodes, lvl, ntmax, K, F, Dinv, Y);
                BSM_HIP_TRY(hipGetLastError());
                nd_selinv_below<T><<<(unsigned)(nf * ntmax), 256, 0, s>>>(p.nodes, lvl, ntmax, K, Y, Z);
                BSM_HIP_TRY(hipGetLastError());
            }
            nd_selinv_diag<T><<<(unsigned)nf, 256, 0, s>>>(p.nodes, lvl, K, Dinv, Y, Z);
            BSM_HIP_TRY(hipGetLastError());
        }
    }
    stage_mark("nd_selinv", s);
    if (diag_dev) {
        nd_selinv_diag_out<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, p.owner, p.nodes, p.perm, Z, static_cast<T*>(diag_dev));
        BSM_HIP_TRY(hipGetLastError());
    }
    if (pattern_dev && f.nnz > 0) {
        const char* const pb = f.pattern->as<char>();
        nd_selinv_lookup_csr<T><<<nd_blocks((int64_t)f.nnz, 256), 256, 0, s>>>(
            N, (int64_t)f.nnz, (const int64_t*)pb, (const int32_t*)(pb + nd_pattern_rp_bytes(N)), p.pinv, p.owner,
            p.nodes, p.st, Z, static_cast<T*>(pattern_dev));
        BSM_HIP_TRY(hipGetLastError());
    }
    unsigned long long h[2] = {0, ~0ull};
    if (nq > 0) {
        BSM_HIP_TRY(hipMemcpyAsync(ms.p, h, sizeof(h), hipMemcpyHostToDevice, s));
        nd_selinv_lookup<T><<<nd_blocks((int64_t)nq, 256), 256, 0, s>>>((int64_t)nq, rows_dev, cols_dev, p.pinv, p.owner,
                                                                       p.nodes, p.st, Z, static_cast<T*>(vals_dev),
                                                                       ms.as<unsigned long long>());
        BSM_HIP_TRY(hipGetLastError());
        BSM_HIP_TRY(read_dev(h, ms.p, sizeof(h), s));
    }
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    stage_mark("nd_selinv_out", s);
    *n_miss = h[0];
    *first_miss = h[1];
    return BSM_OK;
}

}  // namespace

int nd_factor_selinv(const bsm_nd_factor* f, void* diag_dev, uint64_t nq, const uint64_t* rows_dev,
                     const uint64_t* cols_dev, void* vals_dev, uint64_t* n_miss, uint64_t* first_miss,
                     hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    ND_REQUIRE_VALUES(f);
    *n_miss = 0;
    *first_miss = 0;
    if (f->n == 0) return BSM_OK;
    return f->dtype == BSM_F64
               ? nd_factor_selinv_t<double>(*f, diag_dev, nq, rows_dev, cols_dev, vals_dev, n_miss, first_miss, s)
               : nd_factor_selinv_t<float>(*f, diag_dev, nq, rows_dev, cols_dev, vals_dev, n_miss, first_miss, s);
}

int nd_factor_inv_pattern(const bsm_nd_factor* f, void* out_dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    ND_REQUIRE_VALUES(f);
    if (f->n == 0 || f->nnz == 0) return BSM_OK;
    uint64_t n_miss = 0, first = 0;
    return f->dtype == BSM_F64
               ? nd_factor_selinv_t<double>(*f, nullptr, 0, nullptr, nullptr, nullptr, &n_miss, &first, s, out_dev)
               : nd_factor_selinv_t<float>(*f, nullptr, 0, nullptr, nullptr, nullptr, &n_miss, &first, s, out_dev);
}

}  // namespace bsm

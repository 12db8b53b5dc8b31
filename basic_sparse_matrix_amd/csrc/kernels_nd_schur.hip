// kernels_nd_schur.hip -- a kept nd factor's Schur complement on the vertices its root owns (§4.9o, below)
#include <algorithm>

#include "nd_internal.hpp"

namespace bsm {
namespace {

// A factor made with a set G (bsm_nd_factor_create_schur) has G as its root
// front's own columns and one child under it, the tree of the other vertices I.
// Then the root front as assembled, before it is factored, is
//     S = A_GG - A_GI A_II^-1 A_IG = A_GG + U,
// U the child's update block, which the factorisation leaves in the child's
// trailing tiles (both pipelines: nd_extend2 only reads it), and what the
// root's forward step gathers is the condensed right-hand side
//     g = b_G - A_GI A_II^-1 b_I = b_G + u,
// u the child's update vector after the forward levels below the root. Nothing
// here reads the root's own L: S and g are formed from the child alone.
//
// The root's column p holds the vertex of rank p in the sorted set; the caller
// names the set in any order: spos[i] = the root column of the caller's
// i-th vertex, cidx its inverse (bsm_nd_factor::schur_map).

// the place of the root's column p among the child's front rows (rc: their places in the root, ascending), or -1
__device__ __forceinline__ int nd_schur_child_row(const int32_t* __restrict__ rc, int mc, int p) {
    if (mc <= 0) return -1;
    const int a = lower_bound_i32(rc, mc, p);
    return a < mc && rc[a] == p ? a : -1;
}

// S (m x m, the factor's dtype T) from a (values S2, converted as the factor's
// input is) and the child's update block. One workgroup per lower 64 x 64
// tile (PR, PC) of S in the ROOT's order; the tile is built in LDS and then
// written twice, as it stands and transposed, through cidx into the caller's
// order, so every element of `out` is written by one thread, once:
//   1. the tile cleared;
//   2. A's stored entries (j <= i, as nd_assemble reads them) between the
//      vertices of the tile's rows and columns, each at (max, min) of its two
//      root places: four lanes per vertex row, striding its entries (the
//      rows are short, and a walk row after row is a chain of dependent
//      loads). The rows of both ranges are walked (an entry is stored with
//      the vertex of the larger INDEX, which may have the smaller place);
//   3. + U[a(r)][a(c)] where the child has both rows: lane = r, so a wave
//      reads consecutive rows of a column of U (column-major, st ascending
//      with the root's columns: coalesced, with gaps where the child lacks a
//      row). A first, then U: one addition per element, in a fixed order.
// No atomics; the bits repeat, and do not depend on the caller's order.
template <typename T, typename S2>
__global__ __launch_bounds__(256) void nd_schur_gather(int m, const NdDev* __restrict__ nodes, int root,
                                                       const int64_t* __restrict__ perm,
                                                       const int32_t* __restrict__ pinv,
                                                       const int32_t* __restrict__ ri, const int64_t* __restrict__ rp,
                                                       const int32_t* __restrict__ col, const S2* __restrict__ val,
                                                       const T* __restrict__ F, const int32_t* __restrict__ cidx,
                                                       T* __restrict__ out, int64_t ldo) {
    const int PR = blockIdx.x, PC = blockIdx.y;
    if (PR < PC) return;
    __shared__ T tile[64][65];
    __shared__ int ac[64], cr[64], cc[64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const NdDev& rt = nodes[root];
    const int kid = rt.kid0;  // the root's one child (none: the set is every vertex)
    const int mc = kid >= 0 ? nodes[kid].m : 0;
    const int32_t* const rc = kid >= 0 ? ri + nodes[kid].st_off : nullptr;
    const int pr = 64 * PR + lane;
    const int ar = pr < m ? nd_schur_child_row(rc, mc, pr) : -1;
#pragma unroll
    for (int u = 0; u < 16; ++u) tile[lane][4 * u + w] = (T)0;
    if (tid < 64) {
        const int pc = 64 * PC + tid;
        ac[tid] = pc < m ? nd_schur_child_row(rc, mc, pc) : -1;
        cr[tid] = pr < m ? cidx[pr] : 0;
        cc[tid] = pc < m ? cidx[pc] : 0;
    }
    __syncthreads();
    for (int half = 0; half < (PR == PC ? 1 : 2); ++half) {
        const int p = 64 * (half ? PC : PR) + (tid >> 2);
        if (p >= m) continue;
        const int64_t i = perm[rt.start + p];
        for (int64_t e = rp[i] + (tid & 3); e < rp[i + 1]; e += 4) {
            const int64_t j = col[e];
            if (j > i) continue;
            const int64_t q = (int64_t)pinv[j] - rt.start;
            if (q < 0) continue;
            const int lr = (int)(p > q ? p : q) - 64 * PR, lc = (int)(p > q ? q : p) - 64 * PC;
            if (lr >= 0 && lr < 64 && lc >= 0 && lc < 64) tile[lr][lc] = (T)val[e];
        }
    }
    __syncthreads();
    if (mc > 0) {  // every load unconditional (indices clamped to the block), so they go out together
        const NdDev& c = nodes[kid];
        const T* const U = F + c.foff + (int64_t)c.np_pad * c.ld + c.np_pad;
        const int a = ar > 0 ? ar : 0;
        T v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int b = ac[4 * u + w];
            v[u] = U[(int64_t)(b > 0 ? b : 0) * c.ld + a];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int b = ac[4 * u + w];
            if (ar >= 0 && b >= 0 && ar >= b) tile[lane][4 * u + w] = tile[lane][4 * u + w] + v[u];
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int cl = 4 * u + w, pc = 64 * PC + cl;
        if (pr < m && pc < m && pr >= pc) out[(int64_t)cc[cl] * ldo + cr[lane]] = tile[lane][cl];
        // the mirror: lanes along the tile's columns, which are rows of the upper triangle
        const int qr = 64 * PR + cl, qc = 64 * PC + lane;
        if (qr < m && qc < m && qr > qc) out[(int64_t)cr[cl] * ldo + cc[lane]] = tile[cl][lane];
    }
}

// g = b over the root's columns plus the child's update-vector entries landing
// there: nd_forward's own gather (v = b, then v[ri[a]] += u[a]) for the root,
// one addition per row, written in the caller's order. g row-major m x k.
template <typename T>
__global__ __launch_bounds__(256) void nd_schur_rhs(int m, int k, const NdDev* __restrict__ nodes, int root,
                                                    const int32_t* __restrict__ ri, const int32_t* __restrict__ spos,
                                                    int64_t n, const T* __restrict__ bp, const T* __restrict__ V,
                                                    int64_t vtot, T* __restrict__ g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const NdDev& rt = nodes[root];
    const int kid = rt.kid0;
    const int p = spos[i];
    const int a = kid >= 0 ? nd_schur_child_row(ri + nodes[kid].st_off, nodes[kid].m, p) : -1;
    const T* const u = a >= 0 ? V + nodes[kid].voff + nodes[kid].np_pad + a : nullptr;
    for (int c = 0; c < k; ++c) {
        T v = bp[(int64_t)c * n + rt.start + p];
        if (u) v = v + u[(int64_t)c * vtot];
        g[(int64_t)i * k + c] = v;
    }
}

// x over the root's columns, where the root's backward step would have left it
// for its descendants (xp of nd_backward): xg row-major m x k in the caller's order
template <typename T>
__global__ __launch_bounds__(256) void nd_schur_put(int m, int k, const NdDev* __restrict__ nodes, int root,
                                                    const int32_t* __restrict__ spos, int64_t n,
                                                    const T* __restrict__ xg, T* __restrict__ bp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t q = nodes[root].start + spos[i];
    for (int c = 0; c < k; ++c) bp[(int64_t)c * n + q] = xg[(int64_t)i * k + c];
}

template <typename T, typename S2>
int nd_schur_gather_launch(const bsm_nd_factor& f, const bsm_csr* a, void* out_dev, uint64_t ld, hipStream_t s) {
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const int m = (int)f.schur_idx.size();
    const unsigned nt = nd_blocks(m, 64);
    nd_schur_gather<T, S2><<<dim3(nt, nt), 256, 0, s>>>(m, p.nodes, C.nn - 1, p.perm, p.pinv, p.ri, a->row_ptr, a->col,
                                                        static_cast<const S2*>(a->vals), f.fr.as<T>(),
                                                        f.schur_map.as<int32_t>() + m, static_cast<T*>(out_dev),
                                                        (int64_t)ld);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// condense (xg_dev == null: g into out_dev) or expand (x into out_dev). The
// forward levels below the root are nd_solve_passes' own, on the same
// temporaries; the root is the plan's last node, alone on the top level.
template <typename T>
int nd_schur_solve_t(const bsm_nd_factor& f, uint64_t k, const void* b_dev, const void* xg_dev, void* out_dev,
                     hipStream_t s) {
    stage_reset(s);
    const int64_t N = (int64_t)f.n;
    const NdOpts opt = nd_options();
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const int m = (int)f.schur_idx.size(), root = C.nn - 1;
    const int32_t top = C.n_levels - 1;  // the root's level
    NdGrid g;
    BSM_TRY(NdHost<T>::grid(false, true, g));
    DBuf bpb, vb, tfl;  // as nd_solve_tmp's
    const int64_t n_pf = (C.dinv_elems / 4096) * (int64_t)k;
    const size_t n_tf = 2 * (size_t)n_pf + 2 * (size_t)C.n_levels;
    BSM_TRY(bpb.alloc((size_t)N * k * sizeof(T), s));
    BSM_TRY(vb.alloc((size_t)std::max<int64_t>(C.vtot, 1) * k * sizeof(T), s));
    BSM_TRY(tfl.alloc((n_tf + 1) * sizeof(int), s));
    NdDrainOnError drain{s, true};  // the handle's mutex is released after this guard runs
    T* const bp = bpb.as<T>();
    T* const V = vb.as<T>();
    const T* const F = f.fr.as<T>();
    const T* const Dinv = f.dv.as<T>();
    int* const d_yf = tfl.as<int>();
    int* const d_xf = d_yf + n_pf;
    int* const d_ftk = d_xf + n_pf;
    int* const d_btk = d_ftk + C.n_levels;
    int* const d_status = tfl.as<int>() + n_tf;
    const int32_t* const spos = f.schur_map.as<int32_t>();
    BSM_TRY(NdHost<T>::permute_launch(true, C, N, k, static_cast<const T*>(b_dev), bp, s));
    BSM_HIP_TRY(hipMemsetAsync(tfl.p, 0, (n_tf + 1) * sizeof(int), s));
    BSM_TRY(NdHost<T>::forward_levels(C, opt, g, N, k, F, Dinv, bp, V, d_yf, d_ftk, d_status, s, top));
    stage_mark("nd_forward", s);
    if (!xg_dev) {
        nd_schur_rhs<T><<<nd_blocks(m, 256), 256, 0, s>>>(m, (int)k, p.nodes, root, p.ri, spos, N, bp, V, C.vtot,
                                                          static_cast<T*>(out_dev));
        BSM_HIP_TRY(hipGetLastError());
        return nd_status_end(false, d_status, drain, "nd_schur_rhs", s);
    }
    nd_schur_put<T><<<nd_blocks(m, 256), 256, 0, s>>>(m, (int)k, p.nodes, root, spos, N, static_cast<const T*>(xg_dev),
                                                      bp);
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(NdHost<T>::backward_levels(C, opt, g, N, k, F, Dinv, bp, V, d_xf, d_btk, d_status, s, top));
    stage_mark("nd_backward", s);
    BSM_TRY(NdHost<T>::permute_launch(false, C, N, k, bp, static_cast<T*>(out_dev), s));
    return nd_status_end(false, d_status, drain, "nd_copy_out", s);
}

// what the three calls refuse, under f->mu
int nd_schur_ready(const bsm_nd_factor* f, const char* what) {
    BSM_REQUIRE(!f->schur_idx.empty(), BSM_ERR_INVALID,
                "nd factor %s: the factor was made without a Schur set (bsm_nd_factor_create_schur)", what);
    ND_REQUIRE_VALUES(f);
    BSM_REQUIRE(!f->stale_blocks, BSM_ERR_UNSUPPORTED,
                "nd factor %s: an update or downdate has run since the last factorisation (the fronts' update blocks "
                "are stale); refactor first",
                what);
    return BSM_OK;
}

}  // namespace

int nd_factor_schur(const bsm_nd_factor* f, const bsm_csr* a, void* out_dev, uint64_t ld, hipStream_t s) {
    BSM_TRY(nd_refactor_matches(f, a));
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_TRY(nd_schur_ready(f, "schur"));
    stage_reset(s);
    BSM_TRY(nd_pattern_same(a, *f, s));
    stage_mark("nd_pattern_same", s);
    NdDrainOnError drain{s, true};
    const bool a64 = a->dtype == BSM_F64;
    int rc;
    if (f->dtype == BSM_F64)
        rc = a64 ? (nd_schur_gather_launch<double, double>)(*f, a, out_dev, ld, s)
                 : (nd_schur_gather_launch<double, float>)(*f, a, out_dev, ld, s);
    else
        rc = a64 ? (nd_schur_gather_launch<float, double>)(*f, a, out_dev, ld, s)
                 : (nd_schur_gather_launch<float, float>)(*f, a, out_dev, ld, s);
    BSM_TRY(rc);
    return nd_status_end(false, nullptr, drain, "nd_schur_gather", s);
}

int nd_factor_schur_condense(const bsm_nd_factor* f, uint64_t k, const void* b_dev, void* g_dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_TRY(nd_schur_ready(f, "schur_condense"));
    if (k == 0) return BSM_OK;
    return f->dtype == BSM_F64 ? nd_schur_solve_t<double>(*f, k, b_dev, nullptr, g_dev, s)
                               : nd_schur_solve_t<float>(*f, k, b_dev, nullptr, g_dev, s);
}

int nd_factor_schur_expand(const bsm_nd_factor* f, uint64_t k, const void* b_dev, const void* xg_dev, void* x_dev,
                           hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_TRY(nd_schur_ready(f, "schur_expand"));
    if (k == 0) return BSM_OK;
    return f->dtype == BSM_F64 ? nd_schur_solve_t<double>(*f, k, b_dev, xg_dev, x_dev, s)
                               : nd_schur_solve_t<float>(*f, k, b_dev, xg_dev, x_dev, s);
}

}  // namespace bsm

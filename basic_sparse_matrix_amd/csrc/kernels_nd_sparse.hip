// kernels_nd_sparse.hip -- a kept nd factor's solve with sparse right-hand sides and selected rows (§4.9k, below)
#include <algorithm>
#include <vector>

#include "nd_internal.hpp"

namespace bsm {
namespace {

// A x = b for a column-compressed b, x wanted at some rows: the forward pass on
// the fronts on the paths from b's entries to the root, the backward pass on
// those from the requested rows' fronts (reach_rule.hpp), per level over the
// active fronts alone (nd_forward_path / nd_backward_path: nd_forward's and
// nd_backward's own bodies). Every value returned goes through the operations
// of the dense solve in its order: the same bits, but for a -0 that a skipped
// +0 addition leaves. No flags, no tickets: every dependency is a launch
// boundary or a __syncthreads. Columns go in chunks of ND_SPARSE_CHUNK, so bp
// and V are the dense solve's of that many columns. With rows requested V is
// never cleared (the fronts that are not active are neither read nor
// written); with every row wanted the dense solve's own backward levels run
// on all fronts, over a V cleared first (y = 0 off the forward set).

constexpr uint64_t ND_SPARSE_CHUNK = 32;

// own[i] = the front owning row rows[i] (A's order, < n)
__global__ __launch_bounds__(256) void nd_sparse_owners(int64_t cnt, const uint64_t* __restrict__ rows,
                                                        const int32_t* __restrict__ pinv,
                                                        const int32_t* __restrict__ owner, int32_t* __restrict__ own) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) own[i] = owner[pinv[rows[i]]];
}

// Place, first half: what nd_forward_path reads of bp, the pivots of the
// forward-active fronts, cleared. One workgroup per (active front, column).
template <typename T>
__global__ __launch_bounds__(256) void nd_sparse_clear(const NdDev* __restrict__ nodes,
                                                       const ReachFront* __restrict__ act, int64_t n,
                                                       T* __restrict__ bp) {
    const NdDev& nd = nodes[act[blockIdx.x].node];
    T* const d = bp + (int64_t)blockIdx.y * n + nd.start;
    for (int r = threadIdx.x; r < nd.np; r += 256) d[r] = (T)0;
}

// Place, second half (after a launch boundary): column c0 + blockIdx.x of b
// into column blockIdx.x of bp, in the new order. Rows are strictly ascending
// within a column: no two entries meet.
template <typename T>
__global__ __launch_bounds__(64) void nd_sparse_place(const int64_t* __restrict__ colptr,
                                                      const uint64_t* __restrict__ rows, const T* __restrict__ vals,
                                                      const int32_t* __restrict__ pinv, int64_t n, int64_t c0,
                                                      T* __restrict__ bp) {
    const int64_t col = c0 + blockIdx.x;
    T* const d = bp + (int64_t)blockIdx.x * n;
    for (int64_t e = colptr[col] + threadIdx.x; e < colptr[col + 1]; e += 64) d[pinv[rows[e]]] = vals[e];
}

// x[e][c0 + c] = x_c at row xrows[e] (xrows == null: row e) for the chunk's kc
// columns; x row-major with ldx columns
template <typename T>
__global__ __launch_bounds__(256) void nd_sparse_gather(int64_t nout, const uint64_t* __restrict__ xrows,
                                                        const int32_t* __restrict__ pinv, int64_t n, int kc,
                                                        const T* __restrict__ bp, T* __restrict__ x, int64_t ldx,
                                                        int64_t c0) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nout) return;
    const int64_t q = pinv[xrows ? (int64_t)xrows[e] : e];
    for (int c = 0; c < kc; ++c) x[e * ldx + c0 + c] = bp[(int64_t)c * n + q];
}

// The caller holds f.mu and has found f valid and every index < n. b on the
// host (col_ptr k + 1, rows and vals col_ptr[k]); xrows: nq rows on the host,
// or null for every row. x_dev: ROW-major nq x k (n x k).
template <typename T>
int nd_factor_solve_sparse_t(const bsm_nd_factor& f, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                             const void* vals, uint64_t nq, const uint64_t* xrows, void* x_dev, uint32_t* info,
                             hipStream_t s) {
    stage_reset(s);
    const int64_t N = (int64_t)f.n;
    const NdOpts opt = nd_options();
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const bool all = xrows == nullptr;
    const uint64_t nnz = col_ptr[k], nout = all ? (uint64_t)N : nq, nidx = nnz + nq;
    const uint64_t kc_max = std::min<uint64_t>(k, ND_SPARSE_CHUNK), chunks = (k + ND_SPARSE_CHUNK - 1) / ND_SPARSE_CHUNK;
    // everything that can fail before the first launch
    NdGrid g;
    if (all) BSM_TRY(NdHost<T>::grid(false, true, g));
    DBuf cpb, idxb, valb, ownb, bpb, vb, tfl;
    BSM_TRY(cpb.alloc((size_t)(k + 1) * 8, s));
    BSM_TRY(idxb.alloc((size_t)nidx * 8, s));
    BSM_TRY(valb.alloc((size_t)nnz * sizeof(T), s));
    BSM_TRY(ownb.alloc((size_t)nidx * sizeof(int32_t), s));
    const size_t bp_b = (size_t)N * kc_max * sizeof(T), v_b = (size_t)std::max<int64_t>(C.vtot, 1) * kc_max * sizeof(T);
    BSM_TRY(bpb.alloc(bp_b, s));
    BSM_TRY(vb.alloc(v_b, s));
    // every front's backward pass (the dense solve's levels): its flags, tickets and status word
    const int64_t n_pf = (C.dinv_elems / 4096) * (int64_t)kc_max;
    const size_t n_tf = (size_t)n_pf + (size_t)C.n_levels;
    if (all) BSM_TRY(tfl.alloc((n_tf + 1) * sizeof(int), s));
    NdDrainOnError drain{s, true};  // the handle's mutex is released after this guard runs
    uint64_t* const d_idx = idxb.as<uint64_t>();
    BSM_TRY(h2d_staged(cpb.p, col_ptr, (size_t)(k + 1) * 8, s));
    if (nnz) {
        BSM_TRY(h2d_staged(d_idx, rows, (size_t)nnz * 8, s));
        BSM_TRY(h2d_staged(valb.p, vals, (size_t)nnz * sizeof(T), s));
    }
    if (nq) BSM_TRY(h2d_staged(d_idx + nnz, xrows, (size_t)nq * 8, s));
    // the owners of b's rows and of the requested rows, copied back once
    std::vector<int32_t> own((size_t)nidx);
    if (nidx) {
        nd_sparse_owners<<<nd_blocks((int64_t)nidx, 256), 256, 0, s>>>((int64_t)nidx, d_idx, p.pinv, p.owner,
                                                                         ownb.as<int32_t>());
        BSM_HIP_TRY(hipGetLastError());
        BSM_HIP_TRY(read_dev(own.data(), ownb.p, (size_t)nidx * sizeof(int32_t), s));
    }
    stage_mark("nd_sparse_owners", s);
    const size_t nn = (size_t)C.nn;
    std::vector<unsigned char> fmark, bmark;
    ReachSet fw, bw;
    reach_set(nn, C.h_parent.data(), C.h_level.data(), C.h_kid0.data(), C.h_kid1.data(), own.data(), (size_t)nnz, fmark,
              fw);
    if (!all) {
        reach_set(nn, C.h_parent.data(), C.h_level.data(), nullptr, nullptr, own.data() + nnz, (size_t)nq, bmark, bw);
        for (ReachFront& b : bw.fronts) b.kids = fmark[(size_t)b.node];  // y from the forward pass, else 0
    }
    const size_t nf = fw.fronts.size(), nb = bw.fronts.size();
    DBuf actb;
    BSM_TRY(actb.alloc((nf + nb) * sizeof(ReachFront), s));
    const ReachFront* const d_fw = actb.as<ReachFront>();
    const ReachFront* const d_bw = d_fw + nf;
    if (nf) BSM_TRY(h2d_staged(actb.p, fw.fronts.data(), nf * sizeof(ReachFront), s));
    if (nb) BSM_TRY(h2d_staged(actb.as<ReachFront>() + nf, bw.fronts.data(), nb * sizeof(ReachFront), s));
    T* const bp = bpb.as<T>();
    T* const V = vb.as<T>();
    const T* const F = f.fr.as<T>();
    const T* const Dinv = f.dv.as<T>();
    int* const d_status = all ? tfl.as<int>() + n_tf : nullptr;
    for (uint64_t c0 = 0; c0 < k; c0 += ND_SPARSE_CHUNK) {
        const unsigned kc = (unsigned)std::min<uint64_t>(ND_SPARSE_CHUNK, k - c0);
        // BSM_ND_POISON=1 (tests): nothing the passes did not write may be read
        if (opt.poison) {
            BSM_HIP_TRY(hipMemsetAsync(bpb.p, 0xff, bp_b, s));
            BSM_HIP_TRY(hipMemsetAsync(vb.p, 0xff, v_b, s));
        }
        if (all) {  // the dense backward levels read y of every front: 0 where the forward pass does not run
            BSM_HIP_TRY(hipMemsetAsync(vb.p, 0, (size_t)std::max<int64_t>(C.vtot, 1) * kc * sizeof(T), s));
            BSM_HIP_TRY(hipMemsetAsync(tfl.p, 0, (n_tf + 1) * sizeof(int), s));
        }
        if (nf) {
            nd_sparse_clear<T><<<dim3((unsigned)nf, kc), 256, 0, s>>>(p.nodes, d_fw, N, bp);
            BSM_HIP_TRY(hipGetLastError());
            nd_sparse_place<T><<<kc, 64, 0, s>>>(cpb.as<int64_t>(), d_idx, valb.as<T>(), p.pinv, N, (int64_t)c0, bp);
            BSM_HIP_TRY(hipGetLastError());
        }
        for (size_t li = 0; li < fw.levels.size(); ++li) {
            const int32_t a0 = fw.first(li), cnt = fw.last(li) - a0;
            BSM_TRY(NdHost<T>::path_launch(true, C, d_fw + a0, (unsigned)cnt, kc, N, bp, V, F, Dinv, s));
        }
        stage_mark("nd_sparse_forward", s);
        if (all) {
            BSM_TRY(NdHost<T>::backward_levels(C, opt, g, N, kc, F, Dinv, bp, V, tfl.as<int>(), tfl.as<int>() + n_pf,
                                               d_status, s, C.n_levels));
        } else {
            for (size_t li = bw.levels.size(); li-- > 0;) {
                const int32_t a0 = bw.first(li), cnt = bw.last(li) - a0;
                BSM_TRY(NdHost<T>::path_launch(false, C, d_bw + a0, (unsigned)cnt, kc, N, bp, V, F, Dinv, s));
            }
        }
        stage_mark("nd_sparse_backward", s);
        if (nout) {
            nd_sparse_gather<T><<<nd_blocks((int64_t)nout, 256), 256, 0, s>>>(
                (int64_t)nout, all ? nullptr : d_idx + nnz, p.pinv, N, (int)kc, bp, static_cast<T*>(x_dev), (int64_t)k,
                (int64_t)c0);
            BSM_HIP_TRY(hipGetLastError());
        }
    }
    BSM_TRY(nd_status_end(false, d_status, drain, "nd_sparse_gather", s));  // d_status: null unless `all`
    if (info) {
        info[0] = (uint32_t)nf;
        info[1] = (uint32_t)(all ? nn : nb);
        info[2] = (uint32_t)nn;
        info[3] = (uint32_t)chunks;
    }
    return BSM_OK;
}

}  // namespace

int nd_factor_solve_sparse(const bsm_nd_factor* f, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                           const void* vals, uint64_t nq, const uint64_t* xrows, void* x_dev, uint32_t* info,
                           hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    ND_REQUIRE_VALUES(f);
    return f->dtype == BSM_F64
               ? nd_factor_solve_sparse_t<double>(*f, k, col_ptr, rows, vals, nq, xrows, x_dev, info, s)
               : nd_factor_solve_sparse_t<float>(*f, k, col_ptr, rows, vals, nq, xrows, x_dev, info, s);
}

}  // namespace bsm

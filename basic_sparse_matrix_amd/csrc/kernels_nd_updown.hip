// kernels_nd_updown.hip -- the rank-k update and downdate of a kept nd factor (below)
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "nd_internal.hpp"
#include "updown_rule.hpp"

namespace bsm {
namespace {

#include "solve_tiles.hpp"

// L L^T +- W W^T in place, by the column-by-column method of updown_rule.hpp.
// A column of W lies inside one front (its first vertex's: the other entries
// are own columns or front rows of it), so its remainder rides up the tree
// through ri, as a solve's update vector does, and only the fronts on the
// columns' paths to the root (the ACTIVE fronts) are touched. Per level,
// bottom-up, over the active fronts alone:
//     nd_updown_pivots  one workgroup per front: the children's rows gathered,
//                       then per pivot tile the 64 x 64 diagonal tile on one
//                       wave (lane = row) and the pivot rows below on all
//                       threads; the coefficients (c, s) of every (pivot,
//                       column) stored
//     nd_updown_rows    the front rows: a thread per row applies every
//                       pivot's coefficients (the rows are independent)
// and once at the end nd_updown_dinv, the inverse diagonal tiles again. No
// flags, no tickets: every dependency is a launch boundary or a
// __syncthreads. WRITE = false is the dry pass of a downdate: the same
// arithmetic with the new L kept in registers, so a W W^T that takes the
// matrix out of the positive definite ones is found before a bit of the
// factor has changed. Never read: what nd_export never reads (the padding
// pivots, a pivot tile above its diagonal, the update blocks).

constexpr int ND_UPDOWN_MAX_K = 16;
constexpr unsigned long long ND_UPDOWN_OK = ~0ull;  // the status word: else the first failing (node, pivot, column)

// An active front, in level order. Its work columns: ld per column of W, in
// the front's own row order; its coefficients: [pivot * k + column].
struct NdUpFront {
    int64_t wf_off, cf_off;
    int32_t node;
    int32_t a0, a1;  // the active fronts among its children (-1: none)
    int32_t pad;
};

// lane j's v in every lane (j wave-uniform): v_readlane, no LDS round trip
template <typename T>
__device__ __forceinline__ T nd_lane_bcast(T v, int j) {
    if constexpr (sizeof(T) == 8) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, j);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), j);
        return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
    } else {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
    }
}

// One wave per column of W (column-compressed, rows in A's order). The
// column's start front owns its smallest new index; every entry must be an own
// column or a front row of it (nd_selinv_lookup's search). slot == null: the
// check alone -- start[col] = that front (-1: an empty column), a column with
// an entry outside counted in miss[0], the first such column in miss[1].
// Else: the entries into the start front's work column, rounded once to T.
template <typename T, typename S>
__global__ __launch_bounds__(64) void nd_updown_place(const int64_t* __restrict__ colptr,
                                                      const uint64_t* __restrict__ rows, const S* __restrict__ vals,
                                                      const int32_t* __restrict__ pinv,
                                                      const int32_t* __restrict__ owner,
                                                      const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                                      const NdUpFront* __restrict__ act,
                                                      const int32_t* __restrict__ slot, T* __restrict__ Wf,
                                                      int32_t* __restrict__ start,
                                                      unsigned long long* __restrict__ miss) {
    const int col = blockIdx.x, lane = threadIdx.x;
    const int64_t e0 = colptr[col], e1 = colptr[col + 1];
    if (e0 == e1) {  // wave-uniform
        if (!slot && lane == 0) start[col] = -1;
        return;
    }
    long long lo = 0x7fffffffffffffffll;
    for (int64_t e = e0 + lane; e < e1; e += 64) lo = min(lo, (long long)pinv[rows[e]]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
    const int32_t own = owner[lo];
    const NdDev& nd = nodes[own];
    T* const w = slot ? Wf + act[slot[col]].wf_off + (int64_t)col * nd.ld : nullptr;
    bool outside = false;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int64_t q = pinv[rows[e]];
        int64_t r = q - nd.start;
        bool hit = true;
        if (q >= nd.start + nd.np) {
            const int32_t* const fs = st + nd.st_off;
            const int32_t a = lower_bound_i32(fs, nd.m, q);
            hit = a < nd.m && fs[a] == q;
            r = nd.np_pad + a;
        }
        outside = outside || !hit;
        if (w && hit) w[r] = (T)vals[e];
    }
    if (slot) return;
    const bool any = __ballot(outside) != 0ull;
    if (lane == 0) {
        start[col] = own;
        if (any) {
            atomicAdd(&miss[0], 1ull);
            atomicMin(&miss[1], (unsigned long long)col);
        }
    }
}

// the rows of the work columns that are read: the real pivots and the front rows
template <typename T>
__global__ __launch_bounds__(256) void nd_updown_zero(const NdDev* __restrict__ nodes,
                                                      const NdUpFront* __restrict__ act, int k, T* __restrict__ Wf) {
    const NdUpFront& me = act[blockIdx.x];
    const NdDev& nd = nodes[me.node];
    T* const w = Wf + me.wf_off;
    const int f = nd.np_pad + nd.m;
    for (int col = 0; col < k; ++col)
        for (int r = threadIdx.x; r < f; r += 256)
            if (r < nd.np || r >= nd.np_pad) w[(int64_t)col * nd.ld + r] = (T)0;
}

// One row against the jn pivots of a tile: lrow = &L[row][the tile's first
// pivot], wr = the row's k entries of the work columns, cs = the tile's
// coefficients [pivot * k + column] (LDS: every thread reads the same one).
// Eight pivots' loads go out together; a skipped (pivot, column) is a
// workgroup-uniform branch.
template <typename T, bool WRITE>
__device__ __forceinline__ void nd_updown_apply(T* lrow, int64_t ld, int jn, T (&wr)[ND_UPDOWN_MAX_K], int k, int sign,
                                                const UpdownCoef<T>* cs) {
    for (int j0 = 0; j0 < jn; j0 += 8) {
        T lv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) lv[t] = j0 + t < jn ? lrow[(int64_t)(j0 + t) * ld] : (T)0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (j0 + t < jn) {
#pragma unroll
                for (int col = 0; col < ND_UPDOWN_MAX_K; ++col)
                    if (col < k) updown_row(lv[t], wr[col], sign, cs[(j0 + t) * k + col]);
                if constexpr (WRITE) lrow[(int64_t)(j0 + t) * ld] = lv[t];
            }
        }
    }
}

template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void nd_updown_pivots(const NdDev* __restrict__ nodes,
                                                        const NdUpFront* __restrict__ act, int first,
                                                        const int32_t* __restrict__ ri, int k, int sign, T* F, T* Wf,
                                                        UpdownCoef<T>* __restrict__ Cf, unsigned long long* status) {
    __shared__ UpdownCoef<T> cs[64 * ND_UPDOWN_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const NdUpFront& me = act[first + blockIdx.x];  // act whole: a0 / a1 are places in all of it
    const NdDev& nd = nodes[me.node];
    const int64_t ld = nd.ld;
    T* const w = Wf + me.wf_off;
    // a child's front rows into this front's rows. A column has one path, so
    // all but one of a row's sources (placed here, child 0, child 1) are
    // exact zeros: the sum is that one value, in any order
    for (int s = 0; s < 2; ++s) {
        const int a = s == 0 ? me.a0 : me.a1;
        if (a < 0) continue;
        const NdUpFront& ch = act[a];
        const NdDev& c = nodes[ch.node];
        const T* const u = Wf + ch.wf_off + c.np_pad;
        const int32_t* const rc = ri + c.st_off;
        for (int b = tid; b < c.m; b += 256) {
            const int r = rc[b];
            for (int col = 0; col < k; ++col) w[(int64_t)col * ld + r] += u[(int64_t)col * c.ld + b];
        }
        __syncthreads();
    }
    T* const Fn = F + nd.foff;
    UpdownCoef<T>* const cf = Cf + me.cf_off;
    for (int K = 0; K < nd.npt; ++K) {
        const int jn = min(64, nd.np - 64 * K);  // the tile's real pivots
        if (wv == 0) {
            const int r = 64 * K + lane;
            const bool live = lane < jn;
            T wr[ND_UPDOWN_MAX_K];
#pragma unroll
            for (int col = 0; col < ND_UPDOWN_MAX_K; ++col)
                wr[col] = col < k && live ? w[(int64_t)col * ld + r] : (T)0;
            for (int j = 0; j < jn; ++j) {
                T* const colp = Fn + (int64_t)(64 * K + j) * ld;
                T l = live && lane >= j ? colp[r] : (T)0;
#pragma unroll
                for (int col = 0; col < ND_UPDOWN_MAX_K; ++col) {
                    if (col >= k) continue;  // wave-uniform
                    T d = nd_lane_bcast(l, j);  // L_jj as the columns before this one left it
                    const T wj = nd_lane_bcast(wr[col], j);
                    UpdownCoef<T> c1;
                    const bool ok = updown_pivot(d, wj, sign, c1);  // the same in every lane
                    if (lane == j) l = d;
                    else if (lane > j) updown_row(l, wr[col], sign, c1);
                    if (lane == 0) {
                        cs[j * k + col] = c1;
                        cf[(int64_t)(64 * K + j) * k + col] = c1;
                        if (!ok)
                            atomicMin(status, ((unsigned long long)(unsigned)me.node << 32) |
                                                  ((unsigned long long)(unsigned)(64 * K + j) << 8) | (unsigned)col);
                    }
                }
                if constexpr (WRITE)
                    if (live && lane >= j) colp[r] = l;
            }
        }
        __syncthreads();
        // the pivot rows below the tile (which is then a full one)
        for (int r = 64 * (K + 1) + tid; r < nd.np; r += 256) {
            T wr[ND_UPDOWN_MAX_K];
#pragma unroll
            for (int col = 0; col < ND_UPDOWN_MAX_K; ++col) wr[col] = col < k ? w[(int64_t)col * ld + r] : (T)0;
            nd_updown_apply<T, WRITE>(Fn + (int64_t)64 * K * ld + r, ld, 64, wr, k, sign, cs);
#pragma unroll
            for (int col = 0; col < ND_UPDOWN_MAX_K; ++col)
                if (col < k) w[(int64_t)col * ld + r] = wr[col];
        }
        __syncthreads();  // the rows' w for the next tile's other threads; cs is free again
    }
}

// grid (the level's active fronts, from act[first] on; 256-row chunks of the largest front)
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void nd_updown_rows(const NdDev* __restrict__ nodes,
                                                      const NdUpFront* __restrict__ act, int first, int k, int sign,
                                                      T* F, T* Wf, const UpdownCoef<T>* __restrict__ Cf) {
    __shared__ UpdownCoef<T> cs[64 * ND_UPDOWN_MAX_K];
    const int tid = threadIdx.x;
    const NdUpFront& me = act[first + blockIdx.x];
    const NdDev& nd = nodes[me.node];
    if ((int)blockIdx.y * 256 >= nd.m || nd.np == 0) return;  // uniform; without pivots the rows pass through as they are
    const int b = (int)blockIdx.y * 256 + tid;
    const bool live = b < nd.m;
    const int64_t ld = nd.ld;
    const int r = nd.np_pad + (live ? b : 0);
    T* const w = Wf + me.wf_off + r;
    T wr[ND_UPDOWN_MAX_K];
#pragma unroll
    for (int col = 0; col < ND_UPDOWN_MAX_K; ++col) wr[col] = col < k && live ? w[(int64_t)col * ld] : (T)0;
    const UpdownCoef<T>* const cf = Cf + me.cf_off;
    for (int K = 0; K < nd.npt; ++K) {
        const int jn = min(64, nd.np - 64 * K);
        __syncthreads();
        for (int i = tid; i < jn * k; i += 256) cs[i] = cf[(int64_t)64 * K * k + i];
        __syncthreads();
        if (live) nd_updown_apply<T, WRITE>(F + nd.foff + (int64_t)64 * K * ld + r, ld, jn, wr, k, sign, cs);
    }
    if (live) {
#pragma unroll
        for (int col = 0; col < ND_UPDOWN_MAX_K; ++col)
            if (col < k) w[(int64_t)col * ld] = wr[col];
    }
}

// Dinv of the new diagonal tiles: grid (active fronts, the largest npt), one
// wave per tile, lane q the column q of Linv by forward substitution in a
// fixed order (L from LDS, the same entry in every lane; x in registers).
// Padding pivots are identity pivots. Dinv[q * 64 + l] = Linv[l][q].
template <typename T>
__global__ __launch_bounds__(64) void nd_updown_dinv(const NdDev* __restrict__ nodes,
                                                     const NdUpFront* __restrict__ act, const T* __restrict__ F,
                                                     T* __restrict__ Dinv) {
    __shared__ T Ls[64 * 64];  // Ls[t * 64 + l] = L[l][t]
    const NdDev& nd = nodes[act[blockIdx.x].node];
    const int K = blockIdx.y, q = threadIdx.x;
    if (K >= nd.npt) return;
    const int jn = min(64, nd.np - 64 * K);
    const T* const tile = F + nd.foff + (int64_t)64 * K * nd.ld + 64 * K;
    for (int t = 0; t < 64; ++t)
        Ls[t * 64 + q] = (q < jn && t < jn && q >= t) ? tile[(int64_t)t * nd.ld + q] : (q == t ? (T)1 : (T)0);
    __syncthreads();
    T x[64];
#pragma unroll
    for (int l = 0; l < 64; ++l) {
        T acc = l == q ? (T)1 : (T)0;
#pragma unroll
        for (int t = 0; t < l; ++t) acc = fma_t(-Ls[t * 64 + l], x[t], acc);
        x[l] = acc / Ls[l * 64 + l];
    }
    T* const out = Dinv + nd.dinv_off + (int64_t)K * 4096 + (int64_t)q * 64;
#pragma unroll
    for (int l = 0; l < 64; ++l) out[l] = x[l];
}

// The columns' paths to the root: the active fronts in (level, node) order,
// each with its active children, and the work and coefficient arrays' sizes.
struct NdUpPlan {
    std::vector<NdUpFront> act;
    std::vector<int32_t> col_slot;            // per column: its start front's place in act (-1: an empty column)
    std::vector<std::pair<int32_t, int32_t>> levels;  // per level with active fronts: the level and its first place in act
    std::vector<char> has_rows;               // per such level: some front has a parent (front rows to update)
    int64_t wf_elems = 0, cf_elems = 0;
    int32_t npt_max = 0;
};
void nd_updown_plan(const NdCached& C, const std::vector<int32_t>& start, int k, NdUpPlan& U) {
    std::vector<int32_t> nodes;
    for (int32_t n0 : start)
        for (int32_t n = n0; n >= 0; n = C.h_parent[(size_t)n]) nodes.push_back(n);
    std::sort(nodes.begin(), nodes.end(), [&](int32_t a, int32_t b) {
        const int32_t la = C.h_level[(size_t)a], lb = C.h_level[(size_t)b];
        return la != lb ? la < lb : a < b;
    });
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    auto slot_of = [&](int32_t n) {
        for (size_t i = 0; i < nodes.size(); ++i)
            if (nodes[i] == n) return (int32_t)i;
        return (int32_t)-1;
    };
    U.act.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        const int32_t lv = C.h_level[(size_t)nodes[i]];
        NdUpFront& a = U.act[i];
        a.node = nodes[i];
        a.a0 = a.a1 = -1;
        a.pad = 0;
        // the level's largest front bounds this one's ld and np_pad
        a.wf_off = U.wf_elems;
        U.wf_elems += (int64_t)64 * C.lvl_nt[(size_t)lv] * k;
        a.cf_off = U.cf_elems;
        U.cf_elems += (int64_t)64 * C.lvl_npt[(size_t)lv] * k;
        U.npt_max = std::max(U.npt_max, C.lvl_npt[(size_t)lv]);
        if (U.levels.empty() || U.levels.back().first != lv) {
            U.levels.emplace_back(lv, (int32_t)i);
            U.has_rows.push_back(0);
        }
        if (C.h_parent[(size_t)nodes[i]] >= 0) U.has_rows.back() = 1;
    }
    for (size_t i = 0; i < nodes.size(); ++i) {  // children before parents: a0 is the lower (level, node)
        const int32_t p = C.h_parent[(size_t)nodes[i]];
        if (p < 0) continue;
        NdUpFront& a = U.act[(size_t)slot_of(p)];
        (a.a0 < 0 ? a.a0 : a.a1) = (int32_t)i;
    }
    U.col_slot.resize(start.size());
    for (size_t c = 0; c < start.size(); ++c) U.col_slot[c] = start[c] < 0 ? -1 : slot_of(start[c]);
}

// The caller holds f.mu and has found f valid. W on the device: colptr (k + 1),
// rows (A's order), vals (S = the factored matrix's dtype), no stored zeros.
// n_miss > 0: nothing was written (a column outside the pattern).
template <typename T, typename S>
int nd_factor_updown_t(bsm_nd_factor& f, int sign, int k, const int64_t* colptr_dev, const uint64_t* rows_dev,
                       const void* vals_dev, uint64_t* n_miss, uint64_t* first_miss, hipStream_t s) {
    stage_reset(s);
    const NdOpts opt = nd_options();
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const S* const vals = static_cast<const S*>(vals_dev);
    DBuf hd;  // start fronts (k int32, padded), then the miss pair, then the status word
    const size_t o_miss = ((size_t)k * sizeof(int32_t) + 7) / 8 * 8, o_status = o_miss + 16;
    BSM_TRY(hd.alloc(o_status + 8, s));
    NdDrainOnError drain{s, true};
    int32_t* const d_start = hd.as<int32_t>();
    unsigned long long* const d_miss = (unsigned long long*)(hd.as<char>() + o_miss);
    unsigned long long* const d_status = (unsigned long long*)(hd.as<char>() + o_status);
    const unsigned long long init[3] = {0ull, ~0ull, ND_UPDOWN_OK};
    BSM_HIP_TRY(hipMemcpyAsync(d_miss, init, sizeof(init), hipMemcpyHostToDevice, s));
    nd_updown_place<T, S><<<(unsigned)k, 64, 0, s>>>(colptr_dev, rows_dev, vals, p.pinv, p.owner, p.nodes, p.st, nullptr,
                                                    nullptr, (T*)nullptr, d_start, d_miss);
    BSM_HIP_TRY(hipGetLastError());
    std::vector<char> hb(o_status);
    BSM_HIP_TRY(read_dev(hb.data(), hd.p, o_status, s));
    unsigned long long miss[2];
    memcpy(miss, hb.data() + o_miss, sizeof(miss));
    if (miss[0]) {
        drain.armed = false;
        *n_miss = miss[0];
        *first_miss = miss[1];
        return BSM_OK;
    }
    std::vector<int32_t> start((size_t)k);
    memcpy(start.data(), hb.data(), (size_t)k * sizeof(int32_t));
    NdUpPlan U;
    nd_updown_plan(C, start, k, U);
    const size_t na = U.act.size();
    if (na == 0) {  // every column empty
        drain.armed = false;
        return BSM_OK;
    }
    DBuf ab, wb, cb;  // the active fronts and the columns' places; the work columns; the coefficients
    const size_t act_b = na * sizeof(NdUpFront), wf_b = (size_t)U.wf_elems * sizeof(T),
                 cf_b = (size_t)std::max<int64_t>(U.cf_elems, 1) * sizeof(UpdownCoef<T>);
    BSM_TRY(ab.alloc(act_b + (size_t)k * sizeof(int32_t), s));
    BSM_TRY(wb.alloc(wf_b, s));
    BSM_TRY(cb.alloc(cf_b, s));
    const NdUpFront* const d_act = ab.as<NdUpFront>();
    const int32_t* const d_slot = (const int32_t*)(ab.as<char>() + act_b);
    T* const Wf = wb.as<T>();
    UpdownCoef<T>* const Cf = cb.as<UpdownCoef<T>>();
    BSM_TRY(h2d_staged(ab.p, U.act.data(), act_b, s));
    BSM_TRY(h2d_staged(ab.as<char>() + act_b, U.col_slot.data(), (size_t)k * sizeof(int32_t), s));
    T* const F = f.fr.as<T>();
    auto sweep = [&](auto write) -> int {
        constexpr bool WRITE = decltype(write)::value;
        // BSM_ND_POISON=1 (tests): nothing the sweep did not write may be read
        if (opt.poison) {
            BSM_HIP_TRY(hipMemsetAsync(wb.p, 0xff, wf_b, s));
            BSM_HIP_TRY(hipMemsetAsync(cb.p, 0xff, cf_b, s));
        }
        nd_updown_zero<T><<<(unsigned)na, 256, 0, s>>>(p.nodes, d_act, k, Wf);
        BSM_HIP_TRY(hipGetLastError());
        nd_updown_place<T, S><<<(unsigned)k, 64, 0, s>>>(colptr_dev, rows_dev, vals, p.pinv, p.owner, p.nodes, p.st, d_act,
                                                        d_slot, Wf, nullptr, nullptr);
        BSM_HIP_TRY(hipGetLastError());
        stage_mark("nd_updown_place", s);
        for (size_t li = 0; li < U.levels.size(); ++li) {
            const int32_t lv = U.levels[li].first, a0 = U.levels[li].second;
            const unsigned nf = (unsigned)((li + 1 < U.levels.size() ? (size_t)U.levels[li + 1].second : na) - (size_t)a0);
            nd_updown_pivots<T, WRITE><<<nf, 256, 0, s>>>(p.nodes, d_act, a0, p.ri, k, sign, F, Wf, Cf, d_status);
            BSM_HIP_TRY(hipGetLastError());
            if (!U.has_rows[li]) continue;
            const unsigned chunks = (unsigned)((64 * C.lvl_nt[(size_t)lv] + 255) / 256);
            nd_updown_rows<T, WRITE><<<dim3(nf, chunks), 256, 0, s>>>(p.nodes, d_act, a0, k, sign, F, Wf, Cf);
            BSM_HIP_TRY(hipGetLastError());
        }
        return BSM_OK;
    };
    auto status = [&](unsigned long long* h) -> int {
        BSM_HIP_TRY(read_dev(h, d_status, sizeof(*h), s));
        return BSM_OK;
    };
    const char* const not_pd =
        "cholesky: matrix is not positive definite (a pivot is <= 0 or not finite): nd factor %s, at pivot %llu of "
        "front %llu, column %llu of W";
    unsigned long long h = ND_UPDOWN_OK;
    if (sign < 0) {  // the dry pass: the factor's bits stay as they are
        BSM_TRY(sweep(std::false_type{}));
        BSM_TRY(status(&h));
        stage_mark("nd_updown_sweep", s);
        if (h != ND_UPDOWN_OK) {
            drain.armed = false;
            BSM_REQUIRE(false, BSM_ERR_UNSUPPORTED, not_pd, "downdate", (h >> 8) & 0xffffffull, h >> 32, h & 0xffull);
        }
    }
    f.valid = false;  // until the writing pass is through
    f.nnz_l = 0;
    f.stale_blocks = true;  // the trailing tiles keep the update blocks of the panels as they were
    BSM_TRY(sweep(std::true_type{}));
    stage_mark("nd_updown_sweep", s);
    if (U.npt_max > 0) {
        nd_updown_dinv<T><<<dim3((unsigned)na, (unsigned)U.npt_max), 64, 0, s>>>(p.nodes, d_act, F, f.dv.as<T>());
        BSM_HIP_TRY(hipGetLastError());
    }
    BSM_TRY(status(&h));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    stage_mark("nd_updown_dinv", s);
    // an update's r^2 = d^2 + w^2 fails only by overflow or a value that is
    // not finite: the factor is then partly rewritten and holds no values
    BSM_REQUIRE(h == ND_UPDOWN_OK, BSM_ERR_UNSUPPORTED, not_pd, sign < 0 ? "downdate" : "update",
                (h >> 8) & 0xffffffull, h >> 32, h & 0xffull);
    f.valid = true;
    return BSM_OK;
}

}  // namespace

int nd_factor_updown(bsm_nd_factor* f, int sign, uint64_t k, uint64_t nnz_w, const int64_t* colptr_dev,
                     const uint64_t* rows_dev, const void* vals_dev, uint64_t* n_miss, uint64_t* first_miss,
                     hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    ND_REQUIRE_VALUES(f);
    *n_miss = 0;
    *first_miss = 0;
    if (f->n == 0 || k == 0 || nnz_w == 0) return BSM_OK;
    const bool f64 = f->dtype == BSM_F64, s64 = f->src_dtype == BSM_F64;
    const int kk = (int)k;
    if (f64 && s64) return nd_factor_updown_t<double, double>(*f, sign, kk, colptr_dev, rows_dev, vals_dev, n_miss, first_miss, s);
    if (f64) return nd_factor_updown_t<double, float>(*f, sign, kk, colptr_dev, rows_dev, vals_dev, n_miss, first_miss, s);
    if (s64) return nd_factor_updown_t<float, double>(*f, sign, kk, colptr_dev, rows_dev, vals_dev, n_miss, first_miss, s);
    return nd_factor_updown_t<float, float>(*f, sign, kk, colptr_dev, rows_dev, vals_dev, n_miss, first_miss, s);
}

}  // namespace bsm

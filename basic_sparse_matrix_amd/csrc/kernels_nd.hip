// kernels_nd.hip -- solve(order="nd"): x = A^-1 b (src/lib.rs:11-24) by a
// multifrontal Cholesky of P A P^T on the nested-dissection separator tree
// (nd_order.cpp), on gfx950. DESIGN.md §4.9.
//
// Each tree node is a dense front F (f_pad x f_pad, column-major): its own
// np columns (padded to np_pad = 64 * npt with identity pivots), then its m
// front rows st (ancestors' columns), f = np_pad + m, f_pad = 64 * nt. Per
// level of the tree (height), bottom-up:
//   nd_factor  -- partial Cholesky of every front of the level: left-looking
//                 64 x 64 tiles on f64 MFMA, tickets in column order across
//                 the level's fronts, one flag per tile (write-through
//                 hand-offs as in blk_chol). Pivot tiles: L and the inverse
//                 diagonal tiles Dinv; trailing tiles: the update block
//                 U = F22 - L21 L21^T left in place.
//   the extend-add -- U of each child added into its parent's front (the
//                 lower-level child first, then slot 0: a fixed order, so
//                 the bits repeat): by default inside the parent's nd_factor
//                 tiles as they load (the "pull"); the plain pipeline
//                 (BSM_ND_PLAIN=1) runs nd_extend2 after each level.
// The solves walk the same levels: forward bottom-up (a child's update
// vector into its parent), backward top-down (the ancestors' x gathered).
// Not bit-exact with the reference (another elimination order, FMA); within
// the north star's f64 tolerance (tests/test_gpu_solver_nd.py).
// The plan is kernels_nd_plan.hip's; a kept factor (bsm_nd_factor) answers more
// in kernels_nd_selinv / _updown / _sparse / _partial.hip (nd_internal.hpp).
#include <algorithm>
#include <vector>

#include "nd_internal.hpp"

namespace bsm {
namespace {

#include "solve_tiles.hpp"

// A's lower triangle (j <= i, as band_fill reads it) into the fronts: entry
// (i, j) goes to the front owning column min(pinv i, pinv j)
template <typename T>
__global__ __launch_bounds__(256) void nd_assemble(int64_t n, const int64_t* __restrict__ rp,
                                                   const int32_t* __restrict__ col, const T* __restrict__ val,
                                                   const int32_t* __restrict__ pinv, const int32_t* __restrict__ owner,
                                                   const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                                   T* __restrict__ F) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t pi = pinv[i];
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        const int64_t j = col[e];
        if (j > i) continue;
        const int64_t pj = pinv[j];
        const int64_t r = pi > pj ? pi : pj, c = pi > pj ? pj : pi;
        const NdDev& nd = nodes[owner[c]];
        const int64_t lc = c - nd.start;
        const int64_t lr = r < nd.start + nd.np ? r - nd.start : nd.np_pad + lower_bound_i32(st + nd.st_off, nd.m, r);
        F[nd.foff + lc * nd.ld + lr] = val[e];
    }
}

// per solve: the entries' values in tile order (a contiguous read per tile)
template <typename T>
__global__ __launch_bounds__(256) void nd_aent_vals(int64_t na, const int64_t* __restrict__ aent,
                                                    const T* __restrict__ val, T* __restrict__ av) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < na) av[q] = val[aent[q] >> 12];
}

// zero the fronts' lower tiles (the only ones any kernel reads: every tile
// of the factor's lists): 55 % of the bytes a memset of the whole squares
// writes (the plain pipeline; the default one never reads F before writing it)
template <typename T>
__global__ __launch_bounds__(256) void nd_zero_tiles(const NdDev* __restrict__ nodes, const int4* __restrict__ tiles,
                                                     T* __restrict__ F) {
    const int4 tl = tiles[blockIdx.x];
    const NdDev& nd = nodes[tl.x];
    T* const t0 = F + nd.foff + (int64_t)64 * tl.z * nd.ld + 64 * tl.y;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = threadIdx.x + 256 * u;
        t0[(int64_t)(e >> 6) * nd.ld + (e & 63)] = (T)0;
    }
}

// identity on the padding pivots [np, np_pad) of every front
template <typename T>
__global__ __launch_bounds__(64) void nd_pad_pivots(const NdDev* __restrict__ nodes, T* __restrict__ F) {
    const NdDev& nd = nodes[blockIdx.x];
    for (int d = nd.np + (int)threadIdx.x; d < nd.np_pad; d += 64) F[nd.foff + (int64_t)d * nd.ld + d] = (T)1;
}

// Partial Cholesky of the fronts of one level. tiles[t] = (node, I, K, 0):
// column-major order across the level's fronts (K; the diagonal tiles of all
// fronts, then the tiles below them), so a tile only waits on tiles of
// earlier tickets. Tile (I, K), I >= K:
//     S = F_IK - sum_{J < min(K, npt)} L_IJ L_KJ^T
//     K < npt, I == K: L_KK = chol(S), Dinv_K = L_KK^-1   (flag)
//     K < npt, I >  K: L_IK = S L_KK^-T                    (flag)
//     K >= npt       : U_IK = S (the update block, for the extend-add)
// aent (the default pipeline): the tile starts from A's entries in it, staged
// from the plan's per-tile lists, plus its children's update blocks pulled
// through the task's descriptors (pdesc), and a diagonal tile skips its
// padding panels. aent == nullptr (the plain pipeline): the tile is read
// from F as nd_zero_tiles, nd_assemble, nd_pad_pivots and nd_extend2 left it,
// nothing is pulled or folded, and all four diagonal panels are factored.
// fV (the forward solve folded in, one right-hand side; BSM_ND_FOLD): the
// diagonal tile (I, I) also forms w_I = b_I + the children's update-vector
// entries landing in its rows - sum_{J < min(I, npt)} L_IJ y_J (the L_IJ are
// the tiles its products stage anyway; y_J is published before the flags
// its waits follow), then y_I = Linv_I w_I for a pivot tile or the update
// vector u_I = w_I for a front-row tile, into fV (V's layout: the separate
// forward's output), so no forward pass reads L again.
// STAMPS (BSM_ND_STAMPS=1, a diagnostic instantiation: the counters cost
// SGPRs the product build cannot spare): per workgroup,
// thread 0's shader-clock cycles in the flag waits, the products (loads,
// LDS staging, MFMA), the diagonal factors, the sub-diagonal solves, the
// update tiles' stores and the drains, and the tile counts of each kind,
// added into stamps[0..11] at the end
constexpr int ND_NSTAMP = 18;  // per level: BSM_ND_STAMPS's counters
template <typename T, bool STAMPS = false>
__global__ __launch_bounds__(256, 2) void nd_factor(const NdDev* __restrict__ nodes, const int4* __restrict__ tiles,
                                                 int64_t ntiles, T* __restrict__ F, T* __restrict__ Dinv,
                                                 int* __restrict__ flags, int* __restrict__ ticket,
                                                 int* __restrict__ status, const int32_t* __restrict__ ri,
                                                 T* __restrict__ fV, const T* __restrict__ fbp,
                                                 const int64_t* __restrict__ aent, const T* __restrict__ av,
                                                 const int2* __restrict__ tq, const NdPull* __restrict__ pdesc,
                                                 unsigned long long* __restrict__ stamps = nullptr) {
    long long c_wait = 0, c_prod = 0, c_diag = 0, c_trsm = 0, c_upd = 0, c_drain = 0;
    long long n_prod = 0, n_diag = 0, n_trsm = 0, n_upd = 0, c_total = 0, n_tiles = 0;
    long long c_pl[4] = {0, 0, 0, 0}, n_pull = 0;  // the pull's phases: tile + first child's loads, its adds, second, read-back
    const long long c_start = STAMPS ? (long long)clock64() : 0;
    __shared__ T PT[64][TLD];
    __shared__ T QT[64][TLD];
    __shared__ T rd[64];
    __shared__ T Di[4 * 256];
    __shared__ T Tb[3 * 256];
    __shared__ int pcs[2][64];  // the pull: a child block's columns' places in the tile
    __shared__ T fw[64], fyk[64], fpart[4][64];  // the folded forward solve (fV): w, y_J, partial sums
    __shared__ int tk;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = 16 * w + (lane >> 4), cm = lane & 15;
    lds_t<T>* const PTl = (lds_t<T>*)&PT[0][0];
    lds_t<T>* const QTl = (lds_t<T>*)&QT[0][0];
    // the poll has no break (the structurizer's hazard in nd_backward_tiles)
    auto wait_flag = [&](const int* f) {
        long long spins = 0;
        while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && spins <= SPIN_LIMIT) {
            __builtin_amdgcn_s_sleep(1);
            ++spins;
        }
        if (spins > SPIN_LIMIT && lane == 0) atomicOr(status, ST_TIMEOUT);
    };
    // the ticket at the END of each task and counted inner loops (the
    // control-flow shape of nd_backward_tiles)
    if (tid == 0) tk = atomicAdd(ticket, 1);
    __syncthreads();
    int64_t t = __builtin_amdgcn_readfirstlane(tk);
    while (t < ntiles) {
        const int4 tl = tiles[t];
        const NdDev& nd = nodes[tl.x];
        const int npt = nd.npt;
        const int I = tl.y, K = tl.z;
        const int64_t ld = nd.ld;
        T* const Fn = F + nd.foff;
        int* const fl = flags + nd.flag_off;
        // tile (I2, J) of L into registers (sc1: other workgroups wrote it),
        // then X[t][r] = L[64 I2 + r][64 J + t] in LDS
        auto load = [&](T (&v)[16], int I2, int J) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = tid + 256 * u, r = e & 63, c = e >> 6;
                v[u] = ld_sc1(&Fn[(int64_t)(64 * J + c) * ld + 64 * I2 + r]);
            }
        };
        auto store = [&](T (*X)[TLD], const T (&v)[16]) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = tid + 256 * u;
                X[e >> 6][e & 63] = v[u];
            }
        };
        long long c0 = STAMPS ? (long long)clock64() : 0;
        T acc[4][4];
        // the folded forward solve on this diagonal tile: w = b (pivot rows)
        const bool fold = fV && I == K;
        if (fold && tid < 64) fw[tid] = 64 * K + tid < nd.np ? fbp[nd.start + 64 * K + tid] : (T)0;
        if (aent) {
            // The tile starts from A's entries in it (and the padding
            // pivots' identity), staged in LDS from the plan's per-tile lists,
            // instead of from F (no zeroing, no assembly, no read of F): the
            // same values, written the same way.
            // The children's update blocks, pulled into this tile (no
            // nd_extend2 launches): the entries (a, b), a >= b, of child c
            // with ri[a] in tile row I and ri[b] in tile column K, i.e. a in
            // [tb[I], tb[I + 1]), b in [tb[K], tb[K + 1]) (ri ascending; the
            // task's descriptors hold these ranges, nd_task_pull).
            // The tile goes to LDS by coalesced columns; thread (lane, wave)
            // takes the child's a = a0 + lane and b = b0 + 4 u + w, its
            // row's place one load per lane and the columns' places through
            // LDS (pcs). Every load is unconditional (indices clamped to
            // the block, so they all go out together), and each child's 16
            // additions read their LDS elements first and then write them
            // (the block's places are distinct). The children's entries are
            // added in the order nd_extend2 adds them (the lower level first,
            // then slot 0): F + U_first + U_second, the same roundings, the
            // same bits.
            struct Blk {
                const T* U;
                const int32_t* rc;
                const T* u;  // the child's update vector (fold)
                int ld, a0, ra, b0, rbn;
            } bk[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // ra = 0: no such child, or none of its entries in this tile
                const NdPull& o = pdesc[2 * t + h];
                bk[h].U = F + o.uoff;
                bk[h].rc = ri + o.rcoff;
                bk[h].u = fV ? fV + o.uvoff : nullptr;
                bk[h].ld = o.ld;
                bk[h].a0 = o.a0;
                bk[h].ra = o.ra;
                bk[h].b0 = o.b0;
                bk[h].rbn = o.rbn;
            }
            T v[16];
            int pr[2] = {0, 0};
            // the rows' places (per lane) and the columns' (into pcs, read
            // back wave-uniform) of both children
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (bk[h].ra > 0) {
                    pr[h] = bk[h].rc[bk[h].a0 + min(lane, bk[h].ra - 1)] - 64 * I;
                    if (tid < 64) pcs[h][tid] = bk[h].rc[bk[h].b0 + min(tid, bk[h].rbn - 1)] - 64 * K;
                }
            T uv = (T)0;
            auto issue = [&](const Blk& k) {
                const int a = k.a0 + min(lane, k.ra - 1);
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = k.U[(int64_t)(k.b0 + min(4 * u + w, k.rbn - 1)) * k.ld + a];
                if (fold && w == 0) uv = k.u[a];
            };
            auto add = [&](const Blk& k, int h) {
                T cur[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) cur[u] = PT[pr[h]][pcs[h][4 * u + w]];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int bl = 4 * u + w;
                    if (lane < k.ra && bl < k.rbn && k.a0 + lane >= k.b0 + bl) PT[pr[h]][pcs[h][bl]] = cur[u] + v[u];
                }
                if (fold && w == 0 && lane < k.ra) fw[pr[h]] += uv;
            };
            const int2 rq = tq[t];
#pragma unroll
            for (int u = 0; u < 16; ++u) PT[lane][4 * u + w] = (T)0;
            __syncthreads();
            for (int q = tid; q < rq.y; q += 256) {
                const int64_t x = aent[rq.x + q];
                PT[x & 63][(x >> 6) & 63] = av[rq.x + q];
            }
            if (I == K && K < npt && tid < 64 && 64 * K + tid >= nd.np) PT[tid][tid] = (T)1;
            if (bk[0].ra > 0) issue(bk[0]);
            long long ps = 0;
            auto pstamp = [&](int i) {
                if (STAMPS) {
                    const long long c = (long long)clock64();
                    c_pl[i] += c - ps;
                    ps = c;
                }
            };
            if (STAMPS) ps = c0, ++n_pull;
            __syncthreads();  // the staged tile
            pstamp(0);
            if (bk[0].ra > 0) add(bk[0], 0);
            pstamp(1);
            if (bk[1].ra > 0) {
                issue(bk[1]);
                __syncthreads();  // the first child's additions
                add(bk[1], 1);
            }
            pstamp(2);
            __syncthreads();
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[cb][q] = PT[rb + 4 * q][16 * cb + cm];
            __syncthreads();  // PT is the products' staging next
            pstamp(3);
        } else {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[cb][q] = Fn[(int64_t)(64 * K + 16 * cb + cm) * ld + 64 * I + rb + 4 * q];
        }
        // left-looking products (two workgroups per CU: __launch_bounds__
        // (256, 2) caps the registers at 256 per lane; the f64 kernel uses
        // 255 with no scratch. With one workgroup per CU the C5 factor took
        // 8.5 instead of 5.7 ms)
        const int Jn = K < npt ? K : npt;
        T fp = (T)0;  // fold: this thread's share of (L_IJ y_J)[lane], terms 16 w .. 16 w + 15
        for (int J = 0; J < Jn; ++J) {
            const long long cw = STAMPS ? (long long)clock64() : 0;
            wait_flag(&fl[I * npt + J]);
            if (I != K) wait_flag(&fl[K * npt + J]);
            if (STAMPS) c_wait += (long long)clock64() - cw;
            T va[16];
            load(va, I, J);
            if (fold && tid < 64) fyk[tid] = ld_sc1(&fV[nd.voff + 64 * J + tid]);  // y_J (before (J, J)'s flag)
            store(PT, va);
            if (I != K) {
                load(va, K, J);
                store(QT, va);
            }
            __syncthreads();
            mfma_tile<T, true>(PTl, I != K ? QTl : PTl, acc, w, lane);
            if (fold) {
#pragma unroll
                for (int t = 0; t < 16; ++t) fp = fma_t((T)PT[16 * w + t][lane], fyk[16 * w + t], fp);  // PT[t][r] = L[r][t]
            }
            __syncthreads();
        }
        if (fold) {  // w_I = b + children's entries - sum_J L_IJ y_J
            fpart[w][lane] = fp;
            __syncthreads();
            if (tid < 64) fw[tid] = fw[tid] - ((fpart[0][tid] + fpart[1][tid]) + (fpart[2][tid] + fpart[3][tid]));
            __syncthreads();
        }
        if (STAMPS) {
            const long long c1 = (long long)clock64();
            c_prod += c1 - c0;
            n_prod += Jn;
            c0 = c1;
        }
        if (K < npt && I == K) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) PT[rb + 4 * q][16 * cb + cm] = acc[cb][q];
            __syncthreads();
            // the panels holding real pivots (the front's last pivot tile may
            // end in identity padding: blk_diag_panels skips those panels;
            // the plain pipeline factors all four)
            const int rem = nd.np - 64 * K;
            blk_diag_panels<T>(PTl, QTl, (lds_t<T>*)Di, (lds_t<T>*)Tb, (lds_t<T>*)rd, status, tid, nullptr, nullptr,
                               nullptr, nullptr, rem >= 64 || !aent ? 4 : (rem + 15) / 16);
            __syncthreads();
            T* const dk = Dinv + nd.dinv_off + (int64_t)K * 4096;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = tid + 256 * u, q = e >> 6, l = e & 63;
                st_sc1(&dk[e], (T)QT[q][l]);  // Dinv[q * 64 + l] = Linv[l][q]
                const int r = e & 63, c = e >> 6;
                Fn[(int64_t)(64 * K + c) * ld + 64 * K + r] = r >= c ? (T)PT[r][c] : (T)0;
            }
            if (fold) {  // y_K = Linv_K w_K (QT[q][l] = Linv[l][q]), published with the tile's flag
                T y = (T)0;
#pragma unroll
                for (int j = 0; j < 16; ++j) y = fma_t((T)QT[16 * w + j][lane], fw[16 * w + j], y);
                fpart[w][lane] = y;
                __syncthreads();
                if (tid < 64)
                    st_sc1(&fV[nd.voff + 64 * K + tid], (fpart[0][tid] + fpart[1][tid]) + (fpart[2][tid] + fpart[3][tid]));
            }
        } else if (K < npt) {
            wait_flag(&fl[K * npt + K]);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) PT[16 * cb + cm][rb + 4 * q] = acc[cb][q];  // S^T
            const T* const dk = Dinv + nd.dinv_off + (int64_t)K * 4096;
            T v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = ld_sc1(&dk[tid + 256 * u]);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = tid + 256 * u;
                QT[e >> 6][e & 63] = v[u];  // QT[s][c] = Linv[c][s]
            }
            __syncthreads();
            T o[4][4] = {};
            mfma_tile<T, false, true>(PTl, QTl, o, w, lane);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    st_sc1(&Fn[(int64_t)(64 * K + 16 * cb + cm) * ld + 64 * I + rb + 4 * q], o[cb][q]);
        } else {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) Fn[(int64_t)(64 * K + 16 * cb + cm) * ld + 64 * I + rb + 4 * q] = acc[cb][q];
            if (fold && tid < 64) st_sc1(&fV[nd.voff + 64 * K + tid], (T)fw[tid]);  // the update vector u_K
        }
        long long c2 = 0;
        if (STAMPS) {
            c2 = (long long)clock64();
            if (K < npt && I == K) c_diag += c2 - c0, ++n_diag;
            else if (K < npt) c_trsm += c2 - c0, ++n_trsm;
            else c_upd += c2 - c0, ++n_upd;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (K < npt && tid == 0) __hip_atomic_store(&fl[I * npt + K], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (STAMPS) c_drain += (long long)clock64() - c2, ++n_tiles;
        __syncthreads();
        if (tid == 0) tk = atomicAdd(ticket, 1);
        __syncthreads();
        t = __builtin_amdgcn_readfirstlane(tk);
    }
    if (STAMPS && tid == 0) {
        c_total = (long long)clock64() - c_start;
        const long long v[ND_NSTAMP] = {c_total, c_wait, c_prod,  c_diag,  c_trsm,  c_upd,  c_drain, n_tiles,
                                        n_prod,  n_diag, n_trsm,  n_upd,   c_pl[0], c_pl[1], c_pl[2], c_pl[3],
                                        n_pull,  0};
        for (int i = 0; i < ND_NSTAMP; ++i) atomicAdd(&stamps[i], (unsigned long long)v[i]);
    }
}

// U of the children into their parent's front (the plain pipeline), both
// children of a parent in one launch: task (c0, b0, c1, b1) adds column b0 of
// child c0's update block, rows a >= b0, at (ri[a], ri[b0]), then column b1
// of child c1's, into the SAME parent column (ri[b0] of c0 == ri[b1] of c1;
// -1: that child has none), in that order, on one wave; the tasks of a
// launch own distinct parent columns. The second child's loads are
// write-through (the first child's stores came from other lanes of this
// wave) after the wave's stores drain.
template <typename T>
__global__ __launch_bounds__(256) void nd_extend2(const NdDev* __restrict__ nodes, const int4* __restrict__ tasks,
                                                  int64_t ntasks, const int32_t* __restrict__ ri, T* __restrict__ F) {
    const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task >= ntasks) return;
    const int lane = threadIdx.x & 63;
    const int4 tk = tasks[task];
    auto add = [&](int ci, int b, bool coherent) {
        const NdDev& c = nodes[ci];
        const NdDev& p = nodes[c.parent];
        const int32_t* rc = ri + c.st_off;
        const T* src = F + c.foff + (int64_t)(c.np_pad + b) * c.ld + c.np_pad;
        T* dst = F + p.foff + (int64_t)rc[b] * p.ld;
        for (int a = b + lane; a < c.m; a += 64) {
            T* d = dst + rc[a];
            *d = (coherent ? ld_sc1(d) : *d) + src[a];
        }
    };
    if (tk.x >= 0) add(tk.x, tk.y, false);
    if (tk.z >= 0) {
        if (tk.x >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        add(tk.z, tk.w, tk.x >= 0);
    }
}

// right-hand sides into the new order: bp[col * n + q] = b[perm[q] * k + col] (b row-major n x k).
// perm == null: the identity (b is in the new order already: the L and L^T systems of a kept factor)
template <typename T>
__global__ __launch_bounds__(256) void nd_gather(int64_t n, int64_t k, const int64_t* __restrict__ perm,
                                                 const T* __restrict__ b, T* __restrict__ bp) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int64_t o = perm ? perm[q] : q;
    for (int64_t c = 0; c < k; ++c) bp[c * n + q] = b[o * k + c];
}
template <typename T>
__global__ __launch_bounds__(256) void nd_scatter(int64_t n, int64_t k, const int64_t* __restrict__ perm,
                                                  const T* __restrict__ xp, T* __restrict__ x) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int64_t o = perm ? perm[q] : q;
    for (int64_t c = 0; c < k; ++c) x[o * k + c] = xp[c * n + q];
}

// The two passes of a solve hand y over in V: over the pivots of each front's
// vector (at voff), not in bp. One pass alone (the L and L^T systems of a
// kept factor) moves y across that boundary, one workgroup per (front,
// column). After the forward levels: the np pivots of v out to bp.
template <typename T>
__global__ __launch_bounds__(256) void nd_y_out(const NdDev* __restrict__ nodes, int64_t n, const T* __restrict__ V,
                                                int64_t vtot, T* __restrict__ bp) {
    const NdDev& nd = nodes[blockIdx.x];
    const int64_t col = blockIdx.y;
    const T* const v = V + col * vtot + nd.voff;
    for (int r = threadIdx.x; r < nd.np; r += 256) bp[col * n + nd.start + r] = v[r];
}
// Before the backward levels: y from bp over the pivots, and 0 over every
// other row of the front's 64 nt: the backward kernels read whole tiles of w
// and rely on the padding pivots and the rows past f being exactly 0 (the
// front rows they overwrite with the ancestors' x themselves).
template <typename T>
__global__ __launch_bounds__(256) void nd_y_in(const NdDev* __restrict__ nodes, int64_t n, const T* __restrict__ bp,
                                               T* __restrict__ V, int64_t vtot) {
    const NdDev& nd = nodes[blockIdx.x];
    const int64_t col = blockIdx.y;
    T* const v = V + col * vtot + nd.voff;
    const int fp = 64 * nd.nt;
    for (int r = threadIdx.x; r < fp; r += 256) v[r] = r < nd.np ? bp[col * n + nd.start + r] : (T)0;
}

// Forward solve of one level, one workgroup per (node, column): v = the
// node's pivots of bp plus its children's update vectors; per pivot tile K
// y_K = Dinv_K v_K, then v_I -= L_IK y_K below. v (at V + voff) ends as y
// over the pivots and the update vector u over the front rows. V is read and
// written write-through (rows change hands between threads). Every product's
// loads are issued together (unrolled): a loop of load, wait, FMA is one
// L2 round trip per term, 64 per tile step.
// The body is nd_forward_front: nd_forward runs it on every front of a level
// with both children, nd_forward_path (the sparse right-hand sides, §4.9k) on
// the active fronts alone with their ACTIVE children (kids: bit 0 = kid0,
// bit 1 = kid1; an inactive child's update vector would be +0 and its V is
// never written).
template <typename T>
__device__ __forceinline__ void nd_forward_front(const NdDev* __restrict__ nodes, const NdDev& nd, int kids,
                                                 int64_t col, int64_t n, const T* __restrict__ bp, T* __restrict__ V,
                                                 int64_t vtot, const T* __restrict__ F, const T* __restrict__ Dinv,
                                                 const int32_t* __restrict__ ri) {
    __shared__ T vk[64], yk[64];
    __shared__ T part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    T* const v = V + col * vtot + nd.voff;
    const int fp = 64 * nd.nt;
    for (int r = tid; r < fp; r += 256) st_sc1(&v[r], r < nd.np ? bp[col * n + nd.start + r] : (T)0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int kid = s == 0 ? nd.kid0 : nd.kid1;
        if (kid < 0 || !((kids >> s) & 1)) continue;
        const NdDev& c = nodes[kid];
        const T* u = V + col * vtot + c.voff + c.np_pad;
        const int32_t* rc = ri + c.st_off;
        for (int a = tid; a < c.m; a += 256) {
            T* d = &v[rc[a]];
            st_sc1(d, ld_sc1(d) + u[a]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const T* const Fn = F + nd.foff;
    const int64_t ld = nd.ld;
    for (int K = 0; K < nd.npt; ++K) {
        if (tid < 64) vk[tid] = ld_sc1(&v[64 * K + tid]);
        __syncthreads();
        {  // y_K = Dinv_K v_K: wave wv sums terms q in [16 wv, 16 wv + 16)
            const T* g = Dinv + nd.dinv_off + (int64_t)K * 4096 + 16 * wv * 64 + lane;
            T gv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) gv[j] = g[j * 64];
            T y0 = (T)0, y1 = (T)0;
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                y0 = fma_t(gv[j], vk[16 * wv + j], y0);
                y1 = fma_t(gv[j + 1], vk[16 * wv + j + 1], y1);
            }
            part[wv][lane] = y0 + y1;
        }
        __syncthreads();
        if (tid < 64) {
            const T y = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
            yk[tid] = y;
            st_sc1(&v[64 * K + tid], y);
        }
        __syncthreads();
        // rows past f and the pivot padding rows are zero in L (and stay
        // zero in v): skipped whole (the loads inside stay unconditional, so
        // they go out together)
        const int f = nd.np_pad + nd.m;
        for (int r = 64 * (K + 1) + tid; r < f; r += 256) {
            if (r >= nd.np && r < nd.np_pad) continue;
            // the row's 64 terms in two halves of 32 loads in flight: at 226
            // VGPRs (all 64 at once) two workgroups fit a CU, at <= 128 four
            // (the leaf level is latency bound: 7,699 fronts at C5); same
            // accumulators, same order, same bits
            const T* lc = Fn + (int64_t)64 * K * ld + r;
            const T vr = ld_sc1(&v[r]);
            T s0 = (T)0, s1 = (T)0, s2 = (T)0, s3 = (T)0;
#pragma unroll
            for (int h = 0; h < 64; h += 32) {
                T lv[32];
#pragma unroll
                for (int t = 0; t < 32; ++t) lv[t] = lc[(int64_t)(h + t) * ld];
#pragma unroll
                for (int t = 0; t < 32; t += 4) {
                    s0 = fma_t(lv[t], yk[h + t], s0);
                    s1 = fma_t(lv[t + 1], yk[h + t + 1], s1);
                    s2 = fma_t(lv[t + 2], yk[h + t + 2], s2);
                    s3 = fma_t(lv[t + 3], yk[h + t + 3], s3);
                }
            }
            st_sc1(&v[r], vr - ((s0 + s1) + (s2 + s3)));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256, 4) void nd_forward(const NdDev* __restrict__ nodes, const int32_t* __restrict__ lvl,
                                                  int64_t n, const T* __restrict__ bp, T* __restrict__ V, int64_t vtot,
                                                  const T* __restrict__ F, const T* __restrict__ Dinv,
                                                  const int32_t* __restrict__ ri) {
    nd_forward_front<T>(nodes, nodes[lvl[blockIdx.x]], 3, blockIdx.y, n, bp, V, vtot, F, Dinv, ri);
}

// one workgroup per (active front, column); act: the level's part of the forward set
template <typename T>
__global__ __launch_bounds__(256, 4) void nd_forward_path(const NdDev* __restrict__ nodes,
                                                       const ReachFront* __restrict__ act, int64_t n,
                                                       const T* __restrict__ bp, T* __restrict__ V, int64_t vtot,
                                                       const T* __restrict__ F, const T* __restrict__ Dinv,
                                                       const int32_t* __restrict__ ri) {
    const ReachFront me = act[blockIdx.x];
    nd_forward_front<T>(nodes, nodes[me.node], me.kids, blockIdx.y, n, bp, V, vtot, F, Dinv, ri);
}

// A solve wave waits on a pivot tile of its own front that a running wave
// publishes within microseconds: ~1 s of polls is a hang (reported as
// ST_TIMEOUT, not spun on for the factor's ~30 s)
constexpr long long ND_SOLVE_SPIN_LIMIT = 1ll << 20;

// Forward solve of one level by tile rows: one wave per (node, tile row I,
// column), taken by ticket in I-major order across the level's fronts (a
// wave only waits on lower tickets, which are running or done). The wave
// forms its 64 rows' v (the pivots of bp, then child 0's and child 1's
// update entries landing in these rows), subtracts L_IK y_K for K < min(I,
// npt) as each y_K is published (flag per node, column and pivot tile), and,
// for a pivot tile, forms y_I = Dinv_I v_I and publishes it. Per row the
// same operations in the same order as nd_forward (one thread per row, the
// 64-term products in four accumulators; y from four 16-term partials):
// the same bits, with the fronts' chains of pivot tiles running on as many
// waves as the front has tile rows instead of one workgroup
// (BSM_ND_FWD_TILES=0: nd_forward, for the A/B).
template <typename T>
__global__ __launch_bounds__(64) void nd_forward_tiles(const NdDev* __restrict__ nodes, const int2* __restrict__ tasks,
                                                       int64_t ntasks, int k, int64_t n, const T* __restrict__ bp,
                                                       T* __restrict__ V, int64_t vtot, const T* __restrict__ F,
                                                       const T* __restrict__ Dinv, const int32_t* __restrict__ ri,
                                                       int* __restrict__ yflags, int* __restrict__ ticket,
                                                       int* __restrict__ status) {
    __shared__ T yk[64];
    __shared__ T add[2][64];
    __shared__ int hit[2][64];
    __shared__ int tk;
    const int lane = threadIdx.x;
    const int64_t total = ntasks * k;
    // The control-flow shape of nd_backward_tiles (whose first form, with the
    // ticket at the loop head, compiled to a loop that never took a new
    // ticket): the ticket is taken at the END of each task, the flag poll has
    // no break, and no barrier sits inside a branch.
    if (lane == 0) tk = atomicAdd(ticket, 1);
    __syncthreads();
    int64_t t = __builtin_amdgcn_readfirstlane(tk);
    while (t < total) {
        const int2 task = tasks[t / k];
        const int col = (int)(t % k);
        const NdDev& nd = nodes[task.x];
        const int I = task.y;
        T* const v = V + (int64_t)col * vtot + nd.voff;
        int* const yf = yflags + (nd.dinv_off / 4096) * k + (int64_t)col * nd.npt;
        const int r = 64 * I + lane;
        T val = r < nd.np ? bp[(int64_t)col * n + nd.start + r] : (T)0;
        // the children's update entries in rows [64 I, 64 I + 64): ri is
        // ascending, so they are one range of each child's entries
        hit[0][lane] = 0;
        hit[1][lane] = 0;
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            const int kid = sl == 0 ? nd.kid0 : nd.kid1;
            if (kid >= 0) {
                const NdDev& c = nodes[kid];
                const int32_t* rc = ri + c.st_off;
                const int32_t lo = lower_bound_i32(rc, c.m, 64 * I), hi = lower_bound_i32(rc, c.m, 64 * I + 64);
                const T* u = V + (int64_t)col * vtot + c.voff + c.np_pad;
                for (int32_t a = lo + lane; a < hi; a += 64) {
                    add[sl][rc[a] - 64 * I] = u[a];
                    hit[sl][rc[a] - 64 * I] = 1;
                }
            }
        }
        __syncthreads();
        if (nd.kid0 >= 0 && hit[0][lane]) val = val + add[0][lane];
        if (nd.kid1 >= 0 && hit[1][lane]) val = val + add[1][lane];
        const T* const lrow = F + nd.foff + r;
        const int64_t ld = nd.ld;
        const int Kn = I < nd.npt ? I : nd.npt;
        for (int K = 0; K < Kn; ++K) {
            if (lane == 0) {
                long long spins = 0;
                while (__hip_atomic_load(&yf[K], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
                       spins < ND_SOLVE_SPIN_LIMIT) {
                    __builtin_amdgcn_s_sleep(1);
                    ++spins;
                }
                if (spins >= ND_SOLVE_SPIN_LIMIT) atomicOr(status, ST_TIMEOUT);
            }
            __syncthreads();
            T lv[64];
#pragma unroll
            for (int q = 0; q < 64; ++q) lv[q] = lrow[(int64_t)(64 * K + q) * ld];
            yk[lane] = ld_sc1(&v[64 * K + lane]);
            __syncthreads();
            T s0 = (T)0, s1 = (T)0, s2 = (T)0, s3 = (T)0;
#pragma unroll
            for (int q = 0; q < 64; q += 4) {
                s0 = fma_t(lv[q], yk[q], s0);
                s1 = fma_t(lv[q + 1], yk[q + 1], s1);
                s2 = fma_t(lv[q + 2], yk[q + 2], s2);
                s3 = fma_t(lv[q + 3], yk[q + 3], s3);
            }
            val = val - ((s0 + s1) + (s2 + s3));
            __syncthreads();
        }
        // a pivot tile: y_I = Dinv_I v_I, as nd_forward's four 16-term partials
        const bool pivot = I < nd.npt;
        yk[lane] = val;
        __syncthreads();
        T out = val;
        if (pivot) {
            const T* g = Dinv + nd.dinv_off + (int64_t)I * 4096 + lane;
            T part[4];
#pragma unroll
            for (int wv = 0; wv < 4; ++wv) {
                T gv[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) gv[j] = g[(16 * wv + j) * 64];
                T y0 = (T)0, y1 = (T)0;
#pragma unroll
                for (int j = 0; j < 16; j += 2) {
                    y0 = fma_t(gv[j], yk[16 * wv + j], y0);
                    y1 = fma_t(gv[j + 1], yk[16 * wv + j + 1], y1);
                }
                part[wv] = y0 + y1;
            }
            out = (part[0] + part[1]) + (part[2] + part[3]);
        }
        st_sc1(&v[r], out);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (lane == 0) {
            if (pivot) __hip_atomic_store(&yf[I], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tk = atomicAdd(ticket, 1);
        }
        __syncthreads();
        t = __builtin_amdgcn_readfirstlane(tk);
    }
}

// Backward solve of one level, one workgroup per (node, column): w = y over
// the pivots, the ancestors' x over the front rows; per pivot tile K from the
// last, x_K = Dinv_K^T (y_K - L_{>K,K}^T w_{>K}); the pivots' x to xp.
// The body is nd_backward_front: nd_backward runs it on every front of a
// level, nd_backward_path (§4.9k) on the fronts on the paths from the requested
// rows to the root. has_y: the forward pass has left y over the pivots (and 0
// over the padding pivots and the rows past f); else the front was not
// forward-active, y = 0, and those rows are written as 0 here (V may hold
// anything there).
template <typename T>
__device__ __forceinline__ void nd_backward_front(const NdDev& nd, bool has_y, int64_t col, int64_t n,
                                                  T* __restrict__ xp, T* __restrict__ V, int64_t vtot,
                                                  const T* __restrict__ F, const T* __restrict__ Dinv,
                                                  const int32_t* __restrict__ st) {
    __shared__ T red[64][65];
    __shared__ T zk[64];
    __shared__ T part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    T* const w = V + col * vtot + nd.voff;
    const int fp = 64 * nd.nt;
    if (!has_y)  // every row but the front rows (written next, by other threads)
        for (int r = tid; r < fp; r += 256)
            if (r < nd.np_pad || r >= nd.np_pad + nd.m) st_sc1(&w[r], (T)0);
    for (int a = tid; a < nd.m; a += 256) st_sc1(&w[nd.np_pad + a], xp[col * n + st[nd.st_off + a]]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const T* const Fn = F + nd.foff;
    const int64_t ld = nd.ld;
    for (int K = nd.npt - 1; K >= 0; --K) {
        // column sums below the tile: wave wv takes columns 16 wv .. 16 wv + 15,
        // lanes the rows, two rows per lane in flight
        T acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = (T)0;
        // rows by tile from the LAST tile down to K + 1 (the front rows, known
        // from the start, first: nd_backward_tiles sums in this order while
        // the pivot tiles' x arrive)
        const T* lc = Fn + (int64_t)(64 * K + 16 * wv) * ld;
        const int rlo = 64 * (K + 1);
        // a zero row of L (past f, or a pivot padding row) has w = 0 exactly:
        // its loads go to a real row's address instead (the same cache lines
        // for every such lane, so no HBM bytes), unconditionally (they still
        // go out together), and the term stays 0 (an accumulator that starts
        // at +0 never becomes -0): the same sums, the same bits
        const int f = nd.np_pad + nd.m;
        auto row = [&](int rr) { return rr >= f ? f - 1 : (rr >= nd.np && rr < nd.np_pad ? nd.np - 1 : rr); };
        int r = fp - 64 + lane;
        for (; r - 64 >= rlo; r -= 128) {
            const T w0 = ld_sc1(&w[r]), w1 = ld_sc1(&w[r - 64]);
            const int q0 = row(r), q1 = row(r - 64);
            T l0[16], l1[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                l0[c] = lc[(int64_t)c * ld + q0];
                l1[c] = lc[(int64_t)c * ld + q1];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = fma_t(l1[c], w1, fma_t(l0[c], w0, acc[c]));
        }
        if (r >= rlo) {
            const T w0 = ld_sc1(&w[r]);
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = fma_t(lc[(int64_t)c * ld + r], w0, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) red[16 * wv + c][lane] = acc[c];
        __syncthreads();
        if (tid < 64) {
            T s0 = (T)0, s1 = (T)0, s2 = (T)0, s3 = (T)0;
#pragma unroll
            for (int l = 0; l < 64; l += 4) {
                s0 += red[tid][l];
                s1 += red[tid][l + 1];
                s2 += red[tid][l + 2];
                s3 += red[tid][l + 3];
            }
            zk[tid] = ld_sc1(&w[64 * K + tid]) - ((s0 + s1) + (s2 + s3));
        }
        __syncthreads();
        {  // x_K = Dinv_K^T z: Linv[q][l] = Dinv[l * 64 + q]; wave wv sums q in [16 wv, 16 wv + 16)
            const T* g = Dinv + nd.dinv_off + (int64_t)K * 4096 + (int64_t)lane * 64 + 16 * wv;
            T gv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) gv[j] = g[j];
            T x0 = (T)0, x1 = (T)0;
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                x0 = fma_t(gv[j], zk[16 * wv + j], x0);
                x1 = fma_t(gv[j + 1], zk[16 * wv + j + 1], x1);
            }
            part[wv][lane] = x0 + x1;
        }
        __syncthreads();
        if (tid < 64) st_sc1(&w[64 * K + tid], (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    for (int p = tid; p < nd.np; p += 256) xp[col * n + nd.start + p] = ld_sc1(&w[p]);
}

template <typename T>
__global__ __launch_bounds__(256) void nd_backward(const NdDev* __restrict__ nodes, const int32_t* __restrict__ lvl,
                                                   int64_t n, T* __restrict__ xp, T* __restrict__ V, int64_t vtot,
                                                   const T* __restrict__ F, const T* __restrict__ Dinv,
                                                   const int32_t* __restrict__ st) {
    nd_backward_front<T>(nodes[lvl[blockIdx.x]], true, blockIdx.y, n, xp, V, vtot, F, Dinv, st);
}

// one workgroup per (active front, column); act: the level's part of the
// backward set, kids != 0: the front was forward-active too
template <typename T>
__global__ __launch_bounds__(256) void nd_backward_path(const NdDev* __restrict__ nodes,
                                                        const ReachFront* __restrict__ act, int64_t n,
                                                        T* __restrict__ xp, T* __restrict__ V, int64_t vtot,
                                                        const T* __restrict__ F, const T* __restrict__ Dinv,
                                                        const int32_t* __restrict__ st) {
    const ReachFront me = act[blockIdx.x];
    nd_backward_front<T>(nodes[me.node], me.kids != 0, blockIdx.y, n, xp, V, vtot, F, Dinv, st);
}

// Backward solve of one level by pivot tiles: one workgroup per (node, pivot
// tile K, column), taken by ticket from the fronts' last pivot tiles down (a
// workgroup only waits on lower tickets). It sums the column products of
// the rows below tile K as nd_backward does, tile by tile from the last: the
// front rows (the ancestors' x, read through st) at once, then each pivot
// tile J > K as its x_J is published (flag per node, column and pivot tile);
// then x_K = Dinv_K^T (y_K - sums) and its pivots to xp. The same operations
// in the same order per lane as nd_backward: the same bits
// (BSM_ND_BWD_TILES=0 for the A/B).
template <typename T>
__global__ __launch_bounds__(256) void nd_backward_tiles(const NdDev* __restrict__ nodes,
                                                         const int2* __restrict__ tasks, int64_t ntasks, int k,
                                                         int64_t n, T* __restrict__ xp, T* __restrict__ V,
                                                         int64_t vtot, const T* __restrict__ F,
                                                         const T* __restrict__ Dinv, const int32_t* __restrict__ st,
                                                         int* __restrict__ xflags, int* __restrict__ ticket,
                                                         int* __restrict__ status) {
    __shared__ T red[64][65];
    __shared__ T zk[64];
    __shared__ T part[4][64];
    __shared__ int tk;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t total = ntasks * k;
    // Control flow kept simple for the structurizer (a first form, with the
    // ticket taken at the loop head and a barrier inside an if / else of the
    // row loop, compiled to a loop whose back edge skipped the ticket: the
    // workgroup redid its first task forever): the ticket is taken at the
    // END of each task, both row loops are plain counted loops, and the
    // flag poll has no break.
    if (tid == 0) tk = atomicAdd(ticket, 1);
    __syncthreads();
    int64_t t = __builtin_amdgcn_readfirstlane(tk);
    while (t < total) {
        const int2 task = tasks[t / k];
        const int col = (int)(t % k);
        const NdDev& nd = nodes[task.x];
        const int K = task.y;
        T* const w = V + (int64_t)col * vtot + nd.voff;
        int* const xf = xflags + (nd.dinv_off / 4096) * k + (int64_t)col * nd.npt;
        const int32_t* const sr = st + nd.st_off;
        const T* const lc = F + nd.foff + (int64_t)(64 * K + 16 * wv) * nd.ld;
        const int64_t ld = nd.ld;
        T acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = (T)0;
        // the front rows' tiles, last first: the ancestors' x (0 past the m rows)
        const int jf = nd.npt > K + 1 ? nd.npt : K + 1;
        for (int J = nd.nt - 1; J >= jf; --J) {
            const int r = 64 * J + lane, a = r - nd.np_pad;
            const T wr = a < nd.m ? xp[(int64_t)col * n + sr[a]] : (T)0;
            T l[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) l[c] = lc[(int64_t)c * ld + r];
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = fma_t(l[c], wr, acc[c]);
        }
        // then the pivot tiles below K, each as its x is published
        for (int J = nd.npt - 1; J > K; --J) {
            if (tid == 0) {
                long long spins = 0;
                while (__hip_atomic_load(&xf[J], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
                       spins < ND_SOLVE_SPIN_LIMIT) {
                    __builtin_amdgcn_s_sleep(1);
                    ++spins;
                }
                if (spins >= ND_SOLVE_SPIN_LIMIT) atomicOr(status, ST_TIMEOUT);
            }
            __syncthreads();
            const int r = 64 * J + lane;
            const T wr = ld_sc1(&w[r]);
            T l[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) l[c] = lc[(int64_t)c * ld + r];
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = fma_t(l[c], wr, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) red[16 * wv + c][lane] = acc[c];
        __syncthreads();
        if (tid < 64) {
            T s0 = (T)0, s1 = (T)0, s2 = (T)0, s3 = (T)0;
#pragma unroll
            for (int l = 0; l < 64; l += 4) {
                s0 += red[tid][l];
                s1 += red[tid][l + 1];
                s2 += red[tid][l + 2];
                s3 += red[tid][l + 3];
            }
            zk[tid] = ld_sc1(&w[64 * K + tid]) - ((s0 + s1) + (s2 + s3));
        }
        __syncthreads();
        {  // x_K = Dinv_K^T z, as nd_backward
            const T* g = Dinv + nd.dinv_off + (int64_t)K * 4096 + (int64_t)lane * 64 + 16 * wv;
            T gv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) gv[j] = g[j];
            T x0 = (T)0, x1 = (T)0;
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                x0 = fma_t(gv[j], zk[16 * wv + j], x0);
                x1 = fma_t(gv[j + 1], zk[16 * wv + j + 1], x1);
            }
            part[wv][lane] = x0 + x1;
        }
        __syncthreads();
        if (tid < 64) {
            const T x = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
            st_sc1(&w[64 * K + tid], x);
            if (64 * K + tid < nd.np) xp[(int64_t)col * n + nd.start + 64 * K + tid] = x;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __hip_atomic_store(&xf[K], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tk = atomicAdd(ticket, 1);
        }
        __syncthreads();
        t = __builtin_amdgcn_readfirstlane(tk);
    }
}

// nd_solve's three pieces, which bsm_nd_factor (below) calls one by one: the
// plan (nd_obtain_plan), the numeric factor (nd_stage_fronts, then
// nd_factor_levels) and the solves (nd_solve_passes).

// The solves' temporaries, from the thread's cache (no hipFree per solve):
// the right-hand sides in the new order, the solve vectors, and the passes'
// flags and tickets followed by one status word (for a solve on a kept
// factor, whose own flags and status are gone)
struct NdSolveTmp {
    DBuf bpb, vb, tfl;
    int64_t n_pf = 0;  // flags per pass: one per node, column, pivot tile
    size_t n_tf = 0;   // forward flags, backward flags, tickets
};
template <typename T>
int nd_solve_tmp(const NdCached& C, int64_t N, uint64_t k, hipStream_t s, NdSolveTmp& t) {
    t.n_pf = (C.dinv_elems / 4096) * (int64_t)k;
    t.n_tf = 2 * (size_t)t.n_pf + 2 * (size_t)C.n_levels;
    BSM_TRY(t.bpb.alloc((size_t)N * k * sizeof(T), s));
    BSM_TRY(t.vb.alloc((size_t)std::max<int64_t>(C.vtot, 1) * k * sizeof(T), s));
    BSM_TRY(t.tfl.alloc((t.n_tf + 1) * sizeof(int), s));
    return BSM_OK;
}

// The numeric factor, first half: the flags cleared and the fronts' input
// staged (the plain pipeline: zeroed, A assembled, the padding pivots set; the
// default one: A's values into the per-tile lists' order, in avb). av: A's
// values as T (a->vals, or their conversion into the factor's dtype)
template <typename T>
int nd_stage_fronts(const bsm_csr* a, const T* av, const NdCached& C, int64_t N, T* F, int* flags, size_t nfl, T* avb,
                    hipStream_t s) {
    const NdPtrs p = nd_ptrs(C);
    BSM_HIP_TRY(hipMemsetAsync(flags, 0, nfl * sizeof(int), s));
    if (C.lay.plain) {
        if (C.n_tiles) {
            nd_zero_tiles<T><<<(unsigned)C.n_tiles, 256, 0, s>>>(p.nodes, p.tiles, F);
            BSM_HIP_TRY(hipGetLastError());
        }
        nd_assemble<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, a->row_ptr, a->col, av, p.pinv, p.owner, p.nodes, p.st, F);
        BSM_HIP_TRY(hipGetLastError());
        nd_pad_pivots<T><<<(unsigned)C.nn, 64, 0, s>>>(p.nodes, F);
        BSM_HIP_TRY(hipGetLastError());
    } else if (C.n_aent > 0) {  // A's values in the per-tile lists' order
        nd_aent_vals<T><<<nd_blocks(C.n_aent, 256), 256, 0, s>>>(C.n_aent, C.aent.as<int64_t>(), av, avb);
        BSM_HIP_TRY(hipGetLastError());
    }
    return BSM_OK;
}

// The numeric factor, second half: nd_factor level by level (and the plain
// pipeline's extend-add after each). flags: the tile flags, then a ticket per
// level, then the status word. fV / fbp: the forward solve folded in (one
// right-hand side), else null. stamps: BSM_ND_STAMPS's counters, else null.
template <typename T>
int nd_factor_levels(const NdCached& C, const NdGrid& g, T* F, T* Dinv, int* flags, const T* avb, T* fV,
                     const T* fbp, unsigned long long* stamps, hipStream_t s) {
    const NdPtrs p = nd_ptrs(C);
    const bool plain = C.lay.plain;
    int* const d_tickets = flags + C.n_flags;
    int* const d_status = d_tickets + C.n_levels;
    const int64_t* const d_aent = plain ? nullptr : C.aent.as<int64_t>();
    const T* const d_av = plain ? nullptr : avb;
    const int2* const d_tq = plain ? nullptr : C.tq.as<int2>();
    const NdPull* const d_pd = plain ? nullptr : C.pdesc.as<NdPull>();
    for (int32_t lv = 0; lv < C.n_levels; ++lv) {
        const int64_t t0 = C.tiles_off[(size_t)lv], nt = C.tiles_off[(size_t)lv + 1] - t0;
        if (nt > 0)
            BSM_TRY(NdHost<T>::factor_launch(p, g, p.tiles + t0, nt, F, Dinv, flags, d_tickets + lv, d_status, fV, fbp, d_aent,
                                        d_av, d_tq ? d_tq + t0 : nullptr, d_pd ? d_pd + 2 * t0 : nullptr,
                                        stamps ? stamps + ND_NSTAMP * lv : nullptr, s));
        const int64_t e0 = C.ext2_off[(size_t)lv], ne = C.ext2_off[(size_t)lv + 1] - e0;
        if (ne > 0) {  // the plain pipeline: this level's update blocks into the parents' fronts
            nd_extend2<T><<<nd_blocks(ne, 4), 256, 0, s>>>(p.nodes, p.ext2 + e0, ne, p.ri, F);
            BSM_HIP_TRY(hipGetLastError());
        }
    }
    return BSM_OK;
}

// The solves on a finished factor (F, Dinv): b into the new order, the
// forward levels bottom-up, the backward levels top-down, x back into A's
// order. folded: nd_factor has formed the forward solve already (t.bpb and
// t.vb hold its b and y), so only the backward pass runs. system (bsm.h's
// BSM_ND_SYS_*): A, both passes; L, the forward pass alone (L y = b); LT, the
// backward pass alone (L^T x = y), b and x then in the NEW order (no
// permutation). Between the passes y lives in V, over each front's pivots:
// the L system copies it out to bp after the forward levels (nd_y_out), the
// LT system loads it from bp before the backward levels (nd_y_in).
template <typename T>
int nd_solve_passes(const NdCached& C, const NdOpts& opt, const NdGrid& g, int64_t N, uint64_t k, const T* F,
                    const T* Dinv, const void* b_dev, void* x_dev, NdSolveTmp& t, bool folded, int* d_status,
                    hipStream_t s, int system = BSM_ND_SYS_A) {
    const NdPtrs p = nd_ptrs(C);
    T* const bp = t.bpb.as<T>();
    T* const V = t.vb.as<T>();
    const bool fwd = !folded && system != BSM_ND_SYS_LT, bwd = system != BSM_ND_SYS_L;
    const int64_t* const perm = system == BSM_ND_SYS_A ? p.perm : nullptr;
    if (!folded) {
        nd_gather<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, (int64_t)k, perm, static_cast<const T*>(b_dev), bp);
        BSM_HIP_TRY(hipGetLastError());
    }
    BSM_HIP_TRY(hipMemsetAsync(t.tfl.p, 0, (t.n_tf + 1) * sizeof(int), s));
    int* const d_yf = t.tfl.as<int>();
    int* const d_xf = d_yf + t.n_pf;
    int* const d_ftk = d_xf + t.n_pf;
    int* const d_btk = d_ftk + C.n_levels;
    if (fwd)
        BSM_TRY(NdHost<T>::forward_levels(C, opt, g, N, k, F, Dinv, bp, V, d_yf, d_ftk, d_status, s, C.n_levels));
    if (system == BSM_ND_SYS_L && C.nn > 0) {
        nd_y_out<T><<<dim3((unsigned)C.nn, (unsigned)k), 256, 0, s>>>(p.nodes, N, V, C.vtot, bp);
        BSM_HIP_TRY(hipGetLastError());
    }
    stage_mark("nd_forward", s);
    if (system == BSM_ND_SYS_LT && C.nn > 0) {
        nd_y_in<T><<<dim3((unsigned)C.nn, (unsigned)k), 256, 0, s>>>(p.nodes, N, bp, V, C.vtot);
        BSM_HIP_TRY(hipGetLastError());
    }
    if (bwd)
        BSM_TRY(NdHost<T>::backward_levels(C, opt, g, N, k, F, Dinv, bp, V, d_xf, d_btk, d_status, s, C.n_levels));
    stage_mark("nd_backward", s);
    nd_scatter<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, (int64_t)k, perm, bp, static_cast<T*>(x_dev));
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

template <typename T>
int nd_solve(const bsm_csr* a, uint64_t k, uint64_t n, const void* b_dev, void* x_dev, hipStream_t s) {
    stage_reset(s);
    const int64_t N = (int64_t)n;
    const NdOpts opt = nd_options();
    const bool shared = opt.shared;
    // Two pipelines. Default: every factor tile stages its
    // own entries of A from the plan's per-tile lists and pulls its
    // children's update blocks through the task's descriptors, a diagonal
    // tile skips its padding panels, and with one right-hand side the
    // forward solve is folded into the factor. Plain (BSM_ND_PLAIN=1, and a
    // pattern whose entries do not fit the lists' 32-bit offsets): the
    // fronts zeroed, A assembled into them, nd_factor on F alone, one
    // nd_extend2 launch after each level, the forward solve as its own pass.
    // The factor has the same bits either way.
    NdLay lay = opt.lay;
    lay.plain = lay.plain || a->nnz >= ((uint64_t)1 << 31);
    const bool plain = lay.plain;
    std::shared_ptr<NdCached> pc;
    // opt.keep: the fronts will be a new plan's own (allocated while the layout runs)
    BSM_TRY(nd_obtain_plan(a, opt, lay, opt.keep ? sizeof(T) : 0, s, pc));
    NdCached& C = *pc;
    nd_trace(opt, C, N, sizeof(T));
    // BSM_ND_FOLD=0: the forward solve as its own pass over L after the
    // factor. By default, with one right-hand side, the default pipeline's
    // diagonal tiles form y and the update vectors themselves
    const bool fold = k == 1 && !plain && opt.fold;
    // numeric storage: the plan's own buffers when this solve may hold them
    std::unique_lock<std::mutex> num_lock(C.num_mu, std::defer_lock);
    const bool keep = opt.keep && num_lock.try_lock();
    DBuf own_fr, own_dv, own_fl;
    DBuf& fr = keep ? C.fr : own_fr;
    DBuf& dv = keep ? C.dv : own_dv;
    DBuf& fl = keep ? C.fl : own_fl;
    const size_t fr_b = (size_t)C.f_elems * sizeof(T), dv_b = (size_t)std::max<int64_t>(C.dinv_elems, 1) * sizeof(T);
    const size_t nfl = (size_t)C.n_flags + (size_t)C.n_levels + 2;
    // a plan serves one dtype per handle; sizes match after the first solve
    BSM_TRY(nd_alloc_numeric(fr, fr_b, &C));
    // BSM_ND_POISON=1 (tests): the fronts start as NaN (nothing may read unzeroed tiles)
    if (opt.poison) BSM_HIP_TRY(hipMemsetAsync(fr.p, 0xff, fr_b, s));
    BSM_TRY(nd_alloc_numeric(dv, dv_b, &C));
    BSM_TRY(nd_alloc_numeric(fl, nfl * sizeof(int), &C));
    if (keep) C.kept_bytes = fr.bytes + dv.bytes + fl.bytes;
    // everything that can fail before the first launch: the occupancy
    // queries and the solves' temporaries (an error return after
    // the launches would release num_mu under running kernels)
    NdGrid g;
    BSM_TRY(NdHost<T>::grid(true, true, g));
    DBuf avb;  // from the thread's cache of temporaries, as the solves' (no hipFree per solve)
    NdSolveTmp tmp;
    if (!plain) BSM_TRY(avb.alloc((size_t)std::max<int64_t>(C.n_aent, 1) * sizeof(T), s));
    if (k > 0) BSM_TRY(nd_solve_tmp<T>(C, N, k, s, tmp));
    DBuf& bpb = tmp.bpb;
    DBuf& vb = tmp.vb;
    NdDrainOnError drain{s, true};  // destroyed before num_lock is released
    int* d_flags = fl.as<int>();
    int* d_status = d_flags + C.n_flags + C.n_levels;
    T* F = fr.as<T>();
    BSM_TRY(nd_stage_fronts<T>(a, static_cast<const T*>(a->vals), C, N, F, d_flags, nfl, avb.as<T>(), s));
    stage_mark("nd_assemble", s);
    // BSM_ND_STAMPS=1: nd_factor's per-level cycle stamps, printed after the solve
    DBuf stamps;
    if (opt.stamps) {
        BSM_TRY(stamps.alloc((size_t)C.n_levels * ND_NSTAMP * sizeof(unsigned long long)));
        BSM_HIP_TRY(hipMemsetAsync(stamps.p, 0, (size_t)C.n_levels * ND_NSTAMP * sizeof(unsigned long long), s));
    }
    if (fold) {  // b into the new order before the factor; V's padding rows stay 0
        nd_gather<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, (int64_t)k, nd_ptrs(C).perm, static_cast<const T*>(b_dev),
                                                       bpb.as<T>());
        BSM_HIP_TRY(hipGetLastError());
        BSM_HIP_TRY(hipMemsetAsync(vb.p, 0, (size_t)std::max<int64_t>(C.vtot, 1) * sizeof(T), s));
    }
    T* const fV = fold ? vb.as<T>() : nullptr;
    const T* const fbp = fold ? bpb.as<T>() : nullptr;
    BSM_TRY(nd_factor_levels<T>(C, g, F, dv.as<T>(), d_flags, avb.as<T>(), fV, fbp, stamps.as<unsigned long long>(), s));
    stage_mark("nd_factor", s);
    if (k > 0) BSM_TRY(nd_solve_passes<T>(C, opt, g, N, k, F, dv.as<T>(), b_dev, x_dev, tmp, fold, d_status, s));
    const int rc = nd_status_end(true, d_status, drain, "nd_copy_out", s);
    if (stamps.p && !drain.armed) {  // the stream has been waited for: the stamps first, then a refusal
        std::vector<unsigned long long> h((size_t)C.n_levels * ND_NSTAMP);
        BSM_HIP_TRY(hipMemcpy(h.data(), stamps.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int32_t lv = 0; lv < C.n_levels; ++lv) {
            const unsigned long long* v = &h[(size_t)lv * ND_NSTAMP];
            const double nt = v[7] ? (double)v[7] : 1.0;
            fprintf(stderr,
                    "[bsm nd stamps] level %2d: %6llu tiles (prod %llu, diag %llu, trsm %llu, upd %llu); cycles per "
                    "tile: wait %.0f, products %.0f, diag %.0f, trsm %.0f, update %.0f, drain %.0f; workgroup total "
                    "%.0f per tile\n",
                    lv, v[7], v[8], v[9], v[10], v[11], v[1] / nt, (v[2] - v[1]) / nt, v[3] / nt, v[4] / nt,
                    v[5] / nt, v[6] / nt, v[0] / nt);
            if (v[16])
                fprintf(stderr,
                        "[bsm nd stamps] level %2d: pull into %llu tiles, cycles per pulling tile: tile and first "
                        "child's loads %.0f, its additions %.0f, second child %.0f, read-back %.0f\n",
                        lv, v[16], (double)v[12] / v[16], (double)v[13] / v[16], (double)v[14] / v[16],
                        (double)v[15] / v[16]);
        }
    }
    if (rc != BSM_OK) return rc;
    if (keep && shared) {  // the cached plans' kept storage within its budget (this plan's stays)
        num_lock.unlock();
        nd_cache_trim(opt.cache_mb << 20, &C);
    }
    return BSM_OK;
}

// ---- the kept factor (bsm_nd_factor) ----------------------------------------
// The export walks L out of the fronts' pivot panels. Column c < np of a
// front is column start + c of L (new order): front rows c .. np - 1 (L rows
// start + r), then front rows np_pad + a, a < m (L rows st[a]); both runs
// ascending and all >= the column, so a column of L is a row of L^T already
// in order, the diagonal first. One wave per column, lanes striding down it
// (contiguous in the column-major front). Never read: the padding rows and
// columns [np, np_pad), a pivot tile above its diagonal, the update block
// (the default pipeline leaves them undefined). Exact zeros are dropped as
// Csr::insert drops them (sparse.rs:229); the diagonal (> 0 in a finished
// factor) is always kept.

// entry i of L's column q = nd.start + c: its value and its row in L
template <typename T>
__device__ __forceinline__ T nd_col_entry(const NdDev& nd, const T* __restrict__ colp, const int32_t* __restrict__ st,
                                          int c, int i, int32_t* row) {
    const int own = nd.np - c;  // the pivot rows c .. np - 1
    const int fr = i < own ? c + i : nd.np_pad + (i - own);
    *row = i < own ? (int32_t)(nd.start + c + i) : st[nd.st_off + (i - own)];
    return colp[fr];
}

// len[q] = stored entries of column q of L (row q of L^T)
template <typename T>
__global__ __launch_bounds__(256) void nd_export_count(int64_t n, const int32_t* __restrict__ owner,
                                                       const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                                       const T* __restrict__ F, int32_t* __restrict__ len) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n) return;  // wave-uniform
    const NdDev& nd = nodes[owner[q]];
    const int c = (int)(q - nd.start);
    const T* const colp = F + nd.foff + (int64_t)c * nd.ld;
    const int total = nd.np - c + nd.m;
    int cnt = 0;
    for (int base = 0; base < total; base += 64) {
        const int i = base + lane;
        bool keep = false;
        if (i < total) {
            int32_t row;
            keep = i == 0 || nd_col_entry<T>(nd, colp, st, c, i, &row) != (T)0;
        }
        cnt += __popcll(__ballot(keep));
    }
    if (lane == 0) len[q] = cnt;
}

// the same walk again, writing row q of L^T at rp[q]: the place of a kept
// entry is the wave's running offset plus the kept lanes below it
template <typename T>
__global__ __launch_bounds__(256) void nd_export_fill(int64_t n, const int32_t* __restrict__ owner,
                                                      const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                                      const T* __restrict__ F, const int64_t* __restrict__ rp,
                                                      int32_t* __restrict__ col, T* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n) return;  // wave-uniform
    const NdDev& nd = nodes[owner[q]];
    const int c = (int)(q - nd.start);
    const T* const colp = F + nd.foff + (int64_t)c * nd.ld;
    const int total = nd.np - c + nd.m;
    int64_t run = rp[q];
    for (int base = 0; base < total; base += 64) {
        const int i = base + lane;
        bool keep = false;
        int32_t row = 0;
        T v = (T)0;
        if (i < total) {
            v = nd_col_entry<T>(nd, colp, st, c, i, &row);
            keep = i == 0 || v != (T)0;
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int64_t at = run + __popcll(mask & ((1ull << lane) - 1));
            col[at] = row;
            val[at] = v;
        }
        run += __popcll(mask);
    }
}

// log det A = 2 sum log L_qq over the n real pivots (a padding pivot in [np,
// np_pad) is never read). Pass 1: a thread takes pivots q in a grid-stride
// loop, finds the front through owner[q] and adds log of its diagonal entry
// in f64 (for both dtypes); the wave's sum by shuffles, the workgroup's
// through LDS: one partial per workgroup. Pass 2 (one workgroup) adds the
// partials in index order. No floating-point atomics, and the grid depends
// on n alone (nd_logdet_blocks), so the sum's order, hence its bits, is the
// same on every call and every device.
constexpr int ND_LOGDET_MAX_BLOCKS = 256;
inline unsigned nd_logdet_blocks(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, ND_LOGDET_MAX_BLOCKS));
}
template <typename T>
__global__ __launch_bounds__(256) void nd_logdet_partial(int64_t n, const int32_t* __restrict__ owner,
                                                         const NdDev* __restrict__ nodes, const T* __restrict__ F,
                                                         double* __restrict__ part) {
    __shared__ double wsum[4];
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
        const NdDev& nd = nodes[owner[q]];
        const int64_t c = q - nd.start;
        acc += log((double)F[nd.foff + c * nd.ld + c]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}
// out[0] = 2 (part[0] + part[1] + ... + part[nb - 1]), left to right
__global__ __launch_bounds__(ND_LOGDET_MAX_BLOCKS) void nd_logdet_sum(int nb, const double* __restrict__ part,
                                                                      double* __restrict__ out) {
    __shared__ double sh[ND_LOGDET_MAX_BLOCKS];
    if ((int)threadIdx.x < nb) sh[threadIdx.x] = part[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < nb; ++i) t += sh[i];
        out[0] = 2.0 * t;
    }
}

// The numeric factor of a into the handle's own fronts, on its plan C: what
// create and refactor share. f.valid is false from the first launch until the
// status word says the factor is whole.
template <typename T>
int nd_factor_numeric_t(const bsm_csr* a, bsm_nd_factor& f, const NdCached& C, const NdOpts& opt, hipStream_t s) {
    const int64_t N = (int64_t)a->rows;
    const size_t nfl = (size_t)C.n_flags + (size_t)C.n_levels + 2;
    NdGrid g;
    BSM_TRY(NdHost<T>::grid(true, false, g));
    DBuf fl, avb, cvt;  // temporaries: the flags, tickets and status; A's values by tile; A's values as T
    BSM_TRY(fl.alloc(nfl * sizeof(int), s));
    const bool convert = a->dtype != f.dtype;  // bsm_nd_factor_create_as: the factor's dtype is not the matrix's
    if (convert) BSM_TRY(cvt.alloc((size_t)std::max<uint64_t>(a->nnz, 1) * sizeof(T), s));
    if (!C.lay.plain) BSM_TRY(avb.alloc((size_t)std::max<int64_t>(C.n_aent, 1) * sizeof(T), s));
    NdDrainOnError drain{s, true};  // the temporaries go back to the thread's cache only after the kernels
    f.valid = false;
    f.nnz_l = 0;
    f.stale_blocks = false;  // every front's update block is written again
    // BSM_ND_POISON=1 (tests): the fronts start as NaN (the export may not read what the factor did not write)
    if (opt.poison) BSM_HIP_TRY(hipMemsetAsync(f.fr.p, 0xff, f.fr.bytes, s));
    int* const d_flags = fl.as<int>();
    if (convert) BSM_TRY(convert_values(a->dtype, f.dtype, a->nnz, a->vals, cvt.p, s));
    const T* const av = convert ? cvt.as<T>() : static_cast<const T*>(a->vals);
    BSM_TRY(nd_stage_fronts<T>(a, av, C, N, f.fr.as<T>(), d_flags, nfl, avb.as<T>(), s));
    stage_mark("nd_assemble", s);
    BSM_TRY(nd_factor_levels<T>(C, g, f.fr.as<T>(), f.dv.as<T>(), d_flags, avb.as<T>(), (T*)nullptr,
                                (const T*)nullptr, nullptr, s));
    stage_mark("nd_factor", s);
    BSM_TRY(nd_status_end(true, d_flags + C.n_flags + C.n_levels, drain, nullptr, s));
    f.valid = true;
    return BSM_OK;
}

// f.schur_idx (non-empty): the plan whose root owns those vertices, the factor's alone (§4.9o)
template <typename T>
int nd_factor_create_t(const bsm_csr* a, bsm_nd_factor& f, hipStream_t s) {
    stage_reset(s);
    const int64_t N = (int64_t)a->rows;
    const NdOpts opt = nd_options();
    NdLay lay = opt.lay;
    lay.plain = lay.plain || a->nnz >= ((uint64_t)1 << 31);  // as nd_solve
    std::shared_ptr<NdCached> pc;
    const std::vector<int64_t> last(f.schur_idx.begin(), f.schur_idx.end());
    // no kept storage asked for on a new plan: the factor's fronts are its own
    BSM_TRY(nd_obtain_plan(a, opt, lay, 0, s, pc, &last));
    NdCached& C = *pc;
    if (!last.empty()) {
        // each vertex's place among the root's columns (its rank in the sorted set), then the inverse map
        const size_t m = last.size();
        std::vector<int32_t> ord(m), map(2 * m);
        for (size_t i = 0; i < m; ++i) ord[i] = (int32_t)i;
        std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return last[(size_t)x] < last[(size_t)y]; });
        for (size_t r = 0; r < m; ++r) {
            map[(size_t)ord[r]] = (int32_t)r;
            map[m + r] = ord[r];
        }
        BSM_TRY(f.schur_map.alloc(2 * m * sizeof(int32_t)));
        BSM_HIP_TRY(hipMemcpyAsync(f.schur_map.p, map.data(), 2 * m * sizeof(int32_t), hipMemcpyHostToDevice, s));
        BSM_HIP_TRY(hipStreamSynchronize(s));  // `map` goes away
    }
    nd_trace(opt, C, N, sizeof(T));
    const size_t fr_b = (size_t)C.f_elems * sizeof(T), dv_b = (size_t)std::max<int64_t>(C.dinv_elems, 1) * sizeof(T);
    BSM_TRY(nd_alloc_numeric(f.fr, fr_b, nullptr));
    BSM_TRY(nd_alloc_numeric(f.dv, dv_b, nullptr));
    {  // the pattern a refactorisation is compared against: the copy the plan's other holders share, else a new one
        std::lock_guard<std::mutex> pl(C.pat_mu);
        f.pattern = C.pattern.lock();
        if (!f.pattern) {
            BSM_TRY(nd_pattern_copy(a, s, f.pattern));
            C.pattern = f.pattern;
        }
    }
    f.nnz = a->nnz;
    BSM_TRY(nd_factor_numeric_t<T>(a, f, C, opt, s));
    f.plan = pc;
    return BSM_OK;
}

template <typename T>
int nd_factor_logdet_t(const bsm_nd_factor& f, double* logdet, hipStream_t s) {
    const int64_t N = (int64_t)f.n;
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const unsigned nb = nd_logdet_blocks(N);
    DBuf part;  // the partials, then the result
    BSM_TRY(part.alloc(((size_t)nb + 1) * sizeof(double), s));
    NdDrainOnError drain{s, true};
    nd_logdet_partial<T><<<nb, 256, 0, s>>>(N, p.owner, p.nodes, f.fr.as<T>(), part.as<double>());
    BSM_HIP_TRY(hipGetLastError());
    nd_logdet_sum<<<1, ND_LOGDET_MAX_BLOCKS, 0, s>>>((int)nb, part.as<double>(), part.as<double>() + nb);
    BSM_HIP_TRY(hipGetLastError());
    double v = 0.0;
    BSM_HIP_TRY(read_dev(&v, part.as<double>() + nb, sizeof(double), s));
    drain.armed = false;
    *logdet = v;
    return BSM_OK;
}

template <typename T>
int nd_factor_solve_t(const bsm_nd_factor& f, int system, uint64_t k, const void* b_dev, void* x_dev, hipStream_t s) {
    stage_reset(s);
    const int64_t N = (int64_t)f.n;
    const NdOpts opt = nd_options();
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    NdGrid g;
    BSM_TRY(NdHost<T>::grid(false, true, g));
    NdSolveTmp tmp;
    BSM_TRY(nd_solve_tmp<T>(C, N, k, s, tmp));
    NdDrainOnError drain{s, true};  // the handle's mutex is released after this guard runs
    int* const d_status = tmp.tfl.as<int>() + tmp.n_tf;  // cleared with the passes' flags
    BSM_TRY(nd_solve_passes<T>(C, opt, g, N, k, f.fr.as<T>(), f.dv.as<T>(), b_dev, x_dev, tmp, false, d_status, s,
                               system));
    return nd_status_end(false, d_status, drain, "nd_copy_out", s);
}

// L^T (new order) out of the fronts: count, scan, fill
template <typename T>
int nd_factor_lstar_t(const bsm_nd_factor& f, bsm_csr** out, hipStream_t s) {
    const int64_t N = (int64_t)f.n;
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    DBuf len, rp, ws;
    const uint64_t ws_b = scan_workspace_bytes((uint64_t)N);
    BSM_TRY(len.alloc((size_t)N * sizeof(int32_t), s));
    BSM_TRY(rp.alloc((size_t)(N + 1) * sizeof(int64_t), s));
    BSM_TRY(ws.alloc(ws_b, s));
    NdDrainOnError drain{s, true};
    nd_export_count<T><<<nd_blocks(N, 4), 256, 0, s>>>(N, p.owner, p.nodes, p.st, f.fr.as<T>(), len.as<int32_t>());
    BSM_HIP_TRY(hipGetLastError());
    BSM_TRY(exclusive_scan_i32_to_i64(len.as<int32_t>(), rp.as<int64_t>(), (uint64_t)N, ws.p, ws_b, s));
    int64_t nnz = 0;
    BSM_HIP_TRY(read_dev(&nnz, rp.as<int64_t>() + N, sizeof(int64_t), s));
    bsm_csr* t = nullptr;
    BSM_TRY(csr_alloc(&t, f.dtype, (uint64_t)N, (uint64_t)N, (uint64_t)nnz));
    hipError_t e = hipMemcpyAsync(t->row_ptr, rp.p, (size_t)(N + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) {
        nd_export_fill<T><<<nd_blocks(N, 4), 256, 0, s>>>(N, p.owner, p.nodes, p.st, f.fr.as<T>(), t->row_ptr, t->col,
                                                          static_cast<T*>(t->vals));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error("nd factor export: %s", hipGetErrorString(e));
        (void)hipStreamSynchronize(s);
        bsm_csr_free(t);
        return BSM_ERR_HIP;
    }
    drain.armed = false;
    f.nnz_l = (uint64_t)nnz;
    *out = t;
    return BSM_OK;
}

}  // namespace

// the current device's NdGrid: the occupancy of the kernels this file launches
template <typename T>
int NdHost<T>::grid(bool factor, bool solves, NdGrid& g) {
    int dev = 0;
    BSM_HIP_TRY(hipGetDevice(&dev));
    BSM_HIP_TRY(hipDeviceGetAttribute(&g.cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (factor) {
        BSM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&g.per_cu, nd_factor<T>, 256, 0));
        BSM_REQUIRE(g.per_cu >= 1, BSM_ERR_UNSUPPORTED, "nd_factor does not fit a CU");
    }
    if (solves) {
        BSM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&g.fper, nd_forward_tiles<T>, 64, 0));
        BSM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&g.bper, nd_backward_tiles<T>, 256, 0));
        BSM_REQUIRE(g.fper >= 1 && g.bper >= 1, BSM_ERR_UNSUPPORTED, "nd solve kernels do not fit a CU");
    }
    return BSM_OK;
}

// nd_factor on nt tasks: a level's (nd_factor_levels) or a partial refactor's selection of one. stamps: else null
template <typename T>
int NdHost<T>::factor_launch(const NdPtrs& p, const NdGrid& g, const int4* tiles, int64_t nt, T* F, T* Dinv,
                             int* flags, int* ticket, int* status, T* fV, const T* fbp, const int64_t* aent,
                             const T* av, const int2* tq, const NdPull* pd, unsigned long long* stamps,
                             hipStream_t s) {
    const int64_t grid = std::min<int64_t>(nt, (int64_t)g.cus * g.per_cu);
    if (stamps)
        nd_factor<T, true><<<(unsigned)grid, 256, 0, s>>>(p.nodes, tiles, nt, F, Dinv, flags, ticket, status, p.ri, fV,
                                                          fbp, aent, av, tq, pd, stamps);
    else
        nd_factor<T><<<(unsigned)grid, 256, 0, s>>>(p.nodes, tiles, nt, F, Dinv, flags, ticket, status, p.ri, fV, fbp,
                                                    aent, av, tq, pd);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// The end of a numeric factor, or of a solve on one (its kernels only time
// out): the status word (null: none) read back, the stream waited for, the
// drain disarmed, `stage` marked (null: none), then the refusals
int nd_status_end(bool factor, const int* d_status, NdDrainOnError& drain, const char* stage, hipStream_t s) {
    int h = 0;
    if (d_status) BSM_HIP_TRY(read_dev(&h, d_status, sizeof(int), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    if (stage) stage_mark(stage, s);
    BSM_REQUIRE(!(h & ST_TIMEOUT), BSM_ERR_HIP, "nd %s: tile hand-off timed out", factor ? "factor" : "solve");
    BSM_REQUIRE(!(factor && (h & ST_NOT_PD)), BSM_ERR_UNSUPPORTED,
                "cholesky: matrix is not positive definite (a pivot is <= 0 or not finite)");
    return BSM_OK;
}

// nd_factor_numeric_t in the factor's dtype, on its plan. The caller holds f.mu.
int nd_factor_numeric(const bsm_csr* a, bsm_nd_factor& f, hipStream_t s) {
    const auto pc = std::static_pointer_cast<NdCached>(f.plan);
    return f.dtype == BSM_F64 ? nd_factor_numeric_t<double>(a, f, *pc, nd_options(), s)
                              : nd_factor_numeric_t<float>(a, f, *pc, nd_options(), s);
}

// The forward levels of a solve, bottom-up over the fronts of levels [0,
// lv_end): b in the new order in bp, y and the update vectors into V. d_yf /
// d_ftk: the pass's cleared flags and tickets, as backward_levels'.
// Levels with fewer (node, column) pairs than CUs run their solves by
// tiles (nd_forward_tiles / nd_backward_tiles: a front's chain of pivot
// tiles on many waves), the others one workgroup per pair (nd_forward /
// nd_backward: less bookkeeping per front). Same bits either way.
// BSM_ND_FWD_TILES / BSM_ND_BWD_TILES = 0: never, 1: every level.
template <typename T>
int NdHost<T>::forward_levels(const NdCached& C, const NdOpts& opt, const NdGrid& g, int64_t N, uint64_t k, const T* F,
                              const T* Dinv, const T* bp, T* V, int* d_yf, int* d_ftk, int* d_status, hipStream_t s,
                              int32_t lv_end) {
    const NdPtrs p = nd_ptrs(C);
    const int64_t fwd_grid = (int64_t)g.cus * g.fper;
    for (int32_t lv = 0; lv < lv_end; ++lv) {
        const int64_t o = C.lvl_off[(size_t)lv], c = C.lvl_off[(size_t)lv + 1] - o;
        if (c <= 0) continue;
        if (opt.fwd_tiles == 1 || (opt.fwd_tiles == 2 && c * (int64_t)k < g.cus)) {
            const int64_t f0 = C.ftask_off[(size_t)lv], nf = C.ftask_off[(size_t)lv + 1] - f0;
            const int64_t grid = std::min<int64_t>(nf * (int64_t)k, fwd_grid);
            if (grid <= 0) continue;  // fronts without rows (no pivots, no front rows)
            nd_forward_tiles<T><<<(unsigned)grid, 64, 0, s>>>(p.nodes, p.ftask + f0, nf, (int)k, N, bp, V, C.vtot, F,
                                                              Dinv, p.ri, d_yf, d_ftk + lv, d_status);
        } else {
            nd_forward<T><<<dim3((unsigned)c, (unsigned)k), 256, 0, s>>>(p.nodes, p.lvl + o, N, bp, V, C.vtot, F, Dinv,
                                                                        p.ri);
        }
        BSM_HIP_TRY(hipGetLastError());
    }
    return BSM_OK;
}

// b (row-major n x k, A's order) into bp (new order, a column after the other), or xp back into x
template <typename T>
int NdHost<T>::permute_launch(bool gather, const NdCached& C, int64_t N, uint64_t k, const T* src, T* dst,
                              hipStream_t s) {
    const NdPtrs p = nd_ptrs(C);
    if (gather) nd_gather<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, (int64_t)k, p.perm, src, dst);
    else nd_scatter<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, (int64_t)k, p.perm, src, dst);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

// The backward levels of a solve, top-down over every front: y over each
// front's pivots in V, x into bp. d_xf / d_btk: the pass's cleared flags (one
// per node, column and pivot tile) and tickets (one per level). Levels with
// fewer (node, column) pairs than CUs run by tiles (forward_levels). Levels
// [0, lv_end): all of them for a solve; without the root's for the Schur
// complement's expansion (§4.9o), which has put x over the root's columns itself.
template <typename T>
int NdHost<T>::backward_levels(const NdCached& C, const NdOpts& opt, const NdGrid& g, int64_t N, uint64_t k,
                               const T* F, const T* Dinv, T* bp, T* V, int* d_xf, int* d_btk, int* d_status,
                               hipStream_t s, int32_t lv_end) {
    const NdPtrs p = nd_ptrs(C);
    const int64_t bwd_grid = (int64_t)g.cus * g.bper;
    for (int32_t lv = lv_end - 1; lv >= 0; --lv) {
        const int64_t o = C.lvl_off[(size_t)lv], c = C.lvl_off[(size_t)lv + 1] - o;
        if (c <= 0) continue;
        if (opt.bwd_tiles == 1 || (opt.bwd_tiles == 2 && c * (int64_t)k < g.cus)) {
            const int64_t b0 = C.btask_off[(size_t)lv], nb = C.btask_off[(size_t)lv + 1] - b0;
            const int64_t grid = std::min<int64_t>(nb * (int64_t)k, bwd_grid);
            if (grid <= 0) continue;  // no pivots on this level
            nd_backward_tiles<T><<<(unsigned)grid, 256, 0, s>>>(p.nodes, p.btask + b0, nb, (int)k, N, bp, V, C.vtot, F,
                                                                Dinv, p.st, d_xf, d_btk + lv, d_status);
        } else {
            nd_backward<T><<<dim3((unsigned)c, (unsigned)k), 256, 0, s>>>(p.nodes, p.lvl + o, N, bp, V, C.vtot, F, Dinv,
                                                                         p.st);
        }
        BSM_HIP_TRY(hipGetLastError());
    }
    return BSM_OK;
}

// One level of the sparse solve (kernels_nd_sparse.hip): cnt active fronts at act, kc columns, forward or backward
template <typename T>
int NdHost<T>::path_launch(bool forward, const NdCached& C, const ReachFront* act, unsigned cnt, unsigned kc, int64_t N,
                           T* bp, T* V, const T* F, const T* Dinv, hipStream_t s) {
    const NdPtrs p = nd_ptrs(C);
    if (forward) nd_forward_path<T><<<dim3(cnt, kc), 256, 0, s>>>(p.nodes, act, N, bp, V, C.vtot, F, Dinv, p.ri);
    else nd_backward_path<T><<<dim3(cnt, kc), 256, 0, s>>>(p.nodes, act, N, bp, V, C.vtot, F, Dinv, p.st);
    BSM_HIP_TRY(hipGetLastError());
    return BSM_OK;
}

template struct NdHost<float>;
template struct NdHost<double>;

int nd_factor_sddmm(const bsm_nd_factor* f, int dtype, uint64_t k, const void* u, const void* v, void* out,
                    hipStream_t s) {
    if (f->n == 0 || f->nnz == 0)  // its checks of dtype and k, no launch
        return sddmm_dispatch(dtype, BSM_SDDMM_SYM_LOWER, 0, 0, 0, nullptr, nullptr, k, u, v, out, s);
    const char* const pb = f->pattern->as<char>();  // immutable for the handle's life: no lock
    return sddmm_dispatch(dtype, BSM_SDDMM_SYM_LOWER, f->n, f->n, f->nnz, (const int64_t*)pb,
                          (const int32_t*)(pb + nd_pattern_rp_bytes((int64_t)f->n)), k, u, v, out, s);
}

int nd_factor_create(const bsm_csr* a, int factor_dtype, bsm_nd_factor** out, hipStream_t s, const uint64_t* idx,
                     uint64_t m) {
    BSM_REQUIRE(a->rows < ((uint64_t)1 << 31), BSM_ERR_UNSUPPORTED, "solve nd: n >= 2^31");
    BSM_REQUIRE(a->dtype == BSM_F64 || a->dtype == BSM_F32, BSM_ERR_INVALID, "solve: f32/f64 only");
    auto f = std::make_unique<bsm_nd_factor>();
    f->schur_idx.assign(idx, idx + m);
    f->dtype = factor_dtype;
    f->src_dtype = a->dtype;
    f->device = a->device;
    f->n = a->rows;
    if (a->rows > 0) {
        int rc = BSM_ERR_INVALID;
        if (factor_dtype == BSM_F64) rc = nd_factor_create_t<double>(a, *f, s);
        else if (factor_dtype == BSM_F32) rc = nd_factor_create_t<float>(a, *f, s);
        else set_error("nd factor: factor_dtype must be BSM_F64 or BSM_F32, got %d", factor_dtype);
        if (rc != BSM_OK) return rc;
    }
    *out = f.release();
    return BSM_OK;
}

// refactor's checks of a matrix against the handle, with its messages
int nd_refactor_matches(const bsm_nd_factor* f, const bsm_csr* a) {
    BSM_REQUIRE(a->device == f->device, BSM_ERR_INVALID,
                "nd factor refactor: device differs (the matrix is on device %d, the factor on %d)", a->device,
                f->device);
    BSM_REQUIRE(a->dtype == f->src_dtype, BSM_ERR_INVALID,
                "nd factor refactor: dtype differs from the factored matrix's (%s was factored, the matrix is %s)",
                f->src_dtype == BSM_F64 ? "f64" : "f32",
                a->dtype == BSM_F64 ? "f64" : a->dtype == BSM_F32 ? "f32" : "not a float");
    BSM_REQUIRE(a->rows == f->n && a->cols == f->n, BSM_ERR_INVALID,
                "nd factor refactor: n differs (the matrix is %llu x %llu, the factor's %llu x %llu)",
                (unsigned long long)a->rows, (unsigned long long)a->cols, (unsigned long long)f->n,
                (unsigned long long)f->n);
    BSM_REQUIRE(f->n == 0 || a->nnz == f->nnz, BSM_ERR_INVALID,
                "nd factor refactor: nnz differs (the matrix has %llu entries, the factored one had %llu)",
                (unsigned long long)a->nnz, (unsigned long long)f->nnz);
    return BSM_OK;
}

// New values on the factor's pattern: the numeric factor again, on the
// handle's plan and into its own storage
int nd_factor_refactor(bsm_nd_factor* f, const bsm_csr* a, hipStream_t s) {
    BSM_TRY(nd_refactor_matches(f, a));  // n == 0: its nnz check passes
    if (f->n == 0) return BSM_OK;
    std::lock_guard<std::mutex> lk(f->mu);
    stage_reset(s);
    BSM_TRY(nd_pattern_same(a, *f, s));
    return nd_factor_numeric(a, *f, s);
}

int nd_factor_refactor_values(bsm_nd_factor* f, int dtype, uint64_t nnz, const void* vals_dev, hipStream_t s) {
    BSM_REQUIRE(dtype == f->src_dtype, BSM_ERR_INVALID,
                "nd factor refactor: dtype differs from the factored matrix's (%s was factored, the values are %s)",
                f->src_dtype == BSM_F64 ? "f64" : "f32",
                dtype == BSM_F64 ? "f64" : dtype == BSM_F32 ? "f32" : "not a float");
    if (f->n == 0) return BSM_OK;
    BSM_REQUIRE(nnz == f->nnz, BSM_ERR_INVALID,
                "nd factor refactor: nnz differs (%llu values given, the factored matrix had %llu entries)",
                (unsigned long long)nnz, (unsigned long long)f->nnz);
    bsm_csr a;  // a view: the kept pattern with the caller's values (nothing is owned, nothing cached on it)
    char* const pb = f->pattern->as<char>();
    a.dtype = dtype;
    a.device = f->device;
    a.rows = a.cols = f->n;
    a.nnz = f->nnz;
    a.row_ptr = (int64_t*)pb;
    a.col = (int32_t*)(pb + nd_pattern_rp_bytes((int64_t)f->n));
    a.vals = const_cast<void*>(vals_dev);
    std::lock_guard<std::mutex> lk(f->mu);
    stage_reset(s);
    return nd_factor_numeric(&a, *f, s);
}

int nd_factor_logdet(const bsm_nd_factor* f, double* logdet, hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    ND_REQUIRE_VALUES(f);
    if (f->n == 0) {
        *logdet = 0.0;
        return BSM_OK;
    }
    return f->dtype == BSM_F64 ? nd_factor_logdet_t<double>(*f, logdet, s) : nd_factor_logdet_t<float>(*f, logdet, s);
}

int nd_factor_solve(const bsm_nd_factor* f, int system, uint64_t k, uint64_t n, const void* b_dev, void* x_dev,
                    hipStream_t s) {
    BSM_REQUIRE(system == BSM_ND_SYS_A || system == BSM_ND_SYS_L || system == BSM_ND_SYS_LT, BSM_ERR_INVALID,
                "nd factor solve: system must be BSM_ND_SYS_A, _L or _LT, got %d", system);
    BSM_REQUIRE(f->n == n, BSM_ERR_PANIC,
                "solve: b has %llu rows but A has %llu (index out of bounds in the reference)", (unsigned long long)n,
                (unsigned long long)f->n);
    std::lock_guard<std::mutex> lk(f->mu);
    ND_REQUIRE_VALUES(f);
    if (n == 0 || k == 0) return BSM_OK;
    return f->dtype == BSM_F64 ? nd_factor_solve_t<double>(*f, system, k, b_dev, x_dev, s)
                               : nd_factor_solve_t<float>(*f, system, k, b_dev, x_dev, s);
}

int nd_factor_perm(const bsm_nd_factor* f, int64_t* perm, hipStream_t s) {
    if (f->n == 0) return BSM_OK;
    const NdCached& C = *std::static_pointer_cast<NdCached>(f->plan);
    BSM_HIP_TRY(hipMemcpyAsync(perm, nd_ptrs(C).perm, (size_t)f->n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    return BSM_OK;
}

int nd_factor_export(const bsm_nd_factor* f, bsm_csr** l, bsm_csr** l_star, hipStream_t s) {
    bsm_csr* ls = nullptr;
    if (f->n == 0) {  // an empty 0 x 0 Csr: row_ptr = {0}
        BSM_TRY(csr_alloc(&ls, f->dtype, 0, 0, 0));
        hipError_t e = hipMemsetAsync(ls->row_ptr, 0, sizeof(int64_t), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("nd factor export: %s", hipGetErrorString(e));
            bsm_csr_free(ls);
            return BSM_ERR_HIP;
        }
    } else {
        std::lock_guard<std::mutex> lk(f->mu);
        ND_REQUIRE_VALUES(f);
        BSM_TRY(f->dtype == BSM_F64 ? nd_factor_lstar_t<double>(*f, &ls, s) : nd_factor_lstar_t<float>(*f, &ls, s));
    }
    if (l) {  // L = (L^T)^T by the stable transpose: rows ascending, the diagonal last
        const int rc = transpose_dispatch(ls, l, s);
        if (rc != BSM_OK) {
            bsm_csr_free(ls);
            return rc;
        }
    }
    if (l_star) *l_star = ls;
    else bsm_csr_free(ls);
    return BSM_OK;
}

// solve (lib.rs:11-24) by the nested-dissection multifrontal factorisation
int solve_dispatch_nd(const bsm_csr* a, uint64_t k, uint64_t n, const void* b_dev, void* x_dev, hipStream_t s) {
    BSM_REQUIRE(a->rows == n, BSM_ERR_PANIC,
                "solve: b has %llu rows but A has %llu (index out of bounds in the reference)", (unsigned long long)n,
                (unsigned long long)a->rows);
    BSM_REQUIRE(n < ((uint64_t)1 << 31), BSM_ERR_UNSUPPORTED, "solve nd: n >= 2^31");
    if (n == 0) return BSM_OK;
    if (a->dtype == BSM_F64) return nd_solve<double>(a, k, n, b_dev, x_dev, s);
    if (a->dtype == BSM_F32) return nd_solve<float>(a, k, n, b_dev, x_dev, s);
    set_error("solve: f32/f64 only");
    return BSM_ERR_INVALID;
}

}  // namespace bsm

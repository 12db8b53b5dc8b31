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
// A kept factor (bsm_nd_factor) also answers the selected inverse, A^-1 on
// the pattern of L + L^T: the same tree walked top-down over a second set of
// fronts (nd_selinv_*). New values at a few entries re-run
// nd_factor on the fronts on those entries' paths to the roots alone
// (nd_partial_*).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "bsm_internal.hpp"
#include "nd.hpp"
#include "partial_rule.hpp"
#include "reach_rule.hpp"
#include "updown_rule.hpp"

namespace bsm {
namespace {

#include "solve_tiles.hpp"

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

// A's entries by tile (once per plan, from the pattern, with nd_assemble's
// addressing): aoff[g] .. aoff[g + 1] are tile g's entries in aent, each
// (CSR index << 12) | (column << 6 | row) within the tile. A counting sort:
// nd_aent_count, nd_scan_tiles, nd_aent_fill (the order within a tile is
// the atomics', but the places are distinct, so the tile they form is not).
__device__ __forceinline__ int64_t nd_aent_key(int64_t i, int64_t j, const int32_t* __restrict__ pinv,
                                               const int32_t* __restrict__ owner, const NdDev* __restrict__ nodes,
                                               const int32_t* __restrict__ st, int32_t* pos) {
    const int64_t pi = pinv[i], pj = pinv[j];
    const int64_t r = pi > pj ? pi : pj, c = pi > pj ? pj : pi;
    const NdDev& nd = nodes[owner[c]];
    const int64_t lc = c - nd.start;
    const int64_t lr = r < nd.start + nd.np ? r - nd.start : nd.np_pad + lower_bound_i32(st + nd.st_off, nd.m, r);
    *pos = (int32_t)((lr & 63) | ((lc & 63) << 6));
    return nd.tile_off + nd_lower_idx(nd.nt, (int32_t)(lr >> 6), (int32_t)(lc >> 6));
}
__global__ __launch_bounds__(256) void nd_aent_count(int64_t n, const int64_t* __restrict__ rp,
                                                     const int32_t* __restrict__ col, const int32_t* __restrict__ pinv,
                                                     const int32_t* __restrict__ owner,
                                                     const NdDev* __restrict__ nodes, const int32_t* __restrict__ st,
                                                     int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        if (col[e] > i) continue;
        int32_t pos;
        atomicAdd(&cnt[nd_aent_key(i, col[e], pinv, owner, nodes, st, &pos)], 1);
    }
}
// cnt[0 .. m) -> its exclusive prefix sums in aoff[0 .. m], one workgroup
__global__ __launch_bounds__(1024) void nd_scan_tiles(int64_t m, const int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ aoff) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t lo = m * t / 1024, hi = m * (t + 1) / 1024;
    int64_t sum = 0;
    for (int64_t g = lo; g < hi; ++g) sum += cnt[g];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan of the chunk sums
        const int64_t v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - sum;
    for (int64_t g = lo; g < hi; ++g) {
        aoff[g] = (int32_t)run;
        run += cnt[g];
    }
    if (t == 1023) aoff[m] = (int32_t)part[1023];
}
__global__ __launch_bounds__(256) void nd_aent_fill(int64_t n, const int64_t* __restrict__ rp,
                                                    const int32_t* __restrict__ col, const int32_t* __restrict__ pinv,
                                                    const int32_t* __restrict__ owner, const NdDev* __restrict__ nodes,
                                                    const int32_t* __restrict__ st, const int32_t* __restrict__ aoff,
                                                    int32_t* __restrict__ cur, int64_t* __restrict__ aent) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        if (col[e] > i) continue;
        int32_t pos;
        const int64_t g = nd_aent_key(i, col[e], pinv, owner, nodes, st, &pos);
        const int32_t slot = atomicAdd(&cur[g], 1);
        aent[aoff[g] + slot] = (e << 12) | pos;
    }
}
// per factor task: its tile's entry range (offset, count)
__global__ __launch_bounds__(256) void nd_task_ranges(int64_t ntasks, const int4* __restrict__ tiles,
                                                      const NdDev* __restrict__ nodes, const int32_t* __restrict__ aoff,
                                                      int2* __restrict__ tq) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntasks) return;
    const int4 tl = tiles[t];
    const NdDev& nd = nodes[tl.x];
    const int64_t g = nd.tile_off + nd_lower_idx(nd.nt, tl.y, tl.z);
    tq[t] = make_int2(aoff[g], aoff[g + 1] - aoff[g]);
}
// per factor task: its children's blocks, first and second in nd_extend2's
// order (NdPull::ra = 0: none), so the tile reads them with its task instead
// of through node -> child -> bounds (tb)
struct NdPull {
    int64_t uoff;   // the child's update block U at F + uoff (U[a][b] at uoff + b ld + a)
    int64_t uvoff;  // its update vector at V + uvoff (the folded forward solve)
    int32_t rcoff, ld, a0, ra, b0, rbn;
};
__global__ __launch_bounds__(256) void nd_task_pull(int64_t ntasks, const int4* __restrict__ tiles,
                                                    const NdDev* __restrict__ nodes, const int32_t* __restrict__ tb,
                                                    NdPull* __restrict__ pd) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntasks) return;
    const int4 tl = tiles[t];
    const NdDev& nd = nodes[tl.x];
    for (int h = 0; h < 2; ++h) {
        NdPull o{0, 0, 0, 0, 0, 0, 0, 0};
        const int c = h == nd.pull_swap ? nd.kid0 : nd.kid1;
        if (c >= 0) {
            const NdDev& cd = nodes[c];
            const int32_t* const tbc = tb + cd.tb_off;
            o.uoff = cd.foff + (int64_t)cd.np_pad * cd.ld + cd.np_pad;
            o.uvoff = cd.voff + cd.np_pad;
            o.rcoff = (int32_t)cd.st_off;
            o.ld = cd.ld;
            o.a0 = tbc[tl.y];
            o.ra = tbc[tl.y + 1] - o.a0;
            o.b0 = tbc[tl.z];
            o.rbn = tbc[tl.z + 1] - o.b0;
            if (o.rbn <= 0) o.ra = 0;
        }
        pd[2 * t + h] = o;
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

inline unsigned nd_blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// the device form of a plan: node descriptors, front rows, tile and task lists
struct NdLayout {
    std::vector<NdDev> dev;
    std::vector<int32_t> st, ri, pinv, owner, lvl_nodes;
    std::vector<int32_t> tb;  // per child: its rows' bounds per tile row of the parent (NdDev::tb_off)
    std::vector<int4> tiles;  // nd_factor's tasks: every front's lower tiles (nd_zero_tiles' too)
    std::vector<int64_t> tiles_off, lvl_off;  // per level
    std::vector<int4> ext2;                    // nd_extend2's tasks (the plain pipeline)
    std::vector<int64_t> ext2_off;             // per level
    std::vector<int2> ftasks;                  // nd_forward_tiles' (node, tile row), I-major
    std::vector<int64_t> ftask_off;            // per level
    std::vector<int2> btasks;                  // nd_backward_tiles' (node, pivot tile), last tiles first
    std::vector<int64_t> btask_off;            // per level
    std::vector<int32_t> parent, level;        // per node, for the host (NdCached::h_parent / h_level)
    std::vector<int32_t> kid0, kid1;           // likewise (NdCached::h_kid0 / h_kid1)
    int64_t f_elems = 0, dinv_elems = 0, n_flags = 0, vtot = 0, n_lower = 0;
};

// The layout's options: part of the plan's keys
struct NdLay {
    int32_t lag = 0;     // the tiles below a diagonal follow it by this many fronts' diagonals (0: by all of them)
    bool plain = false;  // the extend-add by nd_extend2 launches (their task lists are built only then)
    bool operator==(const NdLay& o) const { return lag == o.lag && plain == o.plain; }
};

void nd_layout(const NdPlan& P, NdLay lay, NdLayout& L) {
    const int32_t nn = (int32_t)P.nodes.size();
    L.dev.resize((size_t)nn);
    L.parent.resize((size_t)nn);
    L.level.resize((size_t)nn);
    L.kid0.resize((size_t)nn);
    L.kid1.resize((size_t)nn);
    int64_t st_total = 0;
    for (int32_t i = 0; i < nn; ++i) {
        const NdNode& x = P.nodes[(size_t)i];
        NdDev& d = L.dev[(size_t)i];
        d.np = (int32_t)(x.end - x.start);
        d.npt = (d.np + 63) / 64;
        d.np_pad = 64 * d.npt;
        d.m = (int32_t)x.st.size();
        d.nt = (d.np_pad + d.m + 63) / 64;
        d.ld = 64 * d.nt;
        d.start = x.start;
        d.parent = x.parent;
        L.parent[(size_t)i] = x.parent;
        L.level[(size_t)i] = x.level;
        d.kid0 = x.kids[0];
        d.kid1 = x.kids[1];
        L.kid0[(size_t)i] = x.kids[0];
        L.kid1[(size_t)i] = x.kids[1];
        d.tb_off = -1;
        d.tile_off = (int32_t)L.n_lower;
        L.n_lower += (int64_t)d.nt * (d.nt + 1) / 2;
        d.pull_swap = x.kids[0] >= 0 && x.kids[1] >= 0 &&
                      P.nodes[(size_t)x.kids[1]].level < P.nodes[(size_t)x.kids[0]].level;
        d.foff = L.f_elems;
        L.f_elems += (int64_t)d.ld * d.ld;
        d.dinv_off = L.dinv_elems;
        L.dinv_elems += (int64_t)d.npt * 4096;
        d.flag_off = L.n_flags;
        L.n_flags += (int64_t)d.nt * d.npt;
        d.voff = L.vtot;
        L.vtot += d.ld;
        d.st_off = st_total;
        st_total += d.m;
    }
    int64_t tb_total = 0;  // a child's bounds: its parent's nt + 1 (parents follow their children)
    for (int32_t i = 0; i < nn; ++i)
        if (L.dev[(size_t)i].parent >= 0) {
            L.dev[(size_t)i].tb_off = (int32_t)tb_total;
            tb_total += L.dev[(size_t)L.dev[(size_t)i].parent].nt + 1;
        }
    L.tb.resize((size_t)tb_total);
    L.st.resize((size_t)st_total);
    L.ri.resize((size_t)st_total);
    L.pinv.resize((size_t)P.n);
    L.owner.resize((size_t)P.n);
    // per node, disjoint ranges: on a few threads (the C5 plan's ~1M front
    // rows and 1M columns)
    auto per_node = [&](int32_t lo, int32_t hi) {
        for (int32_t i = lo; i < hi; ++i) {
            const NdNode& x = P.nodes[(size_t)i];
            const NdDev& d = L.dev[(size_t)i];
            for (int64_t q = x.start; q < x.end; ++q) {
                L.owner[(size_t)q] = i;
                L.pinv[(size_t)P.perm[(size_t)q]] = (int32_t)q;
            }
            for (int32_t a = 0; a < d.m; ++a) L.st[(size_t)(d.st_off + a)] = (int32_t)x.st[(size_t)a];
            if (x.parent < 0) continue;
            // a front row of the child is a pivot of the parent or one of its front rows
            const NdNode& px = P.nodes[(size_t)x.parent];
            const NdDev& pd = L.dev[(size_t)x.parent];
            size_t j = 0;
            for (int32_t a = 0; a < d.m; ++a) {
                const int64_t q = x.st[(size_t)a];
                if (q < px.end) {
                    L.ri[(size_t)(d.st_off + a)] = (int32_t)(q - px.start);
                } else {
                    while (px.st[j] < q) ++j;
                    L.ri[(size_t)(d.st_off + a)] = pd.np_pad + (int32_t)j;
                }
            }
            const int32_t* r = L.ri.data() + d.st_off;
            int32_t* t = L.tb.data() + d.tb_off;
            for (int32_t u = 0, a = 0; u <= pd.nt; ++u) {
                while (a < d.m && r[a] < 64 * u) ++a;
                t[u] = a;
            }
        }
    };
    {
        const int nt = (int)std::min<int32_t>(8, std::max<int32_t>(1, nn / 1024));
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; ++t) pool.emplace_back(per_node, (int32_t)((int64_t)nn * t / nt), (int32_t)((int64_t)nn * (t + 1) / nt));
        per_node(0, (int32_t)((int64_t)nn / nt));
        for (auto& th : pool) th.join();
    }
    // per level: the nodes, the factor's tiles (K, node, I) and the extend tasks (slot, node, b)
    std::vector<std::vector<int32_t>> by_level((size_t)P.n_levels);
    for (int32_t i = 0; i < nn; ++i) by_level[(size_t)P.nodes[(size_t)i].level].push_back(i);
    {  // the lists' sizes up front (no regrowth of ~1M-entry vectors)
        size_t zt = 0, ft = 0, bt = 0, ex = 0;
        for (const NdDev& d : L.dev) {
            zt += (size_t)d.nt * (d.nt + 1) / 2;
            ft += (size_t)d.nt;
            bt += (size_t)d.npt;
            ex += d.parent >= 0 && lay.plain ? (size_t)d.m : 0;
        }
        L.tiles.reserve(zt);
        L.ftasks.reserve(ft);
        L.btasks.reserve(bt);
        L.ext2.reserve(ex);
        L.lvl_nodes.reserve((size_t)nn);
    }
    // The levels' lists are independent: built on threads (the leaf level,
    // the largest, sets the time), then concatenated in level order
    struct LevelLists {
        std::vector<int4> tiles, ext2;
        std::vector<int2> ft, bt;
    };
    std::vector<LevelLists> per((size_t)P.n_levels);
    auto build_level = [&](size_t li) {
        const auto& lv = by_level[li];
        LevelLists& o = per[li];
        std::vector<char> used;  // the merge walk's marks, reused
        int32_t kmax = 0;
        for (int32_t i : lv) kmax = std::max(kmax, L.dev[(size_t)i].nt);
        // column K of every front: the diagonal tiles first, then the tiles
        // below (which wait for their diagonal tile's inverse), so the
        // waiting tiles' diagonals are well under way when they are taken.
        // With a lag (lay.lag, in fronts), a front's tiles below the
        // diagonal follow its diagonal tile by `lag` fronts' diagonals
        // instead of all of them: at about the grid's size (512 workgroups)
        // the diagonal is done when they are taken, and the level's other
        // fronts are not held up behind the whole column of diagonals. 0: all
        // of a column's diagonal tiles first (round 5). Either way a tile only
        // waits on earlier tickets.
        std::vector<int32_t> fr;
        for (int32_t K = 0; K < kmax; ++K) {
            fr.clear();
            for (int32_t i : lv)
                if (K < L.dev[(size_t)i].nt) fr.push_back(i);
            const size_t nf = fr.size(), lag = lay.lag ? (size_t)lay.lag : nf;
            for (size_t idx = 0; idx < nf + lag; ++idx) {
                if (idx < nf) o.tiles.push_back(make_int4(fr[idx], K, K, 0));
                if (idx >= lag && idx - lag < nf) {
                    const int32_t i = fr[idx - lag];
                    for (int32_t I = K + 1; I < L.dev[(size_t)i].nt; ++I) o.tiles.push_back(make_int4(i, I, K, 0));
                }
            }
        }
        for (int32_t I = 0; I < kmax; ++I)
            for (int32_t i : lv)
                if (I < L.dev[(size_t)i].nt) o.ft.push_back(make_int2(i, I));
        int32_t pmax = 0;
        for (int32_t i : lv) pmax = std::max(pmax, L.dev[(size_t)i].npt);
        for (int32_t d = 0; d < pmax; ++d)
            for (int32_t i : lv)
                if (d < L.dev[(size_t)i].npt) o.bt.push_back(make_int2(i, L.dev[(size_t)i].npt - 1 - d));
        if (lv.empty() || !lay.plain) return;
        // both slots in one launch: a slot-0 child's columns, each paired with
        // the slot-1 sibling's column landing on the same parent column when
        // that sibling is on this level too, then the sibling's unpaired ones
        const int32_t level = P.nodes[(size_t)lv.front()].level;
        for (int32_t i : lv) {
            const NdNode& x = P.nodes[(size_t)i];
            if (x.parent < 0) continue;
            const NdNode& px = P.nodes[(size_t)x.parent];
            const int32_t sib = px.kids[1 - x.slot];
            const bool pair = sib >= 0 && P.nodes[(size_t)sib].level == level;
            if (pair && x.slot == 1) continue;  // taken with its slot-0 sibling
            const int32_t m0 = L.dev[(size_t)i].m;
            const int32_t* r0 = L.ri.data() + L.dev[(size_t)i].st_off;
            if (!pair) {
                for (int32_t b = 0; b < m0; ++b) o.ext2.push_back(make_int4(i, b, -1, -1));
                continue;
            }
            const int32_t m1 = L.dev[(size_t)sib].m;
            const int32_t* r1 = L.ri.data() + L.dev[(size_t)sib].st_off;
            used.assign((size_t)m1, 0);
            int32_t b1 = 0;
            for (int32_t b = 0; b < m0; ++b) {  // ri ascending on both sides: one merge walk
                while (b1 < m1 && r1[b1] < r0[b]) ++b1;
                const bool hit = b1 < m1 && r1[b1] == r0[b];
                if (hit) used[(size_t)b1] = 1;
                o.ext2.push_back(make_int4(i, b, hit ? sib : -1, hit ? b1 : -1));
            }
            for (int32_t b = 0; b < m1; ++b)
                if (!used[(size_t)b]) o.ext2.push_back(make_int4(sib, b, -1, -1));
        }
    };
    {
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (size_t li; (li = next.fetch_add(1)) < per.size();) build_level(li);
        };
        std::vector<std::thread> pool;
        const int nt = (int)std::min<size_t>(8, per.size());
        for (int t = 1; t < nt; ++t) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
    }
    for (size_t li = 0; li < per.size(); ++li) {
        const auto& lv = by_level[li];
        const LevelLists& o = per[li];
        L.lvl_off.push_back((int64_t)L.lvl_nodes.size());
        L.lvl_nodes.insert(L.lvl_nodes.end(), lv.begin(), lv.end());
        L.tiles_off.push_back((int64_t)L.tiles.size());
        L.tiles.insert(L.tiles.end(), o.tiles.begin(), o.tiles.end());
        L.ftask_off.push_back((int64_t)L.ftasks.size());
        L.ftasks.insert(L.ftasks.end(), o.ft.begin(), o.ft.end());
        L.btask_off.push_back((int64_t)L.btasks.size());
        L.btasks.insert(L.btasks.end(), o.bt.begin(), o.bt.end());
        L.ext2_off.push_back((int64_t)L.ext2.size());
        L.ext2.insert(L.ext2.end(), o.ext2.begin(), o.ext2.end());
    }
    L.lvl_off.push_back((int64_t)L.lvl_nodes.size());
    L.tiles_off.push_back((int64_t)L.tiles.size());
    L.ext2_off.push_back((int64_t)L.ext2.size());
    L.ftask_off.push_back((int64_t)L.ftasks.size());
    L.btask_off.push_back((int64_t)L.btasks.size());
}

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
    // col, as NdCacheEntry::pattern), for whoever still holds it: the
    // cross-handle cache's entry and the kept factors of this plan, which
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

// ---- the plan cache across handles ------------------------------------------
// solve(a: Csr<f32>, b) takes `a` by value (src/lib.rs:11): a drop-in caller
// builds a new Csr, hence a new handle, for every solve, and a plan kept only
// on the handle is rebuilt every time (the host analysis is ~90 % of a cold
// C5 solve). So plans are also kept in a library-wide cache keyed by the
// pattern: (device, n, nnz, leaf) and a 128-bit hash of row_ptr and col
// computed on the device; a hash hit is confirmed by comparing the pattern
// with the entry's own copy of it (no false hit on a collision). Bounded:
// at most BSM_ND_CACHE_ENTRIES entries (default 4, least recently used out)
// and at most BSM_ND_CACHE_MB of kept numeric storage (default 32768) over
// the entries no solve is using; bsm_nd_cache_clear drops them all.

__device__ __forceinline__ uint64_t nd_mix64(uint64_t z) {  // SplitMix64's finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// two sums (mod 2^64) of per-element hashes of (position, value): order-free
// integer sums, so the key does not depend on the grid; one pair of atomics
// per workgroup (one per wave on 4096 workgroups contended for 0.4 ms)
__global__ __launch_bounds__(256) void nd_pattern_hash(const int64_t* __restrict__ rp, int64_t n1,
                                                       const int32_t* __restrict__ col, int64_t nnz,
                                                       unsigned long long* __restrict__ h) {
    __shared__ unsigned long long part[2][4];
    uint64_t s0 = 0, s1 = 0;
    const int64_t total = n1 + nnz;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const uint64_t x = e < n1 ? (uint64_t)rp[e] : (uint64_t)(uint32_t)col[e - n1];
        const uint64_t k = (uint64_t)e * 0x9e3779b97f4a7c15ull;
        s0 += nd_mix64(x ^ k);
        s1 += nd_mix64(x + k + 0x632be59bd9b4e019ull);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += (uint64_t)__shfl_xor((unsigned long long)s0, o);
        s1 += (uint64_t)__shfl_xor((unsigned long long)s1, o);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = s0;
        part[1][threadIdx.x >> 6] = s1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long* p = part[threadIdx.x];
        atomicAdd(&h[threadIdx.x], p[0] + p[1] + p[2] + p[3]);
    }
}

// *diff != 0 when the patterns differ anywhere
__global__ __launch_bounds__(256) void nd_pattern_diff(const int64_t* __restrict__ rpa, const int64_t* __restrict__ rpb,
                                                       int64_t n1, const int32_t* __restrict__ ca,
                                                       const int32_t* __restrict__ cb, int64_t nnz,
                                                       int* __restrict__ diff) {
    bool d = false;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n1 + nnz; e += (int64_t)gridDim.x * 256)
        d |= e < n1 ? rpa[e] != rpb[e] : ca[e - n1] != cb[e - n1];
    if (__any(d) && (threadIdx.x & 63) == 0) atomicOr(diff, 1);
}

struct NdKey {
    int device = 0;
    NdLay lay;
    int64_t n = 0, leaf = 0;
    uint64_t nnz = 0, h0 = 0, h1 = 0;
    bool operator==(const NdKey& o) const {
        return device == o.device && lay == o.lay && n == o.n && leaf == o.leaf && nnz == o.nnz &&
               h0 == o.h0 && h1 == o.h1;
    }
};

struct NdCacheEntry {
    NdKey key;
    uint64_t tick = 0;
    std::shared_ptr<DBuf> pattern;  // row_ptr (n + 1 int64), then col (nnz int32)
    std::shared_ptr<NdCached> plan;
};

struct NdCache {
    std::mutex mu;
    std::vector<NdCacheEntry> entries;
    uint64_t tick = 0, hits = 0, misses = 0;
};

NdCache& nd_cache() {  // never destroyed: no hipFree after the runtime's teardown at exit
    static NdCache* c = new NdCache;
    return *c;
}

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
NdOpts nd_options() {
    auto num = [](const char* name, long long dflt) {
        const char* e = getenv(name);
        return e ? atoll(e) : dflt;
    };
    NdOpts o;
    o.leaf = num("BSM_ND_LEAF", 192);
    o.lay.lag = (int32_t)std::min(0x7ffll, std::max(0ll, num("BSM_ND_LAG", 512)));
    o.lay.plain = num("BSM_ND_PLAIN", 0) == 1;
    o.threads = (int)num("BSM_ND_THREADS", std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())));
    o.cache = num("BSM_ND_CACHE", 1) != 0;
    o.shared = o.cache && num("BSM_ND_SHARED", 1) != 0;
    o.keep = o.cache && num("BSM_ND_KEEP", 1) != 0;
    o.cache_entries = (size_t)num("BSM_ND_CACHE_ENTRIES", 4);
    o.cache_mb = (size_t)num("BSM_ND_CACHE_MB", 32768);
    o.fold = num("BSM_ND_FOLD", 1) != 0;
    o.fwd_tiles = (int)num("BSM_ND_FWD_TILES", 2);
    o.bwd_tiles = (int)num("BSM_ND_BWD_TILES", 2);
    o.poison = num("BSM_ND_POISON", 0) == 1;
    o.hash_zero = num("BSM_ND_HASH_ZERO", 0) == 1;
    o.trace = getenv("BSM_ND_TRACE") != nullptr;
    o.stamps = num("BSM_ND_STAMPS", 0) == 1;
    return o;
}

// The calling thread's page-locked staging buffer (grown on demand, kept for
// the thread's later plans): the pattern's download and the plan's upload
// are direct DMA (~30 MB each at C5) instead of pageable copies.
struct PinnedStage {
    char* buf = nullptr;
    size_t cap = 0;
};
PinnedStage& pinned_stage() {
    thread_local PinnedStage st;
    return st;
}
int pinned_grow(PinnedStage& st, size_t bytes) {
    if (st.cap >= bytes) return BSM_OK;
    if (st.buf) (void)hipHostFree(st.buf);
    st.buf = nullptr;
    st.cap = 0;
    BSM_HIP_TRY(hipHostMalloc((void**)&st.buf, bytes, hipHostMallocDefault));
    st.cap = bytes;
    return BSM_OK;
}
int pinned_staging(size_t bytes, char** out) {
    PinnedStage& st = pinned_stage();
    BSM_TRY(pinned_grow(st, bytes));
    *out = st.buf;
    return BSM_OK;
}

// An upper bound of nd_build_plan's packed plan bytes, from the analysis
// alone (the same arrays as the layout; the merged extend tasks and the
// factor's tasks are at most the child columns and the lower tiles)
size_t nd_plan_bytes_bound(const NdPlan& P, NdLay lay) {
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t sm = 0, zt = 0, ft = 0, bt = 0;
    for (const auto& x : P.nodes) {
        const int64_t npt = (x.end - x.start + 63) / 64, nt = (64 * npt + (int64_t)x.st.size() + 63) / 64;
        sm += x.st.size();
        zt += (size_t)(nt * (nt + 1) / 2);
        ft += (size_t)nt;
        bt += (size_t)npt;
    }
    const size_t nn = P.nodes.size(), n = (size_t)P.n;
    // the children's tile bounds: at most two children of nt + 1 per node
    return al(nn * sizeof(NdDev)) + 2 * al(sm * 4) + 2 * al(n * 4) + al(nn * 4) + al(zt * sizeof(int4)) +
           al(lay.plain ? sm * sizeof(int4) : 0) + al(ft * sizeof(int2)) + al(bt * sizeof(int2)) + al(n * 8) +
           al(2 * (ft + nn) * 4);
}

// es > 0: the fronts (es-byte values) are allocated into C.fr on a helper
// thread while the layout, the packing and the plan's upload run: a first
// solve's 5 GB hipMalloc (C5) then costs no time of its own
int nd_build_plan(const bsm_csr* a, int64_t leaf, NdLay lay, int threads, size_t es, hipStream_t s, NdCached& C) {
    const int64_t N = (int64_t)a->rows;
    // A's pattern to the host for the analysis
    char* stg = nullptr;
    const size_t rp_bytes = ((size_t)(N + 1) * sizeof(int64_t) + 255) / 256 * 256;
    BSM_TRY(pinned_staging(rp_bytes + (size_t)a->nnz * sizeof(int32_t), &stg));
    const int64_t* rp = (const int64_t*)stg;
    const int32_t* cl = (const int32_t*)(stg + rp_bytes);
    BSM_HIP_TRY(hipMemcpyAsync(stg, a->row_ptr, (size_t)(N + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (a->nnz)
        BSM_HIP_TRY(hipMemcpyAsync(stg + rp_bytes, a->col, (size_t)a->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    stage_mark("nd_pattern_d2h", s);
    NdPlan P;
    const int arc = nd_analyse(N, rp, cl, leaf, threads, P);
    BSM_REQUIRE(arc == 0, BSM_ERR_UNSUPPORTED,
                "cholesky: rows must have strictly increasing columns (get_row_complete semantics)");
    std::thread pre;
    struct Join {
        std::thread& t;
        ~Join() {
            if (t.joinable()) t.join();
        }
    } join_pre{pre};
    // on the helper as well (the pattern in the staging buffer is no longer
    // read): the plan's device buffer and the calling thread's page-locked
    // staging buffer, both at an upper bound of the packed plan (~42 MB at
    // C5), so the packing and the upload below allocate nothing
    const size_t plan_bound = nd_plan_bytes_bound(P, lay);
    PinnedStage* const stage = &pinned_stage();
    {
        const int dev0 = a->device;
        pre = std::thread([&C, plan_bound, stage, dev0] {
            if (hipSetDevice(dev0) != hipSuccess) return;
            (void)C.plan.alloc(plan_bound);      // the main thread allocates again if this failed
            (void)pinned_grow(*stage, plan_bound);  // likewise (pinned_staging)
        });
    }
    std::thread pre_fronts;
    struct JoinF {
        std::thread& t;
        ~JoinF() {
            if (t.joinable()) t.join();
        }
    } join_fronts{pre_fronts};
    if (es) {
        int64_t f_elems = 0, dinv_elems = 0, n_flags = 0;  // nd_layout's sums (fronts, inverse tiles, flags)
        for (const auto& x : P.nodes) {
            const int64_t npt = (x.end - x.start + 63) / 64, np_pad = 64 * npt;
            const int64_t nt = (np_pad + (int64_t)x.st.size() + 63) / 64, ld = 64 * nt;
            f_elems += ld * ld;
            dinv_elems += npt * 4096;
            n_flags += nt * npt;
        }
        // the inverse diagonal tiles and the flags too, at the sizes nd_solve
        // asks for (a fresh hipMalloc of ~0.8 GB took ms inside the first
        // solve when the box had just freed memory)
        const size_t dv_bytes = (size_t)std::max<int64_t>(dinv_elems, 1) * es;
        const size_t fl_bytes = ((size_t)n_flags + (size_t)P.n_levels + 2) * sizeof(int);
        const int dev = a->device;
        pre_fronts = std::thread([&C, f_elems, es, dev, dv_bytes, fl_bytes] {
            if (hipSetDevice(dev) != hipSuccess || C.fr.alloc((size_t)f_elems * es) != BSM_OK) return;
            (void)C.dv.alloc(dv_bytes);  // nd_solve allocates again if this failed
            (void)C.fl.alloc(fl_bytes);
        });
    }
    const auto tl0 = host_now();
    NdLayout L;
    C.lay = lay;
    nd_layout(P, lay, L);
    C.ms_layout = ms_since(tl0);
    C.leaf = leaf;
    C.nn = (int32_t)L.dev.size();
    C.n_levels = P.n_levels;
    C.tiles_off = L.tiles_off;
    C.lvl_off = L.lvl_off;
    C.ext2_off = L.ext2_off;
    C.ftask_off = L.ftask_off;
    C.btask_off = L.btask_off;
    C.h_parent = std::move(L.parent);
    C.h_level = std::move(L.level);
    C.h_kid0 = std::move(L.kid0);
    C.h_kid1 = std::move(L.kid1);
    C.f_elems = L.f_elems;
    C.dinv_elems = L.dinv_elems;
    C.n_flags = L.n_flags;
    C.vtot = L.vtot;
    C.n_tiles = L.tiles.size();
    C.n_lower = L.n_lower;
    C.n_ext2 = L.ext2.size();
    C.ms_graph = P.ms_graph;
    C.ms_order = P.ms_order;
    C.ms_symbolic = P.ms_symbolic;
    for (const auto& d : L.dev) C.max_front = std::max<int64_t>(C.max_front, d.ld);
    C.lvl_nt.assign((size_t)P.n_levels, 0);
    C.lvl_npt.assign((size_t)P.n_levels, 0);
    for (int32_t lv = 0; lv < P.n_levels; ++lv)
        for (int64_t q = L.lvl_off[(size_t)lv]; q < L.lvl_off[(size_t)lv + 1]; ++q) {
            const NdDev& d = L.dev[(size_t)L.lvl_nodes[(size_t)q]];
            C.lvl_nt[(size_t)lv] = std::max(C.lvl_nt[(size_t)lv], d.nt);
            C.lvl_npt[(size_t)lv] = std::max(C.lvl_npt[(size_t)lv], d.npt);
        }
    stage_mark("nd_analyse", s);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    C.o_dev = 0;
    C.o_st = C.o_dev + al(L.dev.size() * sizeof(NdDev));
    C.o_ri = C.o_st + al(L.st.size() * 4);
    C.o_pinv = C.o_ri + al(L.ri.size() * 4);
    C.o_owner = C.o_pinv + al(L.pinv.size() * 4);
    C.o_lvl = C.o_owner + al(L.owner.size() * 4);
    C.o_tiles = C.o_lvl + al(L.lvl_nodes.size() * 4);
    C.o_ext2 = C.o_tiles + al(L.tiles.size() * sizeof(int4));
    C.o_ftask = C.o_ext2 + al(L.ext2.size() * sizeof(int4));
    C.o_btask = C.o_ftask + al(L.ftasks.size() * sizeof(int2));
    C.o_perm = C.o_btask + al(L.btasks.size() * sizeof(int2));
    C.o_tb = C.o_perm + al((size_t)N * 8);
    const size_t total = C.o_tb + al(L.tb.size() * 4);
    if (pre.joinable()) pre.join();  // the plan's buffers (device, page-locked staging)
    const auto tp0 = host_now();
    char* hp = nullptr;
    BSM_TRY(pinned_staging(total, &hp));  // the pattern is no longer needed
    // the arrays into the staging buffer in 1-MiB pieces on four threads
    // (~40 MB at C5: one thread's memcpy into fresh pinned pages is ms)
    struct Piece {
        size_t o;
        const char* p;
        size_t b;
    };
    std::vector<Piece> pieces;
    auto put = [&](size_t o, const void* p, size_t b) {
        for (size_t c = 0; c < b; c += (1 << 20))
            pieces.push_back({o + c, static_cast<const char*>(p) + c, std::min<size_t>(b - c, 1 << 20)});
    };
    put(C.o_dev, L.dev.data(), L.dev.size() * sizeof(NdDev));
    put(C.o_st, L.st.data(), L.st.size() * 4);
    put(C.o_ri, L.ri.data(), L.ri.size() * 4);
    put(C.o_pinv, L.pinv.data(), L.pinv.size() * 4);
    put(C.o_owner, L.owner.data(), L.owner.size() * 4);
    put(C.o_lvl, L.lvl_nodes.data(), L.lvl_nodes.size() * 4);
    put(C.o_tiles, L.tiles.data(), L.tiles.size() * sizeof(int4));
    put(C.o_ext2, L.ext2.data(), L.ext2.size() * sizeof(int4));
    put(C.o_ftask, L.ftasks.data(), L.ftasks.size() * sizeof(int2));
    put(C.o_btask, L.btasks.data(), L.btasks.size() * sizeof(int2));
    put(C.o_perm, P.perm.data(), (size_t)N * 8);
    put(C.o_tb, L.tb.data(), L.tb.size() * 4);
    {
        std::atomic<size_t> next{0};
        auto copy = [&] {
            for (size_t i; (i = next.fetch_add(1)) < pieces.size();) memcpy(hp + pieces[i].o, pieces[i].p, pieces[i].b);
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < 4 && (size_t)t < pieces.size(); ++t) pool.emplace_back(copy);
        copy();
        for (auto& th : pool) th.join();
    }
    C.ms_pack = ms_since(tp0);
    if (C.plan.bytes < total) BSM_TRY(C.plan.alloc(total));
    // every buffer before anything is queued: an error return afterwards
    // would free buffers queued kernels still write, and leave the upload
    // reading the staging buffer (the guard drains the stream)
    DBuf cnt;  // per lower tile: A's entries' count, the fill's cursor, then the n_lower + 1 offsets
    if (!lay.plain) {
        BSM_TRY(cnt.alloc((size_t)(3 * C.n_lower + 1) * sizeof(int32_t), s));
        BSM_TRY(C.aent.alloc((size_t)std::max<uint64_t>(a->nnz, 1) * sizeof(int64_t)));
        BSM_TRY(C.tq.alloc((size_t)std::max<size_t>(C.n_tiles, 1) * sizeof(int2)));
        BSM_TRY(C.pdesc.alloc((size_t)std::max<size_t>(C.n_tiles, 1) * 2 * sizeof(NdPull)));
    }
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    BSM_HIP_TRY(hipMemcpyAsync(C.plan.p, hp, total, hipMemcpyHostToDevice, s));
    // The default pipeline's lists. A's entries by tile: count, scan, fill;
    // then the factor tasks' ranges and their children's blocks. (The offsets
    // are 32-bit: nd_solve takes the plain pipeline for a pattern with 2^31
    // or more entries.)
    int32_t na = 0;
    if (!lay.plain) {
        char* pb = C.plan.as<char>();
        const int32_t* d_pinv = (const int32_t*)(pb + C.o_pinv);
        const int32_t* d_owner = (const int32_t*)(pb + C.o_owner);
        const NdDev* d_dev = (const NdDev*)(pb + C.o_dev);
        const int32_t* d_st = (const int32_t*)(pb + C.o_st);
        int32_t* d_cnt = cnt.as<int32_t>();
        int32_t* d_aoff = d_cnt + 2 * C.n_lower;
        BSM_HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)(2 * C.n_lower) * sizeof(int32_t), s));
        nd_aent_count<<<nd_blocks(N, 256), 256, 0, s>>>(N, a->row_ptr, a->col, d_pinv, d_owner, d_dev, d_st, d_cnt);
        BSM_HIP_TRY(hipGetLastError());
        nd_scan_tiles<<<1, 1024, 0, s>>>(C.n_lower, d_cnt, d_aoff);
        BSM_HIP_TRY(hipGetLastError());
        nd_aent_fill<<<nd_blocks(N, 256), 256, 0, s>>>(N, a->row_ptr, a->col, d_pinv, d_owner, d_dev, d_st, d_aoff,
                                                       d_cnt + C.n_lower, C.aent.as<int64_t>());
        BSM_HIP_TRY(hipGetLastError());
        if (C.n_tiles) {
            nd_task_ranges<<<nd_blocks((int64_t)C.n_tiles, 256), 256, 0, s>>>(
                (int64_t)C.n_tiles, (const int4*)(pb + C.o_tiles), d_dev, d_aoff, C.tq.as<int2>());
            BSM_HIP_TRY(hipGetLastError());
            nd_task_pull<<<nd_blocks((int64_t)C.n_tiles, 256), 256, 0, s>>>(
                (int64_t)C.n_tiles, (const int4*)(pb + C.o_tiles), d_dev, (const int32_t*)(pb + C.o_tb),
                C.pdesc.as<NdPull>());
            BSM_HIP_TRY(hipGetLastError());
        }
        BSM_HIP_TRY(hipMemcpyAsync(&na, d_aoff + C.n_lower, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    BSM_HIP_TRY(hipStreamSynchronize(s));  // also: the staging buffer is reused by the next plan
    C.n_aent = na;
    stage_mark("nd_upload", s);
    if (pre_fronts.joinable()) {  // the fronts' allocation: the wait for it as a stage of its own
        pre_fronts.join();
        stage_mark("nd_fronts_alloc", s);
    }
    return BSM_OK;
}

size_t nd_pattern_rp_bytes(int64_t n) { return ((size_t)(n + 1) * sizeof(int64_t) + 255) / 256 * 256; }

// the pattern's key (synchronous on s: a ~6M-element pass at C5, ~10 us)
int nd_pattern_key(const bsm_csr* a, int64_t leaf, NdLay lay, bool hash_zero, hipStream_t s, NdKey& key) {
    const int64_t n = (int64_t)a->rows, total = n + 1 + (int64_t)a->nnz;
    key.device = a->device;
    key.lay = lay;
    key.n = n;
    key.leaf = leaf;
    key.nnz = a->nnz;
    DBuf hb;
    BSM_TRY(hb.alloc(16, s));
    BSM_HIP_TRY(hipMemsetAsync(hb.p, 0, 16, s));
    nd_pattern_hash<<<(unsigned)std::min<int64_t>((total + 255) / 256, 1024), 256, 0, s>>>(
        a->row_ptr, n + 1, a->col, (int64_t)a->nnz, hb.as<unsigned long long>());
    BSM_HIP_TRY(hipGetLastError());
    uint64_t h[2] = {0, 0};
    BSM_HIP_TRY(read_dev(h, hb.p, 16, s));
    key.h0 = h[0];
    key.h1 = h[1];
    if (hash_zero) key.h0 = key.h1 = 0;  // BSM_ND_HASH_ZERO=1 (tests): every pattern of one (n, nnz) collides
    return BSM_OK;
}

// Drop kept numeric storage, least recently used first, until the entries'
// total is at most `budget` bytes; `keep` and storage a running solve holds
// stay. The caller holds the cache's mutex.
void nd_cache_trim_locked(NdCache& c, size_t budget, const NdCached* keep) {
    std::vector<NdCacheEntry*> by_age;
    size_t total = 0;
    for (auto& e : c.entries) {
        total += e.plan->kept_bytes;
        by_age.push_back(&e);
    }
    std::sort(by_age.begin(), by_age.end(), [](auto* x, auto* y) { return x->tick < y->tick; });
    for (NdCacheEntry* e : by_age) {
        if (total <= budget) break;
        if (e->plan.get() == keep) continue;
        const size_t b = e->plan->kept_bytes;
        if (b && e->plan->release_numeric()) total -= b;
    }
}

void nd_cache_trim(size_t budget, const NdCached* keep) {
    NdCache& c = nd_cache();
    std::lock_guard<std::mutex> l(c.mu);
    nd_cache_trim_locked(c, budget, keep);
}

// A cached plan for this pattern (confirmed against the entry's copy of the
// pattern), or null
int nd_cache_find(const bsm_csr* a, const NdKey& key, hipStream_t s, std::shared_ptr<NdCached>& out) {
    out.reset();
    NdCache& c = nd_cache();
    std::shared_ptr<DBuf> pat;
    std::shared_ptr<NdCached> plan;
    {
        std::lock_guard<std::mutex> l(c.mu);
        for (auto& e : c.entries)
            if (e.key == key) {
                e.tick = ++c.tick;
                pat = e.pattern;
                plan = e.plan;
                break;
            }
    }
    if (plan) {
        const int64_t n1 = key.n + 1, total = n1 + (int64_t)key.nnz;
        const char* pb = pat->as<char>();
        DBuf db;
        BSM_TRY(db.alloc(4, s));
        BSM_HIP_TRY(hipMemsetAsync(db.p, 0, 4, s));
        nd_pattern_diff<<<(unsigned)std::min<int64_t>((total + 255) / 256, 4096), 256, 0, s>>>(
            a->row_ptr, (const int64_t*)pb, n1, a->col, (const int32_t*)(pb + nd_pattern_rp_bytes(key.n)),
            (int64_t)key.nnz, db.as<int>());
        BSM_HIP_TRY(hipGetLastError());
        int diff = 1;
        BSM_HIP_TRY(read_dev(&diff, db.p, 4, s));
        if (!diff) out = plan;
    }
    std::lock_guard<std::mutex> l(c.mu);
    ++(out ? c.hits : c.misses);
    return BSM_OK;
}

// A device copy of a's pattern: row_ptr (n + 1 int64, padded to 256 bytes), then col (nnz int32)
int nd_pattern_copy(const bsm_csr* a, hipStream_t s, std::shared_ptr<DBuf>& out) {
    auto pat = std::make_shared<DBuf>();
    const size_t rpb = nd_pattern_rp_bytes((int64_t)a->rows);
    BSM_TRY(pat->alloc(rpb + (size_t)a->nnz * sizeof(int32_t)));
    BSM_HIP_TRY(hipMemcpyAsync(pat->p, a->row_ptr, (size_t)(a->rows + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (a->nnz)
        BSM_HIP_TRY(hipMemcpyAsync(pat->as<char>() + rpb, a->col, (size_t)a->nnz * sizeof(int32_t),
                                   hipMemcpyDeviceToDevice, s));
    BSM_HIP_TRY(hipStreamSynchronize(s));  // a lookup on another stream may compare against it next
    out = std::move(pat);
    return BSM_OK;
}

int nd_cache_insert(const bsm_csr* a, const NdKey& key, const std::shared_ptr<NdCached>& plan, size_t max_entries,
                    hipStream_t s) {
    std::shared_ptr<DBuf> pat;
    BSM_TRY(nd_pattern_copy(a, s, pat));
    {
        std::lock_guard<std::mutex> pl(plan->pat_mu);
        plan->pattern = pat;
    }
    NdCache& c = nd_cache();
    std::lock_guard<std::mutex> l(c.mu);
    c.entries.erase(std::remove_if(c.entries.begin(), c.entries.end(),
                                   [&](const NdCacheEntry& e) { return e.key == key; }),
                    c.entries.end());
    NdCacheEntry e;
    e.key = key;
    e.tick = ++c.tick;
    e.pattern = std::move(pat);
    e.plan = plan;
    c.entries.push_back(std::move(e));
    const size_t cap = std::max<size_t>(1, max_entries);
    while (c.entries.size() > cap) {
        auto old = std::min_element(c.entries.begin(), c.entries.end(),
                                    [](const NdCacheEntry& x, const NdCacheEntry& y) { return x.tick < y.tick; });
        c.entries.erase(old);  // a handle still holding the plan keeps it alive
    }
    return BSM_OK;
}

// Numeric storage for a solve: on BSM_ERR_OOM, drop every other cached
// plan's kept storage and try once more
int nd_alloc_numeric(DBuf& b, size_t bytes, const NdCached* keep) {
    if (b.bytes == bytes) return BSM_OK;
    int rc = b.alloc(bytes);
    if (rc == BSM_ERR_OOM) {
        nd_cache_trim(0, keep);
        rc = b.alloc(bytes);
    }
    return rc;
}

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

// nd_solve's three pieces, which bsm_nd_factor (below) calls one by one: the
// plan (nd_obtain_plan), the numeric factor (nd_stage_fronts, then
// nd_factor_levels) and the solves (nd_solve_passes).

// The plan of a's pattern: the one on the handle, else the cross-handle
// cache's, else a new one (then kept in both, as the switches allow). es > 0:
// a new plan allocates its kept numeric storage while it is built.
int nd_obtain_plan(const bsm_csr* a, const NdOpts& opt, NdLay lay, size_t es, hipStream_t s,
                   std::shared_ptr<NdCached>& pc) {
    const bool cache = opt.cache, shared = opt.shared;
    const int64_t leaf = opt.leaf;
    if (cache) {
        std::lock_guard<std::mutex> lk(a->plan_mu);
        auto c = std::static_pointer_cast<NdCached>(a->nd_plan);
        if (c && c->leaf == leaf && c->lay == lay) pc = c;
    }
    NdKey key;
    if (pc) {
        stage_mark("nd_plan_cached", s);
    } else {
        if (shared) {
            BSM_TRY(nd_pattern_key(a, leaf, lay, opt.hash_zero, s, key));
            BSM_TRY(nd_cache_find(a, key, s, pc));
            stage_mark(pc ? "nd_plan_shared" : "nd_pattern_key", s);
        }
        if (!pc) {
            pc = std::make_shared<NdCached>();
            BSM_TRY(nd_build_plan(a, leaf, lay, opt.threads, es, s, *pc));
            if (shared) BSM_TRY(nd_cache_insert(a, key, pc, opt.cache_entries, s));
        }
        if (cache) {
            std::lock_guard<std::mutex> lk(a->plan_mu);
            a->nd_plan = pc;
        }
    }
    return BSM_OK;
}

void nd_trace(const NdOpts& opt, const NdCached& C, int64_t N, size_t es) {
    if (opt.trace)
        fprintf(stderr,
                "[bsm nd] n %lld nodes %d levels %d: graph %.1f ms, bisection %.1f ms, symbolic %.1f ms, layout "
                "%.1f ms, packing %.1f ms; fronts %.3f GB (largest %lld), tiles %zu, extend tasks %zu\n",
                (long long)N, C.nn, C.n_levels, C.ms_graph, C.ms_order, C.ms_symbolic, C.ms_layout, C.ms_pack,
                (double)C.f_elems * es * 1e-9, (long long)C.max_front, C.n_tiles, C.n_ext2);
}

// the plan's device arrays
struct NdPtrs {
    const NdDev* nodes;
    const int32_t *st, *ri, *pinv, *owner, *lvl;
    const int4 *tiles, *ext2;
    const int2 *ftask, *btask;
    const int64_t* perm;
};
NdPtrs nd_ptrs(const NdCached& C) {
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
template <typename T>
int nd_grid(bool factor, bool solves, NdGrid& g) {
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
        if (nt > 0) {
            const int64_t grid = std::min<int64_t>(nt, (int64_t)g.cus * g.per_cu);
            if (stamps)
                nd_factor<T, true><<<(unsigned)grid, 256, 0, s>>>(
                    p.nodes, p.tiles + t0, nt, F, Dinv, flags, d_tickets + lv, d_status, p.ri, fV, fbp, d_aent, d_av,
                    d_tq ? d_tq + t0 : nullptr, d_pd ? d_pd + 2 * t0 : nullptr, stamps + ND_NSTAMP * lv);
            else
                nd_factor<T><<<(unsigned)grid, 256, 0, s>>>(p.nodes, p.tiles + t0, nt, F, Dinv, flags, d_tickets + lv,
                                                            d_status, p.ri, fV, fbp, d_aent, d_av,
                                                            d_tq ? d_tq + t0 : nullptr, d_pd ? d_pd + 2 * t0 : nullptr);
            BSM_HIP_TRY(hipGetLastError());
        }
        const int64_t e0 = C.ext2_off[(size_t)lv], ne = C.ext2_off[(size_t)lv + 1] - e0;
        if (ne > 0) {  // the plain pipeline: this level's update blocks into the parents' fronts
            nd_extend2<T><<<nd_blocks(ne, 4), 256, 0, s>>>(p.nodes, p.ext2 + e0, ne, p.ri, F);
            BSM_HIP_TRY(hipGetLastError());
        }
    }
    return BSM_OK;
}

// The backward levels of a solve, top-down over every front: y over each
// front's pivots in V, x into bp. d_xf / d_btk: the pass's cleared flags (one
// per node, column and pivot tile) and tickets (one per level). Levels with
// fewer (node, column) pairs than CUs run by tiles (nd_solve_passes).
template <typename T>
int nd_backward_levels(const NdCached& C, const NdOpts& opt, const NdGrid& g, int64_t N, uint64_t k, const T* F,
                       const T* Dinv, T* bp, T* V, int* d_xf, int* d_btk, int* d_status, hipStream_t s) {
    const NdPtrs p = nd_ptrs(C);
    const int64_t bwd_grid = (int64_t)g.cus * g.bper;
    for (int32_t lv = C.n_levels - 1; lv >= 0; --lv) {
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
    const int cus = g.cus;
    T* const bp = t.bpb.as<T>();
    T* const V = t.vb.as<T>();
    const bool fwd = !folded && system != BSM_ND_SYS_LT, bwd = system != BSM_ND_SYS_L;
    const int64_t* const perm = system == BSM_ND_SYS_A ? p.perm : nullptr;
    if (!folded) {
        nd_gather<T><<<nd_blocks(N, 256), 256, 0, s>>>(N, (int64_t)k, perm, static_cast<const T*>(b_dev), bp);
        BSM_HIP_TRY(hipGetLastError());
    }
    // Levels with fewer (node, column) pairs than CUs run their solves by
    // tiles (nd_forward_tiles / nd_backward_tiles: a front's chain of pivot
    // tiles on many waves), the others one workgroup per pair (nd_forward /
    // nd_backward: less bookkeeping per front). Same bits either way.
    // BSM_ND_FWD_TILES / BSM_ND_BWD_TILES = 0: never, 1: every level.
    auto by_tiles = [&](int mode, int64_t pairs) { return mode == 1 || (mode == 2 && pairs < cus); };
    BSM_HIP_TRY(hipMemsetAsync(t.tfl.p, 0, (t.n_tf + 1) * sizeof(int), s));
    int* const d_yf = t.tfl.as<int>();
    int* const d_xf = d_yf + t.n_pf;
    int* const d_ftk = d_xf + t.n_pf;
    int* const d_btk = d_ftk + C.n_levels;
    const int64_t fwd_grid = (int64_t)cus * g.fper;
    for (int32_t lv = 0; lv < C.n_levels && fwd; ++lv) {
        const int64_t o = C.lvl_off[(size_t)lv], c = C.lvl_off[(size_t)lv + 1] - o;
        if (c <= 0) continue;
        if (by_tiles(opt.fwd_tiles, c * (int64_t)k)) {
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
    if (system == BSM_ND_SYS_L && C.nn > 0) {
        nd_y_out<T><<<dim3((unsigned)C.nn, (unsigned)k), 256, 0, s>>>(p.nodes, N, V, C.vtot, bp);
        BSM_HIP_TRY(hipGetLastError());
    }
    stage_mark("nd_forward", s);
    if (system == BSM_ND_SYS_LT && C.nn > 0) {
        nd_y_in<T><<<dim3((unsigned)C.nn, (unsigned)k), 256, 0, s>>>(p.nodes, N, bp, V, C.vtot);
        BSM_HIP_TRY(hipGetLastError());
    }
    if (bwd) BSM_TRY(nd_backward_levels<T>(C, opt, g, N, k, F, Dinv, bp, V, d_xf, d_btk, d_status, s));
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
    BSM_TRY(nd_grid<T>(true, true, g));
    DBuf avb;  // from the thread's cache of temporaries, as the solves' (no hipFree per solve)
    NdSolveTmp tmp;
    if (!plain) BSM_TRY(avb.alloc((size_t)std::max<int64_t>(C.n_aent, 1) * sizeof(T), s));
    if (k > 0) BSM_TRY(nd_solve_tmp<T>(C, N, k, s, tmp));
    DBuf& bpb = tmp.bpb;
    DBuf& vb = tmp.vb;
    NdDrainOnError drain{s};  // destroyed before num_lock is released
    drain.armed = true;
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
    int h = 0;
    BSM_HIP_TRY(read_dev(&h, d_status, sizeof(int), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    stage_mark("nd_copy_out", s);
    if (stamps.p) {
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
    BSM_REQUIRE(!(h & ST_TIMEOUT), BSM_ERR_HIP, "nd factor: tile hand-off timed out");
    BSM_REQUIRE(!(h & ST_NOT_PD), BSM_ERR_UNSUPPORTED,
                "cholesky: matrix is not positive definite (a pivot is <= 0 or not finite)");
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
    BSM_TRY(nd_grid<T>(true, false, g));
    DBuf fl, avb, cvt;  // temporaries: the flags, tickets and status; A's values by tile; A's values as T
    BSM_TRY(fl.alloc(nfl * sizeof(int), s));
    const bool convert = a->dtype != f.dtype;  // bsm_nd_factor_create_as: the factor's dtype is not the matrix's
    if (convert) BSM_TRY(cvt.alloc((size_t)std::max<uint64_t>(a->nnz, 1) * sizeof(T), s));
    if (!C.lay.plain) BSM_TRY(avb.alloc((size_t)std::max<int64_t>(C.n_aent, 1) * sizeof(T), s));
    NdDrainOnError drain{s};  // the temporaries go back to the thread's cache only after the kernels
    drain.armed = true;
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
    int h = 0;
    BSM_HIP_TRY(read_dev(&h, d_flags + C.n_flags + C.n_levels, sizeof(int), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    BSM_REQUIRE(!(h & ST_TIMEOUT), BSM_ERR_HIP, "nd factor: tile hand-off timed out");
    BSM_REQUIRE(!(h & ST_NOT_PD), BSM_ERR_UNSUPPORTED,
                "cholesky: matrix is not positive definite (a pivot is <= 0 or not finite)");
    f.valid = true;
    return BSM_OK;
}

template <typename T>
int nd_factor_create_t(const bsm_csr* a, bsm_nd_factor& f, hipStream_t s) {
    stage_reset(s);
    const int64_t N = (int64_t)a->rows;
    const NdOpts opt = nd_options();
    NdLay lay = opt.lay;
    lay.plain = lay.plain || a->nnz >= ((uint64_t)1 << 31);  // as nd_solve
    std::shared_ptr<NdCached> pc;
    // no kept storage asked for on a new plan: the factor's fronts are its own
    BSM_TRY(nd_obtain_plan(a, opt, lay, 0, s, pc));
    NdCached& C = *pc;
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

// New values on the factor's pattern: the numeric factor again, on the
// handle's plan and into its own storage. The caller holds f.mu.
template <typename T>
int nd_factor_refactor_t(const bsm_csr* a, bsm_nd_factor& f, hipStream_t s) {
    stage_reset(s);
    const auto pc = std::static_pointer_cast<NdCached>(f.plan);
    const NdCached& C = *pc;
    bool same_plan = false;  // a finalised handle's pattern never changes
    {
        std::lock_guard<std::mutex> lk(a->plan_mu);
        same_plan = a->nd_plan.get() == f.plan.get();
    }
    if (!same_plan) {
        const int64_t n1 = (int64_t)f.n + 1, nnz = (int64_t)f.nnz;
        const char* pb = f.pattern->as<char>();
        const int64_t* rpb = (const int64_t*)pb;
        const int32_t* cb = (const int32_t*)(pb + nd_pattern_rp_bytes((int64_t)f.n));
        DBuf db;
        BSM_TRY(db.alloc(8, s));
        BSM_HIP_TRY(hipMemsetAsync(db.p, 0, 8, s));
        nd_pattern_diff<<<(unsigned)std::min<int64_t>((n1 + 255) / 256, 4096), 256, 0, s>>>(
            a->row_ptr, rpb, n1, a->col, cb, 0, db.as<int>());
        BSM_HIP_TRY(hipGetLastError());
        if (nnz > 0) {
            nd_pattern_diff<<<(unsigned)std::min<int64_t>((nnz + 255) / 256, 4096), 256, 0, s>>>(
                a->row_ptr, rpb, 0, a->col, cb, nnz, db.as<int>() + 1);
            BSM_HIP_TRY(hipGetLastError());
        }
        int diff[2] = {1, 1};
        BSM_HIP_TRY(read_dev(diff, db.p, 8, s));
        BSM_REQUIRE(!diff[0], BSM_ERR_INVALID, "nd factor refactor: row_ptr differs from the factored matrix's");
        BSM_REQUIRE(!diff[1], BSM_ERR_INVALID, "nd factor refactor: col differs from the factored matrix's");
    }
    return nd_factor_numeric_t<T>(a, f, C, nd_options(), s);
}

template <typename T>
int nd_factor_logdet_t(const bsm_nd_factor& f, double* logdet, hipStream_t s) {
    const int64_t N = (int64_t)f.n;
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const unsigned nb = nd_logdet_blocks(N);
    DBuf part;  // the partials, then the result
    BSM_TRY(part.alloc(((size_t)nb + 1) * sizeof(double), s));
    NdDrainOnError drain{s};
    drain.armed = true;
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
    BSM_TRY(nd_grid<T>(false, true, g));
    NdSolveTmp tmp;
    BSM_TRY(nd_solve_tmp<T>(C, N, k, s, tmp));
    NdDrainOnError drain{s};  // the handle's mutex is released after this guard runs
    drain.armed = true;
    int* const d_status = tmp.tfl.as<int>() + tmp.n_tf;  // cleared with the passes' flags
    BSM_TRY(nd_solve_passes<T>(C, opt, g, N, k, f.fr.as<T>(), f.dv.as<T>(), b_dev, x_dev, tmp, false, d_status, s,
                               system));
    int h = 0;
    BSM_HIP_TRY(read_dev(&h, d_status, sizeof(int), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    stage_mark("nd_copy_out", s);
    BSM_REQUIRE(!(h & ST_TIMEOUT), BSM_ERR_HIP, "nd solve: tile hand-off timed out");
    return BSM_OK;
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
    NdDrainOnError drain{s};
    drain.armed = true;
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

// ---- the selected inverse ----------------------------------
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
    NdDrainOnError drain{s};  // Z and the panels are freed, and the handle's mutex released, after this guard runs
    drain.armed = true;
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

// ---- the rank-k update and downdate -------------------------
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
    NdDrainOnError drain{s};
    drain.armed = true;
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

// ---- sparse right-hand sides and selected solution rows -----
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
    if (all) BSM_TRY(nd_grid<T>(false, true, g));
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
    NdDrainOnError drain{s};  // the handle's mutex is released after this guard runs
    drain.armed = true;
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
            nd_forward_path<T><<<dim3((unsigned)cnt, kc), 256, 0, s>>>(p.nodes, d_fw + a0, N, bp, V, C.vtot, F, Dinv,
                                                                      p.ri);
            BSM_HIP_TRY(hipGetLastError());
        }
        stage_mark("nd_sparse_forward", s);
        if (all) {
            BSM_TRY(nd_backward_levels<T>(C, opt, g, N, kc, F, Dinv, bp, V, tfl.as<int>(), tfl.as<int>() + n_pf,
                                          d_status, s));
        } else {
            for (size_t li = bw.levels.size(); li-- > 0;) {
                const int32_t a0 = bw.first(li), cnt = bw.last(li) - a0;
                nd_backward_path<T><<<dim3((unsigned)cnt, kc), 256, 0, s>>>(p.nodes, d_bw + a0, N, bp, V, C.vtot, F,
                                                                           Dinv, p.st);
                BSM_HIP_TRY(hipGetLastError());
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
    int h = 0;
    if (all) BSM_HIP_TRY(read_dev(&h, d_status, sizeof(int), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    stage_mark("nd_sparse_gather", s);
    BSM_REQUIRE(!(h & ST_TIMEOUT), BSM_ERR_HIP, "nd solve: tile hand-off timed out");
    if (info) {
        info[0] = (uint32_t)nf;
        info[1] = (uint32_t)(all ? nn : nb);
        info[2] = (uint32_t)nn;
        info[3] = (uint32_t)chunks;
    }
    return BSM_OK;
}

// ---- the partial refactor ------------------------------------
// New values at a few places of the factored pattern: nd_factor again on the
// fronts on the paths from those entries' fronts to the roots (reach_rule.hpp),
// and on no other. In the default pipeline a tile is built from A's entries in
// it (aent / tq, values in avb) and its children's update blocks (pdesc),
// never from F, and the children's blocks stay in their trailing tiles after a
// factorisation: an active front pulls an inactive child's block as the last
// factorisation left it and an active child's as the level below has just
// rewritten it. Each level that occurs runs nd_factor itself on a contiguous
// copy of its active fronts' tiles / tq / pdesc entries in the plan's order (a
// subsequence of the ticket order: every dependency of a tile is a tile of its
// own front, still ahead of it), so every addition happens in refactor's
// order: the same bits. The flags, tickets and status word are a cleared
// temporary; avb is filled over the selected tiles' ranges alone.

constexpr int32_t ND_PARTIAL_CHUNK = 256;

// Per named pair (i, j): is (max, min) stored in a (a binary search of row max:
// columns ascend within a row; a row that does not ascend is walked)? Its start
// front, nd_assemble's owner[min(pinv i, pinv j)], else -1 and a miss counted.
__global__ __launch_bounds__(256) void nd_partial_owners(int64_t nc, const uint64_t* __restrict__ rows,
                                                         const uint64_t* __restrict__ cols,
                                                         const int64_t* __restrict__ rp,
                                                         const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ pinv,
                                                         const int32_t* __restrict__ owner,
                                                         int32_t* __restrict__ start,
                                                         unsigned long long* __restrict__ miss) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nc) return;
    const int64_t x = (int64_t)rows[e], y = (int64_t)cols[e];
    const int64_t i = x > y ? x : y, j = x > y ? y : x;
    const int64_t b = rp[i], len = rp[i + 1] - b;
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (col[b + mid] < j) lo = mid + 1;
        else hi = mid;
    }
    bool hit = lo < len && col[b + lo] == j;
    for (int64_t q = 0; q < len && !hit; ++q) hit = col[b + q] == j;
    if (!hit) {
        atomicAdd(&miss[0], 1ull);
        atomicMin(&miss[1], (unsigned long long)e);
    }
    const int64_t pi = pinv[i], pj = pinv[j];
    start[e] = hit ? owner[pi < pj ? pi : pj] : -1;
}

// The `since` form: every stored entry with col <= row whose source bits differ
// between the two matrices (U: the values as unsigned words, so NaN and -0
// count) marks its start front in act (a byte per front; every writer stores 1)
// and is counted (integer atomics: any order gives the same sum).
template <typename U>
__global__ __launch_bounds__(256) void nd_partial_diff(int64_t n, const int64_t* __restrict__ rp,
                                                       const int32_t* __restrict__ col, const U* __restrict__ va,
                                                       const U* __restrict__ vb, const int32_t* __restrict__ pinv,
                                                       const int32_t* __restrict__ owner,
                                                       unsigned char* __restrict__ act,
                                                       unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t pi = pinv[i];
    unsigned long long c = 0;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        const int64_t j = col[e];
        if (j > i || va[e] == vb[e]) continue;
        const int64_t pj = pinv[j];
        act[owner[pi < pj ? pi : pj]] = 1;
        ++c;
    }
    if (c) atomicAdd(count, c);
}

// Task selection, order-preserving, over the levels that occur (partial_rule.hpp):
// mark (a chunk's tasks whose node is active, counted), scan (per level, the
// chunks' places from the level's o0), scatter (each kept task's tiles / tq /
// pdesc entries to its place).
__global__ __launch_bounds__(256) void nd_partial_mark(const PartialChunk* __restrict__ ch,
                                                       const unsigned char* __restrict__ act,
                                                       const int4* __restrict__ tiles, int32_t* __restrict__ cnt) {
    const PartialChunk c = ch[blockIdx.x];
    const int t = threadIdx.x;
    const int on = t < c.len && act[tiles[c.t0 + t].x];
    const int n = __syncthreads_count(on);
    if (t == 0) cnt[blockIdx.x] = n;
}
__global__ __launch_bounds__(256) void nd_partial_scan(const PartialLevel* __restrict__ lv,
                                                       const int32_t* __restrict__ cnt, int64_t* __restrict__ base,
                                                       int* __restrict__ err) {
    __shared__ int64_t part[256];
    const PartialLevel L = lv[blockIdx.x];
    const int t = threadIdx.x;
    const int64_t lo = (int64_t)L.nchunks * t / 256, hi = (int64_t)L.nchunks * (t + 1) / 256;
    int64_t sum = 0;
    for (int64_t g = lo; g < hi; ++g) sum += cnt[L.c0 + g];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the threads' sums
        const int64_t v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    if (t == 255 && part[255] != L.cnt) atomicOr(err, 1);  // the device's count is not the host's
    int64_t run = L.o0 + part[t] - sum;
    for (int64_t g = lo; g < hi; ++g) {
        base[L.c0 + g] = run;
        run += cnt[L.c0 + g];
    }
}
// err: a level's count is not the host's, or a kept task's place lies outside
// its level's share: nothing is written there, and the call fails before
// nd_factor sees the lists
__global__ __launch_bounds__(256) void nd_partial_scatter(
    const PartialChunk* __restrict__ ch, const PartialLevel* __restrict__ lv, const unsigned char* __restrict__ act,
    const int4* __restrict__ tiles, const int2* __restrict__ tq, const NdPull* __restrict__ pd,
    const int64_t* __restrict__ base, int4* __restrict__ otiles, int2* __restrict__ otq, NdPull* __restrict__ opd,
    int* __restrict__ err) {
    __shared__ int wsum[4];
    const PartialChunk c = ch[blockIdx.x];
    const PartialLevel L = lv[c.li];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t src = c.t0 + t;
    const bool on = t < c.len && act[tiles[c.t0 + (t < c.len ? t : 0)].x];
    const unsigned long long b = __ballot(on);
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1));
    for (int q = 0; q < w; ++q) before += wsum[q];
    if (!on) return;
    const int64_t dst = base[blockIdx.x] + before;
    if (dst < L.o0 || dst >= L.o0 + L.cnt) {
        atomicOr(err, 1);
        return;
    }
    otiles[dst] = tiles[src];
    otq[dst] = tq[src];
    opd[2 * dst] = pd[2 * src];
    opd[2 * dst + 1] = pd[2 * src + 1];
}

// nd_aent_vals over the selected tasks' ranges alone (a wave per task), the
// source values converted as convert_values converts them
template <typename T, typename S>
__global__ __launch_bounds__(256) void nd_partial_vals(int64_t ntask, const int2* __restrict__ otq,
                                                       const int64_t* __restrict__ aent, const S* __restrict__ val,
                                                       T* __restrict__ av) {
    const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task >= ntask) return;  // wave-uniform
    const int2 rq = otq[task];
    for (int q = threadIdx.x & 63; q < rq.y; q += 64) av[rq.x + q] = (T)val[aent[rq.x + q] >> 12];
}

// refactor's comparison of a's pattern with the factored one (its messages)
int nd_partial_pattern(const bsm_csr* a, const bsm_nd_factor& f, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(a->plan_mu);
        if (a->nd_plan.get() == f.plan.get()) return BSM_OK;  // a finalised handle's pattern never changes
    }
    const int64_t n1 = (int64_t)f.n + 1, nnz = (int64_t)f.nnz;
    const char* pb = f.pattern->as<char>();
    const int64_t* rpb = (const int64_t*)pb;
    const int32_t* cb = (const int32_t*)(pb + nd_pattern_rp_bytes((int64_t)f.n));
    DBuf db;
    BSM_TRY(db.alloc(8, s));
    BSM_HIP_TRY(hipMemsetAsync(db.p, 0, 8, s));
    nd_pattern_diff<<<(unsigned)std::min<int64_t>((n1 + 255) / 256, 4096), 256, 0, s>>>(a->row_ptr, rpb, n1, a->col, cb,
                                                                                       0, db.as<int>());
    BSM_HIP_TRY(hipGetLastError());
    if (nnz > 0) {
        nd_pattern_diff<<<(unsigned)std::min<int64_t>((nnz + 255) / 256, 4096), 256, 0, s>>>(a->row_ptr, rpb, 0, a->col,
                                                                                            cb, nnz, db.as<int>() + 1);
        BSM_HIP_TRY(hipGetLastError());
    }
    int diff[2] = {1, 1};
    BSM_HIP_TRY(read_dev(diff, db.p, 8, s));
    BSM_REQUIRE(!diff[0], BSM_ERR_INVALID, "nd factor refactor: row_ptr differs from the factored matrix's");
    BSM_REQUIRE(!diff[1], BSM_ERR_INVALID, "nd factor refactor: col differs from the factored matrix's");
    return BSM_OK;
}

// each node's tile rows on the host, read back once per plan
int nd_partial_node_nt(NdCached& C, hipStream_t s, const int32_t** out) {
    std::lock_guard<std::mutex> lk(C.part_mu);
    if (C.h_nt.size() != (size_t)C.nn) {
        std::vector<NdDev> dev((size_t)C.nn);
        BSM_TRY(d2h_staged(dev.data(), nd_ptrs(C).nodes, dev.size() * sizeof(NdDev), s));
        std::vector<int32_t> nt((size_t)C.nn);
        for (size_t i = 0; i < nt.size(); ++i) nt[i] = dev[i].nt;
        C.h_nt.swap(nt);
    }
    *out = C.h_nt.data();
    return BSM_OK;
}

// The caller holds f.mu and has made every check; f holds a factor of a's
// pattern whose update blocks are in place (the default pipeline). start: ns
// start fronts (negative: skipped). n_active: the fronts factored again.
template <typename T>
int nd_factor_partial_t(const bsm_csr* a, bsm_nd_factor& f, const int32_t* start, size_t ns, uint64_t* n_active,
                        hipStream_t s) {
    NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdOpts opt = nd_options();
    const NdPtrs p = nd_ptrs(C);
    *n_active = 0;
    const int32_t* node_nt = nullptr;
    BSM_TRY(nd_partial_node_nt(C, s, &node_nt));
    std::vector<unsigned char> mark;
    ReachSet R;
    reach_set((size_t)C.nn, C.h_parent.data(), C.h_level.data(), nullptr, nullptr, start, ns, mark, R);
    if (R.fronts.empty()) return BSM_OK;
    PartialPlan P;
    partial_plan(R, node_nt, C.tiles_off.data(), ND_PARTIAL_CHUNK, P);
    const size_t nl = P.levels.size(), nch = P.chunks.size(), tot = (size_t)P.total;
    BSM_REQUIRE(nl <= (size_t)C.n_levels && tot <= C.n_tiles, BSM_ERR_HIP,
                "nd partial refactor: the plan is inconsistent");
    // everything that can fail before the first write to the factor
    const size_t nfl = (size_t)C.n_flags + (size_t)C.n_levels + 2;
    NdGrid g;
    BSM_TRY(nd_grid<T>(true, false, g));
    auto up8 = [](size_t b) { return (b + 7) / 8 * 8; };
    // the host's lists in one upload: levels, chunks, the active map; then the device's own: chunk places, chunk
    // counts and the error word
    const size_t o_ch = nl * sizeof(PartialLevel), o_act = o_ch + nch * sizeof(PartialChunk),
                 o_base = up8(o_act + (size_t)C.nn), o_cnt = o_base + nch * sizeof(int64_t),
                 sel_b = o_cnt + (nch + 1) * sizeof(int32_t);
    DBuf fl, avb, selb, tlb, tqb, pdb;
    BSM_TRY(fl.alloc(nfl * sizeof(int), s));
    const size_t av_b = (size_t)std::max<int64_t>(C.n_aent, 1) * sizeof(T);
    BSM_TRY(avb.alloc(av_b, s));
    BSM_TRY(selb.alloc(sel_b, s));
    BSM_TRY(tlb.alloc(std::max<size_t>(tot, 1) * sizeof(int4), s));
    BSM_TRY(tqb.alloc(std::max<size_t>(tot, 1) * sizeof(int2), s));
    BSM_TRY(pdb.alloc(std::max<size_t>(tot, 1) * 2 * sizeof(NdPull), s));
    NdDrainOnError drain{s};  // the temporaries go back to the thread's cache only after the kernels
    drain.armed = true;
    std::vector<char> hb(o_act + (size_t)C.nn);
    memcpy(hb.data(), P.levels.data(), o_ch);
    memcpy(hb.data() + o_ch, P.chunks.data(), nch * sizeof(PartialChunk));
    memcpy(hb.data() + o_act, mark.data(), (size_t)C.nn);
    BSM_TRY(h2d_staged(selb.p, hb.data(), hb.size(), s));
    char* const sb = selb.as<char>();
    const PartialLevel* const d_lv = (const PartialLevel*)sb;
    const PartialChunk* const d_ch = (const PartialChunk*)(sb + o_ch);
    const unsigned char* const d_act = (const unsigned char*)(sb + o_act);
    int64_t* const d_base = (int64_t*)(sb + o_base);
    int32_t* const d_cnt = (int32_t*)(sb + o_cnt);
    int* const d_err = (int*)(d_cnt + nch);
    int* const d_flags = fl.as<int>();
    BSM_HIP_TRY(hipMemsetAsync(d_flags, 0, nfl * sizeof(int), s));
    BSM_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int), s));
    // BSM_ND_POISON=1 (tests): the temporaries start as NaN (the fronts hold live values: the inactive ones' are read)
    if (opt.poison) {
        BSM_HIP_TRY(hipMemsetAsync(avb.p, 0xff, av_b, s));
        BSM_HIP_TRY(hipMemsetAsync(tlb.p, 0xff, tlb.bytes, s));
        BSM_HIP_TRY(hipMemsetAsync(tqb.p, 0xff, tqb.bytes, s));
        BSM_HIP_TRY(hipMemsetAsync(pdb.p, 0xff, pdb.bytes, s));
    }
    int4* const o_tiles = tlb.as<int4>();
    int2* const o_tq = tqb.as<int2>();
    NdPull* const o_pd = pdb.as<NdPull>();
    if (nch) {
        nd_partial_mark<<<(unsigned)nch, 256, 0, s>>>(d_ch, d_act, p.tiles, d_cnt);
        BSM_HIP_TRY(hipGetLastError());
        nd_partial_scan<<<(unsigned)nl, 256, 0, s>>>(d_lv, d_cnt, d_base, d_err);
        BSM_HIP_TRY(hipGetLastError());
        nd_partial_scatter<<<(unsigned)nch, 256, 0, s>>>(d_ch, d_lv, d_act, p.tiles, C.tq.as<int2>(),
                                                        C.pdesc.as<NdPull>(), d_base, o_tiles, o_tq, o_pd, d_err);
        BSM_HIP_TRY(hipGetLastError());
    }
    if (tot) {
        if (a->dtype == BSM_F64)
            nd_partial_vals<T, double><<<nd_blocks((int64_t)tot, 4), 256, 0, s>>>(
                (int64_t)tot, o_tq, C.aent.as<int64_t>(), static_cast<const double*>(a->vals), avb.as<T>());
        else
            nd_partial_vals<T, float><<<nd_blocks((int64_t)tot, 4), 256, 0, s>>>(
                (int64_t)tot, o_tq, C.aent.as<int64_t>(), static_cast<const float*>(a->vals), avb.as<T>());
        BSM_HIP_TRY(hipGetLastError());
    }
    int err = 1;
    BSM_HIP_TRY(read_dev(&err, d_err, sizeof(int), s));
    stage_mark("nd_partial_select", s);
    if (err) {
        drain.armed = false;
        BSM_REQUIRE(false, BSM_ERR_HIP, "nd partial refactor: the selected tasks do not fit the host's counts");
    }
    f.valid = false;  // from the first write until the status word says the factor is whole
    f.nnz_l = 0;
    int* const d_tickets = d_flags + C.n_flags;
    int* const d_status = d_tickets + C.n_levels;
    for (size_t li = 0; li < nl; ++li) {
        const PartialLevel& L = P.levels[li];
        if (L.cnt == 0) continue;
        const int64_t grid = std::min<int64_t>(L.cnt, (int64_t)g.cus * g.per_cu);
        nd_factor<T><<<(unsigned)grid, 256, 0, s>>>(p.nodes, o_tiles + L.o0, L.cnt, f.fr.as<T>(), f.dv.as<T>(), d_flags,
                                                    d_tickets + li, d_status, p.ri, (T*)nullptr, (const T*)nullptr,
                                                    C.aent.as<int64_t>(), avb.as<T>(), o_tq + L.o0, o_pd + 2 * L.o0);
        BSM_HIP_TRY(hipGetLastError());
    }
    int h = 0;
    BSM_HIP_TRY(read_dev(&h, d_status, sizeof(int), s));
    BSM_HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    stage_mark("nd_partial_factor", s);
    BSM_REQUIRE(!(h & ST_TIMEOUT), BSM_ERR_HIP, "nd factor: tile hand-off timed out");
    BSM_REQUIRE(!(h & ST_NOT_PD), BSM_ERR_UNSUPPORTED,
                "cholesky: matrix is not positive definite (a pivot is <= 0 or not finite)");
    f.valid = true;
    *n_active = R.fronts.size();
    return BSM_OK;
}

// The start fronts of a partial refactor, under f.mu, after refactor's checks:
// from the named pairs (a miss refuses the call) or from the differing entries
// of a_old and a. changed: the pairs named / the entries found.
int nd_partial_starts(const bsm_nd_factor& f, const bsm_csr* a_old, const bsm_csr* a, uint64_t nc,
                      const uint64_t* rows, const uint64_t* cols, std::vector<int32_t>& start, uint64_t* changed,
                      hipStream_t s) {
    const NdCached& C = *std::static_pointer_cast<NdCached>(f.plan);
    const NdPtrs p = nd_ptrs(C);
    const int64_t N = (int64_t)f.n;
    start.clear();
    *changed = 0;
    if (a_old) {
        DBuf mb;  // a byte per front, then the count
        const size_t o_cnt = ((size_t)C.nn + 7) / 8 * 8;
        BSM_TRY(mb.alloc(o_cnt + 8, s));
        NdDrainOnError drain{s};
        drain.armed = true;
        BSM_HIP_TRY(hipMemsetAsync(mb.p, 0, o_cnt + 8, s));
        unsigned long long* const d_count = (unsigned long long*)(mb.as<char>() + o_cnt);
        if (a->dtype == BSM_F64)
            nd_partial_diff<uint64_t><<<nd_blocks(N, 256), 256, 0, s>>>(
                N, a->row_ptr, a->col, static_cast<const uint64_t*>(a_old->vals), static_cast<const uint64_t*>(a->vals),
                p.pinv, p.owner, mb.as<unsigned char>(), d_count);
        else
            nd_partial_diff<uint32_t><<<nd_blocks(N, 256), 256, 0, s>>>(
                N, a->row_ptr, a->col, static_cast<const uint32_t*>(a_old->vals), static_cast<const uint32_t*>(a->vals),
                p.pinv, p.owner, mb.as<unsigned char>(), d_count);
        BSM_HIP_TRY(hipGetLastError());
        std::vector<char> hb(o_cnt + 8);
        BSM_TRY(d2h_staged(hb.data(), mb.p, hb.size(), s));  // the map and the count, once
        drain.armed = false;
        unsigned long long cnt = 0;
        memcpy(&cnt, hb.data() + o_cnt, 8);
        *changed = cnt;
        for (int32_t i = 0; i < C.nn; ++i)
            if (hb[(size_t)i]) start.push_back(i);
        return BSM_OK;
    }
    *changed = nc;
    if (nc == 0) return BSM_OK;
    DBuf ib, ob;  // the pairs (rows, then cols); the start fronts, then the miss count and the first miss
    const size_t o_miss = ((size_t)nc * sizeof(int32_t) + 7) / 8 * 8;
    BSM_TRY(ib.alloc((size_t)nc * 16, s));
    BSM_TRY(ob.alloc(o_miss + 16, s));
    NdDrainOnError drain{s};
    drain.armed = true;
    BSM_TRY(h2d_staged(ib.p, rows, (size_t)nc * 8, s));
    BSM_TRY(h2d_staged(ib.as<uint64_t>() + nc, cols, (size_t)nc * 8, s));
    const unsigned long long init[2] = {0ull, ~0ull};
    unsigned long long* const d_miss = (unsigned long long*)(ob.as<char>() + o_miss);
    BSM_HIP_TRY(hipMemcpyAsync(d_miss, init, sizeof(init), hipMemcpyHostToDevice, s));
    nd_partial_owners<<<nd_blocks((int64_t)nc, 256), 256, 0, s>>>((int64_t)nc, ib.as<uint64_t>(), ib.as<uint64_t>() + nc,
                                                                  a->row_ptr, a->col, p.pinv, p.owner, ob.as<int32_t>(),
                                                                  d_miss);
    BSM_HIP_TRY(hipGetLastError());
    std::vector<char> hb(o_miss + 16);
    BSM_TRY(d2h_staged(hb.data(), ob.p, hb.size(), s));  // the start fronts and the misses, once
    drain.armed = false;
    unsigned long long miss[2];
    memcpy(miss, hb.data() + o_miss, sizeof(miss));
    BSM_REQUIRE(miss[0] == 0, BSM_ERR_INVALID,
                "nd factor refactor_partial: %llu of the %llu named pairs are not stored entries of the matrix; the "
                "first is pair %llu, (%llu, %llu)",
                miss[0], (unsigned long long)nc, miss[1], (unsigned long long)rows[miss[1]],
                (unsigned long long)cols[miss[1]]);
    start.resize((size_t)nc);
    memcpy(start.data(), hb.data(), (size_t)nc * sizeof(int32_t));
    return BSM_OK;
}

}  // namespace

int nd_factor_solve_sparse(const bsm_nd_factor* f, uint64_t k, const uint64_t* col_ptr, const uint64_t* rows,
                           const void* vals, uint64_t nq, const uint64_t* xrows, void* x_dev, uint32_t* info,
                           hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    return f->dtype == BSM_F64
               ? nd_factor_solve_sparse_t<double>(*f, k, col_ptr, rows, vals, nq, xrows, x_dev, info, s)
               : nd_factor_solve_sparse_t<float>(*f, k, col_ptr, rows, vals, nq, xrows, x_dev, info, s);
}

int nd_factor_updown(bsm_nd_factor* f, int sign, uint64_t k, uint64_t nnz_w, const int64_t* colptr_dev,
                     const uint64_t* rows_dev, const void* vals_dev, uint64_t* n_miss, uint64_t* first_miss,
                     hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
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

int nd_factor_selinv(const bsm_nd_factor* f, void* diag_dev, uint64_t nq, const uint64_t* rows_dev,
                     const uint64_t* cols_dev, void* vals_dev, uint64_t* n_miss, uint64_t* first_miss,
                     hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    *n_miss = 0;
    *first_miss = 0;
    if (f->n == 0) return BSM_OK;
    return f->dtype == BSM_F64
               ? nd_factor_selinv_t<double>(*f, diag_dev, nq, rows_dev, cols_dev, vals_dev, n_miss, first_miss, s)
               : nd_factor_selinv_t<float>(*f, diag_dev, nq, rows_dev, cols_dev, vals_dev, n_miss, first_miss, s);
}

int nd_factor_inv_pattern(const bsm_nd_factor* f, void* out_dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_REQUIRE(f->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first");
    if (f->n == 0 || f->nnz == 0) return BSM_OK;
    uint64_t n_miss = 0, first = 0;
    return f->dtype == BSM_F64
               ? nd_factor_selinv_t<double>(*f, nullptr, 0, nullptr, nullptr, nullptr, &n_miss, &first, s, out_dev)
               : nd_factor_selinv_t<float>(*f, nullptr, 0, nullptr, nullptr, nullptr, &n_miss, &first, s, out_dev);
}

int nd_factor_sddmm(const bsm_nd_factor* f, int dtype, uint64_t k, const void* u, const void* v, void* out,
                    hipStream_t s) {
    if (f->n == 0 || f->nnz == 0)  // its checks of dtype and k, no launch
        return sddmm_dispatch(dtype, BSM_SDDMM_SYM_LOWER, 0, 0, 0, nullptr, nullptr, k, u, v, out, s);
    const char* const pb = f->pattern->as<char>();  // immutable for the handle's life: no lock
    return sddmm_dispatch(dtype, BSM_SDDMM_SYM_LOWER, f->n, f->n, f->nnz, (const int64_t*)pb,
                          (const int32_t*)(pb + nd_pattern_rp_bytes((int64_t)f->n)), k, u, v, out, s);
}

int nd_factor_create(const bsm_csr* a, int factor_dtype, bsm_nd_factor** out, hipStream_t s) {
    BSM_REQUIRE(a->rows < ((uint64_t)1 << 31), BSM_ERR_UNSUPPORTED, "solve nd: n >= 2^31");
    BSM_REQUIRE(a->dtype == BSM_F64 || a->dtype == BSM_F32, BSM_ERR_INVALID, "solve: f32/f64 only");
    auto f = std::make_unique<bsm_nd_factor>();
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

// the state a failed refactorisation leaves behind (under f->mu)
#define ND_REQUIRE_VALUES(f) \
    BSM_REQUIRE((f)->valid, BSM_ERR_INVALID, "nd factor: factor holds no values; refactor first")

int nd_factor_refactor(bsm_nd_factor* f, const bsm_csr* a, hipStream_t s) {
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
    if (f->n == 0) return BSM_OK;
    BSM_REQUIRE(a->nnz == f->nnz, BSM_ERR_INVALID,
                "nd factor refactor: nnz differs (the matrix has %llu entries, the factored one had %llu)",
                (unsigned long long)a->nnz, (unsigned long long)f->nnz);
    std::lock_guard<std::mutex> lk(f->mu);
    return f->dtype == BSM_F64 ? nd_factor_refactor_t<double>(a, *f, s) : nd_factor_refactor_t<float>(a, *f, s);
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
    const auto pc = std::static_pointer_cast<NdCached>(f->plan);
    return f->dtype == BSM_F64 ? nd_factor_numeric_t<double>(&a, *f, *pc, nd_options(), s)
                               : nd_factor_numeric_t<float>(&a, *f, *pc, nd_options(), s);
}

// refactor's checks of a matrix against the handle, with its messages
static int nd_refactor_matches(const bsm_nd_factor* f, const bsm_csr* a) {
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

int nd_factor_refactor_partial(bsm_nd_factor* f, const bsm_csr* a_old, const bsm_csr* a, uint64_t nc,
                               const uint64_t* rows, const uint64_t* cols, uint64_t* info, hipStream_t s) {
    BSM_TRY(nd_refactor_matches(f, a));
    if (a_old) BSM_TRY(nd_refactor_matches(f, a_old));
    uint64_t inf[3] = {0, 0, a_old ? 0 : nc};
    if (f->n == 0) {
        for (int i = 0; i < 3 && info; ++i) info[i] = inf[i];
        return BSM_OK;
    }
    for (uint64_t e = 0; e < nc && !a_old; ++e)
        BSM_REQUIRE(rows[e] < f->n && cols[e] < f->n, BSM_ERR_OUT_OF_BOUNDS,
                    "nd factor refactor_partial: pair %llu is (%llu, %llu), the matrix is %llu x %llu",
                    (unsigned long long)e, (unsigned long long)rows[e], (unsigned long long)cols[e],
                    (unsigned long long)f->n, (unsigned long long)f->n);
    std::lock_guard<std::mutex> lk(f->mu);
    BSM_REQUIRE(!f->stale_blocks, BSM_ERR_UNSUPPORTED,
                "nd factor refactor_partial: an update or downdate has run since the last factorisation (the fronts' "
                "update blocks are stale); refactor first");
    stage_reset(s);
    BSM_TRY(nd_partial_pattern(a, *f, s));
    if (a_old) BSM_TRY(nd_partial_pattern(a_old, *f, s));
    std::vector<int32_t> start;
    BSM_TRY(nd_partial_starts(*f, a_old, a, nc, rows, cols, start, &inf[2], s));
    stage_mark("nd_partial_owners", s);
    const auto pc = std::static_pointer_cast<NdCached>(f->plan);
    inf[1] = (uint64_t)pc->nn;
    int rc = BSM_OK;
    if (start.empty()) {
        // nothing named, nothing differing: the factor's bits stay
    } else if (pc->lay.plain || !f->valid) {
        // the plain pipeline assembles into F and cannot restart a front; a handle without values has no update
        // blocks to pull: the full numeric factorisation, every front
        rc = f->dtype == BSM_F64 ? nd_factor_numeric_t<double>(a, *f, *pc, nd_options(), s)
                                 : nd_factor_numeric_t<float>(a, *f, *pc, nd_options(), s);
        inf[0] = inf[1];
    } else {
        rc = f->dtype == BSM_F64 ? nd_factor_partial_t<double>(a, *f, start.data(), start.size(), &inf[0], s)
                                 : nd_factor_partial_t<float>(a, *f, start.data(), start.size(), &inf[0], s);
    }
    if (rc != BSM_OK) return rc;
    for (int i = 0; i < 3 && info; ++i) info[i] = inf[i];
    return BSM_OK;
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

// ---- C-ABI: the nd plan cache across handles ----
extern "C" int bsm_nd_cache_clear(void) {
    bsm::NdCache& c = bsm::nd_cache();
    std::vector<bsm::NdCacheEntry> gone;
    {
        std::lock_guard<std::mutex> l(c.mu);
        gone.swap(c.entries);
    }
    return BSM_OK;  // `gone` frees outside the lock (a handle still holding a plan keeps it)
}

extern "C" int bsm_nd_cache_info(uint64_t* entries, uint64_t* kept_bytes, uint64_t* hits, uint64_t* misses) {
    bsm::NdCache& c = bsm::nd_cache();
    std::lock_guard<std::mutex> l(c.mu);
    uint64_t kb = 0;
    for (const auto& e : c.entries) kb += e.plan->kept_bytes;
    if (entries) *entries = c.entries.size();
    if (kept_bytes) *kept_bytes = kb;
    if (hits) *hits = c.hits;
    if (misses) *misses = c.misses;
    return BSM_OK;
}

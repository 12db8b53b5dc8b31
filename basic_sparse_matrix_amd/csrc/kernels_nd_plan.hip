// kernels_nd_plan.hip -- the plan of solve(order="nd") (kernels_nd.hip,
// DESIGN.md §4.9): the device layout of the separator tree's fronts
// (nd_layout), the per-tile lists of A's entries and the factor tasks'
// descriptors (nd_aent_*, nd_task_*), and where plans are kept: on the
// handle and in the cross-handle cache keyed by the pattern's hash
// (nd_obtain_plan). Also the environment's switches (nd_options).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <thread>
#include <utility>
#include <vector>

#include "nd.hpp"
#include "nd_internal.hpp"

namespace bsm {
namespace {

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
// per factor task: its children's blocks (NdPull)
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
// last: the vertices the root owns (nd_analyse), or null
int nd_build_plan(const bsm_csr* a, int64_t leaf, NdLay lay, int threads, size_t es, hipStream_t s, NdCached& C,
                  const std::vector<int64_t>* last = nullptr) {
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
    const int arc = nd_analyse(N, rp, cl, leaf, threads, P, last ? last->data() : nullptr,
                               last ? (int64_t)last->size() : 0);
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
    Join join_fronts{pre_fronts};
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

}  // namespace

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

void nd_cache_trim(size_t budget, const NdCached* keep) {
    NdCache& c = nd_cache();
    std::lock_guard<std::mutex> l(c.mu);
    nd_cache_trim_locked(c, budget, keep);
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

// A refactorisation's matrix against the factored pattern (refactor's messages)
int nd_pattern_same(const bsm_csr* a, const bsm_nd_factor& f, hipStream_t s) {
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

// The plan of a's pattern: the one on the handle, else the cross-handle
// cache's, else a new one (then kept in both, as the switches allow). es > 0:
// a new plan allocates its kept numeric storage while it is built.
// last (non-empty): the plan whose root owns these vertices (§4.9o), always a
// new one and kept nowhere but with the caller: neither cache's key knows the
// set, so neither ever holds, or hands out, such a plan.
int nd_obtain_plan(const bsm_csr* a, const NdOpts& opt, NdLay lay, size_t es, hipStream_t s,
                   std::shared_ptr<NdCached>& pc, const std::vector<int64_t>* last) {
    const bool cache = opt.cache, shared = opt.shared;
    const int64_t leaf = opt.leaf;
    if (last && !last->empty()) {
        pc = std::make_shared<NdCached>();
        return nd_build_plan(a, leaf, lay, opt.threads, es, s, *pc, last);
    }
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

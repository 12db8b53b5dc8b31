// kernels_nd_partial.hip -- the partial refactor of a kept nd factor (below)
#include <algorithm>
#include <cstring>
#include <vector>

#include "nd_internal.hpp"
#include "partial_rule.hpp"

namespace bsm {
namespace {

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
    BSM_TRY(NdHost<T>::grid(true, false, g));
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
    NdDrainOnError drain{s, true};  // the temporaries go back to the thread's cache only after the kernels
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
        BSM_TRY(NdHost<T>::factor_launch(p, g, o_tiles + L.o0, L.cnt, f.fr.as<T>(), f.dv.as<T>(), d_flags, d_tickets + li,
                                    d_status, (T*)nullptr, (const T*)nullptr, C.aent.as<int64_t>(), avb.as<T>(),
                                    o_tq + L.o0, o_pd + 2 * L.o0, nullptr, s));
    }
    BSM_TRY(nd_status_end(true, d_status, drain, "nd_partial_factor", s));
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
        NdDrainOnError drain{s, true};
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
    NdDrainOnError drain{s, true};
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
    BSM_TRY(nd_pattern_same(a, *f, s));
    if (a_old) BSM_TRY(nd_pattern_same(a_old, *f, s));
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
        rc = nd_factor_numeric(a, *f, s);
        inf[0] = inf[1];
    } else {
        rc = f->dtype == BSM_F64 ? nd_factor_partial_t<double>(a, *f, start.data(), start.size(), &inf[0], s)
                                 : nd_factor_partial_t<float>(a, *f, start.data(), start.size(), &inf[0], s);
    }
    if (rc != BSM_OK) return rc;
    for (int i = 0; i < 3 && info; ++i) info[i] = inf[i];
    return BSM_OK;
}

}  // namespace bsm

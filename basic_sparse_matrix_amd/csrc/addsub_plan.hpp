// addsub_plan.hpp -- the host arithmetic of add_sparse / sub_sparse
// (sparse_addsub_dispatch, kernels_sparse.hip): which path a
// call takes, when the output is allocated at its bound, the long rows' chunk
// list, the pieces' starts from the chunks' counts, and where the three
// uploads lie in the pinned staging buffer. The thresholds WROW_CAP, LONG_ROW
// and LR_CHUNK live here and nowhere else; the kernels use them under these
// names. Kept apart so that a plain C++ program drives it
// (tests/cpp/addsub_plan_test.cpp). Header-only, no device types.
//
// Everything is in the unnamed namespace kernels_sparse.hip keeps its kernels
// in: LrChunk is a kernel parameter type, so its namespace is part of those
// kernels' symbols. One translation unit of the library includes this header.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsm {
namespace {

constexpr int WROW_CAP = 2048;      // longest self row + longest rhs row at or below: one wave per row (LDS slots)
constexpr int64_t LONG_ROW = 64;    // la + lb above this: cut the row into pieces (one thread's merge costs
                                    // ~350 ns per step, dependent global loads: a 2,000-entry row took 55 + 108
                                    // us of count + fill at e = 100k)
constexpr int64_t LR_CHUNK = 2048;  // entries of a long row's side per chunk (one workgroup of chunk_reduce)

struct LrChunk {
    int64_t l;     // long-row index
    int64_t side;  // 0: self row, 1: rhs row
    int64_t b, e;  // entry range
    int64_t off;   // occurrences of M in the earlier chunks of the same row side
};

// The output holds at most nnz(a) + nnz(b) entries of 4 + es bytes (column
// and value). Up to 1 GiB it is allocated at that bound, so nothing waits
// for the count; above, the count is read first.
inline bool addsub_out_at_bound(uint64_t nnz_a, uint64_t nnz_b, size_t es) {
    return (nnz_a + nnz_b) * (sizeof(int32_t) + es) <= (1ull << 30);
}

// One wave per row (addsub_wave_path) when both operands are analysed, their
// longest rows fit WROW_CAP together and the output can be allocated at its
// bound; else the general path. BSM_SS_WAVE (env_set, its value as an int):
// 0 the general path always, anything else as unset. max_row_len is only
// meaningful on an analysed operand.
inline bool addsub_wave_rule(bool env_set, int env_value, bool a_analysed, bool b_analysed, uint64_t a_max_row_len,
                             uint64_t b_max_row_len, uint64_t nnz_a, uint64_t nnz_b, size_t es) {
    const bool wave_ok = !env_set || env_value != 0;
    return wave_ok && a_analysed && b_analysed && a_max_row_len + b_max_row_len <= (uint64_t)WROW_CAP &&
           addsub_out_at_bound(nnz_a, nnz_b, es);
}

// ext[4 l ..]: long row l's self entries [ext0, ext1) and rhs entries
// [ext2, ext3). Row by row, self side before rhs side, in steps of LR_CHUNK;
// off is filled by addsub_piece_plan.
inline std::vector<LrChunk> addsub_chunk_list(int64_t n_long, const int64_t* ext) {
    std::vector<LrChunk> hc;
    for (int64_t l = 0; l < n_long; ++l)
        for (int64_t side = 0; side < 2; ++side)
            for (int64_t b0 = ext[4 * l + 2 * side]; b0 < ext[4 * l + 2 * side + 1]; b0 += LR_CHUNK)
                hc.push_back({l, side, b0, std::min(b0 + LR_CHUNK, ext[4 * l + 2 * side + 1]), 0});
    return hc;
}

// hcnt[i]: occurrences of row hc[i].l's largest column M in chunk i. Sets
// every chunk's off, cnt_side[2 l + side] to the side's total, and the
// pieces' starts: row l has one piece per M pair (min of its two sides'
// counts) and the tails. Returns the number of pieces, ps[n_long].
inline int64_t addsub_piece_plan(int64_t n_long, std::vector<LrChunk>& hc, const std::vector<int64_t>& hcnt,
                                 std::vector<int64_t>& cnt_side, std::vector<int64_t>& ps) {
    cnt_side.assign(2 * n_long, 0);
    ps.assign(n_long + 1, 0);
    for (size_t i = 0; i < hc.size(); ++i) {
        hc[i].off = cnt_side[2 * hc[i].l + hc[i].side];
        cnt_side[2 * hc[i].l + hc[i].side] += hcnt[i];
    }
    for (int64_t l = 0; l < n_long; ++l) ps[l + 1] = ps[l] + std::min(cnt_side[2 * l], cnt_side[2 * l + 1]) + 1;
    return ps[n_long];
}

// one workgroup per piece: the grid's x dimension
inline bool addsub_pieces_fit(int64_t n_pieces) { return n_pieces < (1ll << 31); }
// the cuts-only first pass hands the full pass pre_cuts + 1 slots per piece
inline bool addsub_presplit_fits(int64_t n_pieces, int pre_cuts) {
    return (uint64_t)n_pieces * (pre_cuts + 1) < (1ull << 31);
}

// The pinned staging buffer of one call: the chunk list as chunk_reduce reads
// it, the chunk list with its offsets as chunk_pieces reads it (a second
// region: the first copy may still be in flight), and the pieces' starts.
struct AddsubStaging {
    size_t chunks, chunks_off, pstart, total;
};
inline AddsubStaging addsub_staging(size_t chunk_bytes, size_t pstart_bytes) {
    const size_t al = (chunk_bytes + 255) & ~size_t(255);
    return {0, al, 2 * al, 2 * al + pstart_bytes};
}

}  // namespace
}  // namespace bsm

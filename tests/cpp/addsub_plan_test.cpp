// addsub_plan.hpp (the host arithmetic of add_sparse / sub_sparse: the path
// rule, the output-at-bound rule, the long rows' chunk list, the piece plan
// and the staging layout) as a plain C++ program. Every answer is compared
// with one written out here (a literal, or a restatement in other words),
// not with the header's own functions.
// Built with -fsanitize=address,undefined by tests/test_addsub_plan.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "addsub_plan.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_fail;                                                      \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                  \
    } while (0)

using bsm::LrChunk;
constexpr int64_t C = 2048;  // LR_CHUNK, written out

// ---- the path rule ---------------------------------------------------------
// the switch as (set, value): unset, off, on
struct Sw {
    bool set;
    int value;
};
static const Sw UNSET = {false, 0}, OFF = {true, 0}, ON = {true, 1};

static bool wave(Sw sw, bool aa, bool ba, uint64_t amax, uint64_t bmax, uint64_t nnz_a = 5000, uint64_t nnz_b = 5000,
                 size_t es = 8) {
    return bsm::addsub_wave_rule(sw.set, sw.value, aa, ba, amax, bmax, nnz_a, nnz_b, es);
}

static void test_path_rule() {
    // the longest rows' sum against WROW_CAP, however it is split
    for (Sw sw : {UNSET, ON, Sw{true, 7}, Sw{true, -1}}) {
        CHECK(wave(sw, true, true, 2047, 0) && wave(sw, true, true, 0, 2047) && wave(sw, true, true, 1024, 1023));
        CHECK(wave(sw, true, true, 2048, 0) && wave(sw, true, true, 0, 2048) && wave(sw, true, true, 1024, 1024));
        CHECK(wave(sw, true, true, 1, 2047) && wave(sw, true, true, 0, 0));
        CHECK(!wave(sw, true, true, 2049, 0) && !wave(sw, true, true, 0, 2049) && !wave(sw, true, true, 1025, 1024));
        CHECK(!wave(sw, true, true, 1, 2048) && !wave(sw, true, true, 2048, 2048));
        CHECK(!wave(sw, true, true, UINT64_MAX, 0));
        // either operand not analysed: the general path, whatever its (stale) longest row says
        CHECK(!wave(sw, false, true, 10, 10) && !wave(sw, true, false, 10, 10) && !wave(sw, false, false, 0, 0));
    }
    // the switch off: never
    CHECK(!wave(OFF, true, true, 10, 10) && !wave(OFF, true, true, 2048, 0) && !wave(OFF, true, true, 0, 0));
    CHECK(!wave(OFF, false, true, 10, 10) && !wave(OFF, true, true, 2049, 0));

    // the output at its bound: (nnz_a + nnz_b) entries of 4 + es bytes, 2^30 bytes at the most.
    // es = 4: 2^27 entries are 2^30 bytes, one more entry is past it
    const uint64_t at4 = 1ull << 27;
    CHECK(at4 * 8 == (1ull << 30));
    // es = 8: 89478485 entries are 2^30 - 4 bytes (the most that fit), one more is 2^30 + 8
    const uint64_t at8 = 89478485ull;
    CHECK(at8 * 12 == (1ull << 30) - 4 && (at8 + 1) * 12 == (1ull << 30) + 8);
    for (uint64_t in_a : {(uint64_t)0, (uint64_t)1, (uint64_t)1000}) {  // only the sum counts
        CHECK(bsm::addsub_out_at_bound(in_a, at4 - in_a, 4) && !bsm::addsub_out_at_bound(in_a, at4 + 1 - in_a, 4));
        CHECK(bsm::addsub_out_at_bound(in_a, at8 - in_a, 8) && !bsm::addsub_out_at_bound(in_a, at8 + 1 - in_a, 8));
        CHECK(wave(UNSET, true, true, 100, 100, in_a, at4 - in_a, 4));
        CHECK(wave(UNSET, true, true, 100, 100, at8 - in_a, in_a, 8));
        CHECK(!wave(UNSET, true, true, 100, 100, in_a, at4 + 1 - in_a, 4));
        CHECK(!wave(UNSET, true, true, 100, 100, at8 + 1 - in_a, in_a, 8));
    }
    CHECK(bsm::addsub_out_at_bound(0, 0, 4) && bsm::addsub_out_at_bound(0, 0, 8));
    // one byte past 2^30 cannot be reached by whole entries; an entry count whose bytes are far past it
    CHECK(!bsm::addsub_out_at_bound(1ull << 40, 1ull << 40, 8) && !bsm::addsub_out_at_bound(1ull << 29, 0, 4));
    // 4-byte entries at the 8-byte count: past the bound of es = 8, inside that of es = 4
    CHECK(bsm::addsub_out_at_bound(at8 + 1, 0, 4) && !bsm::addsub_out_at_bound(at4, 0, 8));
}

// ---- the chunk list --------------------------------------------------------
// rows given as (self start, self length, rhs start, rhs length)
struct Row {
    int64_t a0, la, b0, lb;
};

static std::vector<int64_t> extents(const std::vector<Row>& rows) {
    std::vector<int64_t> ext;
    for (const Row& r : rows)
        for (int64_t v : {r.a0, r.a0 + r.la, r.b0, r.b0 + r.lb}) ext.push_back(v);
    return ext;
}

// every entry of every side covered exactly once, in order: row by row, self
// side before rhs side, no chunk empty, every chunk but a side's last full
static void check_chunks(const std::vector<Row>& rows, const std::vector<LrChunk>& hc) {
    size_t i = 0;
    for (size_t l = 0; l < rows.size(); ++l)
        for (int64_t side = 0; side < 2; ++side) {
            const int64_t begin = side ? rows[l].b0 : rows[l].a0, len = side ? rows[l].lb : rows[l].la;
            int64_t at = begin;
            while (at < begin + len) {
                CHECK(i < hc.size());
                if (i >= hc.size()) return;
                const LrChunk& ch = hc[i++];
                CHECK(ch.l == (int64_t)l && ch.side == side && ch.off == 0);
                CHECK(ch.b == at && ch.e > ch.b && ch.e - ch.b <= C && ch.e <= begin + len);
                CHECK(ch.e - ch.b == C || ch.e == begin + len);
                at = ch.e;
            }
        }
    CHECK(i == hc.size());
}

static std::vector<LrChunk> chunk_list(const std::vector<Row>& rows) {
    const std::vector<int64_t> ext = extents(rows);
    return bsm::addsub_chunk_list((int64_t)rows.size(), ext.data());
}

static void test_chunk_list() {
    CHECK(sizeof(LrChunk) == 40 && bsm::LR_CHUNK == C && bsm::LONG_ROW == 64 && bsm::WROW_CAP == 2048);
    CHECK(bsm::addsub_chunk_list(0, nullptr).empty());  // n_long = 0
    const int64_t lens[] = {0, 1, C - 1, C, C + 1, 2 * C + 1};
    const size_t n_of[] = {0, 1, 1, 1, 2, 3};  // chunks of a side that long
    for (int ia = 0; ia < 6; ++ia)
        for (int ib = 0; ib < 6; ++ib) {  // each side on its own
            for (Row r : {Row{0, lens[ia], 0, lens[ib]}, Row{777, lens[ia], 123456789, lens[ib]}}) {
                const std::vector<LrChunk> hc = chunk_list({r});
                CHECK(hc.size() == n_of[ia] + n_of[ib]);
                check_chunks({r}, hc);
            }
            // three rows, the middle one with these lengths, extents that do not start at 0
            const std::vector<Row> rows = {{5, C + 1, 9, 70}, {5 + C + 1 + 33, lens[ia], 500, lens[ib]},
                                           {100000, 3, 200000, 3 * C}};
            const std::vector<LrChunk> hc = chunk_list(rows);
            CHECK(hc.size() == 3 + n_of[ia] + n_of[ib] + 4);
            check_chunks(rows, hc);
        }
    // written out: sides of 2 C + 1 and 1 entries from 10 and 20
    const std::vector<LrChunk> hc = chunk_list({{10, 2 * C + 1, 20, 1}});
    CHECK(hc.size() == 4);
    if (hc.size() == 4) {
        CHECK(hc[0].side == 0 && hc[0].b == 10 && hc[0].e == 10 + C);
        CHECK(hc[1].side == 0 && hc[1].b == 10 + C && hc[1].e == 10 + 2 * C);
        CHECK(hc[2].side == 0 && hc[2].b == 10 + 2 * C && hc[2].e == 11 + 2 * C);
        CHECK(hc[3].side == 1 && hc[3].b == 20 && hc[3].e == 21 && hc[3].l == 0);
    }
}

// ---- the piece plan --------------------------------------------------------
struct Plan {
    std::vector<LrChunk> hc;
    std::vector<int64_t> cnt_side, ps;
    int64_t n_pieces;
};

static Plan plan(const std::vector<Row>& rows, const std::vector<int64_t>& hcnt) {
    Plan p;
    p.hc = chunk_list(rows);
    CHECK(p.hc.size() == hcnt.size());
    p.cnt_side = {99, 99, 99};  // stale contents are replaced
    p.ps = {7};
    p.n_pieces = bsm::addsub_piece_plan((int64_t)rows.size(), p.hc, hcnt, p.cnt_side, p.ps);
    return p;
}

static void test_piece_plan() {
    // four rows, one chunk per side: M counts 0:4, 3:5, 5:3 and 4:4 give 1, 4, 4 and 5 pieces
    {
        const Plan p = plan({{0, 100, 0, 100}, {100, 100, 100, 100}, {200, 100, 200, 100}, {300, 100, 300, 100}},
                            {0, 4, 3, 5, 5, 3, 4, 4});
        CHECK((p.ps == std::vector<int64_t>{0, 1, 5, 9, 14}) && p.n_pieces == 14 && p.n_pieces == 1 + 4 + 4 + 5);
        CHECK((p.cnt_side == std::vector<int64_t>{0, 4, 3, 5, 5, 3, 4, 4}));
        for (const LrChunk& ch : p.hc) CHECK(ch.off == 0);  // each the first chunk of its side
    }
    // offsets across 1, 2 and 3 chunks of a side: the running count within the row side, from 0 in every row
    {
        const std::vector<Row> rows = {{0, 3 * C, 0, C}, {3 * C, C + 1, C, 2 * C + 5}, {9 * C, 70, 9 * C, 0}};
        // chunks: row 0 self x3, rhs x1; row 1 self x2, rhs x3; row 2 self x1 (its rhs side is empty)
        const Plan p = plan(rows, {2, 0, 7, 11, 1, 1, 4, 5, 6, 3});
        const int64_t off[] = {0, 2, 2, 0, 0, 1, 0, 4, 9, 0};
        CHECK(p.hc.size() == 10);
        for (size_t i = 0; i < p.hc.size() && i < 10; ++i) CHECK(p.hc[i].off == off[i]);
        CHECK((p.cnt_side == std::vector<int64_t>{9, 11, 2, 15, 3, 0}));
        // min(9, 11) + 1, min(2, 15) + 1, and one piece for the row with an empty side
        CHECK((p.ps == std::vector<int64_t>{0, 10, 13, 14}) && p.n_pieces == 14);
        for (size_t l = 0; l + 1 < p.ps.size(); ++l) CHECK(p.ps[l] < p.ps[l + 1]);
    }
    // no long rows: no pieces
    {
        const Plan p = plan({}, {});
        CHECK(p.n_pieces == 0 && (p.ps == std::vector<int64_t>{0}) && p.cnt_side.empty());
    }
    // the two 2^31 limits from both sides, reached through the counts of one row of two chunks
    const struct {
        int64_t count, pieces;
        bool fit, presplit;
    } edges[] = {{(1ll << 28) - 2, (1ll << 28) - 1, true, true},   // 8 slots per piece: 2^31 - 8
                 {(1ll << 28) - 1, 1ll << 28, true, false},        //                    2^31
                 {(1ll << 31) - 2, (1ll << 31) - 1, true, false},  // the grid's x dimension
                 {(1ll << 31) - 1, 1ll << 31, false, false},
                 {1ll << 40, (1ll << 40) + 1, false, false}};
    for (const auto& e : edges) {
        const Plan p = plan({{0, 100, 0, 100}}, {e.count, e.count + 3});
        CHECK(p.n_pieces == e.pieces && p.ps.back() == e.pieces);
        CHECK(bsm::addsub_pieces_fit(p.n_pieces) == e.fit && bsm::addsub_presplit_fits(p.n_pieces, 7) == e.presplit);
    }
    CHECK(bsm::addsub_pieces_fit(0) && bsm::addsub_pieces_fit(1) && bsm::addsub_presplit_fits(1, 7));
    CHECK(bsm::addsub_presplit_fits((1ll << 30) - 1, 1) && !bsm::addsub_presplit_fits(1ll << 30, 1));
}

// ---- the staging layout ----------------------------------------------------
static void test_staging() {
    const size_t bytes[] = {0, 1, 255, 256, 257}, second[] = {0, 256, 256, 256, 512};
    for (int i = 0; i < 5; ++i)
        for (size_t ps_b : {(size_t)8, (size_t)16, (size_t)4096}) {
            const bsm::AddsubStaging at = bsm::addsub_staging(bytes[i], ps_b);
            CHECK(at.chunks == 0 && at.chunks_off == second[i] && at.pstart == 2 * second[i]);
            CHECK(at.total == 2 * second[i] + ps_b);
            CHECK(at.chunks % 256 == 0 && at.chunks_off % 256 == 0 && at.pstart % 256 == 0);
            // [chunks, +bytes), [chunks_off, +bytes), [pstart, +ps_b) in this order, none over the next
            CHECK(at.chunks + bytes[i] <= at.chunks_off && at.chunks_off + bytes[i] <= at.pstart);
            CHECK(at.pstart + ps_b <= at.total);
        }
    // a chunk list of 3 records (120 bytes) and 2 long rows
    const bsm::AddsubStaging at = bsm::addsub_staging(3 * sizeof(LrChunk), 3 * sizeof(int64_t));
    CHECK(at.chunks == 0 && at.chunks_off == 256 && at.pstart == 512 && at.total == 536);
}

int main() {
    test_path_rule();
    test_chunk_list();
    test_piece_plan();
    test_staging();
    std::printf("addsub_plan: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

// spmm_rule.hpp (which kernel launch_spmm launches, and when the integer split
// schedule replaces it) as a plain C++ program: every threshold from both
// sides, every value of the three A/B overrides and junk ones, written out as
// expected kernels, not as a second copy of the rule.
// Built with -fsanitize=address,undefined by tests/test_spmm_rule.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "spmm_rule.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_fail;                                                      \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                  \
    } while (0)

using K = bsm::SpmmKernel;
constexpr uint64_t UNKNOWN = UINT64_MAX;

// the six scalar types as (is_f64, is_float)
struct Ty {
    bool f64, flt;
};
static const Ty TYPES[] = {{true, true}, {false, true}, {false, false}};

static K rule(Ty t, uint64_t rows, uint64_t nnz, uint64_t k, uint64_t max_len, bool aligned = true, int sv = 0,
              int items = 4, int mv = 0) {
    return bsm::spmm_kernel_rule(t.f64, t.flt, rows, nnz, k, max_len, aligned, sv, items, mv);
}

int main() {
    const Ty F64 = TYPES[0], F32 = TYPES[1], INT = TYPES[2];

    // the codes are part of the C ABI (include/bsm.h)
    CHECK((int)K::None == 0 && (int)K::SpmvThread12 == 1 && (int)K::SpmvWave8 == 2 && (int)K::SpmvWave12 == 3);
    CHECK((int)K::SpmvWave16 == 4 && (int)K::SpmvRows16 == 5 && (int)K::SpmvStream2 == 6 && (int)K::SpmvStream4 == 7);
    CHECK((int)K::SpmvStream8 == 8 && (int)K::K32Rows4U4 == 9 && (int)K::K32Rows4U2 == 10 && (int)K::K32Wave4 == 11);
    CHECK((int)K::K32Wave4Pipe == 12 && (int)K::K32Wave8Pipe == 13 && (int)K::RowWave2_4 == 14);
    CHECK((int)K::RowWave4_4 == 15 && (int)K::RowWave8_4 == 16 && (int)K::RowWave16_8 == 17);
    CHECK((int)K::RowWave32_8 == 18 && (int)K::RowWave64_8 == 19);

    // rows == 0: nothing, whatever else is asked for
    for (Ty t : TYPES)
        for (uint64_t k : {1, 2, 32, 65})
            for (int v = 0; v <= 6; ++v) CHECK(rule(t, 0, 0, k, 0, true, v, 4, v) == K::None);

    for (Ty t : TYPES) {
        // ---- k = 1: nnz == 12 rows against 12 rows + 1, on every override
        for (uint64_t rows : {1ul, 1000ul, 16384ul, 16385ul, (uint64_t)1 << 33}) {
            const uint64_t at = 12 * rows, past = at + 1;
            // default: spmv_thread for few short rows, else spmv_wave<8>
            CHECK(rule(t, rows, at, 1, 48) == (rows <= 16384 ? K::SpmvThread12 : K::SpmvWave8));
            CHECK(rule(t, rows, 0, 1, 0) == (rows <= 16384 ? K::SpmvThread12 : K::SpmvWave8));
            CHECK(rule(t, rows, past, 1, 48) == K::SpmvStream4);
            CHECK(rule(t, rows, at, 1, 48, true, 1) == K::SpmvStream4);
            CHECK(rule(t, rows, at, 1, 48, true, 2) == K::SpmvRows16);
            CHECK(rule(t, rows, at, 1, 48, true, 3) == K::SpmvWave16);
            CHECK(rule(t, rows, at, 1, 48, true, 4) == K::SpmvWave12);
            CHECK(rule(t, rows, at, 1, 48, true, 5) == K::SpmvWave8);
            CHECK(rule(t, rows, at, 1, 48, true, 6) == K::SpmvThread12);
            for (int sv : {-1, 7, 100, INT32_MIN, INT32_MAX})  // junk: the default, but never spmv_thread
                CHECK(rule(t, rows, at, 1, 48, true, sv) == K::SpmvWave8);
            for (int sv = -1; sv <= 8; ++sv) {  // past the average every variant is spmv_stream
                CHECK(rule(t, rows, past, 1, 48, true, sv) == K::SpmvStream4);
                CHECK(rule(t, rows, past, 1, 48, true, sv, 2) == K::SpmvStream2);
                CHECK(rule(t, rows, past, 1, 48, true, sv, 8) == K::SpmvStream8);
            }
            // BSM_SPMV_ITEMS under variant 1, and that it changes nothing else
            for (int items : {2, 4, 8, 0, 1, 3, 5, 6, 7, 9, 16, -2, -8, INT32_MIN, INT32_MAX}) {
                const K want = items == 2 ? K::SpmvStream2 : items == 8 ? K::SpmvStream8 : K::SpmvStream4;
                CHECK(rule(t, rows, at, 1, 48, true, 1, items) == want);
                CHECK(rule(t, rows, past, 1, 48, true, 0, items) == want);
                CHECK(rule(t, rows, at, 1, 48, true, 5, items) == K::SpmvWave8);
                CHECK(rule(t, rows, at, 2, 48, true, 0, items) == K::RowWave2_4);
            }
            // alignment and BSM_SPMM_VARIANT do not touch k = 1
            for (int mv = -1; mv <= 7; ++mv) {
                CHECK(rule(t, rows, at, 1, 49, false, 0, 4, mv) == K::SpmvWave8);
                CHECK(rule(t, rows, past, 1, 49, false, 0, 4, mv) == K::SpmvStream4);
            }
        }
        // ---- spmv_thread: rows 16384 / 16385 crossed with max_row_len 48 / 49 / unknown
        CHECK(rule(t, 16384, 100, 1, 48) == K::SpmvThread12);
        CHECK(rule(t, 16384, 100, 1, 49) == K::SpmvWave8);
        CHECK(rule(t, 16385, 100, 1, 48) == K::SpmvWave8);
        CHECK(rule(t, 16385, 100, 1, 49) == K::SpmvWave8);
        CHECK(rule(t, 1, 1, 1, 0) == K::SpmvThread12);
        for (uint64_t rows : {1ul, 3ul, 1024ul, 16384ul, 16385ul})  // the device-level call
            CHECK(rule(t, rows, rows, 1, UNKNOWN) == K::SpmvWave8);
        CHECK(rule(t, 1024, 1024, 1, UNKNOWN, true, 6) == K::SpmvThread12);  // forced only

        // ---- k >= 2 outside k = 32 f64: the row-wave family by k alone
        struct {
            uint64_t k;
            K want;
        } const ks[] = {{2, K::RowWave2_4},   {3, K::RowWave4_4},   {4, K::RowWave4_4},   {5, K::RowWave8_4},
                        {8, K::RowWave8_4},   {9, K::RowWave16_8},  {16, K::RowWave16_8}, {17, K::RowWave32_8},
                        {31, K::RowWave32_8}, {33, K::RowWave64_8}, {64, K::RowWave64_8}, {65, K::RowWave64_8},
                        {128, K::RowWave64_8}, {129, K::RowWave64_8}, {(uint64_t)1 << 20, K::RowWave64_8}};
        for (auto c : ks)
            for (int mv = -1; mv <= 7; ++mv)
                for (bool al : {true, false})
                    for (int sv = 0; sv <= 6; ++sv) {
                        CHECK(rule(t, 1000, 5000, c.k, 40, al, sv, 4, mv) == c.want);
                        CHECK(rule(t, 1000, 50000, c.k, UNKNOWN, al, sv, 8, mv) == c.want);
                    }
        if (!t.f64)  // k = 32 of every other type: row-wave<32, 8>, aligned or not, any variant
            for (int mv = -1; mv <= 7; ++mv)
                for (bool al : {true, false}) {
                    CHECK(rule(t, 1000, 5000, 32, 40, al, 0, 4, mv) == K::RowWave32_8);
                    CHECK(rule(t, 1000, 50000, 32, 400, al, 0, 4, mv) == K::RowWave32_8);
                }
    }

    // ---- k = 32 f64: nnz == 24 rows against 24 rows + 1, every BSM_SPMM_VARIANT
    for (uint64_t rows : {1ul, 901ul, (uint64_t)1 << 31}) {
        const uint64_t at = 24 * rows, past = at + 1;
        for (uint64_t ml : {0ul, 24ul, 5000ul, UNKNOWN}) {  // the longest row plays no part
            CHECK(rule(F64, rows, at, 32, ml) == K::K32Rows4U4);
            CHECK(rule(F64, rows, 0, 32, ml) == K::K32Rows4U4);
            CHECK(rule(F64, rows, past, 32, ml) == K::K32Wave4Pipe);
            for (uint64_t nnz : {at, past}) {
                CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, 1) == K::RowWave32_8);
                CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, 2) == K::K32Wave4);
                CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, 3) == K::K32Wave4Pipe);
                CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, 4) == K::K32Wave8Pipe);
                CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, 5) == K::K32Rows4U4);
                CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, 6) == K::K32Rows4U2);
                for (int mv : {-1, 7, 99, INT32_MIN, INT32_MAX})  // junk: one row per wave, pipelined x4
                    CHECK(rule(F64, rows, nnz, 32, ml, true, 0, 4, mv) == K::K32Wave4Pipe);
                // misaligned x or y: the generic kernel, whatever the variant
                for (int mv = -1; mv <= 7; ++mv) CHECK(rule(F64, rows, nnz, 32, ml, false, 0, 4, mv) == K::RowWave32_8);
                // BSM_SPMV_* do not touch k = 32
                for (int sv = 0; sv <= 6; ++sv)
                    for (int items : {2, 4, 8, 0})
                        CHECK(rule(F64, rows, nnz, 32, ml, true, sv, items) ==
                              (nnz == at ? K::K32Rows4U4 : K::K32Wave4Pipe));
            }
        }
    }
    // k next to 32 in f64 is the generic family
    CHECK(rule(F64, 10, 10, 31, 1) == K::RowWave32_8);
    CHECK(rule(F64, 10, 10, 33, 1) == K::RowWave64_8);
    CHECK(rule(F32, 10, 10, 32, 1) == K::RowWave32_8);
    CHECK(rule(INT, 10, 10, 32, 1) == K::RowWave32_8);

    // ---- the split schedule: max_row_len 8191 / 8192, k 1 / 2, floats never, env 0 / 1 / junk
    using bsm::spmm_split_rule;
    CHECK(!spmm_split_rule(false, 2, 8191, false, 0));
    CHECK(spmm_split_rule(false, 2, 8192, false, 0));
    CHECK(spmm_split_rule(false, 2, UNKNOWN, false, 0));
    CHECK(!spmm_split_rule(false, 1, 8192, false, 0));
    CHECK(!spmm_split_rule(false, 0, 8192, false, 0));
    CHECK(!spmm_split_rule(false, 1, UNKNOWN, false, 0));
    CHECK(spmm_split_rule(false, 129, 8192, false, 0));
    CHECK(spmm_split_rule(false, 2, 8192, false, 1));  // env_value is ignored while env_set is false
    CHECK(!spmm_split_rule(false, 2, 8191, false, 1));
    for (uint64_t ml : {0ul, 8191ul, 8192ul, UNKNOWN}) {
        CHECK(!spmm_split_rule(false, 2, ml, true, 0));  // BSM_SPMM_SPLIT=0: never
        for (int e : {1, 2, -1, INT32_MIN, INT32_MAX}) {
            CHECK(spmm_split_rule(false, 2, ml, true, e));  // set and nonzero: always, from k = 2 on
            CHECK(spmm_split_rule(false, 65, ml, true, e));
            CHECK(!spmm_split_rule(false, 1, ml, true, e));
            CHECK(!spmm_split_rule(true, 2, ml, true, e));  // floats never: their sums are ordered
            CHECK(!spmm_split_rule(true, 1, ml, true, e));
        }
        CHECK(!spmm_split_rule(true, 2, ml, false, 0));
        CHECK(!spmm_split_rule(true, 32, ml, false, 0));
    }

    CHECK(bsm::spmv_items_rule(2) == 2 && bsm::spmv_items_rule(4) == 4 && bsm::spmv_items_rule(8) == 8);
    CHECK(bsm::spmv_items_rule(0) == 4 && bsm::spmv_items_rule(-8) == 4 && bsm::spmv_items_rule(16) == 4);

    std::printf("spmm_rule: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

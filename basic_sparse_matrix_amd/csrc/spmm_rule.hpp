// spmm_rule.hpp -- which kernel Y = A X runs (launch_spmm, kernels_spmm.hip;
// DESIGN.md "SpMM kernels") and whether the integer split schedule replaces
// it (spmm_wants_split), as host rules over the shape and the A/B overrides.
// launch_spmm reads the environment and switches on spmm_kernel_rule's answer;
// bsm_dev_spmm_kernel (include/bsm.h) reads the same environment and returns
// the same answer, so a test can name the kernel it compares. The thresholds
// live here and nowhere else. Kept apart so that a plain C++ program drives
// it (tests/cpp/spmm_rule_test.cpp). Header-only, no device types.
#pragma once

#include <cstdint>

namespace bsm {

// One value per kernel instantiation launch_spmm can launch; the values are
// bsm_dev_spmm_kernel's return codes (include/bsm.h), so they do not move.
enum class SpmmKernel : int {
    None = 0,          // rows == 0: nothing is launched
    SpmvThread12 = 1,  // spmv_thread<T, 12>
    SpmvWave8 = 2,     // spmv_wave<T, 8>
    SpmvWave12 = 3,
    SpmvWave16 = 4,
    SpmvRows16 = 5,    // spmv_rows<T, 16>
    SpmvStream2 = 6,   // spmv_stream<T, 2>
    SpmvStream4 = 7,
    SpmvStream8 = 8,
    K32Rows4U4 = 9,    // spmm_k32_f64_rows4<4>
    K32Rows4U2 = 10,   // spmm_k32_f64_rows4<2>
    K32Wave4 = 11,     // spmm_k32_f64<4, false>
    K32Wave4Pipe = 12, // spmm_k32_f64<4, true>
    K32Wave8Pipe = 13, // spmm_k32_f64<8, true>
    RowWave2_4 = 14,   // spmm_rowwave<T, 2, 4>
    RowWave4_4 = 15,
    RowWave8_4 = 16,
    RowWave16_8 = 17,
    RowWave32_8 = 18,
    RowWave64_8 = 19,
};

constexpr uint64_t SHORT_ROW_AVG = 24;  // k = 32 f64, nnz/rows at or below: four rows per wave
constexpr uint64_t SPMV_THREAD_ROWS = 16384, SPMV_THREAD_MAX_LEN = 48;  // spmv_thread's shapes
constexpr uint64_t SPMV_ROWS_AVG = 12;    // k = 1, nnz/rows at or below: the rows-blocked SpMV kernels
constexpr uint64_t SPLIT_MIN_ROW = 8192;  // integers, k >= 2: the split kernel when some row is this long

// spmv_stream's entries per thread from BSM_SPMV_ITEMS (2, 4 or 8; anything else is 4)
inline int spmv_items_rule(int env_items) { return (env_items == 2 || env_items == 8) ? env_items : 4; }

// is_f64 / is_float: the scalar type. max_row_len: the longest row, UINT64_MAX
// when unknown (the device-level call: never spmv_thread). xy_aligned16: both
// dense operands on 16-byte addresses (the k = 32 f64 kernels load double2).
// spmv_variant = BSM_SPMV_VARIANT (0 when unset): 1 spmv_stream, 2 spmv_rows<16>,
// 3/4/5 spmv_wave<16/12/8>, 6 spmv_thread, anything else as 0 but never
// spmv_thread. spmv_items = BSM_SPMV_ITEMS (4 when unset). spmm_variant =
// BSM_SPMM_VARIANT (0 when unset): 1 generic row-wave, 2 k32 unpipelined,
// 3 pipelined x4, 4 pipelined x8, 5 / 6 four rows per wave with U = 4 / 2.
inline SpmmKernel spmm_kernel_rule(bool is_f64, bool is_float, uint64_t rows, uint64_t nnz, uint64_t k,
                                   uint64_t max_row_len, bool xy_aligned16, int spmv_variant, int spmv_items,
                                   int spmm_variant) {
    (void)is_float;  // no threshold depends on it today; the split rule below does
    if (rows == 0) return SpmmKernel::None;
    // short rows on average (C2: 10): the rows-blocked SpMV; BSM_SPMV_VARIANT=1
    // forces the nnz-balanced spmv_stream (A/B)
    if (k == 1 && nnz <= SPMV_ROWS_AVG * rows && spmv_variant != 1) {
        switch (spmv_variant) {
        case 2: return SpmmKernel::SpmvRows16;  // the workgroup-chunk version (A/B)
        case 3: return SpmmKernel::SpmvWave16;
        case 4: return SpmmKernel::SpmvWave12;
        case 5: return SpmmKernel::SpmvWave8;
        case 6: return SpmmKernel::SpmvThread12;
        default: break;
        }
        // few short rows (C1: 1,024 x ~10): latency-bound, one thread per row
        // has the fewest dependent round trips (4.5 against 6.4 us at C1,
        // profiles/r05_z_*)
        if (spmv_variant == 0 && rows <= SPMV_THREAD_ROWS && max_row_len <= SPMV_THREAD_MAX_LEN)
            return SpmmKernel::SpmvThread12;
        // default (C2: 111 us against 117-167 for the others, scripts/perf/spmv_variants.py)
        return SpmmKernel::SpmvWave8;
    }
    if (k == 1) {
        const int items = spmv_items_rule(spmv_items);
        return items == 2 ? SpmmKernel::SpmvStream2 : items == 8 ? SpmmKernel::SpmvStream8 : SpmmKernel::SpmvStream4;
    }
    if (is_f64 && k == 32 && spmm_variant != 1 && xy_aligned16) {
        // short rows on average: four rows per wave (variants 5/6 force it)
        const bool short_rows = nnz <= SHORT_ROW_AVG * rows;
        if (spmm_variant == 6) return SpmmKernel::K32Rows4U2;
        if (spmm_variant == 5 || (spmm_variant == 0 && short_rows)) return SpmmKernel::K32Rows4U4;
        if (spmm_variant == 2) return SpmmKernel::K32Wave4;
        if (spmm_variant == 4) return SpmmKernel::K32Wave8Pipe;
        return SpmmKernel::K32Wave4Pipe;
    }
    if (k <= 2) return SpmmKernel::RowWave2_4;
    if (k <= 4) return SpmmKernel::RowWave4_4;
    if (k <= 8) return SpmmKernel::RowWave8_4;
    if (k <= 16) return SpmmKernel::RowWave16_8;
    if (k <= 32) return SpmmKernel::RowWave32_8;
    return SpmmKernel::RowWave64_8;
}

// The nnz-balanced integer schedule (spmm_split_dispatch) in place of the
// kernel above: integers only (their sums wrap, so they are order-free), k >= 2,
// and some row of SPLIT_MIN_ROW entries or more; BSM_SPMM_SPLIT (env_set, its
// value as an int) replaces the row-length test: 0 never, anything else always.
inline bool spmm_split_rule(bool is_float, uint64_t k, uint64_t max_row_len, bool env_set, int env_value) {
    if (is_float || k < 2) return false;
    if (env_set) return env_value != 0;
    return max_row_len >= SPLIT_MIN_ROW;
}

}  // namespace bsm

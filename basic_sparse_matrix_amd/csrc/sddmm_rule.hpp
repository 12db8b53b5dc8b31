// sddmm_rule.hpp -- the order of the SDDMM's dot product (kernels_sddmm.hip;
// DESIGN.md §4.9m). Host and device code, no HIP calls: the kernel follows
// this rule with shuffles, the CPU test (tests/cpp/sddmm_rule_test.cpp) and
// the GPU tests' numpy restatement check it.
//
// dot(u, v) over k columns: t[c] = u[c] * v[c] (rounded), then for k <= 64 a
// tree of width W = the smallest power of two >= k: for h = W/2, W/4, ..., 1
// t[c] += t[c + h] for every c < h whose partner exists (c + h < live), and
// the live terms become the first min(live, h). For k > 64 the columns go in
// chunks of 64, each reduced by that tree, and the chunk sums are added in
// ascending chunk order. The order depends on k alone.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define BSM_SDDMM_HD __host__ __device__
#else
#define BSM_SDDMM_HD
#endif

namespace bsm {

constexpr uint64_t SDDMM_CHUNK = 64;  // columns per tree: one lane each

// W(k): the smallest power of two >= k (k >= 1)
BSM_SDDMM_HD inline uint64_t sddmm_width(uint64_t k) {
    uint64_t w = 1;
    while (w < k) w *= 2;
    return w;
}

// the lanes that share one stored entry: W(k), at most a wave
BSM_SDDMM_HD inline uint32_t sddmm_lanes(uint64_t k) {
    return (uint32_t)(k >= SDDMM_CHUNK ? SDDMM_CHUNK : sddmm_width(k));
}

// the tree over t[0..k), 1 <= k <= 64, in place; the result is t[0]
template <typename T>
BSM_SDDMM_HD inline T sddmm_tree64(T* t, uint64_t k) {
    uint64_t live = k;
    for (uint64_t h = sddmm_width(k) / 2; h >= 1; h /= 2) {
        for (uint64_t c = 0; c < h && c + h < live; ++c) t[c] = t[c] + t[c + h];
        if (h < live) live = h;
    }
    return t[0];
}

// the sum of the k >= 1 products t[0..k) in the SDDMM's order (t is scratch)
template <typename T>
BSM_SDDMM_HD inline T sddmm_tree(T* t, uint64_t k) {
    T acc = sddmm_tree64(t, k < SDDMM_CHUNK ? k : SDDMM_CHUNK);
    for (uint64_t c0 = SDDMM_CHUNK; c0 < k; c0 += SDDMM_CHUNK)
        acc = acc + sddmm_tree64(t + c0, k - c0 < SDDMM_CHUNK ? k - c0 : SDDMM_CHUNK);
    return acc;
}

}  // namespace bsm

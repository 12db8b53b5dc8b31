// Stand-alone CPU test of csrc/sddmm_rule.hpp (the order of the SDDMM's dot
// product), built with -fsanitize=address,undefined by
// tests/test_sddmm_rule.py: sddmm_tree against an independently written
// recursive pairwise definition for k = 1..130 in f32 and f64 (bit for bit),
// and W(k) / the lanes per entry at the sizes where they change.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "sddmm_rule.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) {                                                             \
            ++g_fail;                                                              \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                          \
    } while (0)

// The value that sits at position c once the array is w wide, top-down: at
// the top width the product itself; below it the position's own value one
// width up plus its partner's at c + w, where that partner exists among the k
// terms. The whole sum is the value at position 0 of width 1.
template <typename T>
static T at(const T* t, uint64_t k, uint64_t top, uint64_t c, uint64_t w) {
    if (w == top) return t[c];
    const T own = at(t, k, top, c, 2 * w);
    if (c + w >= k) return own;
    return own + at(t, k, top, c + w, 2 * w);
}

template <typename T>
static T reference(const T* t, uint64_t k) {
    T acc = T(0);
    for (uint64_t c0 = 0; c0 < k; c0 += 64) {
        const uint64_t kk = k - c0 < 64 ? k - c0 : 64;
        uint64_t top = 1;
        while (top < kk) top *= 2;
        const T part = at(t + c0, kk, top, 0, 1);
        acc = c0 ? acc + part : part;
    }
    return acc;
}

template <typename T>
static bool same_bits(T a, T b) {
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

template <typename T>
static void run(std::mt19937_64& rng) {
    std::normal_distribution<double> nd(0.0, 1.0);
    for (uint64_t k = 1; k <= 130; ++k) {
        for (int rep = 0; rep < 8; ++rep) {
            std::vector<T> t(k), scratch;  // exactly k: the sanitizer sees a read past the live terms
            for (auto& x : t) {
                const double d = nd(rng) * (rep % 2 ? 1e6 : 1.0);
                x = (rng() % 9 == 0) ? (rng() % 2 ? T(0) : -T(0)) : (T)d;
            }
            scratch = t;
            const T got = bsm::sddmm_tree<T>(scratch.data(), k);
            CHECK(same_bits(got, reference<T>(t.data(), k)));
        }
    }
    // the signs of zero survive: no term is added to a +0 that is not there
    for (uint64_t k : {1u, 2u, 3u, 64u, 65u, 128u, 130u}) {
        std::vector<T> t(k, -T(0));
        const T got = bsm::sddmm_tree<T>(t.data(), k);
        CHECK(same_bits(got, -T(0)));
    }
}

int main() {
    std::mt19937_64 rng(20240607);
    run<float>(rng);
    run<double>(rng);
    const uint64_t ks[] = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 129};
    const uint64_t ws[] = {1, 2, 4, 4, 8, 32, 32, 64, 64, 64, 128, 256};
    const uint32_t ls[] = {1, 2, 4, 4, 8, 32, 32, 64, 64, 64, 64, 64};
    for (int i = 0; i < 12; ++i) {
        CHECK(bsm::sddmm_width(ks[i]) == ws[i]);
        CHECK(bsm::sddmm_lanes(ks[i]) == ls[i]);
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}

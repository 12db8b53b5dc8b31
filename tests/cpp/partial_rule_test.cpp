// partial_rule.hpp (the launch plan of a partial refactor) as a plain C++
// program: on random forests with random tile rows per node and the plan's
// per-level task lists built the way nd_layout builds them (every lower tile of
// every front of the level, interleaved across the fronts), partial_plan's
// levels, counts, places and chunks against a brute-force selection.
// Built with -fsanitize=address,undefined by tests/test_partial_rule.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "partial_rule.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_fail;                                                      \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                  \
    } while (0)

int main() {
    std::mt19937 rng(12345);
    for (int trial = 0; trial < 300; ++trial) {
        // a forest: node i's parent is a later node or none; level = height
        const int nn = 1 + (int)(rng() % 40);
        std::vector<int32_t> parent((size_t)nn, -1), level((size_t)nn, 0), nt((size_t)nn);
        for (int i = 0; i < nn; ++i) {
            if (i + 1 < nn && rng() % 5) parent[(size_t)i] = i + 1 + (int)(rng() % (unsigned)(nn - i - 1));
            nt[(size_t)i] = (int32_t)(rng() % 5);  // 0: a front without tiles
        }
        for (int i = 0; i < nn; ++i)
            if (parent[(size_t)i] >= 0) level[(size_t)parent[(size_t)i]] = std::max(level[(size_t)parent[(size_t)i]], level[(size_t)i] + 1);
        int n_levels = 0;
        for (int i = 0; i < nn; ++i) n_levels = std::max(n_levels, level[(size_t)i] + 1);
        // the plan's tasks per level: column K of every front, then the next column
        std::vector<int32_t> task_node;
        std::vector<int64_t> tiles_off;
        for (int lv = 0; lv < n_levels; ++lv) {
            tiles_off.push_back((int64_t)task_node.size());
            for (int K = 0; K < 5; ++K)
                for (int i = 0; i < nn; ++i)
                    if (level[(size_t)i] == lv)
                        for (int I = K; I < nt[(size_t)i]; ++I) task_node.push_back(i);
        }
        tiles_off.push_back((int64_t)task_node.size());
        const size_t ns = rng() % 6;
        std::vector<int32_t> start(ns);
        for (auto& s : start) s = rng() % 7 ? (int32_t)(rng() % (unsigned)nn) : -1;
        std::vector<unsigned char> mark;
        bsm::ReachSet R;
        bsm::reach_set((size_t)nn, parent.data(), level.data(), nullptr, nullptr, start.data(), ns, mark, R);
        const int32_t chunk = 1 + (int32_t)(rng() % 7);
        bsm::PartialPlan P;
        bsm::partial_plan(R, nt.data(), tiles_off.data(), chunk, P);
        CHECK(P.levels.size() == R.levels.size());
        int64_t run = 0;
        size_t nchunks = 0;
        for (size_t li = 0; li < P.levels.size(); ++li) {
            const bsm::PartialLevel& L = P.levels[li];
            CHECK(L.level == R.levels[li].first);
            CHECK(L.t0 == tiles_off[(size_t)L.level] && L.t0 + L.nt == tiles_off[(size_t)L.level + 1]);
            int64_t want = 0;
            for (int64_t t = L.t0; t < L.t0 + L.nt; ++t) want += mark[(size_t)task_node[(size_t)t]];
            CHECK(L.cnt == want && L.o0 == run);
            run += L.cnt;
            // the chunks tile [t0, t0 + nt) in order, none empty, none longer than `chunk`
            CHECK(L.c0 == (int32_t)nchunks);
            int64_t at = L.t0;
            for (int32_t c = 0; c < L.nchunks; ++c) {
                const bsm::PartialChunk& ch = P.chunks[(size_t)(L.c0 + c)];
                CHECK(ch.t0 == at && ch.len >= 1 && ch.len <= chunk && ch.li == (int32_t)li);
                at += ch.len;
            }
            CHECK(at == L.t0 + L.nt);
            nchunks += (size_t)L.nchunks;
        }
        CHECK(P.total == run && P.chunks.size() == nchunks);
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}

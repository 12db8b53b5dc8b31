// partial_rule.hpp -- the launch plan of a partial refactor of a kept factor
// (bsm_nd_factor_refactor_partial, kernels_nd_partial.hip). Given the
// active fronts (reach_rule.hpp: the paths from the changed entries' fronts to
// the roots, in (level, node) order), every level that occurs re-runs nd_factor
// on the active fronts' tasks alone, in the plan's own order. A front of nt
// tile rows has nt (nt + 1) / 2 tasks, one per lower tile, all on its level, so
// the host knows each level's selected count and where its selected tasks go
// in the contiguous arrays before the device has marked one. The level's tasks
// [t0, t0 + nt) are cut into chunks of `chunk` for the device's mark / scan /
// scatter. Header-only, no device types (tests/cpp/partial_rule_test.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "reach_rule.hpp"

namespace bsm {

// one level that occurs: its tasks in the plan, its selected tasks' place and
// count in the contiguous arrays, its chunks
struct PartialLevel {
    int64_t t0, nt;   // the plan's tasks of this level: tiles[t0 .. t0 + nt)
    int64_t o0, cnt;  // the selected ones: out[o0 .. o0 + cnt)
    int32_t level, c0, nchunks, pad;
};

// tasks [t0, t0 + len) of the plan, len <= chunk, of levels[li]
struct PartialChunk {
    int64_t t0;
    int32_t len, li;
};

struct PartialPlan {
    std::vector<PartialLevel> levels;
    std::vector<PartialChunk> chunks;
    int64_t total = 0;  // selected tasks over all levels
};

// node_nt: tile rows per node; tiles_off: n_levels + 1 task offsets per level
inline void partial_plan(const ReachSet& R, const int32_t* node_nt, const int64_t* tiles_off, int32_t chunk,
                         PartialPlan& out) {
    out.levels.clear();
    out.chunks.clear();
    out.total = 0;
    for (size_t li = 0; li < R.levels.size(); ++li) {
        const int32_t lv = R.levels[li].first;
        PartialLevel L{};
        L.level = lv;
        L.t0 = tiles_off[(size_t)lv];
        L.nt = tiles_off[(size_t)lv + 1] - L.t0;
        L.o0 = out.total;
        for (int32_t i = R.first(li); i < R.last(li); ++i) {
            const int64_t nt = node_nt[(size_t)R.fronts[(size_t)i].node];
            L.cnt += nt * (nt + 1) / 2;
        }
        L.c0 = (int32_t)out.chunks.size();
        for (int64_t t = 0; t < L.nt; t += chunk) {
            const int64_t len = L.nt - t < chunk ? L.nt - t : chunk;
            out.chunks.push_back(PartialChunk{L.t0 + t, (int32_t)len, (int32_t)li});
        }
        L.nchunks = (int32_t)out.chunks.size() - L.c0;
        out.total += L.cnt;
        out.levels.push_back(L);
    }
}

}  // namespace bsm

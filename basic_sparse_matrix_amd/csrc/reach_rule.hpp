// reach_rule.hpp -- which fronts a solve with a sparse right-hand side and
// selected solution rows has to visit (bsm_nd_factor_solve_sparse,
// kernels_nd_sparse.hip). On the separator tree (a forest: every
// node has a parent or is a root, at most two children kid0 / kid1, a level =
// its height, children on lower levels than their parent) the set reached from
// some start nodes is the union of their paths to the roots:
//   forward   from the fronts owning the rows of b: every other front has
//             v = 0, hence y = 0 and an update vector of +0;
//   backward  from the fronts owning the requested rows: x over a front's
//             pivots needs its own y and its ancestors' x, nothing else.
// The set comes out in (level, node) order with the first place of every level
// that occurs (one launch per level), and per front which of its two children
// are in the set (the forward pass adds the update vectors of those alone,
// kid0 before kid1). This is nd_updown_plan's walk, kept apart so that a plain
// C++ program drives it (tests/cpp/reach_rule_test.cpp). Header-only, no
// device types.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace bsm {

// one front of a reached set: `kids` bit 0 = kid0 is in the set, bit 1 = kid1
struct ReachFront {
    int32_t node;
    int32_t kids;
};

struct ReachSet {
    std::vector<ReachFront> fronts;                   // (level, node) ascending
    std::vector<std::pair<int32_t, int32_t>> levels;  // per level that occurs, ascending: the level, its first place in fronts
    // the fronts of levels[li]: [first, last)
    int32_t first(size_t li) const { return levels[li].second; }
    int32_t last(size_t li) const { return li + 1 < levels.size() ? levels[li + 1].second : (int32_t)fronts.size(); }
};

// parent / level / kid0 / kid1: nn entries each (-1: none); kid0 / kid1 may
// both be null (every `kids` is then 0). start: ns nodes, any order, repeats
// allowed, a negative entry is skipped (an empty column). mark: scratch, left
// as the set's indicator (nn entries, 1 = reached). A walk stops at the first
// front already reached, so the cost is the size of the set plus ns.
inline void reach_set(size_t nn, const int32_t* parent, const int32_t* level, const int32_t* kid0,
                      const int32_t* kid1, const int32_t* start, size_t ns, std::vector<unsigned char>& mark,
                      ReachSet& out) {
    mark.assign(nn, 0);
    out.fronts.clear();
    out.levels.clear();
    std::vector<int32_t> nodes;
    for (size_t i = 0; i < ns; ++i)
        for (int32_t x = start[i]; x >= 0 && !mark[(size_t)x]; x = parent[(size_t)x]) {
            mark[(size_t)x] = 1;
            nodes.push_back(x);
        }
    std::sort(nodes.begin(), nodes.end(), [&](int32_t a, int32_t b) {
        const int32_t la = level[(size_t)a], lb = level[(size_t)b];
        return la != lb ? la < lb : a < b;
    });
    out.fronts.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        const int32_t x = nodes[i], lv = level[(size_t)x];
        int32_t kids = 0;
        if (kid0 && kid0[(size_t)x] >= 0 && mark[(size_t)kid0[(size_t)x]]) kids |= 1;
        if (kid1 && kid1[(size_t)x] >= 0 && mark[(size_t)kid1[(size_t)x]]) kids |= 2;
        out.fronts[i] = ReachFront{x, kids};
        if (out.levels.empty() || out.levels.back().first != lv) out.levels.emplace_back(lv, (int32_t)i);
    }
}

}  // namespace bsm

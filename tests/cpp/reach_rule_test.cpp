// csrc/reach_rule.hpp against a brute-force union of root paths, on small
// random forests shaped as the separator tree is: nodes in post-order, at most
// two children, level = height. The forests have roots on several levels,
// nodes with one child (in either slot) and isolated nodes; the start sets are
// empty, single, repeated, with skipped (-1) entries, and everything. Built
// with -fsanitize=address,undefined by tests/test_reach_rule.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "reach_rule.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_fail;                                                      \
            std::fprintf(stderr, "  CHECK failed: %s (line %d)\n", #cond, __LINE__); \
        }                                                                  \
    } while (0)

struct Forest {
    std::vector<int32_t> parent, level, kid0, kid1;
};

// nodes 0 .. nn - 1 in post-order: a new node adopts 0, 1 or 2 of the current roots
static Forest make_forest(std::mt19937& rng, int nn) {
    Forest f;
    f.parent.assign((size_t)nn, -1);
    f.level.assign((size_t)nn, 0);
    f.kid0.assign((size_t)nn, -1);
    f.kid1.assign((size_t)nn, -1);
    std::vector<int32_t> roots;
    for (int32_t i = 0; i < nn; ++i) {
        const int want = (int)(rng() % 4);  // 0: a leaf, 1: one child, 2 or 3: two
        const int take = std::min<int>(want > 2 ? 2 : want, (int)roots.size());
        int32_t kids[2] = {-1, -1};
        for (int t = 0; t < take; ++t) {
            const size_t at = rng() % roots.size();
            kids[t] = roots[at];
            roots.erase(roots.begin() + (long)at);
        }
        if (take == 1 && (rng() & 1)) std::swap(kids[0], kids[1]);  // a single child in slot 1
        for (int t = 0; t < 2; ++t)
            if (kids[t] >= 0) {
                f.parent[(size_t)kids[t]] = i;
                f.level[(size_t)i] = std::max(f.level[(size_t)i], f.level[(size_t)kids[t]] + 1);
            }
        f.kid0[(size_t)i] = kids[0];
        f.kid1[(size_t)i] = kids[1];
        roots.push_back(i);
    }
    return f;
}

static void check_one(const Forest& f, const std::vector<int32_t>& start, bool with_kids) {
    const size_t nn = f.parent.size();
    std::set<int32_t> in;
    for (int32_t s : start)
        for (int32_t x = s; x >= 0; x = f.parent[(size_t)x]) in.insert(x);
    std::vector<int32_t> want(in.begin(), in.end());
    std::sort(want.begin(), want.end(), [&](int32_t a, int32_t b) {
        return f.level[(size_t)a] != f.level[(size_t)b] ? f.level[(size_t)a] < f.level[(size_t)b] : a < b;
    });
    std::vector<unsigned char> mark(3, 7);  // stale scratch of another size
    bsm::ReachSet r;
    r.fronts.push_back({99, 3});  // and a stale result
    r.levels.emplace_back(5, 5);
    bsm::reach_set(nn, f.parent.data(), f.level.data(), with_kids ? f.kid0.data() : nullptr,
                   with_kids ? f.kid1.data() : nullptr, start.data(), start.size(), mark, r);
    CHECK(r.fronts.size() == want.size());
    CHECK(mark.size() == nn);
    for (size_t i = 0; i < nn && i < mark.size(); ++i) CHECK((mark[i] != 0) == (in.count((int32_t)i) != 0));
    for (size_t i = 0; i < want.size() && i < r.fronts.size(); ++i) {
        const int32_t x = want[i];
        CHECK(r.fronts[i].node == x);
        int32_t kids = 0;
        if (with_kids && f.kid0[(size_t)x] >= 0 && in.count(f.kid0[(size_t)x])) kids |= 1;
        if (with_kids && f.kid1[(size_t)x] >= 0 && in.count(f.kid1[(size_t)x])) kids |= 2;
        CHECK(r.fronts[i].kids == kids);
    }
    // the levels: ascending, each the first place of its level, together covering every front
    size_t covered = 0;
    for (size_t li = 0; li < r.levels.size(); ++li) {
        CHECK(li == 0 || r.levels[li - 1].first < r.levels[li].first);
        CHECK(r.first(li) == (int32_t)covered);
        CHECK(r.last(li) > r.first(li));
        for (int32_t a = r.first(li); a < r.last(li); ++a)
            CHECK(f.level[(size_t)r.fronts[(size_t)a].node] == r.levels[li].first);
        covered = (size_t)r.last(li);
    }
    CHECK(covered == r.fronts.size());
    CHECK(r.levels.empty() == want.empty());
    // a child is listed before its parent, so a level's launch finds its children done
    std::vector<int32_t> place(nn, -1);
    for (size_t i = 0; i < r.fronts.size(); ++i) place[(size_t)r.fronts[i].node] = (int32_t)i;
    for (const bsm::ReachFront& a : r.fronts) {
        const int32_t p = f.parent[(size_t)a.node];
        if (p >= 0) CHECK(place[(size_t)p] > place[(size_t)a.node]);
    }
}

int main() {
    std::mt19937 rng(20240607u);
    int several_root_levels = 0, one_child = 0;
    for (int rep = 0; rep < 300; ++rep) {
        const int nn = 1 + (int)(rng() % 40);
        const Forest f = make_forest(rng, nn);
        std::set<int32_t> root_levels;
        for (int i = 0; i < nn; ++i) {
            if (f.parent[(size_t)i] < 0) root_levels.insert(f.level[(size_t)i]);
            one_child += (f.kid0[(size_t)i] >= 0) != (f.kid1[(size_t)i] >= 0);
        }
        several_root_levels += root_levels.size() > 1;
        std::vector<int32_t> all((size_t)nn);
        for (int i = 0; i < nn; ++i) all[(size_t)i] = i;
        check_one(f, {}, true);
        check_one(f, {-1, -1}, true);
        check_one(f, all, true);
        check_one(f, all, false);
        for (int t = 0; t < 6; ++t) {
            std::vector<int32_t> start;
            const int ns = 1 + (int)(rng() % 5);
            for (int i = 0; i < ns; ++i) start.push_back(rng() % 7 == 0 ? -1 : (int32_t)(rng() % (unsigned)nn));
            if (t & 1) start.push_back(start[0]);  // a repeat
            check_one(f, start, true);
        }
    }
    CHECK(several_root_levels > 20);  // the forests are what the docstring says
    CHECK(one_child > 100);
    // no nodes at all
    {
        std::vector<unsigned char> mark;
        bsm::ReachSet r;
        bsm::reach_set(0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, mark, r);
        CHECK(r.fronts.empty() && r.levels.empty() && mark.empty());
    }
    std::printf("summary: %d failed, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}

// nd.hpp -- nested-dissection analysis for solve(order="nd") (host C++).
//
// The plan of the multifrontal solve (kernels_nd_plan.hip): a fill-reducing
// permutation from recursive graph bisection (BFS level-set separators) and
// its separator tree, each node a dense front. Pure host code: no HIP here,
// so the CPU tests drive it through bsm_nd_analyse.
#pragma once

#include <cstdint>
#include <vector>

namespace bsm {

struct NdNode {
    int64_t start = 0, end = 0;   // own columns [start, end) in the new order
    int32_t parent = -1;          // -1: a root
    int32_t level = 0;            // height: leaves 0, a parent above its highest child
    int32_t slot = 0;             // index among the parent's children (0 or 1)
    int32_t kids[2] = {-1, -1};
    std::vector<int64_t> st;      // the front's other rows: new indices >= end, ascending
};

struct NdPlan {
    int64_t n = 0;
    std::vector<int64_t> perm;    // perm[new] = old
    std::vector<int64_t> pinv;    // pinv[old] = new
    std::vector<NdNode> nodes;    // children before parents (post-order), roots last
    int32_t n_levels = 0;
    double ms_graph = 0, ms_order = 0, ms_symbolic = 0, ms_bisect = 0;  // ms_order includes ms_bisect
};

// A's pattern (row_ptr: n + 1 entries, col: row_ptr[n]); the matrix is the
// lower triangle (j <= i, as the band path reads it) mirrored, so the graph
// has an edge {i, j} for every stored j < i. leaf: largest part not split
// further; threads: worker threads for the bisection and the symbolic pass.
// last (m distinct vertices < n, any order; nd_last_check's rule; m == 0: none):
// the root node owns exactly these vertices (perm[n - m .. n) = sorted(last))
// and its only child (kids[0]; kids[1] = -1) is the bisection tree of the
// graph induced on the others.
int nd_analyse(int64_t n, const int64_t* row_ptr, const int32_t* col, int64_t leaf, int threads, NdPlan& plan,
               const int64_t* last = nullptr, int64_t m = 0);

// The largest set nd_analyse's `last` may name: its front is dense, (64 ceil(m / 64))^2 values (2 GiB of f64 here)
constexpr int64_t ND_LAST_MAX = 16384;
// 0: `last` holds m distinct vertices < n; 1: entry *bad is >= n; 2: entry *bad repeats an earlier one.
// Allocates m indices, nothing else.
int nd_last_check(int64_t n, const uint64_t* last, uint64_t m, uint64_t* bad);

}  // namespace bsm

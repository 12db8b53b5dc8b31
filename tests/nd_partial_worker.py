"""Child process of test_gpu_nd_partial_refactor.py::test_pipeline_switches: the
environment's switches (BSM_ND_PLAIN / _LAG / _POISON, BSM_ND_LEAF) are set by
the parent before this process starts. Runs a few partial refactors of one
system and prints one JSON line: whether every piece equals a fresh factor's,
whether everything is finite, the fronts each call reported and the expected
path unions."""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import test_gpu_nd_partial_refactor as t  # noqa: E402

from basic_sparse_matrix_amd import cholesky_nd  # noqa: E402
from nd_support import dense_matrix, dense_system, same_bits  # noqa: E402


def main():
    name = sys.argv[1]
    n, s, _, _ = dense_system(name)
    g = t.groups(name)
    equal, finite, fronts, expected, total = True, True, [], [], 0
    for src, fdt in t.DTYPES:
        with cholesky_nd(dense_matrix(s, src), factor_dtype=fdt) as f:
            cur = s
            for gname in ("leaf-diagonal", "two-leaves", "separator", "seeded-17"):
                pairs = g[gname]
                cur = t.changed(cur, pairs)
                info = f.refactor_partial(dense_matrix(cur, src), *t.rc(pairs))
                got, want = t.bits(f, name), t.fresh_bits(cur, name, src, fdt)
                equal = equal and all(same_bits(x, y) for x, y in zip(got, want))
                finite = finite and all(np.isfinite(x).all() for x in got)
                fronts.append(info.fronts)
                expected.append(len(t.reach(name, t.start_vertices(name, pairs))))
                total = info.total_fronts
    print(json.dumps({"equal": bool(equal), "finite": bool(finite), "fronts": fronts, "expected": expected,
                      "total": total}))


if __name__ == "__main__":
    main()

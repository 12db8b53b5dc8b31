"""bench.py --dump-outputs: the files hold the output Csr of the timed path.

CPU: dump_outputs on a host stand-in for the device handle, whole and sampled
(the sampled rows are a fixed choice and carry exactly their entries). GPU:
a run of bench.py on C1 (whole output, 1024 rows) equals the oracle's
mul_dense on the same seeds, bit for bit, and a plain run leaves the figures
of --full out of the result line."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _HostCsr:
    def __init__(self, rows, cols, k, dtype):
        rng = np.random.default_rng(7)
        lens = rng.integers(0, k + 1, rows)
        self.rows, self.cols = rows, cols
        self.rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.nnz = int(self.rp[-1])
        self.ci = rng.integers(0, cols, self.nnz).astype(np.uint64)
        self.v = rng.random(self.nnz).astype(dtype)

    def download(self):
        return self.rp, self.ci, self.v


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dump_whole_and_sampled(tmp_path, monkeypatch, dtype):
    import bench

    rows, k = 1000, 4
    out = _HostCsr(rows, 50, k, dtype)
    bench.dump_outputs(str(tmp_path / "whole"), out, k)
    w = _load(tmp_path / "whole")
    assert sorted(w) == ["col_index", "row_ptr", "rows", "shape", "values"]
    assert w["values"].dtype == dtype and all(a.dtype == np.float64 for n, a in w.items() if n != "values")
    assert np.array_equal(w["rows"], np.arange(rows)) and np.array_equal(w["row_ptr"], out.rp)
    assert np.array_equal(w["col_index"], out.ci) and np.array_equal(w["values"], out.v)
    assert w["shape"].tolist() == [rows, 50, out.nnz]

    per_row = 16 + k * (8 + np.dtype(dtype).itemsize)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100 * per_row)
    bench.dump_outputs(str(tmp_path / "s1"), out, k)
    bench.dump_outputs(str(tmp_path / "s2"), out, k)
    s, s2 = _load(tmp_path / "s1"), _load(tmp_path / "s2")
    assert all(np.array_equal(s[n], s2[n]) for n in s)  # the same rows every time
    sel, ptr = s["rows"].astype(np.int64), s["row_ptr"].astype(np.int64)
    assert sel.size == 100 and np.all(np.diff(sel) > 0) and sel[-1] < rows
    assert sum(a.nbytes for a in s.values()) <= 100 * per_row + 32
    for i, r in enumerate(sel):
        a, b = int(out.rp[r]), int(out.rp[r + 1])
        assert np.array_equal(s["col_index"][ptr[i]:ptr[i + 1]], out.ci[a:b])
        assert np.array_equal(s["values"][ptr[i]:ptr[i + 1]], out.v[a:b])
    assert s["shape"].tolist() == [rows, 50, out.nnz]


@pytest.mark.gpu
def test_bench_c1_dump_equals_oracle(tmp_path, orc):
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["end_to_end_ms"] is None and line["cpu_baseline"] is None  # those are --full's
    rows = n_cols = 1024
    rp = orc.gen_row_ptr(1000, rows, n_cols, orc.ROWLEN_BINOMIAL, round(0.01 * 2 ** 32), 0)
    ci, v = orc.gen_entries(1000, rp, n_cols)
    erp, eci, ev = orc.mul_dense(rows, n_cols, rp, ci, v, orc.gen_x_cols(1001, n_cols, 1))
    got = _load(d)
    assert got["shape"].tolist() == [rows, 1, int(erp[-1])]
    assert np.array_equal(got["rows"], np.arange(rows))
    assert np.array_equal(got["row_ptr"], erp.astype(np.float64))
    assert np.array_equal(got["col_index"], eci.astype(np.float64))
    assert got["values"].dtype == np.float64 and np.array_equal(got["values"].view(np.uint64), ev.view(np.uint64))

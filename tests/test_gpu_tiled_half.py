"""The two-pass k = 32 f64 kernel of the row-block x column-panel copy
(spmm_tiled_k32_half, kernels_tiled.hip): half-width Y rows on chip, up to 310
per wave and batch, every batch swept once per half of k; chunk positions
split by row parity; meta = col << 8 | row >> 1. Every case forces the mode
with BSM_TILED_HALF=1, proves through info() that the two-pass kernel ran, and
compares Y and row_nnz bit for bit with the one-row-per-wave kernel and with
the full-row copy (BSM_TILED_HALF=0)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from basic_sparse_matrix_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

K = 32


def _dev():
    from basic_sparse_matrix_amd import device

    return device


def _same(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _spmm(blk, x, tiled):
    y = torch.full((blk.rows, x.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    nnz = torch.full((blk.rows,), -1, dtype=torch.int32, device="cuda")
    saved = blk.tiled
    if not tiled:
        blk.tiled = None
    blk.spmm(x, y, nnz)
    blk.tiled = saved
    torch.cuda.synchronize()
    return y, nnz


def _block(rp, ci, v, n_cols):
    device = _dev()
    return device.DeviceCsrBlock(0, len(rp) - 1, n_cols, torch.as_tensor(rp, dtype=torch.int64, device="cuda"),
                                 torch.as_tensor(ci, dtype=torch.int32, device="cuda"),
                                 torch.as_tensor(v, dtype=torch.float64, device="cuda"), np.dtype(np.float64))


def _csr(rng, lens, n_cols, sort=True):
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pick = (lambda n: np.sort(rng.choice(n_cols, size=n, replace=False))) if sort else (
        lambda n: rng.permutation(rng.choice(n_cols, size=n, replace=False)))
    ci = np.concatenate([pick(int(n)) for n in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return rp, ci


@pytest.fixture
def env(monkeypatch):
    def set_env(half, rw=None, waves=None, pshift=None):
        for name, val in (("BSM_TILED_HALF", half), ("BSM_TILED_RW", rw), ("BSM_TILED_WAVES", waves),
                          ("BSM_TILED_PSHIFT", pshift)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(val))

    return set_env


def _check(env, blk, x, rw=None, waves=None, pshift=None, batch_rows=None):
    """Half mode against the one-row-per-wave kernel and the full-row copy;
    returns the half-mode Y and counts."""
    env(1, rw, waves, pshift)
    assert blk.plan_tiled(K, force=True) is not None
    info = blk.tiled.info()
    assert info["passes"] == 2
    if batch_rows is not None:
        assert info["batch_rows"] == batch_rows
    y2, n2 = _spmm(blk, x, True)
    y0, n0 = _spmm(blk, x, False)
    assert _same(y2, y0) and torch.equal(n2, n0)
    env(0, rw, waves, pshift)
    assert blk.plan_tiled(K, force=True) is not None
    info = blk.tiled.info()
    assert info["passes"] == 1 and info["batch_rows"] <= 155
    y1, n1 = _spmm(blk, x, True)
    assert _same(y2, y1) and torch.equal(n2, n1)
    blk.tiled = None
    return y2, n2


def _oracle_rows(orc, blk, x_cols, y, r0, r1):
    rp = blk.row_ptr.cpu().numpy().astype(np.uint64)
    ci, v = blk.col.cpu().numpy(), blk.vals.cpu().numpy()
    sub_rp = (rp[r0:r1 + 1] - rp[r0]).astype(np.uint64)
    erp, eci, ev = orc.mul_dense(r1 - r0, blk.n_cols, sub_rp, ci[rp[r0]:rp[r1]], v[rp[r0]:rp[r1]], x_cols)
    dense = np.zeros((r1 - r0, K))
    for r in range(r1 - r0):
        dense[r, eci[erp[r]:erp[r + 1]]] = ev[erp[r]:erp[r + 1]]
    assert np.array_equal(y[r0:r1].cpu().numpy().view(np.uint64), dense.view(np.uint64))


@pytest.mark.parametrize("pshift", [8, 12])
def test_half_rows_past_256_and_several_batches(orc, env, pshift):
    """2,405 rows on 4 waves: 602 rows per wave in two batches of 301, so row
    indices pass 255 (the ninth row bit) and every wave runs four steps."""
    device = _dev()
    rows, n_cols = 2405, 200_000
    blk = device.DeviceCsrBlock.generate(1000, 0, rows, n_cols, _lib.ROWLEN_UNIFORM, 0, 120)  # empty rows too
    x = device.gen_dense(1001, 0, n_cols, K)
    y, _ = _check(env, blk, x, rw=310, waves=4, pshift=pshift, batch_rows=301)
    x_cols = orc.gen_x_cols(1001, n_cols, K)
    _oracle_rows(orc, blk, x_cols, y, 250, 330)     # rows 250..329 of wave 0's first batch
    _oracle_rows(orc, blk, x_cols, y, 2300, 2405)   # the last wave's short second batch


def test_half_default_geometry(orc, env):
    device = _dev()
    rows, n_cols = 30_000, 200_000
    blk = device.DeviceCsrBlock.generate(1000, 0, rows, n_cols, _lib.ROWLEN_UNIFORM, 0, 120)
    x = device.gen_dense(1001, 0, n_cols, K)
    y, _ = _check(env, blk, x)
    _oracle_rows(orc, blk, orc.gen_x_cols(1001, n_cols, K), y, 12_345, 12_645)


@pytest.mark.parametrize("case", ["even_only", "odd_only", "long_row", "few_rows"])
def test_half_parity_imbalance(env, case):
    """One parity class empty, one 3,000-entry row among short ones (one entry
    per chunk, its class otherwise idle), fewer rows than waves."""
    rng = np.random.default_rng(7)
    n_cols = 5000
    rows, waves = (50, 64) if case == "few_rows" else (700, 4)
    lens = rng.integers(0, 30, size=rows)
    if case == "even_only":
        lens[1::2] = 0
    elif case == "odd_only":
        lens[0::2] = 0
    elif case == "long_row":
        lens[:] = rng.integers(0, 6, size=rows)
        lens[17] = 3000
        lens[3] = 0
    rp, ci = _csr(rng, lens, n_cols)
    blk = _block(rp, ci, rng.standard_normal(rp[-1]), n_cols)
    x = torch.as_tensor(rng.standard_normal((n_cols, K)), device="cuda")
    _check(env, blk, x, rw=310, waves=waves, pshift=8)


def test_half_unsorted_rows_keep_storage_order(env):
    rng = np.random.default_rng(11)
    rows, n_cols = 3000, 40_000
    rp, ci = _csr(rng, rng.integers(1, 80, size=rows), n_cols, sort=False)
    blk = _block(rp, ci, rng.standard_normal(rp[-1]) * 1e3, n_cols)
    x = torch.as_tensor(rng.standard_normal((n_cols, K)), device="cuda")
    _check(env, blk, x, rw=310, waves=8, pshift=9)


def test_half_cancellation_zero_pattern_nan_inf(env):
    """Small signed integers with exact cancellations and -0.0; NaN and inf in
    X, X row 0 included: the dummy entries gather X row 0 with value 0 (NaN
    there) and must stay in the scratch rows."""
    rng = np.random.default_rng(5)
    rows, n_cols = 2000, 3000
    rp, ci = _csr(rng, rng.integers(0, 40, size=rows), n_cols)
    v = rng.integers(-3, 4, size=rp[-1]).astype(np.float64)
    v[v == 0] = -0.0
    xs = rng.integers(-2, 3, size=(n_cols, K)).astype(np.float64)
    xs[0, :] = np.nan
    xs[0, 5] = np.inf
    xs[7, 3] = np.nan
    xs[11, :] = np.inf
    xs[13, 20] = -np.inf
    blk = _block(rp, ci, v, n_cols)
    y, n = _check(env, blk, torch.as_tensor(xs, device="cuda"), rw=310, waves=4, pshift=7)
    assert int((n < K).sum()) > 0  # the zero pattern is exercised
    # rows that do not touch a NaN / inf row of X are finite
    touched = np.zeros(rows, dtype=bool)
    for r in range(rows):
        touched[r] = np.isin(ci[rp[r]:rp[r + 1]], (0, 7, 11, 13)).any()
    assert bool(torch.isfinite(y[torch.as_tensor(~touched, device="cuda")]).all())


@pytest.mark.parametrize("zero_half", [0, 1])
def test_half_counts_come_from_one_half(env, zero_half):
    """X with columns 0-15 (then 16-31) all zero: a row's count comes from one
    pass only, written in the first and added to in the second."""
    rng = np.random.default_rng(13 + zero_half)
    rows, n_cols = 1500, 20_000
    rp, ci = _csr(rng, rng.integers(0, 50, size=rows), n_cols)
    blk = _block(rp, ci, rng.standard_normal(rp[-1]), n_cols)
    xs = rng.standard_normal((n_cols, K))
    xs[:, 16 * zero_half:16 * zero_half + 16] = 0.0
    y, n = _check(env, blk, torch.as_tensor(xs, device="cuda"), rw=310, waves=4, pshift=9)
    lens = torch.as_tensor(np.diff(rp), device="cuda")
    assert torch.equal(n, torch.where(lens > 0, 16, 0).to(torch.int32))


def test_half_top_of_column_range(env):
    """n_cols = 2^24 - 1, the last column the 32-bit meta word holds (col << 8
    | row >> 1), entries in the last panel."""
    device = _dev()
    rng = np.random.default_rng(17)
    rows, n_cols = 400, (1 << 24) - 1
    lens = rng.integers(1, 60, size=rows)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.concatenate([np.sort(np.concatenate([rng.choice(n_cols - 4096, size=n - 1, replace=False),
                                                 [n_cols - 1 - (i % 4096)]]))
                         for i, n in enumerate(lens)]).astype(np.int32)
    assert int(ci.max()) == n_cols - 1
    blk = _block(rp, ci, rng.standard_normal(rp[-1]), n_cols)
    x = device.gen_dense(1001, 0, n_cols, K)
    y, _ = _check(env, blk, x, rw=310, waves=4)
    v = blk.vals.cpu().numpy()
    for r in (0, 123, rows - 1):
        xr = x[torch.as_tensor(ci[rp[r]:rp[r + 1]].astype(np.int64), device="cuda")].cpu().numpy()
        acc = np.zeros(K)
        for e in range(len(xr)):
            acc = acc + v[rp[r] + e] * xr[e]  # f64 multiply, then add: the reference's order
        assert np.array_equal(y[r].cpu().numpy().view(np.uint64), acc.view(np.uint64)), r
    del x
    torch.cuda.empty_cache()


def test_half_public_mul_dense(orc, monkeypatch):
    """Csr.mul_dense with the copy forced into half mode, compaction included:
    the oracle's Csr bit for bit."""
    import ctypes

    from basic_sparse_matrix_amd import Csr, Dense

    rows, n_cols = 20_000, 60_000
    rp, ci, v = orc.gen_csr(1000, rows, n_cols, orc.ROWLEN_UNIFORM, 150, 250)
    x_cols = orc.gen_x_cols(1001, n_cols, K)
    monkeypatch.setenv("BSM_SPMM_TILED", "2")
    monkeypatch.setenv("BSM_TILED_HALF", "1")
    monkeypatch.setenv("BSM_TILED_WAVES", "64")
    a = Csr.from_csr_arrays((rows, n_cols), rp, ci, v)
    got = a.mul_dense(Dense.from_columns(x_cols))
    used = ctypes.c_int(-1)
    _lib.check(_lib.load().bsm_csr_tiled(a._device().handle, ctypes.byref(used)))
    assert used.value == 1
    erp, eci, ev = orc.mul_dense(rows, n_cols, rp, ci, v, x_cols)
    assert np.array_equal(np.asarray(got.row_index), erp)
    assert np.array_equal(np.asarray(got.col_index), eci)
    assert np.array_equal(np.asarray(got.v).view(np.uint64), ev.view(np.uint64))


def test_half_mode_rule(env):
    """f(l) - f(2l) > 12/256 with l = CUs/8 x 620 x density: half at C4 (l =
    1.98), full rows for l below ~0.1 or above ~10.5, never for f32, k = 1 or
    2^24 columns and more; the rule decides a forced plan when the environment
    does not."""
    lib = _lib.load()
    f32, f64 = _lib.DTYPE_CODES[np.dtype(np.float32)], _lib.DTYPE_CODES[np.dtype(np.float64)]
    n = 10_000_000
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 1000 * n, 32, 256) == 1    # C4: l = 1.98
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 1000 * n, 32, 128) == 1    # half the CUs: 0.99
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 40 * n, 32, 256) == 0      # l = 0.079
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 60 * n, 32, 256) == 1      # l = 0.119
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 5000 * n, 32, 256) == 1    # l = 9.9
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 6000 * n, 32, 256) == 0    # l = 11.9
    assert lib.bsm_dev_tiled_half_wanted(f32, n, n, 1000 * n, 32, 256) == 0
    assert lib.bsm_dev_tiled_half_wanted(f64, n, n, 1000 * n, 1, 256) == 0
    assert lib.bsm_dev_tiled_half_wanted(f64, n, 1 << 24, 1000 * n, 32, 256) == 0
    assert lib.bsm_dev_tiled_half_wanted(f64, n, (1 << 24) - 1, 1000 * n, 32, 256) == 1
    # small forced plans, no override: density 1e-4 on the whole device -> two
    # passes; density 0.01 (l ~ 200) -> full rows
    device = _dev()
    env(None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n_cols, expect in ((200_000, 2), (2_000, 1)):
        blk = device.DeviceCsrBlock.generate(1000, 0, 3000, n_cols, _lib.ROWLEN_CONST, 20, 20)
        assert lib.bsm_dev_tiled_half_wanted(f64, 3000, n_cols, blk.nnz, 32, cus) == (expect == 2)
        assert blk.plan_tiled(K, force=True) is not None
        assert blk.tiled.info()["passes"] == expect
    # k = 1 never, whatever the environment says
    env(1)
    blk = device.DeviceCsrBlock.generate(1000, 0, 3000, 200_000, _lib.ROWLEN_CONST, 20, 20)
    assert blk.plan_tiled(1, force=True) is not None
    assert blk.tiled.info()["passes"] == 1

"""GPU tests of the sampled dense-dense product (bsm_dev_sddmm /
device.sddmm, csrc/kernels_sddmm.hip): out[p] for every stored entry of a CSR
pattern, in both modes, compared BIT FOR BIT against a numpy restatement of
the one order in which the k products of an entry are added (a halving tree
of width the smallest power of two >= k for k <= 64; chunks of 64 added in
ascending order above that). The restatement is written here and does not
touch the library.

Patterns: 37 x 53 with empty rows first, in the middle and last and one row
with unsorted columns; 300 x 300 with both triangles stored, one full row and
one empty row (several blocks of 512 entries); 1 x 1; one entry alone; and an
odd number of entries (no multiple of the 64 / W entries a wave takes per step
for any W < 64) past two blocks. Values: normal draws with exact +0.0 and
-0.0 among them. out is prefilled with NaN and followed by a guard band that
must stay NaN."""

import functools

import numpy as np
import pytest

from basic_sparse_matrix_amd import _lib

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8, 31, 32, 33, 64, 65, 130]
DTYPES = [np.float32, np.float64]
GUARD = 64


def tree(t):  # t[..., k] of products, k <= 64
    k = t.shape[-1]
    W = 1
    while W < k:
        W *= 2
    t = t.copy()
    h = W // 2
    while h >= 1:
        m = min(h, max(k - h, 0))
        if m:
            t[..., :m] = t[..., :m] + t[..., h:h + m]
        k = min(k, h)
        h //= 2
    return t[..., 0]


def dot(a, b):
    """Row-wise dot of two (nnz, k) arrays in the SDDMM's order, in their dtype."""
    t = a * b
    acc = tree(t[:, :64])
    for c0 in range(64, t.shape[1], 64):
        acc = acc + tree(t[:, c0:c0 + 64])
    return acc


def reference(rp, col, u, v, sym):
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    cols = col.astype(np.int64)
    if not sym:
        return dot(u[rows], v[cols])
    out = np.zeros(cols.size, dtype=u.dtype)  # +0.0 above the diagonal
    lo, di = cols < rows, cols == rows
    out[lo] = dot(u[rows[lo]], v[cols[lo]]) + dot(u[cols[lo]], v[rows[lo]])
    out[di] = dot(u[rows[di]], v[cols[di]])
    return out


def _csr(rows, cols, lists):
    """row_ptr (int64) and col (int32) from one list of columns per row, kept in the order given."""
    rp = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    col = np.array([c for lst in lists for c in lst], dtype=np.int32)
    assert len(lists) == rows and (col.size == 0 or (col.min() >= 0 and col.max() < cols))
    return rows, cols, rp, col


@functools.lru_cache(maxsize=None)
def patterns():
    rng = np.random.default_rng(5)
    out = {}
    lists = [sorted(rng.choice(53, size=rng.integers(1, 9), replace=False).tolist()) for _ in range(37)]
    for r in (0, 18, 36):
        lists[r] = []
    lists[7] = [40, 3, 52, 0, 17]  # unsorted
    out["rect"] = _csr(37, 53, lists)
    lists = [sorted(rng.choice(300, size=rng.integers(1, 12), replace=False).tolist()) for _ in range(300)]
    lists[123] = list(range(300))
    lists[200] = []
    out["both-triangles"] = _csr(300, 300, lists)
    out["1x1"] = _csr(1, 1, [[0]])
    out["one-entry"] = _csr(6, 6, [[], [], [], [], [1], []])
    lists = [sorted(rng.choice(129, size=8, replace=False).tolist()) for _ in range(129)]
    lists[128] = lists[128][:7]
    out["odd"] = _csr(129, 129, lists)
    assert out["odd"][3].size == 1031 and out["both-triangles"][3].size > 1024
    up = out["both-triangles"]
    r = np.repeat(np.arange(300), np.diff(up[2]))
    assert (up[3] > r).any() and (up[3] < r).any() and (up[3] == r).any()
    return out


def operands(rows, cols, k, dtype, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((rows, k)).astype(dtype)
    v = rng.standard_normal((cols, k)).astype(dtype)
    for a in (u, v):
        a[rng.random(a.shape) < 0.06] = 0.0
        a[rng.random(a.shape) < 0.06] = -0.0
    return u, v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def run(torch, device, rp_t, col_t, u_t, v_t, mode, nnz, stream=None):
    """out (nnz values, as numpy) from a NaN-filled buffer with a guard band behind it, which is checked."""
    buf = torch.full((nnz + GUARD,), float("nan"), dtype=u_t.dtype, device="cuda")
    torch.cuda.synchronize()
    got = device.sddmm(rp_t, col_t, u_t, v_t, mode=mode, out=buf[:nnz], stream=stream)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert np.isnan(host[nnz:]).all(), "the guard band behind out was written"
    return host[:nnz]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("k", KS)
def test_sddmm_bits(k, dtype):
    import torch

    from basic_sparse_matrix_amd import device

    side = torch.cuda.Stream()
    for name, (rows, cols, rp, col) in patterns().items():
        u, v = operands(rows, cols, k, dtype, 100 + k)
        if k == 1:  # (n,) counts as k = 1
            u_t, v_t = torch.tensor(u[:, 0].copy(), device="cuda"), torch.tensor(v[:, 0].copy(), device="cuda")
        else:
            u_t, v_t = torch.tensor(u, device="cuda"), torch.tensor(v, device="cuda")
        rp_t, col_t = torch.tensor(rp, device="cuda"), torch.tensor(col, device="cuda")
        for mode in ("all", "sym_lower") if rows == cols else ("all",):
            want = reference(rp, col, u, v, mode == "sym_lower")
            got = run(torch, device, rp_t, col_t, u_t, v_t, mode, col.size)
            assert not np.isnan(got).any(), (name, mode, "an entry was not written")
            assert np.array_equal(bits(got), bits(want)), (name, mode, k)
            if mode == "sym_lower":
                r = np.repeat(np.arange(rows), np.diff(rp))
                assert not bits(got[col > r]).any(), (name, "an upper entry is not +0.0")
            again = run(torch, device, rp_t, col_t, u_t, v_t, mode, col.size)
            other = run(torch, device, rp_t, col_t, u_t, v_t, mode, col.size, stream=side)
            assert np.array_equal(bits(again), bits(got)) and np.array_equal(bits(other), bits(got)), (name, mode)


def test_sddmm_default_out_and_zero_signs():
    """out defaults to a new tensor; a dot of -0.0 products is -0.0 (nothing is added to a +0 that is not there)."""
    import torch

    from basic_sparse_matrix_amd import device

    rows, cols, rp, col = patterns()["odd"]
    for k in (1, 3, 64, 65):
        u = torch.full((rows, k), -0.0, dtype=torch.float64, device="cuda")
        v = torch.ones((cols, k), dtype=torch.float64, device="cuda")
        got = device.sddmm(torch.tensor(rp, device="cuda"), torch.tensor(col, device="cuda"), u, v)
        assert got.shape == (col.size,) and got.dtype == torch.float64
        assert (bits(got.cpu().numpy()) == np.uint64(1) << np.uint64(63)).all(), k


def test_sddmm_refusals():
    import torch

    from basic_sparse_matrix_amd import device

    lib = _lib.require_device()
    rows, cols, rp, col = patterns()["rect"]
    nnz = col.size
    rp_t, col_t = torch.tensor(rp, device="cuda"), torch.tensor(col, device="cuda")
    u, v = torch.ones((rows, 4), dtype=torch.float64, device="cuda"), torch.ones((cols, 4), dtype=torch.float64,
                                                                                 device="cuda")
    out = torch.full((nnz,), float("nan"), dtype=torch.float64, device="cuda")
    F64, I32 = _lib.DTYPE_CODES[np.dtype(np.float64)], _lib.DTYPE_CODES[np.dtype(np.int32)]
    P = lambda t: t.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream

    def call(dtype=F64, mode=0, r=rows, c=cols, z=nnz, rpp=P(rp_t), cp=P(col_t), k=4, up=P(u), vp=P(v), op=P(out)):
        return lib.bsm_dev_sddmm(dtype, mode, r, c, z, rpp, cp, k, up, vp, op, s)

    for kw, word in ((dict(k=0), "k == 0"), (dict(dtype=I32), "f32/f64"), (dict(dtype=77), "f32/f64"),
                     (dict(mode=2), "mode"), (dict(mode=1), "square"), (dict(rpp=None), "null"),
                     (dict(cp=None), "null"), (dict(up=None), "null"), (dict(vp=None), "null"),
                     (dict(op=None), "null")):
        assert call(**kw) == _lib.BSM_ERR_INVALID, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert call(r=0, z=0) == _lib.BSM_OK and call(z=0) == _lib.BSM_OK  # nothing is launched
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused or empty call wrote to out"
    assert call() == _lib.BSM_OK
    torch.cuda.synchronize()
    assert (out == 4.0).all()
    with pytest.raises(ValueError, match="square"):
        device.sddmm(rp_t, col_t, u, v, mode="sym_lower")
    with pytest.raises(ValueError, match="mode"):
        device.sddmm(rp_t, col_t, u, v, mode="x")
    with pytest.raises(ValueError):
        device.sddmm(rp_t, col_t, u[:, :0].contiguous(), v[:, :0].contiguous())
    with pytest.raises(ValueError):
        device.sddmm(rp_t, col_t, u, v[:, :3].contiguous())
    with pytest.raises(ValueError):
        device.sddmm(rp_t, col_t, u, v.t().contiguous().t())
    with pytest.raises(TypeError):
        device.sddmm(rp_t, col_t, u, v.float())
    with pytest.raises(ValueError):
        device.sddmm(rp_t, col_t, u, v, out=out[:-1])

"""The host transfer pipelines (csrc/transfer.hip and the marshalling of
csrc/capi.hip) under ONE setting of their process-wide switches; started as a
fresh child process per setting by tests/test_gpu_transfer.py (the switches
BSM_XFER_H2D, BSM_XFER_D2H, BSM_STAGE_CHUNK, BSM_COPY_THREADS and
BSM_TOUCH_THREADS are read once per process). Not a test module itself.

argv: out_json case [case ...]. One JSON record per case goes to out_json:
ok, the first mismatching index, the route counters (bsm_xfer_counters) the
case moved and the counts this file works out from the sizes and the
switches, the BSM_* environment, and the seconds it took. Everything is
compared bit for bit with an exact reference: the uploaded arrays themselves,
the oracle's Csr::mul_dense, or numpy's b / d for a power-of-two diagonal.
Every destination is the interior [16:-16] of a larger array filled with
0xA5, so it is not page-aligned and its guard elements show any write outside
the range. The C ABI is called through ctypes with those arrays (the mirror's
own download() would pick its page-locked pool).

cases:
  roundtrip:<dtype>:<nnz>    bsm_csr_upload, bsm_csr_download into plain arrays
  registered:<dtype>:<nnz>   the same into bsm_host_register'ed arrays
  badcols                    three columns >= cols across the upload's chunks
  muldense:<dtype>:<n_cols>  bsm_csr_mul_dense from host columns, k = 32
  trsv:<dtype>:<k>:<n>       bsm_forward_substitution on a diagonal L
  threads                    two threads download two large matrices at once
"""

import ctypes
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from basic_sparse_matrix_amd import _lib  # noqa: E402

PIN_MAX = 32 << 20       # capi.hip: up to here one pinned buffer serves a transfer
PAR_MIN = 4 << 20        # xfer_host.hpp: a chunk copy from here on uses the copy threads
PREFAULT_MIN = 8 << 20   # xfer_host.hpp: result arrays from here on are faulted in ahead
GUARD = 16
FILL = 0xA5
DTYPES = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "u64": np.uint64}
COUNTERS = ("h2d_direct", "h2d_staged", "d2h_direct", "d2h_staged", "prefault", "par_memcpy", "csr_direct",
            "small_pinned")


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


# the switches as transfer.hip reads them
CHUNK = max(int(os.environ.get("BSM_STAGE_CHUNK", 16 << 20)), 1 << 16) & ~255
H2D_STAGED = os.environ.get("BSM_XFER_H2D") == "staged"
D2H_DIRECT = os.environ.get("BSM_XFER_D2H") == "direct"
COPY_THREADS = _clamp(int(os.environ.get("BSM_COPY_THREADS", 4)), 1, 16)
TOUCH_THREADS = _clamp(int(os.environ.get("BSM_TOUCH_THREADS", 8)), 0, 32)


class Expect:
    """The counters a sequence of transfers must leave."""

    def __init__(self):
        self.c = dict.fromkeys(COUNTERS, 0)

    @staticmethod
    def _lens(nbytes):
        return [min(CHUNK, nbytes - o) for o in range(0, nbytes, CHUNK)]

    def _copies(self, lens):
        if COPY_THREADS > 1:
            self.c["par_memcpy"] += sum(1 for n in lens if n >= PAR_MIN)

    def h2d(self, nbytes):
        lens = self._lens(nbytes)
        if H2D_STAGED:
            self.c["h2d_staged"] += len(lens)
            self._copies(lens)
        else:
            self.c["h2d_direct"] += len(lens)

    def d2h(self, nbytes):
        lens = self._lens(nbytes)
        if D2H_DIRECT:
            self.c["d2h_direct"] += len(lens)
        else:
            self.c["d2h_staged"] += len(lens)
            self._copies(lens)
        if TOUCH_THREADS and nbytes >= PREFAULT_MIN:
            self.c["prefault"] += len(lens)

    def csr_upload(self, rows, nnz, es):
        self.h2d((rows + 1) * 8)
        self.h2d(nnz * 8)  # usize columns, narrowed per chunk on the device
        self.h2d(nnz * es)

    def csr_download(self, rows, nnz, es, registered=False):
        if registered and nnz >= 4096:
            self.c["csr_direct"] += 1
        elif (rows + 1) * 8 + nnz * 4 + nnz * es <= PIN_MAX:
            self.c["small_pinned"] += 1
        else:
            self.d2h((rows + 1) * 8)
            self.d2h(nnz * 8)  # widened to usize per chunk on the device
            self.d2h(nnz * es)


def counters():
    out = (ctypes.c_uint64 * 8)()
    _lib.check(_lib.load().bsm_xfer_counters(out))
    return dict(zip(COUNTERS, (int(x) for x in out)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def first_mismatch(got, want):
    """None when got and want hold the same bits, else the first index that differs."""
    g, w = bits(got), bits(np.asarray(want, dtype=got.dtype))
    if g.shape != w.shape:
        return min(g.size, w.size)
    ne = np.flatnonzero(g != w)
    return int(ne[0]) if ne.size else None


class Guarded:
    """A destination of n elements inside a larger array filled with 0xA5."""

    def __init__(self, n, dtype):
        self.n = n
        self.base = np.empty(n + 2 * GUARD, dtype=dtype)
        self.base.view(np.uint8)[:] = FILL
        self.a = self.base[GUARD:GUARD + n]

    def guards_ok(self):
        b = self.base.view(np.uint8)
        g = GUARD * self.base.itemsize
        return bool((b[:g] == FILL).all() and (b[b.size - g:] == FILL).all())


def make_csr(seed, nnz, dtype, cols=1 << 20):
    """Uneven rows (about one in nine empty), unsorted columns, random value bits."""
    rng = np.random.default_rng(seed)
    rows = max(2, nnz // 8)
    cuts = np.sort(rng.integers(0, nnz + 1, rows - 1))
    rp = np.concatenate(([0], cuts, [nnz])).astype(np.uint64)
    ci = rng.integers(0, cols, nnz, dtype=np.uint64)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = rng.standard_normal(nnz).astype(dt)
    else:
        v = rng.integers(0, np.iinfo(np.uint64).max, nnz, dtype=np.uint64, endpoint=True).astype(dt)
    assert (np.diff(rp.astype(np.int64)) == 0).any()
    return rows, cols, rp, ci, v


def upload(rows, cols, rp, ci, v):
    h = ctypes.c_void_p()
    rc = _lib.load().bsm_csr_upload(_lib.DTYPE_CODES[v.dtype], rows, cols, v.size, _lib.ptr(rp), _lib.ptr(ci),
                                    _lib.ptr(v), ctypes.byref(h))
    return rc, h


def shape(h):
    r, c, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.load().bsm_csr_shape(h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(n), None))
    return r.value, c.value, n.value


def download_check(h, rows, nnz, dtype, want, registered=False):
    """bsm_csr_download into guarded arrays -> (first mismatch or None, what failed)."""
    lib = _lib.load()
    dst = [Guarded(rows + 1, np.uint64), Guarded(nnz, np.uint64), Guarded(nnz, dtype)]
    locked = []
    try:
        if registered:
            for d in dst:
                _lib.check(lib.bsm_host_register(d.base.ctypes.data, d.base.nbytes))
                locked.append(d)
        _lib.check(lib.bsm_csr_download(h, _lib.ptr(dst[0].a), _lib.ptr(dst[1].a), _lib.ptr(dst[2].a)))
    finally:
        for d in locked:
            lib.bsm_host_unregister(d.base.ctypes.data)
    for name, d, w in zip(("row_ptr", "col", "vals"), dst, want):
        if not d.guards_ok():
            return 0, name + ": guard elements written"
        i = first_mismatch(d.a, w)
        if i is not None:
            return i, f"{name}[{i}]: got {bits(d.a)[i]:#x}, want {bits(np.asarray(w, dtype=d.a.dtype))[i]:#x}"
    return None, ""


def case_roundtrip(dts, nnz, registered=False):
    dtype = np.dtype(DTYPES[dts])
    rows, cols, rp, ci, v = make_csr(nnz, nnz, dtype)
    lib = _lib.load()
    lib.bsm_xfer_counters_reset()
    rc, h = upload(rows, cols, rp, ci, v)
    if rc != _lib.BSM_OK:
        return dict(ok=False, detail="upload: " + _lib.last_error())
    try:
        i, what = download_check(h, rows, nnz, dtype, (rp, ci, v), registered)
    finally:
        lib.bsm_csr_free(h)
    e = Expect()
    e.csr_upload(rows, nnz, dtype.itemsize)
    e.csr_download(rows, nnz, dtype.itemsize, registered)
    return dict(ok=i is None, first_mismatch=i, detail=what, expected=e.c)


def case_badcols():
    nnz = 3_000_007
    rows, cols, rp, ci, v = make_csr(77, nnz, np.float64)
    lib = _lib.load()
    bad = ci.copy()
    edge = min(CHUNK // 8, nnz - 2)  # the first entry of the second chunk, beside the boundary
    for i in (0, edge, nnz - 1):
        bad[i] = cols + i
    lib.bsm_xfer_counters_reset()
    rc, h = upload(rows, cols, rp, bad, v)
    msg = _lib.last_error()
    if rc != _lib.BSM_ERR_PANIC or "in 3 entries" not in msg or h.value:
        if h.value:
            lib.bsm_csr_free(h)
        return dict(ok=False, detail=f"bad upload: rc {rc}, handle {h.value}, message {msg!r}")
    rc, h = upload(rows, cols, rp, ci, v)
    if rc != _lib.BSM_OK:
        return dict(ok=False, detail="repaired upload: " + _lib.last_error())
    got = shape(h)
    lib.bsm_csr_free(h)
    return dict(ok=got == (rows, cols, nnz), detail=f"repaired upload has shape {got}")


def case_muldense(dts, n_cols, orc):
    dtype = np.dtype(DTYPES[dts])
    rows, k, es = 100_000, 32, dtype.itemsize
    rp, ci, v = orc.gen_csr(5000 + n_cols, rows, n_cols, orc.ROWLEN_CONST, 5, 5, dtype=dtype)
    x_cols = orc.gen_x_cols(6000 + n_cols, n_cols, k, dtype=dtype)
    want = orc.mul_dense(rows, n_cols, rp, ci, v, x_cols)
    lib = _lib.load()
    rc, a = upload(rows, n_cols, rp, ci, v)
    if rc != _lib.BSM_OK:
        return dict(ok=False, detail="upload: " + _lib.last_error())
    out = ctypes.c_void_p()
    lib.bsm_xfer_counters_reset()
    try:
        rc = lib.bsm_csr_mul_dense(a, k, n_cols, _lib.ptr_array(x_cols), ctypes.byref(out))
        if rc != _lib.BSM_OK:
            return dict(ok=False, detail="mul_dense: " + _lib.last_error())
        got_rows, _, nnz = shape(out)
        if (got_rows, nnz) != (rows, len(want[2])):
            return dict(ok=False, detail=f"result has {got_rows} rows, {nnz} entries; the oracle {len(want[2])}")
        i, what = download_check(out, rows, nnz, dtype, want)
    finally:
        lib.bsm_csr_free(a)
        if out.value:
            lib.bsm_csr_free(out)
    e = Expect()
    if n_cols * k * es > PIN_MAX:  # one pipeline per column, then the pack on the device
        for _ in range(k):
            e.h2d(n_cols * es)
    e.csr_download(rows, nnz, es)
    return dict(ok=i is None, first_mismatch=i, detail=what, expected=e.c, result_nnz=nnz)


def case_trsv(dts, k, n):
    dtype = np.dtype(DTYPES[dts])
    rng = np.random.default_rng(n * 10 + k)
    d = np.ldexp(1.0, rng.integers(-3, 4, n)).astype(dtype)  # powers of two: b / d is exact
    rp = np.arange(n + 1, dtype=np.uint64)
    ci = np.arange(n, dtype=np.uint64)
    b_cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    lib = _lib.load()
    rc, h = upload(n, n, rp, ci, d)
    if rc != _lib.BSM_OK:
        return dict(ok=False, detail="upload: " + _lib.last_error())
    dst = [Guarded(n, dtype) for _ in range(k)]
    lib.bsm_xfer_counters_reset()
    try:
        rc = lib.bsm_forward_substitution(h, k, n, _lib.ptr_array(b_cols), _lib.ptr_array([g.a for g in dst]))
    finally:
        lib.bsm_csr_free(h)
    if rc != _lib.BSM_OK:
        return dict(ok=False, detail="forward_substitution: " + _lib.last_error())
    e = Expect()
    if n * k * dtype.itemsize > PIN_MAX:
        for _ in range(k):
            e.h2d(n * dtype.itemsize)
    for _ in range(k):
        e.d2h(n * dtype.itemsize)
    for j, g in enumerate(dst):
        if not g.guards_ok():
            return dict(ok=False, first_mismatch=0, detail=f"column {j}: guard elements written", expected=e.c)
        i = first_mismatch(g.a, b_cols[j] / d)
        if i is not None:
            return dict(ok=False, first_mismatch=i, detail=f"column {j}, row {i}", expected=e.c)
    return dict(ok=True, first_mismatch=None, detail="", expected=e.c)


def case_threads():
    lib = _lib.load()
    mats = [make_csr(11, 3_000_007, np.float64), make_csr(12, 4_400_003, np.float32)]
    handles = []
    for rows, cols, rp, ci, v in mats:
        rc, h = upload(rows, cols, rp, ci, v)
        if rc != _lib.BSM_OK:
            return dict(ok=False, detail="upload: " + _lib.last_error())
        handles.append(h)
    lib.bsm_xfer_counters_reset()
    res = [None, None]
    gate = threading.Barrier(2)

    def run(j):
        rows, cols, rp, ci, v = mats[j]
        try:
            gate.wait()
            res[j] = download_check(handles[j], rows, v.size, v.dtype, (rp, ci, v))
        except Exception as ex:  # a record, not a lost thread
            res[j] = (0, f"{type(ex).__name__}: {ex}")

    th = [threading.Thread(target=run, args=(j,)) for j in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for h in handles:
        lib.bsm_csr_free(h)
    e = Expect()
    for rows, cols, rp, ci, v in mats:
        e.csr_download(rows, v.size, v.dtype.itemsize)
    bad = [(j, r) for j, r in enumerate(res) if r[0] is not None]
    if bad:
        j, (i, what) = bad[0]
        return dict(ok=False, first_mismatch=i, detail=f"thread {j}: {what}", expected=e.c)
    return dict(ok=True, first_mismatch=None, detail="", expected=e.c)


def run_case(name, orc):
    p = name.split(":")
    if p[0] == "roundtrip":
        return case_roundtrip(p[1], int(p[2]))
    if p[0] == "registered":
        return case_roundtrip(p[1], int(p[2]), registered=True)
    if p[0] == "badcols":
        return case_badcols()
    if p[0] == "muldense":
        return case_muldense(p[1], int(p[2]), orc)
    if p[0] == "trsv":
        return case_trsv(p[1], int(p[2]), int(p[3]))
    if p[0] == "threads":
        return case_threads()
    raise ValueError("unknown case " + name)


def main():
    out_json, cases = sys.argv[1], sys.argv[2:]
    from oracle import pyoracle as orc

    _lib.require_device()
    env = {k: v for k, v in os.environ.items() if k.startswith("BSM_")}
    records = []
    for name in cases:
        t0 = time.perf_counter()
        try:
            rec = run_case(name, orc)
        except Exception as ex:
            rec = dict(ok=False, detail=f"{type(ex).__name__}: {ex}")
        rec.setdefault("first_mismatch", None)
        rec.setdefault("expected", None)
        rec.update(case=name, counters=counters(), env=env, chunk=CHUNK, seconds=round(time.perf_counter() - t0, 3))
        records.append(rec)
        print(f"{name}: {'ok' if rec['ok'] else 'FAIL ' + rec['detail']} {rec['seconds']} s", flush=True)
        with open(out_json, "w") as f:  # rewritten per case: what ran is on record if a later case dies
            json.dump(records, f)


if __name__ == "__main__":
    main()

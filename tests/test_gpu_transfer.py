"""The host transfer pipelines (csrc/transfer.hip; the column and CSR
marshalling of csrc/capi.hip) past one chunk, in every mode.

Every host-buffer entry point moves its arrays through this layer: chunked
(16 MiB by default), double-buffered, copied by host threads, the result pages
faulted in ahead of the data, with two alternative modes kept for A/B
(BSM_XFER_H2D=staged, BSM_XFER_D2H=direct). Its switches are read once per
process, so each setting below runs tests/xfer_worker.py in a fresh child
process, one child at a time; the child writes one record per case and the
tests here assert on the records: the data bit for bit (against the uploaded
arrays, the oracle's Csr::mul_dense, or b / d of a power-of-two diagonal),
untouched 0xA5 guards around every destination, and the route counters
(bsm_xfer_counters) equal to the counts worked out from the sizes and the
switches, so that a case meant for the staged pipeline cannot pass by taking
the small pinned path.

A child that ends by a signal or runs out of time stops the module: every
remaining case fails at once and no further child is started.
"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "xfer_worker.py")
SWITCHES = ("BSM_XFER_H2D", "BSM_XFER_D2H", "BSM_STAGE_CHUNK", "BSM_COPY_THREADS", "BSM_TOUCH_THREADS")

ENVS = {
    "A": {},
    "B": {"BSM_STAGE_CHUNK": "65536"},
    "C": {"BSM_XFER_H2D": "staged"},
    "D": {"BSM_XFER_H2D": "staged", "BSM_STAGE_CHUNK": "65536"},
    "E": {"BSM_XFER_D2H": "direct", "BSM_STAGE_CHUNK": "1048576"},
    "F": {"BSM_XFER_H2D": "staged", "BSM_XFER_D2H": "direct", "BSM_TOUCH_THREADS": "0", "BSM_COPY_THREADS": "1"},
    "G": {"BSM_XFER_H2D": "staged", "BSM_COPY_THREADS": "8"},
    "H": {"BSM_XFER_H2D": "staged", "BSM_COPY_THREADS": "16", "BSM_TOUCH_THREADS": "32"},
}

BIG8, BIG4 = 3_000_007, 4_400_003  # 36.0 MB and 35.2 MB of int32 columns + values: past the 32 MiB pinned path
# every case of the issue's list a-c, e, f, h: run under every setting
COMMON = [
    f"roundtrip:f64:{BIG8}", f"roundtrip:u64:{BIG8}", f"roundtrip:f32:{BIG4}", f"roundtrip:i32:{BIG4}",
    "registered:f64:4095", "registered:f64:4096", f"registered:f64:{BIG8}", f"registered:f32:{BIG4}",
    "badcols",
    "muldense:f64:131072", "muldense:f64:131073", "muldense:f32:262144", "muldense:f32:262145",
    "threads",
]
# n * 8 against 64 KiB chunks: one element before, on and after the end of a chunk
UPLOAD_EDGES = [f"roundtrip:f64:{n}" for n in (8191, 8192, 8193, 16384, 16385)]
TRSV_EDGES = [f"trsv:{dt}:{k}:{8192 * j + d}" for dt in ("f64", "f32") for k in (1, 3) for j in (1, 2, 3)
              for d in (-1, 0, 1)]
TRSV_LARGE = ["trsv:f64:1:1100000"]  # 8.8 MB: past the 8 MiB bar of the prefault
EXTRA = {
    "A": TRSV_LARGE,
    "B": UPLOAD_EDGES + TRSV_EDGES,
    "D": UPLOAD_EDGES + TRSV_EDGES,
    # nnz * 8 ends on, before and after a 1 MiB chunk boundary
    "E": [f"roundtrip:f64:{23 * 131072 + d}" for d in (-1, 0, 1)] + TRSV_LARGE,
    # the tail chunk of vals is 4 MiB + 4 bytes: with 8 copy threads a floor-rounded part drops the last element
    "G": ["roundtrip:f32:5242881"],
    # the tail chunk of vals and of the widened columns is 4 MiB + 8 bytes, 16 copy threads
    "H": ["roundtrip:f64:4718593"],
}
CASES = [(e, c) for e in ENVS for c in COMMON + EXTRA.get(e, [])]

_records = {}   # env name -> {case: record} of the child that ran it
_dead = []      # why no further child may start (a child ended by a signal or timed out)


def _child(env_name, tmp_path_factory):
    if env_name in _records:
        return _records[env_name]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    out = tmp_path_factory.mktemp("xfer_" + env_name) / "records.json"
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ENVS[env_name])
    cases = COMMON + EXTRA.get(env_name, [])
    log = ""
    try:
        r = subprocess.run([sys.executable, "-u", WORKER, str(out)] + cases, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        log = r.stdout.decode(errors="replace")[-3000:]
        if r.returncode < 0 or r.returncode in (134, 139):
            _dead.append(f"the child of setting {env_name} ended with status {r.returncode}: {log}")
    except subprocess.TimeoutExpired as ex:
        log = (ex.stdout or b"").decode(errors="replace")[-3000:]
        _dead.append(f"the child of setting {env_name} ran out of time: {log}")
    recs = {}
    if out.exists():
        recs = {rec["case"]: rec for rec in json.loads(out.read_text())}
    recs["__log__"] = log
    _records[env_name] = recs
    return recs


@pytest.mark.parametrize("env_name,case", CASES)
def test_transfer_case(env_name, case, tmp_path_factory):
    recs = _child(env_name, tmp_path_factory)
    rec = recs.get(case)
    if rec is None:
        pytest.fail(f"no record of {case} under setting {env_name}; " + (_dead[0] if _dead else recs["__log__"]))
    for k in SWITCHES:  # the child really ran under the setting
        assert rec["env"].get(k) == ENVS[env_name].get(k), rec["env"]
    assert rec["ok"], f"first mismatch {rec['first_mismatch']}: {rec['detail']}"
    got, want = rec["counters"], rec["expected"]
    if want is not None:
        assert got == want, (got, want)
    if case == "badcols":
        return
    h2d_staged = ENVS[env_name].get("BSM_XFER_H2D") == "staged"
    d2h_direct = ENVS[env_name].get("BSM_XFER_D2H") == "direct"
    kind, size = case.split(":")[0], int(case.split(":")[-1]) if ":" in case else 0
    large = kind == "threads" or (kind in ("roundtrip", "registered") and size >= 1_000_000)
    if large and kind != "threads":  # the upload pipeline of this setting moved more than one chunk
        assert got["h2d_staged" if h2d_staged else "h2d_direct"] >= 2, got
        assert got["h2d_direct" if h2d_staged else "h2d_staged"] == 0, got
    if large and kind != "registered":  # and so did the download pipeline, not the small pinned path
        assert got["d2h_direct" if d2h_direct else "d2h_staged"] >= 2, got
        assert got["d2h_staged" if d2h_direct else "d2h_direct"] == 0, got
        assert got["small_pinned"] == 0 and got["csr_direct"] == 0, got
        touch = int(ENVS[env_name].get("BSM_TOUCH_THREADS", 8))
        assert (got["prefault"] >= 2) == (touch > 0), got
    if kind == "registered":
        assert got["csr_direct"] == (1 if size >= 4096 else 0) and got["small_pinned"] == (0 if size >= 4096 else 1), got
        assert got["d2h_direct"] == 0 and got["d2h_staged"] == 0, got
    if case in ("muldense:f64:131073", "muldense:f32:262145"):  # X one row past the pinned upload: a pipeline per column
        assert got["h2d_staged" if h2d_staged else "h2d_direct"] >= 32, got
    if case in ("muldense:f64:131072", "muldense:f32:262144"):  # X exactly fills the pinned upload
        assert got["h2d_staged"] == 0 and got["h2d_direct"] == 0, got
    if case.startswith("muldense:f64"):  # about 3.2M entries: 39 MB, the staged download
        assert rec["result_nnz"] > 3_000_000 and got["d2h_direct" if d2h_direct else "d2h_staged"] >= 2, (rec, got)
    if kind == "trsv" and size > 1_000_000:
        assert got["prefault"] >= 1, got
    if env_name in ("B", "D") and case.startswith("trsv:f64") and size >= 8193:
        assert got["d2h_staged"] >= 2, got  # download_columns past one chunk
    if env_name in ("B", "D") and kind == "roundtrip" and 8193 <= size < 100_000:
        assert got["h2d_staged" if h2d_staged else "h2d_direct"] >= 4, got  # columns and values took two chunks each
    if env_name in ("G", "H") and large and kind != "registered":
        assert got["par_memcpy"] >= 2, got

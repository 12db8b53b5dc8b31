#!/usr/bin/env python3
"""C5 (north_star config 5): 2D 5-point Poisson on a g x g grid (natural
ordering, N = g^2, band b = g), b = A x_true, solve(A, b) on the GPU through
the reference API (lib.rs:11-24): cholesky_decomp -> transpose -> forward ->
backward substitution. Prints ONE JSON line per order (reference = bit-exact
operation order; blocked = reassociated, within 1e-6 on f64) with

* wall time through the public API (host b in, host x out) and the device
  time of every stage (HIP events on the library's stream, bsm_stage_times);
* the band orders: the factor's flop roofline (N b^2 flops, the band
  Cholesky's multiply-add pairs x 2, against the 78.6 TF/s f64 peak of
  MI355X_MICROARCH.md) and each triangular solve's byte roofline (the band
  of L, 8 N (b+1) bytes, read once, against 8 TB/s);
* the nd order: its own model from its plan (nd_model: the fronts' true and
  64-padded flops, the bytes of its L), never the band's; the cold figure
  (first solve of the pattern, new handle, analysis included) first, since
  solve(a, b) takes `a` by value (lib.rs:11), then new handles of a pattern
  seen before (the plan from the library's cache), then the same handle;
* the CPU baseline: the oracle's band restatement of the same solve (the
  reference's order, one thread; the literal O(N^4) reference loops are out
  of reach beyond N ~ 256), timed on this host's cores on the leading 25 grid
  rows of the system and scaled by N/R (per-row work is constant past the
  first g rows), with a whole 250^2 solve beside it;
* the error of x against x_true (and, for the reference order, bit-equality
  with the committed full-size oracle fixture, tests/golden/c5_poisson_1000.json).
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from basic_sparse_matrix_amd import Csr, Dense, _lib, solve, solver  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402  (inputs, the CPU baseline and the check only)

F64_PEAK_TFS = 78.6
HBM_PEAK_GBS = 8000.0


def system(g, dt):
    rp, ci, v = orc.poisson2d(g)
    n = g * g
    x_true = orc.gen_x_cols(1002, n, 1)[0]
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    b = np.zeros(n)
    np.add.at(b, rows, v * x_true[ci.astype(np.int64)])
    return rp, ci, v.astype(dt), b.astype(dt), x_true


def band_kernel():
    """The reference-order factor kernel the library runs."""
    return "band_chol5"


def leading_system(g, rows_g):
    """The leading principal block of the g x g system: the first rows_g grid
    rows (R = rows_g * g unknowns, band g). Its band Cholesky is the first R
    rows of the full factor, and every row past the first g costs the same
    (g^2/2 multiply-add pairs), so its time x N/R is the full solve's."""
    rp, ci, v = orc.poisson2d(g)
    R = rows_g * g
    lo = rp[:R + 1].astype(np.int64)
    keep = ci[:lo[-1]].astype(np.int64) < R
    row_of = np.repeat(np.arange(R), np.diff(lo))
    rp_s = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=R))]).astype(np.uint64)
    ci_s, v_s = ci[:lo[-1]][keep], v[:lo[-1]][keep]
    x_true = orc.gen_x_cols(1002, R, 1)[0]
    b = np.zeros(R)
    np.add.at(b, row_of[keep], v_s * x_true[ci_s.astype(np.int64)])
    return R, rp_s, ci_s, v_s, b


def nd_model(n, rp, ci, leaf, es):
    """The nested-dissection solve's own work model, from its plan (the host
    analysis alone, solver.nd_analyse, the same call the library makes):
    per front np pivots and m front rows.
    * true flops: sum of np^3/3 + np^2 m + np m^2 (the partial Cholesky of
      the front: its pivot block, the panel below it, the update block);
    * padded flops: what nd_factor executes on 64 x 64 tiles (np padded to
      np_pad = 64 npt, nt = ceil((np_pad + m) / 64) tile rows): per lower
      tile (I, K) min(K, npt) tile products of 2 * 64^3, plus for a pivot
      column the diagonal tile's factor and inverse (2 * 64^3 / 3) or the
      sub-diagonal tile's product with the inverse (2 * 64^3);
    * L bytes: es * (np (np + 1) / 2 + np m) over the fronts, the entries of
      L each triangular solve must read once (the algorithmic bytes), and the
      padded bytes the solve kernels read (the pivot columns' lower tiles and
      the inverse diagonal tiles)."""
    plan = solver.nd_analyse(n, rp, ci, leaf=leaf)
    npv = (plan["end"] - plan["start"]).astype(np.float64)
    m = np.array([len(x) for x in plan["st"]], dtype=np.float64)
    true_flops = float(np.sum(npv ** 3 / 3 + npv ** 2 * m + npv * m ** 2))
    npt = np.ceil(npv / 64)
    nt = np.ceil((64 * npt + m) / 64)
    t3 = 64.0 ** 3
    padded = 0.0
    solve_bytes = 0.0
    for p_, q_ in zip(npt.astype(np.int64), nt.astype(np.int64)):
        # products: tiles (I, K), K < nt, I >= K, each min(K, npt) products
        ks = np.arange(q_)
        padded += 2 * t3 * float(np.sum((q_ - ks) * np.minimum(ks, p_)))
        padded += p_ * 2 * t3 / 3 + 2 * t3 * float(np.sum(q_ - 1 - np.arange(p_)))
        solve_bytes += es * 4096.0 * (float(np.sum(q_ - 1 - np.arange(p_))) + p_)
    l_bytes = float(es * np.sum(npv * (npv + 1) / 2 + npv * m))
    return {"leaf": leaf, "fronts": int(npv.size), "true_flops": true_flops, "padded_flops": padded,
            "l_bytes": l_bytes, "padded_solve_bytes": solve_bytes,
            "l_nnz": int(np.sum(npv * (npv + 1) / 2 + npv * m))}


def cpu_baseline(fixture, g=1000, sample_rows_g=25, small=250):
    """The oracle's band restatement of solve (the reference's operation order,
    one thread of THIS host: on the GPU box, the node's own cores) on a bounded
    sample: the leading sample_rows_g grid rows of the g x g system (its factor
    is the first rows of the full factor; transpose and the tri-solves are
    linear in rows too), scaled by N/R. A whole small system (small^2) is
    timed beside it. The full 1000^2 run of the build container (the committed
    fixture's cpu_seconds) is kept as a cross-check."""
    n = g * g
    R, rp, ci, v, b = leading_system(g, sample_rows_g)
    t0 = time.perf_counter()
    orc.solve(R, rp, ci, v, [b], band=True)
    t_sample = time.perf_counter() - t0
    est = t_sample * n / R
    rp2, ci2, v2, b2, _ = system(small, np.float64)
    t0 = time.perf_counter()
    orc.solve(small * small, rp2, ci2, v2, [b2], band=True)
    t_small = time.perf_counter() - t0
    container = float(sum(fixture["cpu_seconds"].values())) if fixture and fixture.get("cpu_seconds") else None
    return {
        "value_s": round(est, 2),
        "unit": "s per solve",
        "cores": 1,
        "kind": "port",
        "sample": (f"oracle band restatement of solve (lib.rs:11-24, reference operation order; C, -O2 "
                   f"-ffp-contract=off, 1 thread) timed on this host on the leading {sample_rows_g} grid rows "
                   f"of the {g}^2 system (R = {R:,} of N = {n:,} unknowns, band {g}: {t_sample:.2f} s), "
                   f"x N/R = {n / R:g}"),
        "sample_s": round(t_sample, 3),
        "measured_s": {f"{small}x{small}": round(t_small, 3)},
        "build_container_full_run_s": round(container, 1) if container else None,
        "host_cpus": os.cpu_count(),
    }


def roof(work, ms, peak, scale):
    """achieved (work / time, in the unit of `peak`) and its fraction of peak"""
    if not ms:
        return None, None
    a = work / (ms * 1e-3) / scale
    return round(a, 3), round(a / peak, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=1000)
    ap.add_argument("--dtype", default="f64", choices=("f64", "f32"))
    ap.add_argument("--reps", type=int, default=2, help="timed solves per order (after one warm-up)")
    ap.add_argument("--orders", default="reference,blocked,nd")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-grid-rows", type=int, default=25,
                    help="CPU baseline: leading grid rows of the system timed on this host (x N/R)")
    ap.add_argument("--kernel-stats", default=None,
                    help="a rocprofv3 kernel-stats CSV of an earlier run of this command: the nd factor line then "
                         "carries the selected inverse's device time per kernel and call (selinv_kernels_ms)")
    ap.add_argument("--eig", type=int, default=0, metavar="NEV",
                    help="only the eigsh record: the NEV smallest eigenpairs on the kept factor, f64 and f32 factor, "
                         "block 4 and 8 (profiles/nd_eig_c5.jsonl)")
    ap.add_argument("--updown", default=None, metavar="K[,K...]",
                    help="only the update / downdate record: K random stored edges as one call, then the same call "
                         "as a downdate, against refactor (profiles/nd_updown_c5.jsonl), for each K <= 16 given")
    ap.add_argument("--sparse-rhs", action="store_true",
                    help="only the sparse right-hand side record: one entry in and one row out, one entry in and "
                         "every row out, 32 point sources with 32 rows, against the dense solve "
                         "(profiles/nd_sparse_c5.jsonl)")
    ap.add_argument("--partial", default=None, metavar="K[,K...]",
                    help="only the partial refactor record: K seeded stored entries changed and named as one call, "
                         "against refactor in the same session, and one line with an f32 factor "
                         "(profiles/nd_partial_c5.jsonl)")
    ap.add_argument("--grad", default=None, metavar="K[,K...]",
                    help="only the differentiable solve's record: refactor_values against refactor, and for each K "
                         "the solve, the backward's solve, nd_factor_sddmm (with its achieved bytes per second) and "
                         "inv_pattern, operands in HBM (profiles/nd_grad_c5.jsonl)")
    ap.add_argument("--schur", type=int, default=None, metavar="LINE",
                    help="only the Schur complement's record, the set being grid line LINE (m = g): cholesky_nd and "
                         "refactor with and without the set, schur (with the gather kernel's bytes and its share of "
                         "the HBM peak), schur_condense / schur_expand / solve for k = 1 and 32, and inv_block on the "
                         "set (profiles/nd_schur_c5.jsonl)")
    ap.add_argument("--mass", choices=("none", "lumped", "consistent"), default=None,
                    help="with --eig: the generalised problem's mass matrix, block 4 (profiles/nd_eig_gen_c5.jsonl). "
                         "lumped: a diagonal hashed into [0.5, 2); consistent: the 9-point kron(M1, M1), M1 = "
                         "tridiag(1/6, 4/6, 1/6); none: the same record without m, the yardstick of the other two")
    args = ap.parse_args()
    dt = np.float64 if args.dtype == "f64" else np.float32
    g = args.g
    n = g * g
    rp, ci, v, b, x_true = system(g, dt)
    A = Csr.from_csr_arrays((n, n), rp, ci, v)
    B = Dense.from_columns([b])
    if args.updown:
        _lib.stage_timing(True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "nd_updown_c5.jsonl"), "a") as out:
            for line in nd_updown_ops(A, B, [int(k) for k in args.updown.split(",")], max(args.reps, 1),
                                      (n, rp, ci, v)):
                print(json.dumps(line), flush=True)
                out.write(json.dumps(line) + "\n")
        return
    if args.sparse_rhs:
        _lib.stage_timing(True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "nd_sparse_c5.jsonl"), "a") as out:
            for line in nd_sparse_rhs_ops(A, B, max(args.reps, 1), (n, rp, ci, v)):
                print(json.dumps(line), flush=True)
                out.write(json.dumps(line) + "\n")
        return
    if args.partial:
        _lib.stage_timing(True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "nd_partial_c5.jsonl"), "a") as out:
            for line in nd_partial_ops(A, B, [int(k) for k in args.partial.split(",")], max(args.reps, 1),
                                       (n, rp, ci, v)):
                print(json.dumps(line), flush=True)
                out.write(json.dumps(line) + "\n")
        return
    if args.grad:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "nd_grad_c5.jsonl"), "a") as out:
            for line in nd_grad_ops(A, [int(k) for k in args.grad.split(",")], (n, rp, ci, v)):
                print(json.dumps(line), flush=True)
                out.write(json.dumps(line) + "\n")
        return
    if args.schur is not None:
        _lib.stage_timing(True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        line = nd_schur_ops(A, g, args.schur, (n, rp, ci, v))
        print(json.dumps(line), flush=True)
        with open(os.path.join(ROOT, "profiles", "nd_schur_c5.jsonl"), "a") as out:
            out.write(json.dumps(line) + "\n")
        return
    if args.eig:
        _lib.stage_timing(True)
        print(json.dumps(nd_eig_ops(A, B, args.eig, max(args.reps, 1), g, args.mass)), flush=True)
        return
    fixture = None
    fx_path = os.path.join(ROOT, "tests", "golden", f"c5_poisson_{g}.json")
    if os.path.exists(fx_path) and args.dtype == "f64":
        with open(fx_path) as f:
            fixture = json.load(f)
    cpu = None if args.no_cpu_baseline else cpu_baseline(fixture, g, min(args.cpu_sample_grid_rows, g))
    es = np.dtype(dt).itemsize
    flops = float(n) * g * g  # sum over rows of b^2 / 2 multiply-add pairs, x 2
    band_bytes = float(es) * n * (g + 1)
    _lib.stage_timing(True)
    for order in args.orders.split(","):
        cold = by_value = model = nd_solves = None
        if order == "nd":
            leaf = int(os.environ.get("BSM_ND_LEAF", "192"))
            model = nd_model(n, rp, ci, leaf, es)
            # the process's first GPU work (runtime and device set-up, code
            # objects) on a small system of another pattern, outside the clock:
            # "cold" is the first solve of THIS pattern, not the process's first
            wrp, wci, wv = orc.poisson2d(16)
            solve(Csr.from_csr_arrays((256, 256), wrp, wci, wv.astype(dt)),
                  Dense.from_columns([np.ones(256, dtype=dt)]), order="nd")
            nd_solves = {"small_warmup_16x16": 1, "full": 1 + max(args.reps, 1) + 1 + args.reps}
            # cold: the first solve of this pattern in the process, as the
            # reference's solve(a, b) is called (lib.rs:11, `a` by value): a new
            # handle (uploaded inside the clock), the host analysis, the plan
            # upload, the first allocation of the fronts, the solve
            _lib.nd_cache_clear()
            t0 = time.perf_counter()
            A_cold = Csr.from_csr_arrays((n, n), rp, ci, v)
            A_cold._device()
            t_up = time.perf_counter()
            solve(A_cold, B, order=order)
            t1 = time.perf_counter()
            cold = {"wall_ms": round(1e3 * (t1 - t0), 2), "upload_ms": round(1e3 * (t_up - t0), 2),
                    "solve_call_ms": round(1e3 * (t1 - t_up), 2),
                    "stages_ms": {k: round(t, 3) for k, t in _lib.stage_times().items()}}
            del A_cold
            # by value, pattern seen before: a new handle per call again, the
            # plan found in the library's cache by the pattern
            walls, calls, st_bv = [], [], []
            for _ in range(max(args.reps, 1)):
                t0 = time.perf_counter()
                A_bv = Csr.from_csr_arrays((n, n), rp, ci, v)
                A_bv._device()
                t_up = time.perf_counter()
                solve(A_bv, B, order=order)
                t1 = time.perf_counter()
                walls.append(t1 - t0)
                calls.append(t1 - t_up)
                st_bv.append(_lib.stage_times())
                del A_bv
            by_value = {"wall_ms": round(1e3 * float(np.median(walls)), 2),
                        "solve_call_ms": round(1e3 * float(np.median(calls)), 2),
                        "upload_ms": round(1e3 * float(np.median(walls) - np.median(calls)), 2),
                        "stages_ms": {k: round(float(np.mean([s_[k] for s_ in st_bv])), 3) for k in st_bv[-1]},
                        "cache": _lib.nd_cache_info()}
        solve(A, B, order=order)  # warm-up (first call uploads A; nd: attaches the plan to the handle)
        walls, stages = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            x = solve(A, B, order=order).get_col(0)
            walls.append(time.perf_counter() - t0)
            stages.append(_lib.stage_times())
        st = {k: round(float(np.mean([s[k] for s in stages])), 3) for k in stages[-1]}
        rel = float(np.linalg.norm(x.astype(np.float64) - x_true) / np.linalg.norm(x_true))
        line = {
            "metric": "C5 solve: device ms per stage, flop/byte roofline per kernel",
            "config": {"workload": f"c5: 2D 5-point Poisson {g}x{g} (N={n:,}, band {g}), natural ordering, "
                                   f"b = A x_true (seed 1002), 1 RHS", "dtype": args.dtype, "order": order},
            "wall_ms": round(1e3 * float(np.median(walls)), 2),
            "stages_ms": st,
            "device_ms_total": round(sum(st.values()), 2),
        }
        if order == "nd":
            # scored against the nd plan's own work (nd_model), never the band's
            fms, fw, bw = st.get("nd_factor"), st.get("nd_forward"), st.get("nd_backward")
            ta, tf = roof(model["true_flops"], fms, F64_PEAK_TFS, 1e12)
            pa, pf = roof(model["padded_flops"], fms, F64_PEAK_TFS, 1e12)
            # one right-hand side in the default pipeline: the forward solve is folded
            # into the factor's diagonal tiles (BSM_ND_FOLD), its stage only marks time
            folded = os.environ.get("BSM_ND_FOLD", "1") != "0" and os.environ.get("BSM_ND_PLAIN", "0") != "1"
            fa, ff = (None, None) if folded else roof(model["l_bytes"], fw, HBM_PEAK_GBS, 1e9)
            ba, bf = roof(model["l_bytes"], bw, HBM_PEAK_GBS, 1e9)
            line.update({
                "primary": "cold: solve(a, b) takes a by value (lib.rs:11), so a drop-in caller's first solve of "
                           "a pattern pays the analysis; by_value: later calls with new handles of that pattern; "
                           "wall_ms: the same handle again",
                "cold": cold, "by_value": by_value, "model": model, "nd_solves_in_process": nd_solves,
                "factor": {"stage": "nd_factor (zero tiles + assemble are nd_assemble; the extend-adds run inside "
                                    "this stage, so its time bounds the factor kernels' from above"
                                    + ("; the forward solve is folded into it" if folded else "") + ")",
                           "ms": fms, "true_flops": model["true_flops"], "padded_flops": model["padded_flops"],
                           "achieved_TFs_true": ta, "frac_true": tf, "achieved_TFs_padded": pa, "frac_padded": pf,
                           "peak_TFs": F64_PEAK_TFS},
                "forward": ({"ms": fw, "folded": "into nd_factor's diagonal tiles (BSM_ND_FOLD): y and the update "
                                                "vectors formed from the L tiles the factor holds; no pass over L"}
                            if folded else
                            {"ms": fw, "alg_bytes": model["l_bytes"], "padded_bytes_read": model["padded_solve_bytes"],
                             "achieved_GBs": fa, "frac": ff, "peak_GBs": HBM_PEAK_GBS}),
                "backward": {"ms": bw, "alg_bytes": model["l_bytes"], "padded_bytes_read": model["padded_solve_bytes"],
                             "achieved_GBs": ba, "frac": bf, "peak_GBs": HBM_PEAK_GBS},
            })
        else:
            fa, ff = roof(flops, st.get("cholesky"), F64_PEAK_TFS, 1e12)
            wa, wf = roof(band_bytes, st.get("forward"), HBM_PEAK_GBS, 1e9)
            ba, bf = roof(band_bytes, st.get("backward"), HBM_PEAK_GBS, 1e9)
            line.update({
                "factor": {"kernel": {"reference": f"{band_kernel()} (reference order)",
                                      "blocked": "blk_chol (blocked)"}[order],
                           "flops": flops, "ms": st.get("cholesky"), "achieved_TFs": fa, "peak_TFs": F64_PEAK_TFS,
                           "frac": ff},
                "forward": {"bytes": band_bytes, "ms": st.get("forward"), "achieved_GBs": wa,
                            "peak_GBs": HBM_PEAK_GBS, "frac": wf},
                "backward": {"bytes": band_bytes, "ms": st.get("backward"), "achieved_GBs": ba,
                             "peak_GBs": HBM_PEAK_GBS, "frac": bf},
            })
        line.update({
            "rel_err_vs_x_true": rel,
            "cpu_baseline": cpu,
            "vs_cpu": round(cpu["value_s"] / (float(np.median(walls))), 1) if cpu else None,
            "vs_cpu_cold": round(cpu["value_s"] / (cold["wall_ms"] * 1e-3), 1) if cpu and cold else None,
        })
        if fixture is not None:
            h = hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tobytes()).hexdigest()
            line["x_bits_equal_oracle_fixture"] = h == fixture["sha256_x_f64_bits"]
            ex = np.array([int(t, 16) for t in fixture["x_sample_bits"]], dtype=np.uint64).view(np.float64)
            xs = x[::fixture["x_stride"]][:ex.size].astype(np.float64)
            line["max_rel_dev_vs_oracle_x_sample"] = float(np.max(np.abs(xs - ex) / np.abs(ex)))
            line["oracle_fixture_cpu_s"] = fixture.get("cpu_seconds")
        print(json.dumps(line), flush=True)
        if order == "nd":
            print(json.dumps(nd_factor_line(A, B, args, by_value, line["wall_ms"], x, (n, rp, ci, v))), flush=True)
            if args.dtype == "f64":  # a third record: pcg on the kept factor (profiles/nd_pcg_c5.jsonl)
                print(json.dumps(nd_pcg_ops(A, B, max(args.reps, 1), (n, rp, ci, v))), flush=True)


def selinv_kernel_split(path, dtype):
    """{nd_selinv_* kernel: device ms per selected inverse} from a rocprofv3 kernel-stats CSV (one
    nd_selinv_diag_out launch per inv_diag call)."""
    import csv

    tot, calls = {}, {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if "nd_selinv_" not in name or f"<{dtype}>" not in name:
                continue
            short = name[name.index("nd_selinv_"):].split("<")[0]
            tot[short] = tot.get(short, 0) + int(row["TotalDurationNs"])
            calls[short] = calls.get(short, 0) + int(row["Calls"])
    n = calls.get("nd_selinv_diag_out", 0)
    if n == 0:
        return None
    out = {k: round(v * 1e-6 / n, 4) for k, v in sorted(tot.items())}
    out["launches_per_call"] = round(sum(calls.values()) / n, 1)
    out["calls"] = n
    return out


def nd_factor_ops(f, A, B, reps, pattern, kernel_stats=None):
    """What the kept factor does beyond solve and export, host wall ms around
    synchronous calls. refactor_ms: NdFactor.refactor alternating two value
    sets of the pattern (A2 = D A D on a handle of its own, whose pattern the
    factor compares with its copy; A on the handle the plan came from);
    logdet_ms; solve_dev_ms: device.nd_factor_solve, one column, b and x
    resident in HBM; solve_L_ms / solve_Lt_ms: the forward / backward pass
    alone through the host-buffer call; selinv_ms: NdFactor.inv_diag (host
    out), selinv_dev_ms: device.nd_factor_inv_diag into a resident tensor,
    selinv_alloc_ms: the stage before the first kernel (Z and the panels
    allocated; they are freed again inside the call's wall time),
    selinv_device_ms: the levels' kernels between their stage marks. f ends
    holding A's factor again."""
    import torch

    from basic_sparse_matrix_amd import device

    n, rp, ci, v = pattern
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    d = 1.0 + np.random.default_rng(11).random(n)
    A2 = Csr.from_csr_arrays((n, n), rp, ci, (d[rows] * v * d[ci.astype(np.int64)]).astype(v.dtype))
    A2._device()
    f.refactor(A2)  # warm-up: the handle's upload, the temporaries
    f.refactor(A)
    t_re, st_re = [], []
    for i in range(2 * max(reps, 2)):
        t0 = time.perf_counter()
        f.refactor(A if i % 2 else A2)
        t_re.append(time.perf_counter() - t0)
        st_re.append(_lib.stage_times())

    def timed(fn, count):
        fn()  # warm-up
        ts = []
        for _ in range(count):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    count = max(5 * reps, 10)
    t_ld = timed(f.logdet, count)
    logdet = f.logdet()
    bd = torch.tensor(np.ascontiguousarray(B.get_col(0)), device="cuda")
    xd = torch.empty_like(bd)
    t_dev = timed(lambda: device.nd_factor_solve(f, bd, out=xd), count)
    t_l = timed(lambda: f.solve(B, system="L"), count)
    t_lt = timed(lambda: f.solve(B, system="Lt"), count)
    x_host = np.asarray(f.solve(B).get_col(0))
    st_si = []

    def inv_diag_staged():
        f.inv_diag()
        st_si.append(_lib.stage_times())

    n_si = max(reps, 3)
    t_si = timed(inv_diag_staged, n_si)
    dd = torch.empty(n, dtype=bd.dtype, device="cuda")
    t_sid = timed(lambda: device.nd_factor_inv_diag(f, dd), n_si)
    diag = f.inv_diag()
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    mm = lambda t: [round(1e3 * min(t), 3), round(1e3 * max(t), 3)]  # noqa: E731
    return {
        "refactor_ms": med(t_re), "refactor_ms_min_max": mm(t_re), "refactor_calls": len(t_re),
        "refactor_stages_ms": {k: round(float(np.mean([s[k] for s in st_re])), 3) for k in st_re[-1]},
        "logdet_ms": med(t_ld), "logdet": logdet,
        "solve_dev_ms": med(t_dev), "solve_dev_ms_min_max": mm(t_dev),
        "solve_dev_bits_equal_host_solve": bool(np.array_equal(xd.cpu().numpy(), x_host)),
        "solve_L_ms": med(t_l), "solve_Lt_ms": med(t_lt),
        "selinv_ms": med(t_si), "selinv_ms_min_max": mm(t_si), "selinv_calls": len(t_si),
        "selinv_dev_ms": med(t_sid), "selinv_dev_ms_min_max": mm(t_sid),
        "selinv_alloc_ms": round(float(np.median([s.get("nd_selinv_alloc", 0.0) for s in st_si[1:]])), 3),
        "selinv_device_ms": round(float(np.median([s.get("nd_selinv", 0.0) for s in st_si[1:]])), 3),
        "selinv_dev_bits_equal_host": bool(np.array_equal(dd.cpu().numpy(), diag)),
        "selinv_diag_min_max": [float(diag.min()), float(diag.max())],
        "selinv_kernels_ms": selinv_kernel_split(kernel_stats, "double" if v.dtype == np.float64 else "float")
        if kernel_stats else None,
    }


def nd_refine_ops(A, B, reps, f64_nbytes):
    """The mixed-precision path on an f64 system, host wall ms around
    synchronous calls. factor_f32_ms: cholesky_nd(A, factor_dtype=float32) on
    the warm handle (the values converted inside the clock); refined_ms:
    device.nd_factor_solve_refined on that factor with the f64 A, one column,
    b and x resident in HBM (A's symmetric copy built by the warm-up call),
    with its iters and berr; refined_no_correction_ms: the same with
    max_iter=0 (one solve, one residual); solve_dev_f32_ms: the f32 factor's
    plain device solve; resid_ms / update_ms / judge_ms: the last iteration's
    residual pass, iterate update and reduction between their stage marks
    (0 when the stage timer is off); nbytes of both factors."""
    import torch

    from basic_sparse_matrix_amd import cholesky_nd, device

    t_factor = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f = cholesky_nd(A, factor_dtype=np.float32)
        t_factor.append(time.perf_counter() - t0)
        f.close()
    f = cholesky_nd(A, factor_dtype=np.float32)
    bd = torch.tensor(np.ascontiguousarray(B.get_col(0)), device="cuda")
    xd = torch.empty_like(bd)
    b32 = bd.to(torch.float32)
    x32 = torch.empty_like(b32)
    t0 = time.perf_counter()
    _, info = device.nd_factor_solve_refined(f, A, bd, out=xd)  # builds A's symmetric copy
    first_ms = 1e3 * (time.perf_counter() - t0)
    count = max(5 * reps, 10)
    t_ref, t_ref0, t_plain, st = [], [], [], []
    for _ in range(count):
        t0 = time.perf_counter()
        _, info = device.nd_factor_solve_refined(f, A, bd, out=xd)
        t_ref.append(time.perf_counter() - t0)
        st.append(_lib.stage_times())
        t0 = time.perf_counter()
        device.nd_factor_solve_refined(f, A, bd, out=xd, max_iter=0)
        t_ref0.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        device.nd_factor_solve(f, b32, out=x32)
        t_plain.append(time.perf_counter() - t0)
    nbytes = f.nbytes
    f.close()
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    mm = lambda t: [round(1e3 * min(t), 3), round(1e3 * max(t), 3)]  # noqa: E731
    stage = lambda k: round(float(np.median([s.get(k, 0.0) for s in st])), 4)  # noqa: E731
    return {
        "factor_f32_ms": med(t_factor), "factor_f32_ms_min_max": mm(t_factor),
        "refined_ms": med(t_ref), "refined_ms_min_max": mm(t_ref), "refined_calls": len(t_ref),
        "refined_first_call_ms": round(first_ms, 3),
        "refined_iters": int(info.iters[0]), "refined_berr": float(info.berr[0]), "refined_tol": info.tol,
        "refined_converged": bool(info.converged[0]),
        "refined_no_correction_ms": med(t_ref0), "solve_dev_f32_ms": med(t_plain),
        "resid_ms": stage("refine_resid"), "update_ms": stage("refine_update"), "judge_ms": stage("refine_judge"),
        "factor_f32_nbytes": nbytes, "factor_f64_nbytes": f64_nbytes,
    }


def nd_pcg_ops(A, B, reps, pattern):
    """Preconditioned CG on a kept factor against the refined solve, one
    device-resident column, host wall ms around synchronous calls (medians):
    the f32 factor of A on A itself, and the f64 factor of A on A + 0.01 I (a
    stale factor), on 3 A and on A + 1e-6 I (a shift that is small against
    A's smallest eigenvalue at g = 1000, 2e-5, as 0.01 is at the tests'
    g = 11). Per case and solver: iters, berr, converged, ms.
    pcg_stages_ms: the last step's kernels between their stage marks
    (pcg_dots_p: the two dots, beta and p = z + beta p; pcg_spmv_dot: q = S p
    with p . q, and alpha; pcg_step_xr: x, r and their norms, and the rule;
    pcg_verify: the true residual, its rule and the take-over of r), 0 when
    the stage timer is off or the stage did not run."""
    import torch

    from basic_sparse_matrix_amd import cholesky_nd, device

    n, rp, ci, v = pattern
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    diag = rows == ci.astype(np.int64)
    A_stale = Csr.from_csr_arrays((n, n), rp, ci, v + 0.01 * diag)
    A_3 = Csr.from_csr_arrays((n, n), rp, ci, 3.0 * v)
    A_near = Csr.from_csr_arrays((n, n), rp, ci, v + 1e-6 * diag)
    bd = torch.tensor(np.ascontiguousarray(B.get_col(0)), device="cuda")
    xd = torch.empty_like(bd)
    count = max(5 * reps, 10)
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    out = {"metric": "C5 nd factor: pcg against the refined solve, one device column (host wall ms, medians)",
           "config": {"g": int(round(n ** 0.5)), "rhs": 1, "calls": count}, "cases": {}}
    cases = (("f32_factor_on_A", np.float32, A), ("f64_factor_on_A_plus_0.01I", np.float64, A_stale),
             ("f64_factor_on_3A", np.float64, A_3), ("f64_factor_on_A_plus_1e-6I", np.float64, A_near))
    for name, fdt, S in cases:
        with cholesky_nd(A, factor_dtype=fdt) as f:
            device.nd_factor_solve_pcg(f, S, bd, out=xd)  # builds S's symmetric copy, warms the temporaries
            device.nd_factor_solve_refined(f, S, bd, out=xd, max_iter=30)
            t_pcg, t_ref, st = [], [], []
            for _ in range(count):
                t0 = time.perf_counter()
                _, pi = device.nd_factor_solve_pcg(f, S, bd, out=xd)
                t_pcg.append(time.perf_counter() - t0)
                st.append(_lib.stage_times())
                t0 = time.perf_counter()
                _, ri = device.nd_factor_solve_refined(f, S, bd, out=xd, max_iter=30)
                t_ref.append(time.perf_counter() - t0)
        stage = lambda k: round(float(np.median([s.get(k, 0.0) for s in st])), 4)  # noqa: E731
        out["cases"][name] = {
            "pcg_iters": int(pi.iters[0]), "pcg_berr": float(pi.berr[0]), "pcg_converged": bool(pi.converged[0]),
            "pcg_breakdown": bool(pi.breakdown[0]), "pcg_ms": med(t_pcg),
            "pcg_ms_min_max": [round(1e3 * min(t_pcg), 3), round(1e3 * max(t_pcg), 3)],
            "pcg_stages_ms": {k: stage(k) for k in ("pcg_dots_p", "pcg_spmv_dot", "pcg_step_xr", "pcg_verify")},
            "refined_iters": int(ri.iters[0]), "refined_berr": float(ri.berr[0]),
            "refined_converged": bool(ri.converged[0]), "refined_ms": med(t_ref), "tol": pi.tol,
        }
    return out


def nd_updown_ops(A, B, ks, reps, pattern):
    """The kept factor's rank-K update and downdate against refactor, f64: K
    random stored edges (i, j) as one call, W's column sqrt(0.5) (e_i - e_j)
    (half of the edge's conductance again, then taken out again), seeded. Host
    wall ms around the synchronous C-ABI call on column-compressed arrays
    built beforehand (medians of `reps`); python_ms is NdFactor.update on a
    Csr of n rows, whose conversion to columns is host work over n. Stages by
    mark: place (the work columns zeroed and W placed), sweep (a downdate's:
    the dry pass and the writing pass), dinv. active_fronts: the union of the
    K paths, from the host analysis. berr_after: the backward error of one
    solve after the update and its downdate, against the factored matrix. One
    JSON line per case, also appended to profiles/nd_updown_c5.jsonl."""
    from basic_sparse_matrix_amd import cholesky_nd

    n, rp, ci, v = pattern
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    cols = ci.astype(np.int64)
    upper = np.flatnonzero(rows < cols)
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    lib = _lib.require_device()
    lines = []
    with cholesky_nd(A) as f:
        perm = f.perm
        pinv = np.empty(n, dtype=np.int64)
        pinv[perm] = np.arange(n)
        tree = solver.nd_analyse(n, rp, ci, leaf=int(os.environ.get("BSM_ND_LEAF", "192")))
        assert np.array_equal(tree["perm"], perm)
        owner = np.empty(n, dtype=np.int64)
        for i, (a0, a1) in enumerate(zip(tree["start"], tree["end"])):
            owner[a0:a1] = i
        b0 = np.ascontiguousarray(B.get_col(0))
        t_ref = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f.refactor(A)
            t_ref.append(time.perf_counter() - t0)
        ref_stages = {k: round(t, 4) for k, t in _lib.stage_times().items()}
        for K in ks:
            pick = np.random.default_rng(1000 + K).choice(upper, size=K, replace=False)
            cp = (2 * np.arange(K + 1)).astype(np.uint64)
            wr = np.sort(np.stack([rows[pick], cols[pick]], axis=1), axis=1).astype(np.uint64).ravel()
            wv = np.tile(np.array([np.sqrt(0.5), -np.sqrt(0.5)]), K)
            active = set()
            for e in pick:
                x = int(owner[min(pinv[rows[e]], pinv[cols[e]])])
                while x >= 0 and x not in active:
                    active.add(x)
                    x = int(tree["parent"][x])
            wc = np.repeat(np.arange(K), 2)
            o = np.lexsort((wc, wr.astype(np.int64)))
            W = Csr.from_csr_arrays((n, K), np.concatenate([[0], np.cumsum(np.bincount(wr.astype(np.int64), minlength=n))])
                                    .astype(np.uint64), wc[o].astype(np.uint64), wv[o])
            times = {1: [], -1: []}
            stages = {1: [], -1: []}
            for _ in range(reps + 1):  # the first pair warms the temporaries
                for sign in (1, -1):
                    t0 = time.perf_counter()
                    rc = lib.bsm_nd_factor_updown(f.handle, sign, K, _lib.ptr(cp), _lib.ptr(wr), _lib.ptr(wv))
                    times[sign].append(time.perf_counter() - t0)
                    assert rc == 0, _lib.last_error()
                    stages[sign].append(_lib.stage_times())
            x = np.asarray(f.solve(B).get_col(0), dtype=np.float64)
            r = b0 - np.bincount(rows, weights=v * x[cols], minlength=n)
            snorm = float(np.bincount(rows, weights=np.abs(v), minlength=n).max())
            berr = float(np.abs(r).max() / (snorm * np.abs(x).max() + np.abs(b0).max()))
            f.refactor(A)  # each K starts from the fresh factor
            line = {"metric": "C5 nd factor: rank-K update and downdate of K stored edges against refactor "
                              "(host wall ms, medians)",
                    "config": {"g": int(round(n ** 0.5)), "K": int(K), "calls": reps, "dtype": "f64"},
                    "active_fronts": len(active), "fronts": int(len(tree["start"])),
                    "levels": int(tree["level"].max()) + 1, "refactor_ms": med(t_ref),
                    "refactor_stages_ms": ref_stages, "berr_after": berr}
            for sign, name in ((1, "update"), (-1, "downdate")):
                line[name + "_ms"] = med(times[sign][1:])
                line[name + "_ms_min_max"] = [round(1e3 * min(times[sign][1:]), 3), round(1e3 * max(times[sign][1:]), 3)]
                line[name + "_stages_ms"] = {
                    k: round(float(np.median([s_.get(k, 0.0) for s_ in stages[sign][1:]])), 4)
                    for k in ("nd_updown_place", "nd_updown_sweep", "nd_updown_dinv")}
            t0 = time.perf_counter()
            f.update(W)
            line["python_update_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            f.refactor(A)
            lines.append(line)
    return lines


HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, the vendor's figure; a float4 copy reaches 6.29e12 of it


def nd_schur_ops(A, g, line, pattern):
    """The Schur complement on grid line `line` (m = g vertices) of the kept
    factor: host wall ms around synchronous calls, medians of 6 after a
    warm-up pair, all in one session, operands of the solves in HBM. create:
    cholesky_nd on a fresh handle of the pattern (without the set the first is
    the cold analysis and the later ones take the plan from the cache; with
    the set every call analyses: the plan is the factor's alone). The gather
    kernel's bytes are counted from the shapes: the child's update block's
    lower 64 x 64 tiles read once, S written once."""
    import torch

    from basic_sparse_matrix_amd import cholesky_nd, device

    n, rp, ci, v = pattern
    dt = A.dtype
    es = np.dtype(dt).itemsize
    idx = line * g + np.arange(g)
    m = len(idx)
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    fresh = lambda: Csr.from_csr_arrays((n, n), rp, ci, v)  # noqa: E731

    def clock(fn, warm=2, reps=6):
        t = []
        for _ in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return t[warm:]

    out = {"metric": "C5 nd factor: Schur complement on a grid line (host wall ms, medians of 6 after a warm-up pair)",
           "n": n, "m": m, "line": line, "dtype": np.dtype(dt).name}
    create = {}
    for name, sch in (("plain", None), ("schur", idx)):
        _lib.nd_cache_clear()
        t = []
        for _ in range(4):
            a = fresh()
            a._device()
            t0 = time.perf_counter()
            f = cholesky_nd(a, schur=sch)
            t.append(time.perf_counter() - t0)
            f.close()
        create[name] = {"first_ms": round(1e3 * t[0], 2), "later_ms": med(t[1:])}
    out["cholesky_nd_ms"] = create
    rng = np.random.default_rng(77)
    with cholesky_nd(A) as fp, cholesky_nd(A, schur=idx) as fs:
        out["factor_bytes"] = {"plain": fp.nbytes, "schur": fs.nbytes}
        out["refactor_ms"] = {"plain": med(clock(lambda: fp.refactor(A))), "schur": med(clock(lambda: fs.refactor(A)))}
        S_dev = torch.empty((m, m), dtype=device.TORCH_DT[np.dtype(dt)], device="cuda")
        st = []

        def gather():
            device.nd_factor_schur(fs, A, out=S_dev)
            st.append(_lib.stage_times().get("nd_schur_gather", 0.0))

        t = clock(gather)
        nt = (m + 63) // 64
        nbytes = (nt * (nt + 1) // 2) * 4096 * es + m * m * es
        kernel_ms = float(np.median(st[2:]))
        out["schur"] = {"call_ms": med(t), "host_copy_call_ms": med(clock(lambda: fs.schur(A))),
                        "gather_device_ms": round(kernel_ms, 4), "gather_bytes": nbytes,
                        "gather_bytes_per_s": round(nbytes / (kernel_ms * 1e-3), 0) if kernel_ms > 0 else None,
                        "share_of_hbm_peak": round(nbytes / (kernel_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4)
                        if kernel_ms > 0 else None}
        S = S_dev.cpu().numpy().astype(np.float64)
        for k in (1, 32):
            b = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, k)).astype(dt)).cuda()
            x = device.nd_factor_solve(fs, b)
            gk = device.nd_factor_schur_condense(fs, b)
            xg = torch.from_numpy(np.linalg.solve(S, gk.cpu().numpy().astype(np.float64)).astype(dt)).cuda()
            xe = device.nd_factor_schur_expand(fs, b, xg)
            err = float((xe - x).abs().max() / x.abs().max())
            out[f"k{k}"] = {"solve_ms": med(clock(lambda: device.nd_factor_solve(fs, b))),
                            "solve_plain_factor_ms": med(clock(lambda: device.nd_factor_solve(fp, b))),
                            "schur_condense_ms": med(clock(lambda: device.nd_factor_schur_condense(fs, b))),
                            "schur_expand_ms": med(clock(lambda: device.nd_factor_schur_expand(fs, b, xg))),
                            "condense_solve_expand_vs_solve_max_rel": err}
        # the only way to comparable information without the set: |G| solves for A^-1[G, G] (then a dense inverse)
        out["inv_block_ms"] = med(clock(lambda: fp.inv_block(idx, idx), warm=1, reps=3))
    return out


def nd_sparse_rhs_ops(A, B, reps, pattern):
    """The kept factor's solve with sparse right-hand sides and selected rows
    (bsm_nd_factor_solve_sparse) against the dense solve, in the factor's dtype:
    host wall ms around the synchronous C-ABI call on arrays built beforehand
    (medians of `reps` after one warm-up), with the call's info (forward
    fronts, backward fronts, fronts in the plan, column chunks) and its stages
    by mark. Cases: one entry in and one row out (two seeded vertices); one
    entry in and every row out; 32 point sources and 32 rows. Each is checked
    for equality with the dense solve at the rows asked for. dense: the same
    clock around bsm_nd_factor_solve_system for one column and for 32, with
    its forward / backward device ms. One JSON line per case, also appended to
    profiles/nd_sparse_c5.jsonl."""
    from basic_sparse_matrix_amd import cholesky_nd

    n = pattern[0]
    dt = A.dtype
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    lib = _lib.require_device()
    rng = np.random.default_rng(4242)
    src = rng.choice(n, size=32, replace=False).astype(np.uint64)
    want_rows = rng.choice(n, size=32, replace=False).astype(np.uint64)
    lines = []
    with cholesky_nd(A) as f:
        dense = {}
        for k in (1, 32):
            bd = [np.zeros(n, dtype=dt) for _ in range(k)]
            for j in range(k):
                bd[j][src[j]] = 1.0
            xd = [np.zeros(n, dtype=dt) for _ in range(k)]
            t, st = [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                rc = lib.bsm_nd_factor_solve_system(f.handle, 0, k, n, _lib.ptr_array(bd), _lib.ptr_array(xd))
                t.append(time.perf_counter() - t0)
                assert rc == 0, _lib.last_error()
                st.append(_lib.stage_times())
            dense[k] = {"solve_only_ms": med(t[1:]),
                        "stages_ms": {s: round(float(np.median([x.get(s, 0.0) for x in st[1:]])), 4)
                                      for s in ("nd_forward", "nd_backward", "nd_copy_out")},
                        "x": np.stack(xd, axis=1)}
        cases = (("one entry in, one row out", 1, want_rows[:1]), ("one entry in, every row out", 1, None),
                 ("32 point sources, 32 rows out", 32, want_rows))
        for name, k, xr in cases:
            cp = np.arange(k + 1, dtype=np.uint64)
            br = np.ascontiguousarray(src[:k])
            bv = np.ones(k, dtype=dt)
            nout = n if xr is None else len(xr)
            xs = [np.zeros(nout, dtype=dt) for _ in range(k)]
            info = np.zeros(4, dtype=np.uint32)
            t, st = [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                rc = lib.bsm_nd_factor_solve_sparse(f.handle, k, _lib.ptr(cp), _lib.ptr(br), _lib.ptr(bv),
                                                    0 if xr is None else nout, None if xr is None else _lib.ptr(xr),
                                                    _lib.ptr_array(xs), _lib.ptr(info))
                t.append(time.perf_counter() - t0)
                assert rc == 0, _lib.last_error()
                st.append(_lib.stage_times())
            ref = dense[k]["x"] if xr is None else dense[k]["x"][xr.astype(np.int64)]
            lines.append({
                "metric": "C5 nd factor: sparse right-hand sides and selected rows against the dense solve "
                          "(host wall ms around the C call, medians)",
                "config": {"g": int(round(n ** 0.5)), "case": name, "k": k, "rows_out": int(nout), "calls": reps,
                           "dtype": str(np.dtype(dt))},
                "solve_sparse_ms": med(t[1:]),
                "solve_sparse_ms_min_max": [round(1e3 * min(t[1:]), 3), round(1e3 * max(t[1:]), 3)],
                "info": {"forward_fronts": int(info[0]), "backward_fronts": int(info[1]), "fronts": int(info[2]),
                         "chunks": int(info[3])},
                "stages_ms": {s: round(float(np.median([x.get(s, 0.0) for x in st[1:]])), 4)
                              for s in ("nd_sparse_owners", "nd_sparse_forward", "nd_sparse_backward",
                                        "nd_sparse_gather")},
                "equals_dense": bool(np.array_equal(np.stack(xs, axis=1), ref)),
                "dense_solve_only_ms": dense[k]["solve_only_ms"],
                "dense_stages_ms": dense[k]["stages_ms"]})
    return lines


def nd_partial_ops(A, B, ks, reps, pattern):
    """The kept factor's partial refactor (bsm_nd_factor_refactor_partial)
    against refactor in the same session: K seeded stored entries with
    col <= row get new values (a diagonal entry + 1/4, an edge 3/4 of its value:
    the matrix stays diagonally dominant) and are named in one call; the next
    call names them again with the first matrix's values, so every call is a
    partial refactor of K changed entries. Host wall ms around the synchronous
    C-ABI call on device handles made beforehand (medians of `reps` after one
    warm-up pair), the call's info and its stages by mark (owners: the checks
    and the start fronts; select: the task selection and the values; factor:
    nd_factor on the active fronts). refactor: the same clock around
    bsm_nd_factor_refactor, before and after the partial calls. equals_fresh:
    solve(b) and logdet() against cholesky_nd of the changed matrix, by bits.
    One JSON line per K in the matrix's dtype, then one with an f32 factor for
    the first K; also appended to profiles/nd_partial_c5.jsonl."""
    from basic_sparse_matrix_amd import cholesky_nd

    n, rp, ci, v = pattern
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    cols = ci.astype(np.int64)
    lower = np.flatnonzero(cols <= rows)
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    lib = _lib.require_device()
    ha = A._device().handle
    lines = []

    def refactor_ms(f):
        t = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            rc = lib.bsm_nd_factor_refactor(f.handle, ha)
            t.append(time.perf_counter() - t0)
            assert rc == 0, _lib.last_error()
        return t[1:], {k: round(x, 4) for k, x in _lib.stage_times().items()}

    for fdt in (A.dtype, np.dtype(np.float32)):
        if fdt != A.dtype:
            ks = ks[:1]
        Bf = Dense.from_columns([np.ascontiguousarray(np.asarray(B.get_col(0)).astype(fdt))])
        with cholesky_nd(A, factor_dtype=fdt) as f:
            t_ref, ref_stages = refactor_ms(f)
            for K in ks:
                pick = np.random.default_rng(2000 + K).choice(lower, size=K, replace=False)
                v2 = np.array(v)
                v2[pick] = np.where(rows[pick] == cols[pick], v[pick] + 0.25, 0.75 * v[pick])
                A2 = Csr.from_csr_arrays((n, n), rp, ci, v2)
                h2 = A2._device().handle
                r = np.ascontiguousarray(rows[pick].astype(np.uint64))
                c = np.ascontiguousarray(cols[pick].astype(np.uint64))
                info = np.zeros(3, dtype=np.uint64)
                times, stages = {"new": [], "old": []}, {"new": [], "old": []}
                for _ in range(reps + 1):  # the first pair warms the temporaries
                    for key, h in (("new", h2), ("old", ha)):
                        t0 = time.perf_counter()
                        rc = lib.bsm_nd_factor_refactor_partial(f.handle, h, K, _lib.ptr(r), _lib.ptr(c), _lib.ptr(info))
                        times[key].append(time.perf_counter() - t0)
                        assert rc == 0, _lib.last_error()
                        stages[key].append(_lib.stage_times())
                rc = lib.bsm_nd_factor_refactor_partial(f.handle, h2, K, _lib.ptr(r), _lib.ptr(c), _lib.ptr(info))
                assert rc == 0, _lib.last_error()
                with cholesky_nd(A2, factor_dtype=fdt) as fresh:
                    same = (np.array_equal(np.asarray(f.solve(Bf).get_col(0)), np.asarray(fresh.solve(Bf).get_col(0)))
                            and f.logdet() == fresh.logdet())
                rc = lib.bsm_nd_factor_refactor_partial(f.handle, ha, K, _lib.ptr(r), _lib.ptr(c), _lib.ptr(info))
                assert rc == 0, _lib.last_error()
                t_all = times["new"][1:] + times["old"][1:]
                st_all = stages["new"][1:] + stages["old"][1:]
                lines.append({
                    "metric": "C5 nd factor: partial refactor of K changed stored entries against refactor "
                              "(host wall ms around the C call, medians)",
                    "config": {"g": int(round(n ** 0.5)), "K": int(K), "calls": len(t_all),
                               "dtype": str(np.dtype(A.dtype)), "factor_dtype": str(np.dtype(fdt))},
                    "active_fronts": int(info[0]), "fronts": int(info[1]), "changed": int(info[2]),
                    "partial_ms": med(t_all),
                    "partial_ms_min_max": [round(1e3 * min(t_all), 3), round(1e3 * max(t_all), 3)],
                    "partial_stages_ms": {k: round(float(np.median([x.get(k, 0.0) for x in st_all])), 4)
                                          for k in ("nd_partial_owners", "nd_partial_select", "nd_partial_factor")},
                    "equals_fresh": bool(same),
                    "refactor_ms": med(t_ref),
                    "refactor_ms_min_max": [round(1e3 * min(t_ref), 3), round(1e3 * max(t_ref), 3)],
                    "refactor_stages_ms": ref_stages})
            t_after, _ = refactor_ms(f)
            for line in lines:
                if line["config"]["factor_dtype"] == str(np.dtype(fdt)):
                    line["refactor_after_ms"] = med(t_after)
    return lines


def nd_grad_ops(A, ks, pattern):
    """The differentiable solve's calls on the kept factor,
    every operand in HBM: refactor_values against refactor(a) on the same
    matrix, and per K right-hand columns the solve, the backward's solve
    (another right-hand side), nd_factor_sddmm and, once, inv_pattern (every
    call's time and stage marks beside the median: its 6 GB allocation of Z
    stalls now and then). Host wall ms around each call with
    the device drained before and after (medians of 3 after one warm-up). The SDDMM's line carries the achieved
    bytes per second over its compulsory traffic: the pattern once
    (8 (n + 1) + 4 nnz), U and V once each (2 n K es) and out once (nnz es).
    One JSON line per K, also appended to profiles/nd_grad_c5.jsonl."""
    import torch

    from basic_sparse_matrix_amd import cholesky_nd, device

    n, rp, ci, v = pattern
    es = np.dtype(A.dtype).itemsize
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731

    def timed(fn, reps=3):
        t = []
        for _ in range(reps + 1):  # the first call warms the temporaries
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return t[1:]

    lines = []
    vals = torch.tensor(np.ascontiguousarray(v), device="cuda")
    with cholesky_nd(A) as f:
        nnz = f.pattern_nnz
        t_ref = timed(lambda: f.refactor(A))
        ld_ref = f.logdet()
        t_val = timed(lambda: device.nd_factor_refactor_values(f, vals))
        same = f.logdet() == ld_ref
        z = torch.empty((nnz,), dtype=vals.dtype, device="cuda")
        _lib.stage_timing(True)  # the selected inverse's marks: its allocation of Z, the recursion, the read-out
        inv_stages = []
        t_inv = timed(lambda: (device.nd_factor_inv_pattern(f, out=z), inv_stages.append(_lib.stage_times())))
        _lib.stage_timing(False)
        inv_stages = [{k: round(x, 3) for k, x in st.items() if k.startswith("nd_selinv")} for st in inv_stages[1:]]
        for K in ks:
            gen = torch.Generator(device="cuda").manual_seed(3000 + K)
            shape = (n,) if K == 1 else (n, K)
            b = torch.randn(shape, dtype=vals.dtype, device="cuda", generator=gen)
            g = torch.randn(shape, dtype=vals.dtype, device="cuda", generator=gen)
            x, lam, out = torch.empty_like(b), torch.empty_like(b), torch.empty_like(z)
            t_solve = timed(lambda: device.nd_factor_solve(f, b, out=x))
            t_back = timed(lambda: device.nd_factor_solve(f, g, out=lam))
            t_sd = timed(lambda: device.nd_factor_sddmm(f, lam, x, out=out))
            traffic = 8 * (n + 1) + 4 * nnz + 2 * n * K * es + nnz * es
            lines.append({
                "metric": "C5 nd factor: the differentiable solve's calls, operands in HBM (host wall ms around "
                          "each call, device drained, medians of 3)",
                "config": {"g": int(round(n ** 0.5)), "K": int(K), "dtype": str(np.dtype(A.dtype)), "nnz": int(nnz)},
                "refactor_ms": med(t_ref), "refactor_values_ms": med(t_val), "refactor_values_same_logdet": bool(same),
                "solve_ms": med(t_solve), "backward_solve_ms": med(t_back), "sddmm_ms": med(t_sd),
                "sddmm_compulsory_bytes": int(traffic),
                "sddmm_gbs": round(traffic / float(np.median(t_sd)) / 1e9, 1),
                "sddmm_over_backward_solve": round(float(np.median(t_sd)) / float(np.median(t_back)), 4),
                "inv_pattern_ms": med(t_inv), "inv_pattern_ms_each": [round(1e3 * t, 3) for t in t_inv],
                "inv_pattern_stages_ms_each": inv_stages})
    return lines


def mass_matrix(g, kind):
    """The mass matrix of --mass on the g x g grid, built on the host: (Csr, the entries of S_M; both are
    stored whole, so their lower triangle mirrored is themselves)."""
    n = g * g
    if kind == "lumped":  # splitmix64 of the row index, 53 bits into [0.5, 2)
        z = np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        d = 0.5 + 1.5 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)
        idx = np.arange(n, dtype=np.uint64)
        return Csr.from_csr_arrays((n, n), np.arange(n + 1, dtype=np.uint64), idx, d), n
    i, j = np.divmod(np.arange(n, dtype=np.int64), g)
    rows, cols, vals = [], [], []
    for di in (-1, 0, 1):  # ascending columns inside a row
        for dj in (-1, 0, 1):
            ok = (i + di >= 0) & (i + di < g) & (j + dj >= 0) & (j + dj < g)
            rows.append(np.nonzero(ok)[0])
            cols.append(((i + di) * g + j + dj)[ok])
            vals.append(np.full(int(ok.sum()), (4.0 if di == 0 else 1.0) / 6.0 * ((4.0 if dj == 0 else 1.0) / 6.0)))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    return Csr.from_csr_arrays((n, n), rp, cols[order].astype(np.uint64), vals[order]), int(rows.size)


def nd_eig_ops(A, B, nev, reps, g, mass=None):
    """The nev smallest eigenpairs of the f64 system by NdFactor.eigsh (block
    shift-invert Lanczos), f64 and f32 factor, block 4 and 8, vectors left on
    the device; host wall ms around synchronous calls (medians of `reps`).
    Per case: steps, basis columns, wall ms, resid, the error of each lam
    against 4 - 2 cos(p pi / (g + 1)) - 2 cos(q pi / (g + 1)), and
    last_step_stages_ms: the LAST step's kernels between their stage marks
    (the stage list restarts with every solve: eig_solve is only the cast
    after the refined solve, whose own stages precede it; eig_reorth: both
    Gram-Schmidt passes against all ncv_used columns; eig_qr: Cholesky-QR
    twice; eig_ritz: the host's Ritz check of the largest T, the stream idle
    meanwhile; eig_resid: Y = V Z and the residuals). solve_share: steps x the
    median wall ms of a `block`-column device.nd_factor_solve_refined, over
    wall ms. reorth_GBs: 4 n ncv_used 8 bytes over the last step's eig_reorth.
    With `mass` (--mass) the record is the generalised problem's, block 4
    alone: eig_mass is the last step's three products with S_M, eig_qr holds
    the Gram matrix W^T S_M W and the two passes over W and S_M W, the lam
    errors of `consistent` are against (k_p + k_q) / (m_p m_q), k_p = 2 - 2
    cos(p pi / (g + 1)), m_p = (4 + 2 cos(p pi / (g + 1))) / 6 (none for
    `lumped`), and mass_GBs is the byte model of a product (the entries of S_M,
    12 bytes each for f64, its row pointers, and W read and S_M W written once)
    over a third of eig_mass. `none` is the same record without m."""
    import torch

    from basic_sparse_matrix_amd import cholesky_nd, device

    n = g * g
    cs = np.cos(np.arange(1, 40) * np.pi / (g + 1))
    exact = np.sort((4.0 - 2.0 * cs[:, None] - 2.0 * cs[None, :]).ravel())[:nev]
    M, m_nnz = (None, 0) if mass in (None, "none") else mass_matrix(g, mass)
    if mass == "consistent":
        mp = (4.0 + 2.0 * cs) / 6.0
        exact = np.sort((((2.0 - 2.0 * cs)[:, None] + (2.0 - 2.0 * cs)[None, :]) / (mp[:, None] * mp[None, :])).ravel())[:nev]
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    out = {"metric": "C5 nd factor: the smallest eigenpairs by block shift-invert Lanczos (host wall ms, medians)",
           "config": {"g": g, "nev": nev, "calls": reps, "ncv": 128}, "cases": {}}
    if mass is not None:
        out["config"]["mass"] = mass
    for fdt in (np.float64, np.float32):
        with cholesky_nd(A, factor_dtype=fdt) as f:
            for block in ((4, 8) if mass is None else (4,)):
                y = torch.empty((n, nev), dtype=torch.float64, device="cuda")
                bd = torch.ones((n, block), dtype=torch.float64, device="cuda")
                xd = torch.empty_like(bd)
                device.nd_factor_eigsh(f, A, nev, block=block, out=y, m=M)  # builds S (S_M), warms the temporaries
                device.nd_factor_solve_refined(f, A, bd, out=xd)
                t_eig, t_ref, st = [], [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    lam, _, info = device.nd_factor_eigsh(f, A, nev, block=block, out=y, m=M)
                    t_eig.append(time.perf_counter() - t0)
                    st.append(_lib.stage_times())
                    for _ in range(3):
                        t0 = time.perf_counter()
                        device.nd_factor_solve_refined(f, A, bd, out=xd)
                        t_ref.append(time.perf_counter() - t0)
                stage = lambda k: round(float(np.median([s_.get(k, 0.0) for s_ in st])), 4)  # noqa: E731
                stages = {k: stage(k) for k in ("eig_solve", "eig_reorth", "eig_qr", "eig_ritz", "eig_resid")}
                if M is not None:
                    stages["eig_mass"] = stage("eig_mass")
                reorth_bytes = 4.0 * n * info.ncv_used * 8
                case = out["cases"][f"{np.dtype(fdt).name}_factor_block{block}"] = {
                    "steps": info.steps, "ncv_used": info.ncv_used, "converged": int(info.converged.sum()),
                    "exhausted": info.exhausted, "inexact": info.inexact, "tol": info.tol, "eigsh_ms": med(t_eig),
                    "eigsh_ms_min_max": [round(1e3 * min(t_eig), 3), round(1e3 * max(t_eig), 3)],
                    "last_step_stages_ms": stages,
                    "refined_solve_block_cols_ms": med(t_ref),
                    "solve_share": round(info.steps * float(np.median(t_ref)) / float(np.median(t_eig)), 3),
                    "reorth_GBs": round(reorth_bytes / (stages["eig_reorth"] * 1e-3) / 1e9, 1)
                    if stages["eig_reorth"] > 0 else None,
                    "resid": [float(r) for r in info.resid],
                    "lam_err_vs_analytic": [float(e) for e in np.abs(lam - exact)] if mass != "lumped" else None,
                }
                if M is not None:
                    mass_bytes = 12.0 * m_nnz + 8.0 * n + 2.0 * n * block * 8
                    case["mass_GBs"] = round(mass_bytes / (stages["eig_mass"] / 3 * 1e-3) / 1e9, 1) \
                        if stages["eig_mass"] > 0 else None
                    case["lam"] = [float(v) for v in lam]
    return out


def nd_factor_line(A, B, args, by_value, same_handle_wall_ms, x_fused, pattern):
    """The kept factor (cholesky_nd / NdFactor) on the same system: host wall
    clock around synchronous calls. factor_ms: cholesky_nd on the warm handle
    (plan cached; the factor's own fronts allocated inside the clock);
    solve_only_ms: the median of repeated NdFactor.solve calls on ONE factor
    (host b in, host x out, as solve()); export_ms: bsm_nd_factor_export of
    both L and L^T as device handles (no download). The yardsticks from the
    same process: the fused solve by value and on the same handle. Then
    nd_factor_ops' figures."""
    import ctypes

    from basic_sparse_matrix_amd import cholesky_nd

    reps = max(args.reps, 1)
    t_factor = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f = cholesky_nd(A)
        t_factor.append(time.perf_counter() - t0)
        f.close()
    f = cholesky_nd(A)
    f.solve(B)  # warm-up: the solves' temporaries
    t_solve, st = [], []
    for _ in range(max(5 * reps, 10)):
        t0 = time.perf_counter()
        xf = f.solve(B).get_col(0)
        t_solve.append(time.perf_counter() - t0)
        st.append(_lib.stage_times())
    lib = _lib.require_device()
    t_exp, t_ls = [], []
    for _ in range(reps + 1):  # the first one warms the export's temporaries
        l, ls = ctypes.c_void_p(), ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.check(lib.bsm_nd_factor_export(f.handle, ctypes.byref(l), ctypes.byref(ls)))
        t_exp.append(time.perf_counter() - t0)
        lib.bsm_csr_free(l)
        lib.bsm_csr_free(ls)
        ls = ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.check(lib.bsm_nd_factor_export(f.handle, None, ctypes.byref(ls)))
        t_ls.append(time.perf_counter() - t0)
        lib.bsm_csr_free(ls)
    med = lambda t: round(1e3 * float(np.median(t)), 3)  # noqa: E731
    out = {
        "metric": "C5 nd factor object: factor once, solve many, export L (host wall ms around synchronous calls)",
        "config": {"order": "nd", "dtype": args.dtype, "g": args.g, "rhs": 1},
        "factor_ms": med(t_factor),
        "factor_ms_min_max": [round(1e3 * min(t_factor), 3), round(1e3 * max(t_factor), 3)],
        "solve_only_ms": med(t_solve),
        "solve_only_ms_min_max": [round(1e3 * min(t_solve), 3), round(1e3 * max(t_solve), 3)],
        "solve_only_calls": len(t_solve),
        "solve_only_stages_ms": {k: round(float(np.mean([s[k] for s in st])), 3) for k in st[-1]},
        "export_ms": med(t_exp[1:]),
        "export_l_star_only_ms": med(t_ls[1:]),
        "nnz_l": f.nnz_l,
        "factor_nbytes": f.nbytes,
        "fused_solve_by_value_call_ms": by_value["solve_call_ms"] if by_value else None,
        "fused_solve_same_handle_wall_ms": same_handle_wall_ms,
        "rel_dev_vs_fused_solve": float(np.linalg.norm(np.asarray(xf, np.float64) - np.asarray(x_fused, np.float64))
                                        / np.linalg.norm(np.asarray(x_fused, np.float64))),
    }
    out.update(nd_factor_ops(f, A, B, reps, pattern, args.kernel_stats))
    f64_nbytes = f.nbytes
    f.close()
    if args.dtype == "f64":  # the mixed-precision path: an f32 factor of this matrix, refined
        out.update(nd_refine_ops(A, B, reps, f64_nbytes))
    return out


if __name__ == "__main__":
    main()

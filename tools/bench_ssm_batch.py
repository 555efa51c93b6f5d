"""Many small filters in one call (wsmc_ssm_run_batch) against the same filters run one after
another (wsmc_ssm_run on fresh contexts): wsmc.models.sv at n = 1000, forced resampling, T = 1e4,
the filters a grid over phi with their own seeds.

    python tools/bench_ssm_batch.py                     the driver: baseline, then every B
    python tools/bench_ssm_batch.py --leg batch --B 64  one measurement in this process (one JSON line)
    python tools/bench_ssm_batch.py --leg baseline

The driver starts one child process per measurement, each under its own `timeout`; a child that
fails, or runs into its limit, ends the driver: nothing more is started on the device.

  baseline  16 Context.ssm_run calls, one after another, on 16 fresh contexts of one process (the
            contexts made before the clock starts); a warm-up round, then the best of 3. This is
            what a user has without the batch; B filters cost B / 16 of it.
  batch     Context.ssm_run_batch of B filters, B in {1, 16, 64, CUs, 4 CUs, 1024}; a warm-up call,
            then the best of 3. Filter 0's evidence is checked against the baseline's first run.

  --trace   (with --leg batch) the same call untraced and with the per-step trace
            (wsmc_ssm_run_batch_traced) in one process: seconds of both, the trace's share of the
            traced call, and the device memory the trace takes, B T (2 S + 2) 8 bytes. Lines go to
            profiles/ssm_trace.jsonl.

  --smooth  (with --leg batch) the same call untraced and smoothed, asking for the moments only
            (wsmc_ssm_run_batch_smoothed), alternating in one process, T = 1e3 by default: seconds of
            both, the device times of the trace-back's two kernels and the bytes of the log. Lines go
            to profiles/ssm_smooth.jsonl.

`ratio` is batch seconds over the baseline scaled to B; the bar is ratio < 1/16 at B = CU count
(16 is the number of processes that may hold the device at once: the only other way to fill it).
One JSON line per child, appended to profiles/ssm_batch.jsonl (--out). Diagnostics for DESIGN.md
§4; bench.py stays the headline."""
import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "weightedsampling.jl_amd"), str(ROOT / "oracle"), str(ROOT)]

N = 1000
NBASE = 16
OUT = ROOT / "profiles" / "ssm_batch.jsonl"


def filters(B):
    """B sv specs over a grid of phi, and their seeds"""
    from wsmc import models
    phis = [0.90 + 0.09 * k / max(1, B - 1) for k in range(B)]
    return [models.sv(phi=p) for p in phis], [1000 + k for k in range(B)]


def baseline(T: int) -> dict:
    import wsmc
    from wsmc import models
    data = models.sv_data(T)
    specs, seeds = filters(NBASE)
    best, ev0 = float("inf"), None
    for rep in range(4):   # the first round warms up
        ctxs = [wsmc.Context(N, seed=s) for s in seeds]
        for c in ctxs:
            c.sync()
        t0 = time.perf_counter()
        evs = [c.ssm_run(sp, data, ess_perc_min=1.0) for c, sp in zip(ctxs, specs)]
        dt = time.perf_counter() - t0
        assert all(c.ssm_stats()["persistent_runs"] == 1 for c in ctxs)
        for c in ctxs:
            c.close()
        ev0 = evs[0]
        if rep > 0:
            best = min(best, dt)
    return {"leg": "baseline", "n": N, "T": T, "runs": NBASE, "seconds": best, "seconds_per_filter": best / NBASE,
            "filter_steps_per_s": NBASE * T / best, "log_evidence_0": ev0}


def batch_traced(T: int, B: int) -> dict:
    import wsmc
    from wsmc import models
    data = models.sv_data(T)
    specs, seeds = filters(B)
    ctx = wsmc.Context(1, seed=1)
    best = {False: float("inf"), True: float("inf")}
    res = {}
    for rep in range(3):   # the first round warms up; then the best of 2, the two calls alternating
        for trace in (False, True):
            t0 = time.perf_counter()
            res[trace] = ctx.ssm_run_batch(specs, data, N, seeds, ess_perc_min=1.0, trace=trace)
            dt = time.perf_counter() - t0
            if rep > 0:
                best[trace] = min(best[trace], dt)
    st = ctx.ssm_batch_stats()
    assert (res[True].log_evidence == res[False].log_evidence).all()
    assert (res[True].log_evidence_trace[:, -1] == res[True].log_evidence).all()   # sv's last statement is the OBSERVE
    ctx.close()
    S = len(specs[0].cols)
    return {"leg": "batch_traced", "n": N, "T": T, "B": B, "untraced_s": best[False], "traced_s": best[True],
            "trace_share": (best[True] - best[False]) / best[True], "trace_device_bytes": B * T * (2 * S + 2) * 8,
            "blocks_per_cu": st["blocks_per_cu"], "cus": st["cus"], "segments": st["segments"]}


def batch_smoothed(T: int, B: int) -> dict:
    import statistics
    import wsmc
    from wsmc import models
    data = models.sv_data(T)
    specs, seeds = filters(B)
    ctx = wsmc.Context(1, seed=1)
    times = {False: [], True: []}
    res = {}
    for rep in range(8):   # the first round warms up; then the median of 7, the two calls alternating
        for smooth in (False, True):
            t0 = time.perf_counter()
            res[smooth] = ctx.ssm_run_batch(specs, data, N, seeds, ess_perc_min=1.0, smooth=("mean", "var") if smooth else False)
            dt = time.perf_counter() - t0
            if rep > 0:
                times[smooth].append(dt)
    st, sm = ctx.ssm_batch_stats(), ctx.ssm_smooth_stats()
    assert (res[True].log_evidence == res[False].log_evidence).all() and (res[True].n_resamples == T).all()
    assert res[True].smean["h"].shape == (B, T) and res[True].paths is None
    ctx.close()
    u, s = statistics.median(times[False]), statistics.median(times[True])
    return {"leg": "batch_smoothed", "n": N, "T": T, "B": B, "untraced_s": u, "untraced_s_range": [min(times[False]), max(times[False])],
            "smoothed_moments_s": s, "smoothed_moments_s_range": [min(times[True]), max(times[True])],
            "filter_steps_per_s": B * T / s,
            "segments_device_s": sm["segments_s"], "traceback_device_s": sm["traceback_s"], "rows_device_s": sm["rows_s"],
            "traceback_ns_per_step_particle": 1e9 * (sm["traceback_s"] + sm["rows_s"]) / (B * T * N), "log_bytes": sm["log_bytes"],
            "blocks_per_cu": st["blocks_per_cu"], "cus": st["cus"], "segments": st["segments"]}


def batch(T: int, B: int, per_filter_s: float, ev0) -> dict:
    import wsmc
    from wsmc import models
    data = models.sv_data(T)
    specs, seeds = filters(B)
    if B != NBASE:   # filter 0 as the baseline's: phi = 0.90, seed 1000
        assert specs[0].same_shape(filters(NBASE)[0][0])
    ctx = wsmc.Context(1, seed=1)
    best, res, st = float("inf"), None, None
    for rep in range(4):
        t0 = time.perf_counter()
        res = ctx.ssm_run_batch(specs, data, N, seeds, ess_perc_min=1.0)
        dt = time.perf_counter() - t0
        if rep > 0 and dt < best:
            best, st = dt, ctx.ssm_batch_stats()
    assert (res.n_resamples == T).all()
    if ev0 is not None:
        assert float(res.log_evidence[0]) == ev0, (float(res.log_evidence[0]), ev0)
    ctx.close()
    out = {"leg": "batch", "n": N, "T": T, "B": B, "seconds": best, "filter_steps_per_s": B * T / best,
           "blocks_per_cu": st["blocks_per_cu"], "cus": st["cus"], "segments": st["segments"],
           "rounds": -(-B // (st["blocks_per_cu"] * st["cus"]))}
    if per_filter_s:
        out.update(baseline_scaled_s=per_filter_s * B, ratio=best / (per_filter_s * B), speedup=per_filter_s * B / best)
    return out


def probe() -> dict:
    import wsmc
    ctx = wsmc.Context(1, seed=1)
    st = ctx.ssm_batch_stats()
    ctx.close()
    return {"leg": "probe", "cus": st["cus"]}


def driver(T: int, out: pathlib.Path) -> int:
    out.parent.mkdir(exist_ok=True)

    def child(args, limit):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__, "--T", str(T)] + args
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{args}: exit {r.returncode} (limit {limit} s)\n{r.stdout}\n{r.stderr}", flush=True)
            return None   # nothing more is started on the device
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        return line, json.loads(line)

    p = child(["--leg", "probe"], 60)
    if p is None:
        return 1
    cus = p[1]["cus"]
    b = child(["--leg", "baseline"], 180)
    if b is None:
        return 1
    with open(out, "a") as f:
        f.write(b[0] + "\n")
    per, ev0 = b[1]["seconds_per_filter"], b[1]["log_evidence_0"]
    for B in sorted({1, 16, 64, cus, 4 * cus, 1024}):
        # a round of resident filters takes about one single run; four calls, and the host's share
        limit = int(60 + 8 * per * max(1, B // cus + 1) * 4)
        r = child(["--leg", "batch", "--B", str(B), "--per-filter", repr(per), "--ev0", repr(ev0)], limit)
        if r is None:
            return 1
        with open(out, "a") as f:
            f.write(r[0] + "\n")
        if B == cus:
            ok = r[1]["ratio"] < 1.0 / 16
            print(f"bar at B = CUs = {cus}: ratio {r[1]['ratio']:.4f} {'<' if ok else '>='} 1/16", flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["probe", "baseline", "batch"])
    ap.add_argument("--T", type=int, default=10_000)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--per-filter", type=float, default=0.0)
    ap.add_argument("--ev0", type=float, default=None)
    ap.add_argument("--out", type=pathlib.Path, default=OUT)
    ap.add_argument("--trace", action="store_true", help="with --leg batch: untraced against traced")
    ap.add_argument("--smooth", action="store_true", help="with --leg batch: untraced against smoothed (moments only)")
    a = ap.parse_args()
    if a.leg == "probe":
        print(json.dumps(probe()), flush=True)
    elif a.leg == "baseline":
        print(json.dumps(baseline(a.T)), flush=True)
    elif a.leg == "batch" and a.smooth:
        print(json.dumps(batch_smoothed(a.T, a.B)), flush=True)
    elif a.leg == "batch" and a.trace:
        print(json.dumps(batch_traced(a.T, a.B)), flush=True)
    elif a.leg == "batch":
        print(json.dumps(batch(a.T, a.B, a.per_filter, a.ev0)), flush=True)
    else:
        sys.exit(driver(a.T, a.out))

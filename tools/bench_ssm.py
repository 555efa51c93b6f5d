"""The fused run of a specified scalar SSM (wsmc_ssm_run) against the statement route of the same
tree, at N = 1000 with forced resampling: the four models of wsmc.models.SSM_MODELS, and the LGSSM
spec on the generic kernel against wsmc_lgssm1d_run on the hard-coded one.

    python tools/bench_ssm.py                  every model at T = 1e3, 1e4, 1e5 (the driver)
    python tools/bench_ssm.py --leg sv --T 10000    one measurement in this process (one JSON line)

The driver starts one child process per (model, T), each under its own `timeout`: the T = 1e3 run
comes first and sizes the limits of the longer ones. A child that fails, or runs into its limit,
ends the driver: nothing more is started on the device. Each child times, in one process, after a
warm-up run, the best of 2:

  persistent     Context.ssm_run (the persistent workgroup)
  statements     spec.statements on a Context, the Resamples asynchronous (the Python loop over
                 the operators: what a user's own loop costs)
  statements_lib Context.ssm_run with a foreign column present, which sends the same spec through
                 the statement loop inside the library (no Python between the statements)
  lgssm leg only lgssm1d_run (k_lgssm_segment) beside ssm_run of the LGSSM spec (k_ssm_segment)

One JSON line per child, appended to profiles/ssm_fused.jsonl. Diagnostics for DESIGN.md §4;
bench.py stays the headline.

    python tools/bench_ssm.py --trace                    every model at T = 1e4, 1e5
    python tools/bench_ssm.py --trace --leg sv --T 10000

The trace leg (wsmc_ssm_run_traced): the persistent run untraced, traced, and the only other way to
the same rows, spec.statements(ctx, data, trace=True), which waits at every step. Same protocol
(the statements' warm-up is at most 1000 steps long); lines go to profiles/ssm_trace.jsonl.

    python tools/bench_ssm.py --smooth                   sv and lgssm at T = 1e3, 1e4
    python tools/bench_ssm.py --smooth --leg sv --T 1000

The smooth leg (wsmc_ssm_run_smoothed), forced resampling: the persistent run untraced, smoothed
asking for the moments only, smoothed asking for moments and paths, and at T = 1e3 (T n_cols must
stay under the store's 4096 columns) the only other way to the same rows, spec.statements(ctx, data,
smooth=True) on a Context with the lazy store. The routes alternate inside a round; a round runs
each route on fresh contexts (made before the clock starts) as often as fills half a second; the
figure is the median over three rounds after a warm-up round, with the rounds' range beside it.
The device times of the trace-back's two kernels are the library's own (HIP events,
Context.ssm_smooth_stats). Lines go to profiles/ssm_smooth.jsonl.

    python tools/bench_ssm.py --guided                   lgssm1d_guided at T = 1e3, 1e4, 1e5
    python tools/bench_ssm.py --guided --T 10000

The guided leg (an importance Sample a step: the guided kernels), forced resampling, the smooth
leg's protocol (alternating routes, rounds of half a second, the median of three rounds after a
warm-up round with their range): models.lgssm1d_guided() through Context.ssm_run, through
spec.statements on a Context (asynchronous Resamples) and through the library's statement loop
(a foreign column present), and models.lgssm1d_spec() through Context.ssm_run for scale (the
bootstrap filter of the same model on the unguided kernel). Lines go to profiles/ssm_guided.jsonl.

    python tools/bench_ssm.py --backward                 lgssm and sv at T = 1e3, M = 64 and 1024
    python tools/bench_ssm.py --backward --leg sv --T 1000 --M 64

The backward leg (wsmc_ssm_run_backward), forced resampling, the smooth leg's protocol: the
persistent run untraced, the run with M backward-simulated trajectories (the whole call), the
smoothed run with paths for context, and on the same box a vectorised numpy FFBS of the same
sizes over the run's own record (the baseline: float64 numpy, its own random stream, not
bit-compared). The backward kernel's and the rows kernel's device times are the library's own (HIP
events, Context.ssm_backward_stats). Lines go to profiles/ssm_backward.jsonl.

    python tools/bench_ssm.py --conditional              lgssm and sv at T = 1e3, B = 1 and 256
    python tools/bench_ssm.py --conditional --leg sv --T 1000 --B 256

The conditional leg (wsmc_ssm_run_conditional), forced resampling, N = 1e3: one particle-Gibbs
sweep, the conditional batch with one backward trajectory a filter, beside ssm_run_batch(backward=1)
of the same shape (the yardstick: the same kernels but for the pin and the Resample's ancestors),
alternated over rounds on one context; at B = 1 also the same sweep through
SSM.conditional_definition and SSM.backward_definition on Contexts (the operators, with their
downloads and uploads at every Resample), once. Lines go to profiles/ssm_conditional.jsonl."""
import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "weightedsampling.jl_amd"), str(ROOT / "oracle"), str(ROOT)]

N = 1000
LEGS = ["sv", "poisson_count", "kitagawa", "local_trend", "lgssm"]
OUT = ROOT / "profiles" / "ssm_fused.jsonl"
OUT_TRACE = ROOT / "profiles" / "ssm_trace.jsonl"
OUT_SMOOTH = ROOT / "profiles" / "ssm_smooth.jsonl"
OUT_GUIDED = ROOT / "profiles" / "ssm_guided.jsonl"
OUT_BACKWARD = ROOT / "profiles" / "ssm_backward.jsonl"
OUT_CONDITIONAL = ROOT / "profiles" / "ssm_conditional.jsonl"


def best_of(run, reps=2):
    """run() -> (seconds, extra) on a fresh context; a warm-up first, then the best of `reps`"""
    best, extra = float("inf"), None
    for k in range(reps + 1):
        dt, ex = run()
        if k > 0 and dt < best:
            best, extra = dt, ex
    return best, extra


def child(leg: str, T: int) -> dict:
    import wsmc
    from wsmc import models
    if leg == "lgssm":
        spec, data = models.lgssm1d_spec(), models.lgssm1d_data(T)
    else:
        make, gen = models.SSM_MODELS[leg]
        spec, data = make(), gen(T)
    spec.check()

    def persistent():
        ctx = wsmc.Context(N, seed=42)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.ssm_run(spec, data, ess_perc_min=1.0, want_evidence=False)
        dt = time.perf_counter() - t0
        st = ctx.ssm_stats()
        assert st["persistent_runs"] == 1, st
        ex = {"log_evidence": ctx.log_evidence(), "resamples": ctx.get_state()["n_resamples"],
              "host_bookkeeping_s": st["bookkeeping_s"], "host_call_s": st["call_s"], "segments": st["segments"]}
        ctx.close()
        return dt, ex

    def statements():
        ctx = wsmc.Context(N, seed=42)
        ctx.sync()
        t0 = time.perf_counter()
        spec.statements(ctx, data, ess_perc_min=1.0, wait=False)
        ctx.sync()
        dt = time.perf_counter() - t0
        ex = {"log_evidence": ctx.log_evidence(), "resamples": ctx.get_state()["n_resamples"]}
        ctx.close()
        return dt, ex

    def statements_lib():
        ctx = wsmc.Context(N, seed=42)
        ctx.assign(ctx.col_create("_other", 1), models._const([0.0]))   # a foreign column: the statement route
        ctx.sync()
        t0 = time.perf_counter()
        ctx.ssm_run(spec, data, ess_perc_min=1.0, want_evidence=False)
        dt = time.perf_counter() - t0
        assert ctx.ssm_stats()["statement_runs"] == 1
        ex = {"log_evidence": ctx.log_evidence(), "resamples": ctx.get_state()["n_resamples"]}
        ctx.close()
        return dt, ex

    def lgssm_kernel():
        ctx = wsmc.Context(N, seed=42)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.lgssm1d_run(data, ess_perc_min=1.0, want_evidence=False)
        dt = time.perf_counter() - t0
        assert ctx.lgssm_stats()["persistent_runs"] == 1
        ex = {"log_evidence": ctx.log_evidence(), "resamples": ctx.get_state()["n_resamples"]}
        ctx.close()
        return dt, ex

    p, pe = best_of(persistent)
    s, se = best_of(statements)
    sl, sle = best_of(statements_lib)
    # the three routes compute the same thing
    assert pe["log_evidence"] == se["log_evidence"] == sle["log_evidence"], (pe, se, sle)
    assert pe["resamples"] == se["resamples"] == sle["resamples"] == T
    out = {"leg": leg, "N": N, "T": T, "columns": len(spec.cols), "step_statements": spec.spec.n_step,
           "persistent_s": p, "persistent_us_per_step": 1e6 * p / T,
           "statements_s": s, "statements_us_per_step": 1e6 * s / T,
           "statements_lib_s": sl, "statements_lib_us_per_step": 1e6 * sl / T,
           "factor_vs_statements": s / p, "factor_vs_statements_lib": sl / p,
           "host_bookkeeping_s": pe["host_bookkeeping_s"], "host_call_s": pe["host_call_s"], "segments": pe["segments"],
           "log_evidence": pe["log_evidence"]}
    if leg == "lgssm":
        k, ke = best_of(lgssm_kernel)
        assert ke["log_evidence"] == pe["log_evidence"]
        out.update(lgssm1d_run_s=k, lgssm1d_run_us_per_step=1e6 * k / T, generic_over_hard_coded=p / k)
    return out


def child_trace(leg: str, T: int) -> dict:
    import numpy as np
    import wsmc
    from wsmc import models
    if leg == "lgssm":
        spec, data = models.lgssm1d_spec(), models.lgssm1d_data(T)
    else:
        make, gen = models.SSM_MODELS[leg]
        spec, data = make(), gen(T)

    def persistent(trace):
        def run():
            ctx = wsmc.Context(N, seed=42)
            ctx.sync()
            t0 = time.perf_counter()
            r = ctx.ssm_run(spec, data, ess_perc_min=1.0, trace=trace)
            dt = time.perf_counter() - t0
            assert ctx.ssm_stats()["persistent_runs"] == 1
            ctx.close()
            return dt, r
        return run

    first = [True]

    def statements():
        steps = min(T, 1000) if first[0] else T   # the warm-up
        first[0] = False
        ctx = wsmc.Context(N, seed=42)
        ctx.sync()
        t0 = time.perf_counter()
        _, _, tr = spec.statements(ctx, data[:steps], ess_perc_min=1.0, trace=True)
        dt = time.perf_counter() - t0
        ctx.close()
        return dt, tr

    u, ev = best_of(persistent(False))
    p, (ev_t, tr) = best_of(persistent(True))
    s, want = best_of(statements)
    same = lambda a, b: bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    assert ev == ev_t and same(tr.ess, want.ess) and same(tr.log_evidence, want.log_evidence)
    assert all(same(tr.mean[c], want.mean[c]) and same(tr.var[c], want.var[c]) for c in spec.cols)
    return {"leg": leg, "N": N, "T": T, "columns": len(spec.cols), "step_statements": spec.spec.n_step,
            "untraced_s": u, "untraced_us_per_step": 1e6 * u / T, "traced_s": p, "traced_us_per_step": 1e6 * p / T,
            "trace_us_per_step": 1e6 * (p - u) / T, "statements_traced_s": s, "statements_traced_us_per_step": 1e6 * s / T,
            "factor_vs_statements_traced": s / p, "log_evidence": ev}


def child_smooth(leg: str, T: int) -> dict:
    import statistics
    import numpy as np
    import wsmc
    from wsmc import models
    if leg == "lgssm":
        spec, data = models.lgssm1d_spec(), models.lgssm1d_data(T)
    else:
        make, gen = models.SSM_MODELS[leg]
        spec, data = make(), gen(T)
    S = len(spec.cols)
    last = {}

    def fused(smooth):
        def run(ctx):
            r = ctx.ssm_run(spec, data, ess_perc_min=1.0, smooth=smooth)
            assert ctx.ssm_stats()["persistent_runs"] == 1
            if smooth:
                last[smooth if smooth is True else "moments"] = (r, ctx.ssm_smooth_stats())
            else:
                last["untraced"] = (r, None)
        return run

    def statements(ctx):
        ctx.store_set_lazy(True)
        r = spec.statements(ctx, data, ess_perc_min=1.0, smooth=True)
        last["statements"] = ((ctx.log_evidence(), r[2]), None)

    routes = {"untraced": fused(False), "moments": fused(("mean", "var")), "paths": fused(True)}
    if T * S + S <= 4096:
        routes["statements"] = statements
    times = {k: [] for k in routes}
    reps = {k: 1 for k in routes}
    for rnd in range(5):   # round 0 warms up, round 1 sizes the windows, rounds 2..4 are the figures
        for name, run in routes.items():
            ctxs = [wsmc.Context(N, seed=42) for _ in range(reps[name])]
            for c in ctxs:
                c.sync()
            t0 = time.perf_counter()
            for c in ctxs:
                run(c)
            dt = (time.perf_counter() - t0) / len(ctxs)
            for c in ctxs:
                c.close()
            if rnd == 1:
                reps[name] = max(1, min(64, int(0.5 / dt) + 1))
            if rnd >= 2:
                times[name].append(dt)
    last["paths"] = last.pop(True)
    med = {k: statistics.median(v) for k, v in times.items()}
    same = lambda a, b: bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    (ev_p, sm_p), st_p = last["paths"]
    (ev_m, sm_m), st_m = last["moments"]
    assert last["untraced"][0] == ev_p == ev_m
    assert all(same(sm_p.mean[c], sm_m.mean[c]) and same(sm_p.var[c], sm_m.var[c]) for c in spec.cols)
    out = {"leg": leg, "N": N, "T": T, "columns": S, "step_statements": spec.spec.n_step, "runs_per_round": reps,
           "log_evidence": ev_p, "log_bytes": st_p["log_bytes"]}
    for k in routes:
        out[f"{k}_s"] = med[k]
        out[f"{k}_s_range"] = [min(times[k]), max(times[k])]
        out[f"{k}_us_per_step"] = 1e6 * med[k] / T
    tb = st_m["traceback_s"] + st_m["rows_s"]
    out.update(segments_device_s=st_m["segments_s"], traceback_device_s=st_m["traceback_s"], rows_device_s=st_m["rows_s"],
               rows_with_paths_device_s=st_p["rows_s"],
               # (a) what the smoothed call adds to a step beyond the two trace-back kernels: the recording
               # stores, the traced instantiation, the allocation and the flags' memset
               recording_us_per_step=1e6 * (med["moments"] - med["untraced"] - tb) / T,
               recording_device_us_per_step=1e6 * (st_m["segments_s"] - med["untraced"]) / T,
               # (b) the trace-back's device time per step and particle, both kernels
               traceback_ns_per_step_particle=1e9 * tb / (T * N),
               smoothing_share_of_moments_call=(med["moments"] - med["untraced"]) / med["moments"])
    if "statements" in routes:
        (ev_s, sm_s), _ = last["statements"]
        assert ev_s == ev_p
        assert all(same(sm_p.mean[c], sm_s.mean[c]) and same(sm_p.var[c], sm_s.var[c]) and same(sm_p.paths[c], sm_s.paths[c])
                   for c in spec.cols)
        # (c) the speed-up over the only alternative
        out.update(factor_vs_statements_moments=med["statements"] / med["moments"],
                   factor_vs_statements_paths=med["statements"] / med["paths"])
    return out


def child_guided(T: int) -> dict:
    import statistics
    import wsmc
    from wsmc import models
    guided, boot, data = models.lgssm1d_guided(), models.lgssm1d_spec(), models.lgssm1d_data(T)
    guided.check()
    last = {}

    def fused(spec, name):
        def run(ctx):
            ctx.ssm_run(spec, data, ess_perc_min=1.0, want_evidence=False)
            assert ctx.ssm_stats()["persistent_runs"] == 1
            last[name] = (ctx.log_evidence(), ctx.get_state()["n_resamples"])
        return run

    def statements(ctx):
        guided.statements(ctx, data, ess_perc_min=1.0, wait=False)
        ctx.sync()
        last["guided_statements"] = (ctx.log_evidence(), ctx.get_state()["n_resamples"])

    def statements_lib(ctx):
        ctx.ssm_run(guided, data, ess_perc_min=1.0, want_evidence=False)
        assert ctx.ssm_stats()["statement_runs"] == 1
        last["guided_statements_lib"] = (ctx.log_evidence(), ctx.get_state()["n_resamples"])

    routes = {"guided_persistent": fused(guided, "guided_persistent"), "guided_statements": statements,
              "guided_statements_lib": statements_lib, "lgssm_persistent": fused(boot, "lgssm_persistent")}
    times = {k: [] for k in routes}
    reps = {k: 1 for k in routes}
    for rnd in range(5):   # round 0 warms up, round 1 sizes the windows, rounds 2..4 are the figures
        for name, run in routes.items():
            ctxs = [wsmc.Context(N, seed=42) for _ in range(reps[name])]
            for c in ctxs:
                if name == "guided_statements_lib":   # a foreign column: the statement route
                    c.assign(c.col_create("_other", 1), models._const([0.0]))
                c.sync()
            t0 = time.perf_counter()
            for c in ctxs:
                run(c)
            dt = (time.perf_counter() - t0) / len(ctxs)
            for c in ctxs:
                c.close()
            if rnd == 1:
                reps[name] = max(1, min(64, int(0.5 / dt) + 1))
            if rnd >= 2:
                times[name].append(dt)
    # the three guided routes compute the same thing; every Resample after an OBSERVE ran
    assert last["guided_persistent"] == last["guided_statements"] == last["guided_statements_lib"], last
    assert last["guided_persistent"][1] >= T and last["lgssm_persistent"][1] == T, last
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"leg": "lgssm1d_guided", "N": N, "T": T, "columns": len(guided.cols), "step_statements": guided.spec.n_step,
           "runs_per_round": reps, "log_evidence": last["guided_persistent"][0], "resamples": last["guided_persistent"][1],
           "lgssm_log_evidence": last["lgssm_persistent"][0]}
    for k in routes:
        out[f"{k}_s"] = med[k]
        out[f"{k}_s_range"] = [min(times[k]), max(times[k])]
        out[f"{k}_us_per_step"] = 1e6 * med[k] / T
    out.update(factor_vs_statements=med["guided_statements"] / med["guided_persistent"],
               factor_vs_statements_lib=med["guided_statements_lib"] / med["guided_persistent"],
               guided_over_lgssm=med["guided_persistent"] / med["lgssm_persistent"])
    return out


def numpy_ffbs(leg, rec, M, rng):
    """forward filtering, backward simulation over a record, vectorised over the M trajectories: the
    transition density of lgssm1d_spec / sv at their default parameters, the categorical draws by a
    cumulative sum and a search. Returns idx [T, M]"""
    import numpy as np
    a, b, sd = (0.9, 0.0, 1.0) if leg == "lgssm" else (0.95, -1.0 * (1.0 - 0.95), 0.25)
    x, lw = rec.cols[:, 0, :], rec.log_weights
    T, n = lw.shape

    def draw(logw):   # [M, n] -> [M]
        w = np.exp(logw - logw.max(axis=1, keepdims=True))
        c = np.cumsum(w, axis=1)
        u = rng.random(len(c)) * c[:, -1]
        return np.minimum((c <= u[:, None]).sum(axis=1), n - 1)

    idx = np.empty((T, M), dtype=np.int64)
    idx[T - 1] = draw(np.broadcast_to(lw[T - 1], (M, n)))
    for t in range(T - 2, -1, -1):
        z = x[t + 1][idx[t + 1]]
        r = (z[:, None] - (a * x[t][None, :] + b)) / sd
        idx[t] = draw(lw[t][None, :] - 0.5 * r * r)
    return idx


def child_backward(leg: str, T: int, M: int) -> dict:
    import statistics
    import numpy as np
    import wsmc
    from wsmc import models
    spec, data = (models.lgssm1d_spec(), models.lgssm1d_data(T)) if leg == "lgssm" else (models.sv(), models.sv_data(T))
    spec.check()
    last = {}

    def untraced(ctx):
        last["untraced"] = ctx.ssm_run(spec, data, ess_perc_min=1.0)

    def backward(ctx):
        last["backward"] = ctx.ssm_run(spec, data, ess_perc_min=1.0, backward=M, backward_seed=7), ctx.ssm_backward_stats()

    def smoothed(ctx):
        last["smoothed"] = ctx.ssm_run(spec, data, ess_perc_min=1.0, smooth=True)

    routes = {"untraced": untraced, "backward": backward, "smoothed": smoothed}
    times = {k: [] for k in routes}
    reps = {k: 1 for k in routes}
    for rnd in range(5):   # round 0 warms up, round 1 sizes the windows, rounds 2..4 are the figures
        for name, run in routes.items():
            ctxs = [wsmc.Context(N, seed=42) for _ in range(reps[name])]
            for c in ctxs:
                c.sync()
            t0 = time.perf_counter()
            for c in ctxs:
                run(c)
            dt = (time.perf_counter() - t0) / len(ctxs)
            for c in ctxs:
                c.close()
            if rnd == 1:
                reps[name] = max(1, min(64, int(0.5 / dt) + 1))
            if rnd >= 2:
                times[name].append(dt)
    (ev_b, bw), st = last["backward"]
    assert ev_b == last["untraced"] == last["smoothed"][0]
    g = wsmc.Context(N, seed=42)
    rec = g.ssm_run(spec, data, ess_perc_min=1.0, backward=M, backward_seed=7, record=True)[1].record
    g.close()
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    numpy_ffbs(leg, rec, M, rng)   # a warm-up, which also sizes the repetitions
    ft = []
    for _ in range(3 if time.perf_counter() - t0 < 3.0 else 1):
        t0 = time.perf_counter()
        fidx = numpy_ffbs(leg, rec, M, rng)
        ft.append(time.perf_counter() - t0)
    col = spec.cols[0]
    sm = last["smoothed"][1]
    fpaths = np.take_along_axis(rec.cols[:, 0, :], fidx, axis=1)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"leg": leg, "N": N, "T": T, "M": M, "columns": len(spec.cols), "runs_per_round": reps, "log_evidence": ev_b,
           "bytes": st["bytes"]}
    for k in routes:
        out[f"{k}_s"] = med[k]
        out[f"{k}_s_range"] = [min(times[k]), max(times[k])]
    out.update(segments_device_s=st["segments_s"], backward_device_s=st["backward_s"], rows_device_s=st["rows_s"],
               backward_ns_per_evaluation=1e9 * st["backward_s"] / (T * M * N),
               numpy_ffbs_s=statistics.median(ft), numpy_ffbs_s_range=[min(ft), max(ft)],
               numpy_ffbs_ns_per_evaluation=1e9 * statistics.median(ft) / (T * M * N),
               numpy_over_backward_call=statistics.median(ft) / (med["backward"] - med["untraced"]),
               # the estimates' shape, for context (not a comparison of bits): distinct values in the first row, the
               # variance of the state's first-half rows
               distinct_first_row={"backward": int(len(np.unique(bw.paths[col][0]))), "genealogy": int(len(np.unique(sm.paths[col][0]))),
                                   "numpy_ffbs": int(len(np.unique(fpaths[0])))},
               mean_var_first_half={"backward": float(np.mean(bw.var[col][:T // 2])), "genealogy": float(np.mean(sm.var[col][:T // 2])),
                                    "numpy_ffbs": float(np.mean(fpaths[:T // 2].var(axis=1)))})
    return out


def child_conditional(leg: str, T: int, B: int) -> dict:
    import statistics
    import numpy as np
    import wsmc
    from wsmc import models
    spec, data = (models.lgssm1d_spec(), models.lgssm1d_data(T)) if leg == "lgssm" else (models.sv(), models.sv_data(T))
    spec.check()
    seeds, bw_seeds = wsmc.pg_seeds(42, 0, B)
    ctx = wsmc.Context(16, seed=1)
    last = {}

    def unconditional():
        last["unconditional"] = ctx.ssm_run_batch(spec, data, N, seeds, ess_perc_min=1.0, backward=1, backward_seeds=bw_seeds)
        last["unconditional_stats"] = ctx.ssm_backward_stats()

    unconditional()   # (also the first sweep: its trajectories are the reference)
    ref = np.stack([np.stack([last["unconditional"].backward[b].paths[c][:, 0] for c in spec.cols], axis=1) for b in range(B)])

    def conditional():
        last["conditional"] = ctx.ssm_run_conditional(spec, data, N, seeds, ref, ess_perc_min=1.0, backward=1, backward_seeds=bw_seeds)
        last["conditional_stats"] = ctx.ssm_conditional_stats()

    routes = {"unconditional": unconditional, "conditional": conditional}
    times = {k: [] for k in routes}
    for rnd in range(7):   # round 0 warms up, rounds 1..6 are the figures, the two routes alternating
        for name, run in routes.items():
            ctx.sync()
            t0 = time.perf_counter()
            run()
            if rnd >= 1:
                times[name].append(time.perf_counter() - t0)
    assert (last["conditional"].n_resamples == T).all() and (last["unconditional"].n_resamples == T).all()
    out = {"leg": leg, "N": N, "T": T, "B": B, "M": 1, "columns": len(spec.cols), "segments": ctx.ssm_batch_stats()["segments"]}
    for k in routes:
        out[f"{k}_s"] = statistics.median(times[k])
        out[f"{k}_s_range"] = [min(times[k]), max(times[k])]
        st = last[k + "_stats"]
        out[f"{k}_device_s"] = {"segments": st["segments_s"], "backward": st["backward_s"], "rows": st["rows_s"]}
    out["conditional_over_unconditional"] = out["conditional_s"] / out["unconditional_s"]
    out["conditional_over_unconditional_segments"] = (last["conditional_stats"]["segments_s"] /
                                                      last["unconditional_stats"]["segments_s"])
    ctx.close()
    if B == 1:   # the same sweep through the operators, once (its Resamples download and upload every column)
        def make(n, seed):
            return wsmc.Context(n, seed=seed)
        t0 = time.perf_counter()
        rec, end = spec.conditional_definition(make, data, N, int(seeds[0]), ref[0], 1.0)[-2:]
        t1 = time.perf_counter()
        bw = spec.backward_definition(make, rec, data, 1, int(bw_seeds[0]))
        t2 = time.perf_counter()
        got = last["conditional"]
        assert end.log_evidence == got.log_evidence[0] and (bw.idx == got.backward[0].idx).all()
        out.update(definition_filter_s=t1 - t0, definition_backward_s=t2 - t1,
                   definition_over_conditional=(t2 - t0) / out["conditional_s"])
    return out


def driver_conditional(Ts, legs, Bs) -> int:
    OUT_CONDITIONAL.parent.mkdir(exist_ok=True)
    for leg in legs:
        for T in Ts:
            for B in Bs:
                cmd = ["timeout", "-k", "10", "240", sys.executable, __file__, "--conditional", "--leg", leg, "--T", str(T), "--B", str(B)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    print(f"{leg} T={T} B={B}: exit {r.returncode}\n{r.stdout}\n{r.stderr}", flush=True)
                    return 1   # nothing more is started on the device
                line = r.stdout.strip().splitlines()[-1]
                json.loads(line)
                with open(OUT_CONDITIONAL, "a") as f:
                    f.write(line + "\n")
                print(line, flush=True)
    return 0


def driver_backward(Ts, legs, Ms) -> int:
    OUT_BACKWARD.parent.mkdir(exist_ok=True)
    for leg in legs:
        for T in Ts:
            for M in Ms:
                cmd = ["timeout", "-k", "10", "240", sys.executable, __file__, "--backward", "--leg", leg, "--T", str(T), "--M", str(M)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    print(f"{leg} T={T} M={M}: exit {r.returncode}\n{r.stdout}\n{r.stderr}", flush=True)
                    return 1   # nothing more is started on the device
                line = r.stdout.strip().splitlines()[-1]
                json.loads(line)
                with open(OUT_BACKWARD, "a") as f:
                    f.write(line + "\n")
                print(line, flush=True)
    return 0


def driver(Ts, legs, trace=False, smooth=False, guided=False) -> int:
    out = OUT_GUIDED if guided else OUT_SMOOTH if smooth else OUT_TRACE if trace else OUT
    OUT.parent.mkdir(exist_ok=True)
    for leg in legs:
        per_step = None   # seconds a step of one child (all its routes and repetitions), from the run before
        for T in Ts:
            limit = 180 if per_step is None else int(60 + 3 * per_step * T)
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__, "--T", str(T)]
            cmd += ["--guided"] if guided else ["--leg", leg]
            cmd += ["--trace"] if trace else []
            cmd += ["--smooth"] if smooth else []
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                print(f"{leg} T={T}: exit {r.returncode} (limit {limit} s)\n{r.stdout}\n{r.stderr}", flush=True)
                return 1   # nothing more is started on the device
            line = r.stdout.strip().splitlines()[-1]
            json.loads(line)
            with open(out, "a") as f:
                f.write(line + "\n")
            print(line, flush=True)
            per_step = dt / T
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--T", type=int, action="append")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--trace", action="store_true", help="the trace leg (profiles/ssm_trace.jsonl)")
    ap.add_argument("--smooth", action="store_true", help="the smooth leg (profiles/ssm_smooth.jsonl)")
    ap.add_argument("--guided", action="store_true", help="the guided leg (profiles/ssm_guided.jsonl)")
    ap.add_argument("--backward", action="store_true", help="the backward leg (profiles/ssm_backward.jsonl)")
    ap.add_argument("--M", type=int, action="append", help="the backward leg's trajectories")
    ap.add_argument("--conditional", action="store_true", help="the conditional leg (profiles/ssm_conditional.jsonl)")
    ap.add_argument("--B", type=int, action="append", help="the conditional leg's filters")
    a = ap.parse_args()
    if a.conditional and a.leg:
        print(json.dumps(child_conditional(a.leg, (a.T or [1000])[0], (a.B or [1])[0])), flush=True)
        sys.exit(0)
    if a.conditional:
        sys.exit(driver_conditional(a.T or [1000], a.legs.split(",") if a.legs != ",".join(LEGS) else ["lgssm", "sv"], a.B or [1, 256]))
    if a.backward and a.leg:
        print(json.dumps(child_backward(a.leg, (a.T or [1000])[0], (a.M or [64])[0])), flush=True)
        sys.exit(0)
    if a.backward:
        sys.exit(driver_backward(a.T or [1000], a.legs.split(",") if a.legs != ",".join(LEGS) else ["lgssm", "sv"], a.M or [64, 1024]))
    if a.guided and a.T and len(a.T) == 1:
        print(json.dumps(child_guided(a.T[0])), flush=True)
        sys.exit(0)
    if a.guided:
        sys.exit(driver(a.T or [1000, 10_000, 100_000], ["lgssm1d_guided"], guided=True))
    if a.leg:
        print(json.dumps((child_smooth if a.smooth else child_trace if a.trace else child)(a.leg, (a.T or [1000])[0])), flush=True)
        sys.exit(0)
    if a.smooth:
        sys.exit(driver(a.T or [1000, 10_000], a.legs.split(",") if a.legs != ",".join(LEGS) else ["sv", "lgssm"], smooth=True))
    if a.trace:
        sys.exit(driver(a.T or [10_000, 100_000], a.legs.split(","), trace=True))
    sys.exit(driver(a.T or [1000, 10_000, 100_000], a.legs.split(",")))

"""What the log-Gamma families cost on the device, each next to a twin that needs none of them.

    python tools/bench_families.py [--n 1000000] [--steps 100] [--inner 20] [--reps 7]

  ssm     a count state-space model through the statement operators, N particles, T steps:
              x ~ Normal(a x, sigma);  rate = exp(x)  (assign_expr);  y_t => Poisson(rate);  Resample
          and the same loop with  y_t => Normal(rate, 1)  in the same process
  draws   `steps` times N draws of Gamma(alpha, theta) at alpha = 0.5 (the boost's extra exp / log)
          and alpha = 5 against as many of Exponential(theta): what the rejection loop costs a wave

One JSON line per leg: particle-steps (or draws) per second, ms per step, and the statement-batch
kernels launched per step (wsmc_debug_jit_stats). A timed window is `inner` runs of `steps` steps
back to back on one context between two device synchronisations (about 0.1 s at the defaults: a
single run is a few milliseconds, too short to time); each leg is run once untimed (code objects,
the run-time compiled batches), then `reps` windows; the best and the median are reported.
`enqueue_ms_per_step` is the host's time to issue the window's calls, before the closing
synchronisation: where it is close to `ms_per_step` the leg is bound by the host's enqueue (the
Python and C-ABI call per statement), not by the device, and the line is a floor for the device
time, not a measurement of it. Kernel times are not measured here (that takes a profiler run).
The two sides of the ssm pair differ in their whole path, not in the observation's arithmetic
alone: a batch with a log-Gamma family runs one particle a thread and leaves the Resample
statistics to their own kernel, where the Normal twin's batch takes them itself.
Diagnostics for DESIGN.md; bench.py stays the headline.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "weightedsampling.jl_amd"), str(ROOT)]
import numpy as np  # noqa: E402
import wsmc  # noqa: E402
from wsmc import abi, dsl, models  # noqa: E402
from wsmc.dsl import Col  # noqa: E402


def ssm_data(T, a=0.9, sigma=0.3, seed=42):
    rng = np.random.Generator(np.random.Philox(seed))
    x, ys = 0.0, np.empty(T)
    for t in range(T):
        x = a * x + sigma * rng.standard_normal()
        ys[t] = rng.poisson(np.exp(x))
    return ys


def ssm(ctx, ys, family, a=0.9, sigma=0.3):
    R = models.resolver(ctx)
    cx, cr = ctx.col_create("x"), ctx.col_create("rate")
    ctx.sample(cx, wsmc.Normal(0.0, 1.0).dist(R))
    transition = wsmc.Normal(Col("x") * a, sigma).dist(R)
    prog, lens = dsl.xprogram([dsl.exp(Col("x"))], R)
    lik = (wsmc.Poisson(Col("rate")) if family == "poisson" else wsmc.Normal(Col("rate"), 1.0)).dist(R)
    for y in ys:
        ctx.sample(cx, transition)
        ctx.assign_expr(cr, prog, lens)
        ctx.observe(lik, models._const([y]))
        ctx.resample(1.0, wait=False)


def draws(ctx, kern, steps):
    """theta is read from a column on every side: a draw whose distribution reads no column stays
    in the lazy store's batch rows until something reads it, and would time nothing"""
    R = models.resolver(ctx)
    if ctx.col_find("th") < 0:   # the window's first run
        ctx.col_upload(ctx.col_create("th"), np.full(ctx.n, 2.0))
    cx = ctx.col_create("x")
    d = kern.dist(R)
    for _ in range(steps):   # consecutive Samples share statement batches (up to 6 a kernel)
        ctx.sample(cx, d)


def timed(N, reps, body, steps, inner):
    times, enq, launched = [], [], 0
    steps = steps * inner
    for r in range(reps + 1):   # the first window is the warm-up
        ctx = wsmc.Context(N, seed=42)
        ctx.sync()
        j0 = abi.jit_stats()
        t0 = time.perf_counter()
        for _ in range(inner):
            body(ctx)
        t1 = time.perf_counter()
        ctx.sync()
        dt = time.perf_counter() - t0
        j1 = abi.jit_stats()
        ev = ctx.log_evidence()
        ctx.close()
        if r > 0:
            times.append(dt)
            enq.append(t1 - t0)
            launched = (j1["launched"] + j1["interpreted"]) - (j0["launched"] + j0["interpreted"])
    best, med = min(times), statistics.median(times)
    return {"N": N, "steps": steps, "reps": reps, "window_ms": 1e3 * best, "ms_per_step": 1e3 * best / steps,
            "ms_per_step_median": 1e3 * med / steps, "enqueue_ms_per_step": 1e3 * min(enq) / steps,
            "particle_steps_per_s": N * steps / best,
            "batch_kernels_per_step": launched / steps, "log_evidence": ev}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--inner", type=int, default=20, help="runs of `steps` steps in one timed window")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if wsmc.device_count() < 1:
        sys.exit("bench_families: no HIP device")
    ys = ssm_data(a.steps)
    for fam in ("poisson", "normal"):
        r = timed(a.n, a.reps, lambda c: ssm(c, ys, fam), a.steps, a.inner)
        print(json.dumps({"leg": f"ssm, y => {'Poisson(exp x)' if fam == 'poisson' else 'Normal(exp x, 1)'}", **r}),
              flush=True)
    for name, kern in (("Gamma(0.5, 2)", wsmc.Gamma(0.5, Col("th"))), ("Gamma(5, 2)", wsmc.Gamma(5.0, Col("th"))),
                       ("Exponential(2)", wsmc.Exponential(Col("th")))):
        r = timed(a.n, a.reps, lambda c: draws(c, kern, a.steps), a.steps, a.inner)
        r.pop("log_evidence")
        print(json.dumps({"leg": f"draws, x ~ {name}", **r}), flush=True)

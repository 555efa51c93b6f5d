"""Seeded random fused 2D-SSM runs for wsmc_ssm2d_run: generator, runner, comparer, replay.

TEST INFRASTRUCTURE, the companion of tests/progfuzz.py and tests/ssmfuzz.py for the fused 2D run.
A case is plain data built from ``numpy.random.default_rng([seed, salt])`` and nothing else (no
context, no device): a population size, a store mode (keep_history), the context's seed and one or
more runs on that one context, each run (obs[T, 2], x0, v0, q_var, r_var, ess_perc_min, scheme,
want_evidence). `differential` runs a case on a fresh `wsmc.Context` through `ssm2d_run` and on a
fresh `oracle.Oracle` through `models.ssm2d_statements` (the statements issued one by one: by
include/wsmc.h the definition of the run's result) and compares everything bit for bit; a
difference is located by rerunning shorter horizons.

    python tests/ssm2dfuzz.py --seed 3 --profile mixed --drive sync --backend oracle
    python tests/ssm2dfuzz.py --name collapse_5001 --drive sync --backend hip

prints the case and runs it (`--backend hip`: against the oracle, comparing).

`predict_misses` restates, from the oracle's weights alone, at which steps the fused run's guessed
reference point (k_ssm2d_prop: R_g = wsmc_qref(base + lpmax)) is not the canonical one.
"""
from __future__ import annotations

import argparse
import functools
import math
import sys
from dataclasses import dataclass, replace

import numpy as np

import progfuzz  # noqa: F401  (puts the package and the oracle on sys.path)
from progfuzz import _where, same_value

from wsmc import abi, models  # noqa: E402

NS = (1, 2, 3, 63, 65, 1023, 1024, 1025, 2049, 5001, 16384, 16385, 17409, 70001, 262145)
LARGE_NS = NS[-2:]                        # in at most a quarter of the mixed seeds
T_MAX = 12
ESS = (0.3, 0.5, 0.9, 1.0)
MIXED_SEEDS = list(range(32))
_MIXED_N = NS * 2 + (1025, 16385)         # seed -> N: every size twice, the 32 seeds filled up
PROFILES = ("mixed", "directed")
DRIVES = ("sync", "async", "island2", "exact2")
SCHEMES = {"stratified": abi.RESAMPLE_STRATIFIED, "systematic": abi.RESAMPLE_SYSTEMATIC,
           "multinomial": abi.RESAMPLE_MULTINOMIAL}
STATE = ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples", "last_ess_perc")
STATE_NO_HISTORY = ("resampled", "n_resamples", "op_counter")   # what tests/test_gpu_parity.py compares in that mode
UNDETERMINED = 1e-9                       # |U - round(U)| or |M - round(M)| below it: either way
_SALT = 11


# ---- cases are data ---------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Run:
    obs: np.ndarray
    x0: tuple = (0.0, 0.0)
    v0: tuple = (1.0, 0.0)
    q_var: float = 0.1
    r_var: float = 0.5
    ess: float = 0.5
    scheme: int = abi.RESAMPLE_STRATIFIED
    want_evidence: bool = True

    @property
    def T(self) -> int:
        return len(self.obs)

    def kw(self) -> dict:
        """the model's arguments, as Context.ssm2d_run, models.ssm2d_statements and oracle.ssm2d_run_mt take them"""
        return dict(x0=self.x0, v0=self.v0, q_var=self.q_var, r_var=self.r_var, ess_perc_min=self.ess, scheme=self.scheme)

    def cut(self, T) -> "Run":
        return replace(self, obs=self.obs[:T])

    def text(self) -> str:
        names = {v: k for k, v in SCHEMES.items()}
        return (f"T={self.T} x0={self.x0!r} v0={self.v0!r} q_var={self.q_var!r} r_var={self.r_var!r} ess={self.ess} "
                f"{names[self.scheme]}{'' if self.want_evidence else ' no-evidence'}\n" +
                "\n".join(f"    obs[{t}] = ({o[0]!r}, {o[1]!r})" for t, o in enumerate(self.obs.tolist())))


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    N: int
    runs: tuple
    keep_history: bool = True
    ctx_seed: int = 42
    digest: bool = False        # compare the columns by digest (tests/test_gpu_configs.py), for millions of particles

    def routes(self) -> list:
        """per run "fused" or "statements" (include/wsmc.h wsmc_ssm2d_run): on a fresh context a run
        finds a column that is not its own only after a longer run with the history kept (its
        x_{T+2} ..), and then the library issues the statements itself"""
        longest, out = 0, []
        for r in self.runs:
            out.append("statements" if self.keep_history and longest > r.T else "fused")
            longest = max(longest, r.T)
        return out

    def text(self) -> str:
        return (f"{self.name}: N={self.N} keep_history={self.keep_history} seed={self.ctx_seed}\n" +
                "\n".join(f"  run {k}: {r.text()}" for k, r in enumerate(self.runs)))


# ---- the generator ----------------------------------------------------------------------------
def simulate(rng, T, x0, v0, q_var, r_var) -> np.ndarray:
    """T observations of the model itself (examples/2D_ssm.jl), drawn with the generator's rng"""
    x, v = np.array(x0, dtype=float), np.array(v0, dtype=float)
    obs = np.empty((T, 2))
    for t in range(T):
        x = x + v
        v = v + math.sqrt(q_var) * rng.standard_normal(2)
        obs[t] = x + math.sqrt(r_var) * rng.standard_normal(2)
    return obs


def _pow2(x) -> bool:
    return math.frexp(x)[0] == 0.5


# log10(r_var / q_var) by threshold. Forced runs take the whole range U(-0.5, 1.5). A gated run takes
# the part of it where its gate goes both ways within a dozen steps: drawn from the whole range, 17
# of the corpus's 26 gated runs (N >= 65, T >= 4) had both a resampled and a non-resampled step
# after the first (at 0.9 a ratio below ~8 resamples at every step, at 0.5 one below ~1.5 does, at
# 0.3 one above ~10 never does in four steps), and tests/test_ssm2d_random_runs.py asks for 80 %.
# Together the four thresholds still cover the whole range.
RATIO_LOG10 = {1.0: (-0.5, 1.5), 0.9: (0.9, 1.5), 0.5: (0.2, 1.5), 0.3: (-0.5, 1.0)}


def _variances(rng, ess=1.0):
    """q_var = 10^U(-2, 1), r_var = q_var 10^U(RATIO_LOG10[ess]), neither a power of two (1 / r_var
    is then inexact, so a product with the reciprocal is not the quotient)"""
    lo, hi = RATIO_LOG10[ess]
    while True:
        q = float(10.0 ** rng.uniform(-2.0, 1.0))
        r = float(q * 10.0 ** rng.uniform(lo, hi))
        if not _pow2(q) and not _pow2(r):
            return q, r


def _pair(rng, sd):
    a = rng.normal(0.0, sd, 2)
    return (float(a[0]), float(a[1]))


def gen_mixed(seed) -> Case:
    seed = int(seed)
    rng = np.random.default_rng([seed, _SALT])
    N = _MIXED_N[seed]
    runs = []
    for k in range(1 + seed % 3):
        T = 1 + (seed * 5 + seed // T_MAX) % T_MAX if k == 0 else int(rng.integers(1, T_MAX + 1))
        ess = ESS[int(rng.integers(len(ESS)))]
        q, r = _variances(rng, ess)
        x0, v0 = _pair(rng, 5.0), _pair(rng, 2.0)
        scheme = (abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC)[int(rng.integers(2))]
        obs = simulate(rng, T, x0, v0, q, r)
        if seed % 5 == 0 and k == 0:        # an outlier at a middle step: no particle near it
            obs[T // 2] += np.array([30.0, -20.0]) * math.sqrt(r)
        runs.append(Run(obs, x0, v0, q, r, ess, scheme))
    return Case(f"mixed-{seed}", N, tuple(runs), keep_history=seed % 4 != 3, ctx_seed=100 + seed)


# the directed cases' parameters where the case is not about them: nothing the defaults would hide
_P = dict(x0=(0.4, -1.3), v0=(0.8, 0.25), q_var=0.07, r_var=0.3)
_PB = dict(x0=(-1.0, 2.0), v0=(0.1, -0.6), q_var=0.5, r_var=0.9)
COLLAPSE_TAIL = 3.0       # collapse: step 2 is observed this many prior standard deviations out (_collapse_edit)


def _one(name, N, T, ess, scheme=abi.RESAMPLE_STRATIFIED, edit=None, keep=True, digest=False, **par):
    p = dict(_P, **par)
    rng = _rng(name)
    obs = simulate(rng, T, **p)
    if edit:
        edit(obs, p)
    return Case(name, N, (Run(obs, ess=ess, scheme=scheme, **p),), keep, 42, digest)


def _rng(name):
    return np.random.default_rng([sum(name.encode()) * 131 + len(name), _SALT + 1])


def _set(t, c, v):
    def edit(obs, p):
        obs[t, c] = v
    return edit


def _collapse_edit(obs, p):
    # Changed from "the model's own data": that keeps the observation in the bulk of the cloud, where
    # N r_var / (2 q_var) particles lie within the observation noise (2.5 at N = 5001, 35 at 70001),
    # and after a Resample the copies of one ancestor stay tied for a step (x_{t+1} = x_t + v reads
    # nothing drawn since), so no single particle held more than 0.37 of the weight. Step 2 is the
    # step at which every particle is distinct; its observation is moved COLLAPSE_TAIL prior standard
    # deviations out on both axes, where the cloud is exp(-COLLAPSE_TAIL^2) as dense.
    obs[1] += COLLAPSE_TAIL * math.sqrt(p["q_var"]) * np.array([1.0, -1.0])


def _directed() -> dict:
    out = {}

    def add(c):
        out[c.name] = c

    for T in (1, 2, 3):
        for N, scheme in ((1025, abi.RESAMPLE_STRATIFIED), (16385, abi.RESAMPLE_SYSTEMATIC)):
            for tag, ess in (("forced", 1.0), ("gated", 0.5)):
                add(_one(f"t{T}_{N}_{tag}", N, T, ess, scheme))
    rng = _rng("recip")
    add(Case("recip", 5001, (Run(simulate(rng, 8, **_P), ess=1.0, **_P), Run(simulate(rng, 8, **_P), ess=0.5, **_P))))
    # `recip` cannot tell a division by r_var from a product with its reciprocal: for the double 0.3
    # (as for 0.6 and 0.5) fl(s * fl(1 / r_var)) == fl(s / r_var) for every s (none of 10^6 differ;
    # tests/test_ssm2d_random_runs.py). At 0.445 more than half do. Three runs: a gated one that never
    # resamples (raw sums of two densities: a last-bit change of one survives the sum), a forced one,
    # and a gated one that ends on a step that does not resample after one that does (a Resample's
    # log-mean absorbs last-bit changes; horizons do not shrink, so every run is fused)
    rng = _rng("recip_inexact")
    p = dict(_P, r_var=0.445)
    add(Case("recip_inexact", 5001, tuple(Run(simulate(rng, T, **p), ess=e, **p) for T, e in ((2, 0.3), (8, 1.0), (9, 0.5)))))
    add(_one("lpmax_positive", 2049, 8, 0.5, q_var=0.01, r_var=0.01))
    add(_one("loose", 2049, 8, 0.5, q_var=0.1, r_var=1e4))
    for N in (5001, 70001):
        add(_one(f"collapse_{N}", N, 6, 1.0, edit=_collapse_edit, q_var=0.1, r_var=1e-4))
    add(_one("far_start", 1025, 6, 0.5, x0=(1e8, -1e8)))
    add(_one("still", 1025, 6, 0.5, v0=(0.0, 0.0)))
    add(_one("inf_obs", 2049, 8, 1.0, edit=_set(4, 0, math.inf)))
    add(_one("huge_obs", 2049, 8, 1.0, edit=_set(4, 0, 1e200)))
    add(_one("nan_obs", 2049, 8, 1.0, edit=_set(4, 1, math.nan)))
    rng = _rng("grow_T")
    add(Case("grow_T", 4097, tuple(Run(simulate(rng, T, **_P), ess=0.5, **_P) for T in (3, 9, 2))))
    # found by this corpus (mixed seeds 14, 20, 29): a run shorter than an earlier one on the context
    # left that run's later columns (here x_4) out of its Resamples; the statements gather them
    rng = _rng("shorter_run_after_longer")
    add(Case("shorter_run_after_longer", 1025, tuple(Run(simulate(rng, T, **_P), ess=1.0, **_P) for T in (3, 2))))
    rng = _rng("param_switch")
    obs = simulate(rng, 6, **_P)
    # A, B, A, then A, B again: a run's buffers alternate by parity and the graph key holds their
    # addresses, so only the fourth and fifth run meet a graph of the other parameter set there
    add(Case("param_switch", 4097, tuple(Run(obs, ess=0.9, **p) for p in (_P, _PB, _P, _P, _PB))))
    rng = _rng("async_mix")
    runs = []
    for k, T in enumerate((4, 7, 5, 10, 3)):
        q, r = _variances(rng)
        p = dict(x0=_pair(rng, 5.0), v0=_pair(rng, 2.0), q_var=q, r_var=r)
        obs = simulate(rng, T, **p)
        if k == 2:
            obs[2] += np.array([30.0, -20.0]) * math.sqrt(r)
        runs.append(Run(obs, ess=(1.0, 0.5)[k % 2], want_evidence=False, **p))
    add(Case("async_mix", 4097, tuple(runs), keep_history=False))
    add(_one("multinomial", 5001, 8, 0.5, abi.RESAMPLE_MULTINOMIAL))
    for N in (2_999_999, 3_000_000):
        add(_one(f"qstat_edge_{N}", N, 3, 1.0, digest=True))
    return out


SEQUENCES = ("grow_T", "shorter_run_after_longer", "param_switch", "async_mix")     # several runs on one context
_DIRECTED = _directed()
DIRECTED = list(_DIRECTED)


def gen(seed, profile="mixed") -> Case:
    """mixed: seed in MIXED_SEEDS; directed: a name of DIRECTED (or its index)"""
    if profile == "mixed":
        return gen_mixed(seed)
    return _DIRECTED[seed if isinstance(seed, str) else DIRECTED[int(seed)]]


def corpus():
    return [gen(s, "mixed") for s in MIXED_SEEDS] + [gen(n, "directed") for n in DIRECTED]


# ---- the oracle's account of a case ---------------------------------------------------------------
def _wmax(w) -> float:
    return float(np.max(w))      # NaN if any is NaN, as the device's max slots


class _Trace:
    """what the statements leave per run: flags (one per step), and per step the max of the weights
    entering its Observe (`base`), the max after it (`M`) and the largest normalised weight (`top`)"""

    def __init__(self):
        self.flags, self.base, self.M, self.top = [], [], [], []


def oracle_trace(case):
    """[_Trace per run], from a fresh Oracle running models.ssm2d_statements"""
    from oracle import Oracle

    class Rec(Oracle):
        tr = None

        def observe(self, dist, x):
            self.tr.base.append(_wmax(self.weights_download()))
            super().observe(dist, x)
            w = self.weights_download()
            m = _wmax(w)
            self.tr.M.append(m)
            e = np.exp(w - m) if math.isfinite(m) else np.full(len(w), math.nan)
            self.tr.top.append(float(e.max() / e.sum()))

    o = Rec(case.N, seed=case.ctx_seed)
    out = []
    try:
        for run in case.runs:
            o.tr = _Trace()
            o.tr.flags = [bool(f) for f in models.ssm2d_statements(o, run.obs, **run.kw())]
            o.tr.log_evidence = o.log_evidence()
            out.append(o.tr)
    finally:
        o.close()
    return out


@functools.lru_cache(maxsize=None)
def _trace_of(name):
    return oracle_trace(gen(int(name[6:]), "mixed") if name.startswith("mixed-") else gen(name, "directed"))


def qref(M) -> float:
    """include/wsmc_math.h wsmc_qref"""
    return float(math.ceil(M)) if math.isfinite(M) else M


def predict_misses(case, traces=None):
    """Per run {"miss": [t], "hold": [t], "undetermined": [t]} over the steps t = 2 .. T (1-based):
    the fused run takes step t's Resample statistics against R_g = qref(U), U = base + lpmax, base
    the max of the weights entering the step, lpmax = -(c0 + 0.0) * 0.5 with c0 = 2 log 2pi + 2 log
    r_var (k_ssm2d_prop; the logarithm here is numpy's), and misses iff that is not qref(M_t), M_t
    the max after the step's Observe. A step whose U or M_t lies within UNDETERMINED of an integer
    may go either way (the kernel's logarithm and sum are not numpy's to the last bit)."""
    traces = traces if traces is not None else _trace_of(case.name)
    out = []
    for run, tr in zip(case.runs, traces):
        c0 = 2.0 * float(np.log(2.0 * np.pi)) + 2.0 * float(np.log(run.r_var))
        lpmax = -(c0 + 0.0) * 0.5
        p = {"miss": [], "hold": [], "undetermined": []}
        for t in range(2, run.T + 1):
            U, M = tr.base[t - 1] + lpmax, tr.M[t - 1]
            near = any(math.isfinite(v) and abs(v - round(v)) < UNDETERMINED for v in (U, M))
            a, b = qref(U), qref(M)
            p["undetermined" if near else ("miss" if a != b else "hold")].append(t)   # (NaN != NaN: a miss, as on the device)
        out.append(p)
    return out


def counter_bounds(run, pred):
    """(lo, hi) of the growth of run_stats()["missed_steps"] over one synchronous, unsharded run with
    the statistics taken in the propagate, and (lo, hi) of the growth of "replays", from one run's
    prediction. The relation is not equality: k_rs_fill_fused counts a miss per step of the *guessed*
    run, and that run is the oracle's only up to its first miss. At a missed step the decision and
    the fill are taken against a reference point above the canonical one (non-canonical bits; an
    outlier's miss of hundreds of nats leaves every q zero, so the step does not resample at all),
    and the steps after it are counted on that trajectory before wsmc_ssm2d_run discards it and
    re-does the whole run on the exact path (which counts nothing). So: with every step determined,
    no predicted miss <=> the counter does not move and no replay; a first predicted miss at step k
    (every step before it determined) <=> the counter grows by at least 1 and at most T - k + 1, and
    by exactly the prediction's count when k = T; the run adds exactly one replay. An undetermined
    step may go either way, and makes every later step's count free."""
    T = run.T
    und = min(pred["undetermined"], default=None)
    first = min(pred["miss"], default=None)
    if run.scheme == abi.RESAMPLE_MULTINOMIAL:
        return (0, 0), (0, 0)          # (the statistics' own kernel at every step: nothing is guessed)
    if first is not None and (und is None or first < und):
        return (1, T - first + 1), (1, 1)
    if und is not None:
        return (0, T - und + 1), (0, 1)
    return (0, 0), (0, 0)


# ---- the comparer -----------------------------------------------------------------------------
def _digest(a) -> str:
    import hashlib
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


def _same(a, b, digest) -> bool:
    if digest:   # (no NaN in the cases compared this way)
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and _digest(a) == _digest(b)
    return same_value(a, b)


def compare(g, o, ev, run, keep_history=True, digest=False):
    """None, or what differs first between the two backends after the same runs: every column, the
    weights, every state field, the last ancestors (once a Resample has resampled) and both
    evidences (ev: what g's run returned; None: not asked for). Finite values by their bits (-0.0
    differs from 0.0), NaNs equal by position. keep_history=False: g holds x (the oracle's
    x_{T+1}), v and dv, and the state fields that mode keeps."""
    if keep_history:
        ng, no = g.col_names(), o.col_names()
        if ng != no:
            return f"column names {ng} != {no}"
        pairs = [(n, n) for n in ng]
    else:
        pairs = [("x", f"x_{run.T + 1}"), ("v", "v"), ("dv", "dv")]
    for a_name, b_name in pairs:
        a, b = g.col_download(g.col_find(a_name)), o.col_download(o.col_find(b_name))
        if not _same(a, b, digest):
            return f"column {a_name}: " + _where(a, b)
    a, b = g.weights_download(), o.weights_download()
    if not _same(a, b, digest):
        return "weights: " + _where(a, b)
    sg, so = g.get_state(), o.get_state()
    for k in (STATE if keep_history else STATE_NO_HISTORY):
        if not same_value(sg[k], so[k]):
            return f"state.{k}: {sg[k]!r} != {so[k]!r}"
    if so["n_resamples"] > 0:
        a, b = g.last_ancestors(), o.last_ancestors()
        if not _same(a, b, digest):
            return "last_ancestors: " + _where(a, b)
    for what, a in (("the run's log evidence", ev), ("log_evidence()", g.log_evidence())):
        if a is not None and not same_value(a, o.log_evidence()):
            return f"{what}: {a!r} != {o.log_evidence()!r}"
    return None


class Mismatch(AssertionError):
    pass


def replay(case, drive="sync", backend="hip") -> str:
    which = f"--seed {case.name[6:]} --profile mixed" if case.name.startswith("mixed-") else f"--name {case.name}"
    return f"python tests/ssm2dfuzz.py {which} --drive {drive} --backend {backend}"


# ---- the runner -------------------------------------------------------------------------------
def oracle_context(base=None):
    """an Oracle behind Context.ssm2d_run's interface (the statements, which define the run; the
    history is always kept): the CPU tests and `--backend oracle` drive `differential` with it"""
    from oracle import Oracle

    class OracleRun(base or Oracle):
        def ssm2d_run(self, obs, x0=(0.0, 0.0), v0=(1.0, 0.0), q_var=0.1, r_var=0.5, ess_perc_min=0.5,
                      scheme=abi.RESAMPLE_STRATIFIED, keep_history=True, want_evidence=True):
            models.ssm2d_statements(self, obs, x0, v0, q_var, r_var, ess_perc_min, scheme)
            return self.log_evidence() if want_evidence else None

    return OracleRun


def _fresh(case, backend, drive):
    from oracle import Oracle
    shards = 2 if drive in ("island2", "exact2") else 1
    exact = drive == "exact2"
    if backend == "hip":
        import wsmc
        if shards == 1:
            g = wsmc.Context(case.N, seed=case.ctx_seed)
        else:
            g = wsmc.Context.multi(case.N, shards, seed=case.ctx_seed, devices=[0] * shards, transport=abi.TRANSPORT_HOST)
            if exact:
                g.comm_set_shard_mode(abi.SHARD_EXACT)
    else:   # "oracle", or a class made by oracle_context (a test's planted fault)
        cls = oracle_context() if backend == "oracle" else backend
        g = cls(case.N, seed=case.ctx_seed, shards=shards, exact=exact)
    return g, Oracle(case.N, seed=case.ctx_seed, shards=shards, exact=exact)


def _run_case(case, backend, drive, runs=None, stats=None):
    """`runs` (default: the case's) on fresh contexts; (the index of the first run after which the
    backends differ, what differs), or (None, None). sync compares after every run, the other
    drives... see differential. stats: a list that takes, per run, the oracle's flags and the
    growth of the device's run_stats() over it (sync, one unsharded context). On the device every
    run's route (ssm2d_routes) is asserted to be the one Case.routes expects."""
    runs = case.runs if runs is None else tuple(runs)
    g, o = _fresh(case, backend, drive)
    keep = case.keep_history or getattr(g, "is_oracle", False)
    counted = drive == "sync" and hasattr(g, "run_stats")
    routed = hasattr(g, "ssm2d_routes") and runs is case.runs
    try:
        for k, run in enumerate(runs):
            last = k == len(runs) - 1
            want = run.want_evidence and drive != "async"
            before = g.run_stats() if counted else None
            r0 = g.ssm2d_routes() if routed else None
            ev = g.ssm2d_run(run.obs, keep_history=case.keep_history, want_evidence=want, **run.kw())
            if routed:
                r1 = g.ssm2d_routes()
                took = {(1, 0): "fused", (0, 1): "statements"}.get((r1["fused_runs"] - r0["fused_runs"],
                                                                    r1["statement_runs"] - r0["statement_runs"]))
                assert took == case.routes()[k], f"{case.name} run {k}: route {took}, expected {case.routes()[k]} ({r0} -> {r1})"
            flags = models.ssm2d_statements(o, run.obs, **run.kw())
            if stats is not None:
                if counted:
                    g.get_state()       # (folds a run that returned nothing in: its misses are counted then)
                after = g.run_stats() if counted else None
                stats.append({"flags": [bool(f) for f in flags], "qstat_mode": after["qstat_mode"] if counted else None,
                              "missed": after["missed_steps"] - before["missed_steps"] if counted else None,
                              "replays": after["replays"] - before["replays"] if counted else None})
            if drive == "async" and not last:
                continue            # nothing is read until the last run
            d = compare(g, o, ev, run, keep, case.digest)
            if d:
                return k, d
    finally:
        g.close()
        o.close()
    return None, None


def locate(case, backend, drive, k):
    """the first differing step of run k (the runs before it whole): fresh contexts at horizons
    1, 2, 4, ..., then a bisection. (step, what differs at the horizon that first shows it)"""
    def differs(h):
        kk, d = _run_case(case, backend, drive, case.runs[:k] + (case.runs[k].cut(h),))
        return d

    T = case.runs[k].T
    lo, hi, why = 0, None, None      # horizons <= lo agree, horizon hi differs
    h = 1
    while hi is None and h < T:
        d = differs(h)
        if d:
            hi, why = h, d
        else:
            lo, h = h, h * 2
    if hi is None:
        hi, why = T, differs(T)
        if why is None:
            return None, "the rerun at the full horizon agrees (the difference does not reproduce)"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        d = differs(mid)
        if d:
            hi, why = mid, d
        else:
            lo = mid
    return hi, why


def differential(case, backend="hip", drive="sync"):
    """`case` through ssm2d_run on a fresh context and through models.ssm2d_statements on a fresh
    oracle of the same seed. Drives: sync: the evidence returned (where the run asks for it),
    everything compared after every run; async: want_evidence=False, nothing read until the last
    run; island2 / exact2: two shards on one device in one handle against Oracle(shards=2), compared
    after every run. A difference (every call having returned WSMC_OK) is located (async: the first
    run whose prefix differs, then its step) and raised as Mismatch with the replay line; an error
    of a call is raised as it is. Returns the per-run statistics (see _run_case)."""
    if drive not in DRIVES:
        raise ValueError(drive)
    stats = []
    k, d = _run_case(case, backend, drive, stats=stats)
    if d:
        if drive == "async":
            for kk in range(len(case.runs)):
                if _run_case(case, backend, drive, case.runs[:kk + 1])[1]:
                    k = kk
                    break
        step, why = locate(case, backend, drive, k)
        line = replay(case, drive, backend if isinstance(backend, str) else "hip")
        print(f"[{line}]")
        raise Mismatch(f"{case.name} N={case.N} drive={drive}: after run {k}: {d}\n"
                       f"  first differing step of run {k}: {step}: {why}\n  [{line}]\n{case.text()}")
    return stats


# ---- command line -----------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--name", choices=DIRECTED, default=None, help="a directed case")
    ap.add_argument("--profile", choices=PROFILES, default=None)
    ap.add_argument("--drive", choices=DRIVES, default="sync")
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    a = ap.parse_args(argv)
    case = gen(a.name, "directed") if a.name else gen(a.seed, "mixed")
    print(case.text())
    print(f"[{replay(case, a.drive, a.backend)}]")
    traces = oracle_trace(case)
    for k, (tr, p) in enumerate(zip(traces, predict_misses(case, traces))):
        print(f"run {k}: resampled", "".join("x" if f else "." for f in tr.flags), "log_evidence", tr.log_evidence,
              "predicted misses", p["miss"], "undetermined", p["undetermined"])
    try:
        stats = differential(case, a.backend, a.drive)
    except Mismatch as e:
        print("MISMATCH", e)
        return 1
    for k, st in enumerate(stats):
        if st["missed"] is not None:
            print(f"run {k}: missed_steps +{st['missed']} replays +{st['replays']} (statistics mode {st['qstat_mode']})")
    print("same as the oracle" + (" (the oracle against itself)" if a.backend == "oracle" else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())

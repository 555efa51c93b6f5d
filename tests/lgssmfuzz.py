"""Seeded random fused 1D-LGSSM runs for wsmc_lgssm1d_run: generator, runner, comparer, replay.

TEST INFRASTRUCTURE, the companion of tests/ssm2dfuzz.py and tests/ssmfuzz.py for the hard-coded
1D linear-Gaussian run (kernel k_lgssm_segment, csrc/wsmc_lgssm.hip). A case is plain data built
from ``numpy.random.default_rng([seed, salt])`` and nothing else (no context, no device): a
population size, the store mode, the context's seed, statements issued before the first run
(`prelude`), one to five runs on that one context (each with its own data, a, q, r, x0_std,
threshold, scheme, call options, segment length and the statements issued just `before` it), and
statements issued after the last run (`tail`). `differential` runs a case on a fresh
`wsmc.Context` through `lgssm1d_run` and on a fresh `oracle.Oracle` through
`models.lgssm1d_statements` (the statements issued one by one: by include/wsmc.h the definition of
the run's result) and compares everything bit for bit after every run, the score tape the host
wrote included; a difference is located by rerunning shorter horizons.

    python tests/lgssmfuzz.py --seed 3 --profile mixed --backend oracle
    python tests/lgssmfuzz.py --name collapse_1025 --backend hip

prints the case and runs it (`--backend hip`: against the oracle, comparing, once with the case's
segment lengths and once unsegmented).
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
from wsmc.dsl import Col, Normal  # noqa: E402

CAP = 5120                                # csrc/wsmc_internal.h kLgCap (a device run reads lgssm_stats()["cap"])
NS = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, "cap")
_MIXED_N = NS + (65, 129, 1000, 1025, 2049, 3073, 4097, "cap", 257, 1001, 2048, 4096, 3072, 513)   # seed -> N
T_MAX = 12
ESS = (0.3, 0.5, 0.9, 1.0)
MIXED_SEEDS = list(range(32))
PROFILES = ("mixed", "directed")
SCHEMES = {"stratified": abi.RESAMPLE_STRATIFIED, "systematic": abi.RESAMPLE_SYSTEMATIC,
           "multinomial": abi.RESAMPLE_MULTINOMIAL}
STATE = ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples", "last_ess_perc")
DEFAULT_SEGMENT = 2048                    # csrc/wsmc_internal.h kLgSegmentSteps
_SALT = 23


# ---- cases are data ---------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Run:
    data: np.ndarray
    a: float = 0.9
    q: float = 1.0
    r: float = 0.5
    x0_std: float = 1.0
    ess: float = 1.0
    scheme: int = abi.RESAMPLE_STRATIFIED
    want_evidence: bool = True
    ess_trace: bool = True
    segment: int | None = None            # steps per launch (set_lgssm_segment); None: the library's default
    before: tuple = ()                    # statements issued between the run before and this one

    @property
    def T(self) -> int:
        return len(self.data)

    def kw(self) -> dict:
        """the model's arguments, as Context.lgssm1d_run and models.lgssm1d_statements take them"""
        return dict(a=self.a, q=self.q, r=self.r, x0_std=self.x0_std, ess_perc_min=self.ess, scheme=self.scheme)

    def cut(self, T) -> "Run":
        return replace(self, data=self.data[:T])

    def text(self) -> str:
        names = {v: k for k, v in SCHEMES.items()}
        return (f"T={self.T} a={self.a!r} q={self.q!r} r={self.r!r} x0_std={self.x0_std!r} ess={self.ess!r} "
                f"{names[self.scheme]} segment={self.segment}{'' if self.want_evidence else ' no-evidence'}"
                f"{'' if self.ess_trace else ' no-trace'}\n" +
                "".join(f"    before: {st!r}\n" for st in self.before) +
                "    data = [" + ", ".join(repr(float(y)) for y in self.data) + "]")


# A statement is a tuple; `issue` runs one on a context and returns what the call returned.
#   ("col", name, dim)   ("assign", name, value)   ("sample", name, source | None, coef, sigma)
#   ("observe", source, sigma, y)   ("weight", source, sigma, y)   ("resample", ess, scheme)
#   ("move", "rw" | "autorw", name, step)   ("moments", name)   ("median", name)   ("sample_particles", n)
def issue(c, st):
    R = models.resolver(c)
    k = st[0]
    if k == "col":
        c.col_create(st[1], st[2])
    elif k == "assign":
        c.assign(c.col_find(st[1]), models._const([st[2]]))
    elif k == "sample":
        _, name, src, coef, sigma = st
        c.sample(c.col_find(name), (Normal(0.0, sigma) if src is None else Normal(Col(src) * coef, sigma)).dist(R))
    elif k in ("observe", "weight"):
        _, src, sigma, y = st
        getattr(c, k)(Normal(Col(src), sigma).dist(R), models._const([y]))
    elif k == "resample":
        return c.resample(st[1], st[2])
    elif k == "move":
        prop = abi.PROPOSAL_RW if st[1] == "rw" else abi.PROPOSAL_AUTORW
        return c.move(prop, [c.col_find(st[2])], st[3])
    elif k == "moments":
        return c.weighted_moments([abi.Operand.column(c.col_find(st[1]))])
    elif k == "median":
        return c.weighted_median(c.col_find(st[1]))
    elif k == "sample_particles":
        return c.sample_particles(st[1])
    else:
        raise ValueError(st)
    return None


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    N: object                   # an int, "cap" or "cap+1"
    runs: tuple
    lazy: bool = True           # the store mode (store_set_lazy)
    ctx_seed: int = 42
    prelude: tuple = ()
    tail: tuple = ()

    def n(self, cap=CAP) -> int:
        return {"cap": cap, "cap+1": cap + 1}.get(self.N, self.N)

    def routes(self, cap=CAP) -> list:
        """per run "persistent" or "statements", by the rule of include/wsmc.h wsmc_lgssm1d_run: one
        unsharded context (every case here), N <= cap, a scheme that is not multinomial, no column
        but a dim-1 `x`, and the weights unchanged at entry (an Observe or Weight sets
        weights_changed, a Resample clears it, and every run ends with a Resample)."""
        cols, changed, out = {}, False, []

        def apply(st):
            nonlocal changed
            if st[0] == "col":
                cols[st[1]] = st[2]
            elif st[0] in ("observe", "weight"):
                changed = True
            elif st[0] == "resample":
                changed = False

        for st in self.prelude:
            apply(st)
        for r in self.runs:
            for st in r.before:
                apply(st)
            ok = (self.n(cap) <= cap and r.scheme != abi.RESAMPLE_MULTINOMIAL and not changed and
                  all(name == "x" and dim == 1 for name, dim in cols.items()))
            out.append("persistent" if ok else "statements")
            cols.setdefault("x", 1)
            changed = False
        return out

    def text(self) -> str:
        return (f"{self.name}: N={self.N} lazy={self.lazy} seed={self.ctx_seed}\n" +
                "".join(f"  prelude: {st!r}\n" for st in self.prelude) +
                "\n".join(f"  run {k}: {r.text()}" for k, r in enumerate(self.runs)) +
                "".join(f"\n  tail: {st!r}" for st in self.tail))


# ---- the generator ----------------------------------------------------------------------------
def simulate(rng, T, a, q, r, x0_std) -> np.ndarray:
    """T observations of the model itself (q, r and x0_std standard deviations), on the generator's rng"""
    x = x0_std * rng.standard_normal()
    data = np.empty(T)
    for t in range(T):
        x = a * x + q * rng.standard_normal()
        data[t] = x + r * rng.standard_normal()
    return data


def _pow2(x) -> bool:
    return math.frexp(x)[0] in (0.5, -0.5)


def _dyadic(x, m=20) -> bool:
    """x = k / 2^m for an integer k: a product with it can be exact"""
    return float(x * 2.0 ** m).is_integer()


# log10(r / q) by threshold, so that a gated run's gate goes both ways within a dozen steps; drawn
# from one range whatever the threshold the share falls to 0-50 % at the ends (a small r / q
# resamples at every step at 0.9, a large one never does at 0.3). tests/test_lgssm_random_runs.py
# asks for 80 %.
RATIO_LOG10 = {0.3: (-0.5, 0.5), 0.5: (-0.25, 0.5), 0.9: (0.25, 1.0), 1.0: (-0.5, 1.0)}


def _params(rng, ess):
    """a signed with |a| ~ U(0, 1.1), q = 10^U(-1.5, 1), r = q 10^U(RATIO_LOG10[ess]), x0_std =
    10^U(-1, 1); none of q, r, x0_std a power of two and a no k / 2^20 (1 / r is then inexact and
    no product of the step is exact by accident)"""
    lo, hi = RATIO_LOG10[ess]
    while True:
        a = float(rng.uniform(0.0, 1.1)) * (1.0 if rng.random() < 0.5 else -1.0)
        q = float(10.0 ** rng.uniform(-1.5, 1.0))
        r = float(q * 10.0 ** rng.uniform(lo, hi))
        x0 = float(10.0 ** rng.uniform(-1.0, 1.0))
        if not any(_pow2(v) for v in (q, r, x0)) and not _dyadic(a):
            return dict(a=a, q=q, r=r, x0_std=x0)


_SEGMENTS = (None, 1, 2, 3, 7, "T", "T+1")


def gen_mixed(seed) -> Case:
    seed = int(seed)
    rng = np.random.default_rng([seed, _SALT])
    runs = []
    for k in range(1 + seed % 3):
        T = 1 + (seed * 5 + seed // T_MAX) % T_MAX if k == 0 else int(rng.integers(1, T_MAX + 1))
        ess = ESS[(seed + k) % len(ESS)] if k == 0 else ESS[int(rng.integers(len(ESS)))]
        p = _params(rng, ess)
        scheme = (abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC)[int(rng.integers(2))]
        data = simulate(rng, T, **p)
        if seed % 5 == 0 and k == 0:        # an outlier at a middle step: no particle near it
            data[T // 2] += 30.0 * p["r"]
        seg = _SEGMENTS[(seed + 3 * k) % len(_SEGMENTS)]
        seg = {"T": T, "T+1": T + 1}.get(seg, seg)
        runs.append(Run(data, ess=ess, scheme=scheme, want_evidence=bool(rng.random() >= 0.25),
                        ess_trace=bool(rng.random() >= 0.25), segment=seg, **p))
    # the context's seed from the whole 64-bit range; seed 7's has the top bit set
    ctx_seed = int(rng.integers(0, 2 ** 63, dtype=np.uint64)) * 2 + int(rng.integers(2))
    if seed == 7:
        ctx_seed |= 1 << 63
    return Case(f"mixed-{seed}", _MIXED_N[seed], tuple(runs), lazy=seed % 2 == 0, ctx_seed=ctx_seed)


# the directed cases' parameters where the case is not about them: nothing the defaults would hide
_P = dict(a=0.83, q=0.45, r=0.37, x0_std=1.7)
_PB = dict(a=-0.61, q=1.3, r=0.9, x0_std=0.35)
DEGENERATE_AT = 4         # nan_obs, inf_obs, huge_obs: the step (0-based) whose observation is replaced
THRESHOLDS = {"thresholds_0": 0.0, "thresholds_neg1": -1.0, "thresholds_2": 2.0, "thresholds_inf": math.inf,
              "thresholds_nan": math.nan}
NONFINITE = {"nonfinite_a_nan": dict(a=math.nan), "nonfinite_a_inf": dict(a=math.inf), "nonfinite_r_inf": dict(r=math.inf),
             "nonfinite_r_denormal": dict(r=5e-324), "nonfinite_q_inf": dict(q=math.inf), "nonfinite_x0_huge": dict(x0_std=1e300),
             # multinomial: the library issues the statements itself, with its own operand for a x
             "nonfinite_a_inf_statements": dict(a=math.inf, scheme=abi.RESAMPLE_MULTINOMIAL)}


def _rng(name):
    return np.random.default_rng([sum(name.encode()) * 131 + len(name), _SALT + 1])


def _one(name, N, T, ess, scheme=abi.RESAMPLE_STRATIFIED, edit=None, data_of=None, lazy=True, segment=None,
         prelude=(), tail=(), **par):
    """one run; its data from the model at the run's own parameters (data_of: at those, where the
    run's are not finite; the rng by data_of's name, where two cases share their data)"""
    p = dict(_P, **par)
    data = simulate(_rng(name), T, **(data_of or p))
    if edit:
        edit(data)
    return Case(name, N, (Run(data, ess=ess, scheme=scheme, segment=segment, **p),), lazy, 42, tuple(prelude), tuple(tail))


def _set(t, v):
    def edit(data):
        data[t] = v
    return edit


OWN_X_PRELUDE = (("col", "x", 1), ("sample", "x", None, 0.0, 1.3), ("observe", "x", 0.8, 0.4),
                 ("resample", 2.0, abi.RESAMPLE_STRATIFIED))
THEN_TAIL = (("move", "rw", "x", 0.3), ("move", "autorw", "x", 1e-3), ("col", "z", 1), ("sample", "z", "x", 0.5, 0.7),
             ("observe", "z", 0.9, -0.2), ("resample", 0.5, abi.RESAMPLE_STRATIFIED), ("moments", "x"), ("median", "x"),
             ("sample_particles", 17))


def _directed() -> dict:
    out = {}

    def add(c):
        out[c.name] = c

    for N in (2048, 2049, 3072, 3073, 4096, 4097):       # the particles a thread holds go 2 | 3 | 4 | 5
        for tag, ess in (("forced", 1.0), ("gated", 0.5)):
            add(_one(f"p_boundaries_{N}_{tag}", N, 3, ess, abi.RESAMPLE_SYSTEMATIC if N % 2 else abi.RESAMPLE_STRATIFIED))
    for N in ("cap", "cap+1"):
        rng = _rng(N)
        add(Case(N, N, tuple(Run(simulate(rng, 5, **_P), ess=e, **_P) for e in (1.0, 0.5))))
    add(_one("recip_inexact", 1025, 8, 0.5, r=0.3, q=0.07))
    add(_one("unit_a", 1025, 8, 0.5, a=1.0))
    for name, a in (("zero_a", 0.0), ("negzero_a", -0.0)):    # one data set for both
        c = _one("zero_a", 1025, 6, 0.5, a=a)
        add(replace(c, name=name))
    add(_one("neg_a", 1025, 8, 0.5, a=-0.95))
    add(_one("explosive", 1025, 12, 0.5, a=1.1))
    for N in (1025, 4097):
        add(_one(f"collapse_{N}", N, 6, 1.0, abi.RESAMPLE_SYSTEMATIC if N == 4097 else abi.RESAMPLE_STRATIFIED,
                 q=0.45, r=1e-3 * 0.45))
    add(_one("loose", 2049, 8, 0.5, q=0.45, r=1e3 * 0.45))
    for name, ess in THRESHOLDS.items():
        add(_one(name, 1025, 6, ess))
    add(_one("nan_obs", 2049, 8, 1.0, edit=_set(DEGENERATE_AT, math.nan)))
    add(_one("inf_obs", 2049, 8, 1.0, edit=_set(DEGENERATE_AT, math.inf)))
    add(_one("neginf_obs_mid", 2049, 9, 0.5, edit=_set(9 // 2, -math.inf)))
    add(_one("huge_obs", 2049, 8, 1.0, edit=_set(DEGENERATE_AT, 1e308)))
    for name, par in NONFINITE.items():
        add(_one(name, 1025, 4, 1.0, data_of=_P, **par))
    data = simulate(_rng("param_switch"), 6, **_P)
    # A, B, A, A, B: both parameter sets reach the kernel's arguments afresh at every call
    add(Case("param_switch", 4097, tuple(Run(data, ess=0.9, **p) for p in (_P, _PB, _P, _P, _PB))))
    rng = _rng("grow_shrink_T")
    add(Case("grow_shrink_T", 4097, tuple(Run(simulate(rng, T, **_P), ess=0.5, **_P) for T in (3, 9, 2))))
    rng = _rng("route_flip")
    add(Case("route_flip", 1025, (
        Run(simulate(rng, 5, **_P), ess=0.5, **_P),
        Run(simulate(rng, 4, **_PB), ess=0.5, before=(("weight", "x", 1.7, 0.3),), **_PB),    # weights_changed: statements
        Run(simulate(rng, 6, **_P), ess=0.9, **_P),                    # run 2's last Resample cleared it: persistent
        Run(simulate(rng, 3, **_PB), ess=0.5, before=(("resample", 2.0, abi.RESAMPLE_STRATIFIED),), **_PB))))
    for name, lazy in (("own_x", True), ("own_x_eager", False)):
        c = _one("own_x", 1025, 5, 0.5, lazy=lazy, prelude=OWN_X_PRELUDE)
        add(replace(c, name=name))
    rng = _rng("foreign_column")
    add(Case("foreign_column", 1025, tuple(Run(simulate(rng, T, **_P), ess=0.5, **_P) for T in (4, 3)),
             prelude=(("col", "y", 1), ("assign", "y", 0.3))))
    add(_one("multinomial", 1025, 6, 0.5, abi.RESAMPLE_MULTINOMIAL))
    add(_one("then_statements", 1025, 6, 0.5, tail=THEN_TAIL))
    add(_one("seg_every_step", 1000, 12, 0.5, segment=1))
    return out


_DIRECTED = _directed()
DIRECTED = list(_DIRECTED)


def gen(seed, profile="mixed") -> Case:
    """mixed: seed in MIXED_SEEDS; directed: a name of DIRECTED (or its index)"""
    if profile == "mixed":
        return gen_mixed(seed)
    return _DIRECTED[seed if isinstance(seed, str) else DIRECTED[int(seed)]]


def by_name(name) -> Case:
    return gen(int(name[6:]), "mixed") if name.startswith("mixed-") else gen(name, "directed")


def corpus():
    return [gen(s, "mixed") for s in MIXED_SEEDS] + [gen(n, "directed") for n in DIRECTED]


# ---- the oracle's side ----------------------------------------------------------------------------
def _recording():
    from oracle import Oracle

    class Rec(Oracle):
        """An oracle whose Resamples' waited returns (flag, ESS%) are kept, in issue order."""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.resamples = []

        def resample(self, *a, **kw):
            r = super().resample(*a, **kw)
            self.resamples.append(r)
            return r

    return Rec


def oracle_run(o, run):
    """models.lgssm1d_statements on a recording oracle: (flags, ESS% of each step's post-Observe Resample)"""
    n0 = len(o.resamples)
    flags = models.lgssm1d_statements(o, run.data, **run.kw())
    post = o.resamples[n0 + 2::2]    # [0] follows x's prior, then (after Sample, after Observe) per step
    assert [f for f, _ in post] == flags
    return [bool(f) for f in flags], np.array([e for _, e in post])


class _Trace:
    """what the statements leave per run: the flags and the ESS% of every step, the log evidence"""


def oracle_trace(case, cap=CAP):
    """[_Trace per run], from a fresh oracle issuing the case's statements"""
    o = _recording()(case.n(cap), seed=case.ctx_seed)
    out = []
    try:
        for st in case.prelude:
            issue(o, st)
        for run in case.runs:
            for st in run.before:
                issue(o, st)
            tr = _Trace()
            tr.flags, tr.ess = oracle_run(o, run)
            tr.log_evidence = o.log_evidence()
            tr.weights, tr.x = o.weights_download(), o.col_download(o.col_find("x"))
            out.append(tr)
    finally:
        o.close()
    return out


@functools.lru_cache(maxsize=None)
def trace_of(name):
    return oracle_trace(by_name(name))


# ---- the comparer -----------------------------------------------------------------------------
def compare(g, o, ev=None, trace=None, ess=None, depths=()):
    """None, or what differs first between the two backends after the same statements: the column
    names, every column, the weights, every state field, the last ancestors, both evidences (ev:
    what g's run returned; None: not asked for), the ESS traces (trace None: not asked for) and
    score(d) for d in depths and -1 (the tape: on the persistent route the host wrote it). Finite
    values by their bits (-0.0 differs from 0.0), NaNs equal by position."""
    ng, no = g.col_names(), o.col_names()
    if ng != no:
        return f"column names {ng} != {no}"
    for name in ng:
        a, b = g.col_download(g.col_find(name)), o.col_download(o.col_find(name))
        if not same_value(a, b):
            return f"column {name}: " + _where(a, b)
    a, b = g.weights_download(), o.weights_download()
    if not same_value(a, b):
        return "weights: " + _where(a, b)
    sg, so = g.get_state(), o.get_state()
    for k in STATE:
        if not same_value(sg[k], so[k]):
            return f"state.{k}: {sg[k]!r} != {so[k]!r}"
    a, b = g.last_ancestors(), o.last_ancestors()
    if not same_value(a, b):
        return "last_ancestors: " + _where(a, b)
    for what, a in (("the run's log evidence", ev), ("log_evidence()", g.log_evidence())):
        if a is not None and not same_value(a, o.log_evidence()):
            return f"{what}: {a!r} != {o.log_evidence()!r}"
    if trace is not None:
        if ess is None or len(trace) != len(ess):
            return f"ESS trace: {len(trace)} steps != {None if ess is None else len(ess)}"
        if not same_value(trace, ess):
            return "ESS trace (by step): " + _where(trace, ess)
    for d in sorted(set(depths)) + [-1]:
        a, b = g.score(d), o.score(d)
        if not same_value(a, b):
            return f"score({d}): " + _where(a, b)
    return None


class Mismatch(AssertionError):
    pass


def replay(case, backend="hip") -> str:
    which = f"--seed {case.name[6:]} --profile mixed" if case.name.startswith("mixed-") else f"--name {case.name}"
    return f"python tests/lgssmfuzz.py {which} --backend {backend}"


# ---- the runner -------------------------------------------------------------------------------
def oracle_context(base=None):
    """an Oracle behind Context.lgssm1d_run's interface (the statements, which define the run): the
    CPU tests and `--backend oracle` drive `differential` with it, no device"""
    class OracleRun(base or _recording()):
        def lgssm1d_run(self, data, a=0.9, q=1.0, r=0.5, x0_std=1.0, ess_perc_min=1.0, scheme=abi.RESAMPLE_STRATIFIED,
                        want_evidence=True, ess_trace=False):
            _, tr = oracle_run(self, Run(np.asarray(data, dtype=float), a, q, r, x0_std, ess_perc_min, scheme))
            e = self.log_evidence() if want_evidence else None
            return (e, tr) if ess_trace else e

    return OracleRun


def device_cap() -> int:
    import wsmc
    g = wsmc.Context(1, seed=1)
    try:
        return int(g.lgssm_stats()["cap"])
    finally:
        g.close()


def _fresh(case, backend, cap):
    if backend == "hip":
        import wsmc
        g = wsmc.Context(case.n(cap), seed=case.ctx_seed)
    else:   # "oracle", or a class made by oracle_context (a test's planted fault)
        cls = oracle_context() if backend == "oracle" else backend
        g = cls(case.n(cap), seed=case.ctx_seed)
    if hasattr(g, "store_set_lazy"):
        g.store_set_lazy(case.lazy)
    return g, _recording()(case.n(cap), seed=case.ctx_seed)


def _both(g, o, st, where):
    """one statement on both; what differs in what it returned, or None"""
    a, b = issue(g, st), issue(o, st)
    return None if same_value(a, b) else f"{where} {st!r} returned {a!r}, the oracle's {b!r}"


def _run_case(case, backend, segmented=True, runs=None, cap=CAP, stats=None):
    """`runs` (default: the case's, then its tail) on fresh contexts; (the index of the first run
    after which the backends differ, what differs), or (None, None); index -1: the prelude, len(runs):
    the tail. On the device every run's route and segment count (lgssm_stats) is asserted to be what
    Case.routes and the run's segment length say. stats: a list that takes the oracle's flags per run."""
    whole = runs is None
    runs = case.runs if whole else tuple(runs)
    g, o = _fresh(case, backend, cap)
    counted = hasattr(g, "lgssm_stats")
    routes = case.routes(cap)
    try:
        for st in case.prelude:
            d = _both(g, o, st, "prelude")
            if d:
                return -1, d
        for k, run in enumerate(runs):
            for st in run.before:
                d = _both(g, o, st, f"before run {k}:")
                if d:
                    return k, d
            K = run.segment if (segmented and run.segment) else 0
            if counted:
                g.set_lgssm_segment(K)
                s0 = g.lgssm_stats()
            out = g.lgssm1d_run(run.data, want_evidence=run.want_evidence, ess_trace=run.ess_trace, **run.kw())
            ev, trace = out if run.ess_trace else (out, None)
            if counted:
                s1 = g.lgssm_stats()
                took = tuple(s1[f] - s0[f] for f in ("persistent_runs", "statement_runs", "segments"))
                want = (1, 0, -(-run.T // (K or DEFAULT_SEGMENT))) if routes[k] == "persistent" else (0, 1, 0)
                assert took == want, (f"{case.name} run {k}: (persistent, statement, segments) {took}, expected {want} "
                                      f"({routes[k]}, segment {K})")
            d0 = o.get_state()["depth"]
            flags, ess = oracle_run(o, run)
            if stats is not None:
                stats.append(flags)
            d1 = o.get_state()["depth"]
            d = compare(g, o, ev, trace, ess, (0, 1, d0 + (d1 - d0) // 2, d1))
            if d:
                return k, d
        if whole and case.tail:
            for st in case.tail:
                d = _both(g, o, st, "tail")
                if d:
                    return len(runs), d
            d = compare(g, o, depths=(0, 1, o.get_state()["depth"]))
            if d:
                return len(runs), "after the tail: " + d
    finally:
        g.close()
        o.close()
    return None, None


def locate(case, backend, segmented, k, cap=CAP):
    """the first differing step of run k (the runs before it whole): fresh contexts at horizons
    1, 2, 4, ..., then a bisection. (step, what differs at the horizon that first shows it)"""
    def differs(h):
        return _run_case(case, backend, segmented, case.runs[:k] + (case.runs[k].cut(h),), cap)[1]

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


def differential(case, backend="hip", segmented=True, cap=None):
    """`case` through lgssm1d_run on a fresh context and through models.lgssm1d_statements on a fresh
    oracle of the same seed, the prelude, the statements between the runs and the tail on both;
    everything compared after every run (compare) and every statement's return as it comes.
    segmented=False: every run at the library's default segment length. A difference (every call
    having returned WSMC_OK) is located and raised as Mismatch with the replay line; an error of a
    call is raised as it is. Returns the oracle's flags per run."""
    if cap is None:
        cap = device_cap() if backend == "hip" else CAP
    stats = []
    k, d = _run_case(case, backend, segmented, cap=cap, stats=stats)
    if d:
        step, why = (None, "not in a run") if not 0 <= k < len(case.runs) else locate(case, backend, segmented, k, cap)
        line = replay(case, backend if isinstance(backend, str) else "hip")
        print(f"[{line}]")
        raise Mismatch(f"{case.name} N={case.n(cap)} segmented={segmented}: after run {k}: {d}\n"
                       f"  first differing step of run {k}: {step}: {why}\n  [{line}]\n{case.text()}")
    return stats


# ---- command line -----------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--name", choices=DIRECTED, default=None, help="a directed case")
    ap.add_argument("--profile", choices=PROFILES, default=None)
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    a = ap.parse_args(argv)
    case = gen(a.name, "directed") if a.name else gen(a.seed, "mixed")
    print(case.text())
    print(f"[{replay(case, a.backend)}]")
    cap = device_cap() if a.backend == "hip" else CAP
    for k, (tr, route) in enumerate(zip(oracle_trace(case, cap), case.routes(cap))):
        print(f"run {k}: {route}: resampled", "".join("x" if f else "." for f in tr.flags), "log_evidence", tr.log_evidence)
    try:
        for segmented in ((True, False) if a.backend == "hip" else (True,)):
            differential(case, a.backend, segmented, cap)
    except Mismatch as e:
        print("MISMATCH", e)
        return 1
    print("same as the oracle" + (" (the oracle against itself)" if a.backend == "oracle" else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Sampled trajectories and smoothed moments of the fused scalar-SSM runs (wsmc_ssm_run_smoothed,
wsmc_ssm_run_batch_smoothed; csrc/wsmc_ssm_smooth.hip). Every comparison is bit for bit, NaNs by
position and -0.0 apart from 0.0, with the definition: `spec.statements(Oracle(n, seed), data,
smooth=True, trace=True)`, which copies every column at each trace point into a column of its own
that the Resamples which follow gather, and reads them after the last step. Everything else a run
leaves is compared, with ssmfuzz.compare, against the plain statements on a second oracle (the
definition's extra columns and Assigns are not the run's).

The sizes are where the workgroup's layout changes: 1, 2, 63 / 64 / 65 (one particle in the second
wave), 257, 1000, 2049 (three particles a thread, a second tile of the canonical sum) and the cap
of the column count (the trace-back stages one row of the log at a time there). T = 24, with
segments of 1 and 5 steps so that rows of the history and slots of the log cross launch boundaries.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ssmfuzz as sf
import test_gpu_ssm_batch as tb     # bits_equal, the per-filter comparison, the sv parameter sets
import test_gpu_ssm_trace as tt     # the filter trace's comparison
import wsmc
from oracle import Oracle
from ssmfuzz import A, K, O, S, col, dat
from test_gpu_ssm_random_specs import rotated
from wsmc import abi, models

pytestmark = pytest.mark.gpu

STRAT, SYST, MULT = abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL
T = sf.T
SIZES = [1, 2, 63, 64, 65, 257, 1000, 2049, "cap"]
SPECS = {name: (make(), gen(T)) for name, (make, gen) in models.SSM_MODELS.items()}
SPECS["lgssm1d"] = (models.lgssm1d_spec(), models.lgssm1d_data(T))


@pytest.fixture(scope="module")
def ctx(gpu_available):
    g = wsmc.Context(16, seed=1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cap(ctx):
    return ctx.ssm_stats()["cap"]


def smooth_differ(got, want, what=""):
    """None, or the first difference of two SsmSmooth (a part that is None on `got` was not asked for)"""
    parts = [("log_weights", got.log_weights, want.log_weights)]
    for kind, a, b in (("paths", got.paths, want.paths), ("mean", got.mean, want.mean), ("var", got.var, want.var)):
        if a is not None:
            assert list(a) == list(b), (list(a), list(b))
            parts += [(f"{kind}[{c}]", a[c], b[c]) for c in b]
    for name, a, b in parts:
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return f"{what}: {name}: shape {a.shape} != {b.shape}"
        ok = tb.bits_equal(a, b)
        if not ok.all():
            at = tuple(int(v) for v in np.argwhere(~ok)[0])
            return f"{what}: {name} differs first at {at} (step, particle): {a[at]!r} != the oracle's {b[at]!r}"
    return None


# the definition's rows, computed once per (spec, data, n, seed, ess, scheme, steps) and left unchanged
_KEYS = {}


def _key(ssm, data):
    k = (id(ssm), None if data is None else np.asarray(data).tobytes())
    _KEYS.setdefault(k, (ssm, data))
    return k


@functools.lru_cache(maxsize=None)
def _definition(key, n, seed, ess, scheme, steps):
    ssm, data = _KEYS[key]
    o = Oracle(n, seed=seed)
    try:
        _, _, tr, sm = ssm.statements(o, data, ess_perc_min=ess, scheme=scheme, T=steps, trace=True, smooth=True)
        return tr, sm
    finally:
        o.close()


def definition(ssm, data, n, seed, ess, scheme=STRAT, steps=None):
    return _definition(_key(ssm, data), n, seed, ess, scheme, steps)


def run_pair(ssm, data, n, ess, scheme=STRAT, segment=None, steps=None, seed=sf.SEED, trace=True, smooth=True, what=""):
    """the smoothed fused run on a fresh context against the definition, and everything else it leaves
    against the plain statements on a fresh oracle of the same seed; returns (trace, smooth) of the run"""
    g, o = wsmc.Context(n, seed=seed), Oracle(n, seed=seed)
    try:
        if segment is not None:
            g.set_ssm_segment(segment)
        r = g.ssm_run(ssm, data, ess_perc_min=ess, scheme=scheme, T=steps, trace=trace, smooth=smooth)
        ev, tr, sm = (r[0], r[1], r[2]) if trace else (r[0], None, r[1])
        _, etr = ssm.statements(o, data, ess_perc_min=ess, scheme=scheme, T=steps)
        wtr, wsm = definition(ssm, data, n, seed, ess, scheme, steps)
        tag = f"{what} N={n} ess={ess} scheme={scheme} segment={segment}"
        d = sf.compare(g, o, ev, tr.ess if tr is not None and tr.ess is not None else etr, etr)
        assert d is None, f"{tag}: {d}"
        st = g.ssm_stats()
        assert (st["persistent_runs"], st["statement_runs"]) == (1, 0), f"{tag}: runs {st}"
        if tr is not None:
            d = tt.rows_differ(tr, wtr, tag)
            assert d is None, d
        d = smooth_differ(sm, wsm, tag)
        assert d is None, d
        return tr, sm
    finally:
        g.close()
        o.close()


# ---- 1. the models ---------------------------------------------------------------------------------
MODEL_CASES = [(name, n) for name in sorted(SPECS) for n in SIZES]


@pytest.mark.parametrize("name, n", MODEL_CASES, ids=[f"{a}-{b}" for a, b in MODEL_CASES])
def test_models(cap, name, n):
    """every threshold each (1.0: every step resamples; 0.0: none does); the scheme and the segment
    (1, 5, the default) rotate with the case, as test_gpu_ssm_trace.test_models rotates them"""
    ssm, data = SPECS[name]
    k = MODEL_CASES.index((name, n))
    size = cap[len(ssm.cols)] if n == "cap" else n
    for e, ess in enumerate((1.0, 0.5, 0.0)):
        _, sm = run_pair(ssm, data, size, ess, (STRAT, SYST)[(k + e) % 2], (1, 5, None)[(k // 2 + e) % 3], what=name)
        assert all(np.isfinite(v).all() for v in list(sm.mean.values()) + list(sm.var.values()) + list(sm.paths.values()))
        if size == 1:
            assert all((v == 0.0).all() for v in sm.var.values())   # one particle: no spread


# ---- 2. random and directed specs: OBSERVEs anywhere in the step, statements after the last one ----
@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sf.corpus()}


MIXED = [(s, 1001, 0.5, STRAT, None) for s in sf.MIXED_SEEDS] + [(s, 65) + rotated(s)[1:] for s in sf.MIXED_SEEDS]


@pytest.mark.parametrize("case", MIXED, ids=lambda c: "-".join("default" if v is None else str(v) for v in c))
def test_mixed_seed(cases, case):
    seed, n, ess, scheme, segment = case
    c = cases[f"mixed-{seed}"]
    run_pair(c.ssm, c.data, n, ess, scheme, segment, steps=c.T, what=c.name)


def three_observes():
    """three OBSERVEs a step (three slots of the log), a SAMPLE and an ASSIGN after the last one: the
    trace point's columns are not the step's final ones, and the walk passes two slots between rows"""
    rng = np.random.default_rng(11)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.normal(0, 0.5, T), 3)])
    normal = lambda mu, sc: sf.DistD(abi.FAM_NORMAL, mu, K(sc))
    step = [S(0, normal(K(0.0, col(0, 0.9)), 0.5)),
            O(K(0.0, dat(0)), normal(K(0.0, col(0)), 1.0)),
            S(1, normal(K(0.0, col(0, 0.5), col(1, 0.4)), 0.3)),
            O(K(0.0, dat(1)), normal(K(0.0, col(1)), 0.8)),
            O(K(0.0, dat(0)), normal(K(0.0, col(0, 0.5), col(1, 0.5)), 1.5)),
            S(0, normal(K(0.0, col(0, 0.95)), 0.3)),
            A(1, K(1.0, col(0, 2.0)))]
    return sf.Case("three_observes", 2, [S(0, normal(K(0.0), 1.0)), S(1, normal(K(0.0), 1.0))], step, 2, data, T, ["real", "real"])


@pytest.mark.parametrize("n, segment", [(65, 1), (1001, 5), (2049, None)])
def test_three_observes_and_a_sample_after_the_last(n, segment):
    c = three_observes()
    _, sm = run_pair(c.ssm, c.data, n, 1.0, STRAT, segment, steps=c.T, what=c.name)
    g = wsmc.Context(n, seed=sf.SEED)
    g.ssm_run(c.ssm, c.data, ess_perc_min=1.0, T=c.T)
    final = g.col_download(g.col_find("c0"))
    g.close()
    assert not tb.bits_equal(sm.paths["c0"][-1], final).all()   # the SAMPLE after the trace point


@pytest.mark.parametrize("name", ["observe_first", "init_observe", "nodata", "wide_data", "no_init", "full", "all_xops", "partial_support"])
def test_directed(cases, cap, name):
    c = cases[name]
    n = cap[4] if name == "full" else 1001
    _, sm = run_pair(c.ssm, c.data, n, 0.5, SYST, 5, steps=c.T, what=name)
    if name == "all_xops":          # the programs' non-finite columns: rows compared by position, c0's by their bits
        assert np.isfinite(sm.mean["c0"]).all() and not np.isfinite(sm.mean["c1"][1:]).any()
    if name == "partial_support":   # every final weight is -inf: NaN moments, the trajectories all the same
        assert np.isnan(sm.mean["c0"]).all() and np.isfinite(sm.paths["c0"]).all()


# ---- 3. the parts, and what the smoothing leaves alone ---------------------------------------------
@pytest.mark.parametrize("parts", [("paths",), ("mean",), ("var",)])
def test_a_part_alone(parts):
    ssm, data = SPECS["local_trend"]
    _, got = run_pair(ssm, data, 2049, 0.5, SYST, 5, smooth=parts, trace=False, what=str(parts))
    for p in ("paths", "mean", "var"):
        assert (getattr(got, p) is not None) == (p in parts), p


def test_null_smooth_is_the_traced_run():
    """wsmc_ssm_run_smoothed with a NULL smooth, and with every member NULL: the traced call's
    results and routes, with a trace and without one"""
    ssm, data = SPECS["sv"]
    tab = ssm.table(data)
    o = Oracle(1001, seed=3)
    _, _, want = ssm.statements(o, data, ess_perc_min=0.5, trace=True)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for sm in (None, abi.SsmSmoothOut()):
        for traced in (True, False):
            g = wsmc.Context(1001, seed=3)
            ev = C.c_double()
            tr = abi.SsmTraceOut()
            bufs = {"ess": np.empty(T), "mean": np.empty((T, 2)), "var": np.empty((T, 2)), "log_evidence": np.empty(T)}
            if traced:
                for p, a in bufs.items():
                    setattr(tr, p, dp(a))
            abi.check(g._L.wsmc_ssm_run_smoothed(g._h, C.byref(ssm.spec), dp(tab), len(tab), 0.5, STRAT, C.byref(ev),
                                                 C.byref(tr) if traced else None, None if sm is None else C.byref(sm)))
            d = sf.compare(g, o, ev.value)
            assert d is None, d
            assert g.ssm_stats()["persistent_runs"] == 1 and g.ssm_stats()["statement_runs"] == 0
            if traced:
                got = wsmc.SsmTrace(bufs["ess"], {c: bufs["mean"][:, k] for k, c in enumerate(ssm.cols)},
                                    {c: bufs["var"][:, k] for k, c in enumerate(ssm.cols)}, bufs["log_evidence"])
                assert tt.rows_differ(got, want) is None
            g.close()
    o.close()


def _before_the_run(c, foreign=False, weights=False):
    """what a context holds when a reason against the persistent route lies in its state"""
    if foreign:
        c.assign(c.col_create("other", 1), [abi.Operand.const(0.3)])
    if weights:
        c.observe(models.sv().spec.init[0].dist, [abi.Operand.const(0.1)])


def test_refusals_leave_the_context_as_it_was(cap):
    """a smoothed run has the persistent route only: what sends ssm_run through the statements raises
    here, before anything of the context changes (not even the spec's columns are made)"""
    ssm, data = SPECS["sv"]

    def refused(n, word, scheme=STRAT, foreign=False, weights=False):
        g, o = wsmc.Context(n, seed=5), Oracle(n, seed=5)
        try:
            for c in (g, o):
                _before_the_run(c, foreign, weights)
            with pytest.raises(wsmc.WSMCError) as e:
                g.ssm_run(ssm, data, ess_perc_min=0.5, scheme=scheme, smooth=True)
            assert e.value.code == abi.WSMC_EARG and word in str(e.value), str(e.value)
            st = g.ssm_stats()
            assert (st["persistent_runs"], st["statement_runs"]) == (0, 0)
            d = sf.compare(g, o)
            assert d is None, f"{word}: {d}"
        finally:
            g.close()
            o.close()

    refused(cap[2] + 1, "above the cap")
    refused(65, "not the spec's", foreign=True)
    refused(65, "multinomial", scheme=MULT)
    refused(65, "weights_changed", weights=True)
    big = sf.gen("prog97", "directed")
    g = wsmc.Context(65, seed=5)
    with pytest.raises(wsmc.WSMCError, match="program instructions"):
        g.ssm_run(big.ssm, big.data, T=big.T, smooth=True)
    assert g.col_names() == []
    g.close()
    m = wsmc.Context.multi(128, 2, seed=1, devices=[0, 0], transport=abi.TRANSPORT_HOST)
    with pytest.raises(wsmc.WSMCError, match="multi-device"):
        m.ssm_run(ssm, data, smooth=True)
    m.close()


# each single-device reason of the refusals above: (word, n or "cap", the call's scheme, the context's state)
ROUTE_REASONS = [("above the cap", "cap", STRAT, {}), ("not the spec's", 65, STRAT, dict(foreign=True)),
                 ("multinomial", 65, MULT, {}), ("weights_changed", 65, STRAT, dict(weights=True)),
                 ("program instructions", 65, STRAT, {}), (None, 65, STRAT, {})]


@pytest.mark.parametrize("word,n,scheme,state", ROUTE_REASONS, ids=[r[0] or "no reason" for r in ROUTE_REASONS])
def test_what_refuses_a_smoothed_run_sends_an_untraced_one_through_the_statements(cap, word, n, scheme, state):
    """the route rule is stated once: on a context set up exactly as the refused smoothed call's
    was, the untraced ssm_run is one statement run and no persistent one; with no reason present
    the same call is one persistent run and no statement run. T = 4"""
    if word == "program instructions":
        big = sf.gen("prog97", "directed")
        ssm, data, ess = big.ssm, big.data[:4], 1.0
    else:
        ssm, data, ess = SPECS["sv"][0], SPECS["sv"][1][:4], 0.5
    g = wsmc.Context(cap[len(ssm.cols)] + 1 if n == "cap" else n, seed=5)
    try:
        _before_the_run(g, **state)
        if word is not None:   # ... and the smoothed call is refused for this reason
            with pytest.raises(wsmc.WSMCError, match=word):
                g.ssm_run(ssm, data, ess_perc_min=ess, scheme=scheme, smooth=True)
        g.ssm_run(ssm, data, ess_perc_min=ess, scheme=scheme)
        st = g.ssm_stats()
        assert (st["persistent_runs"], st["statement_runs"]) == ((1, 0) if word is None else (0, 1)), (word, st)
    finally:
        g.close()


def test_untraced_and_traced_runs_after_a_smoothed_one():
    """on one context: the log's buffers are the smoothed call's alone"""
    ssm, data = SPECS["kitagawa"]
    n = 1000
    g, o = wsmc.Context(n, seed=8), Oracle(n, seed=8)
    g.set_ssm_segment(5)
    ev, sm = g.ssm_run(ssm, data, ess_perc_min=0.5, smooth=True)
    _, etr = ssm.statements(o, data, ess_perc_min=0.5)
    assert sf.compare(g, o, ev) is None
    assert smooth_differ(sm, definition(ssm, data, n, 8, 0.5)[1], "first") is None
    ev, ess = g.ssm_run(ssm, data, ess_perc_min=0.5, ess_trace=True)       # the columns exist now: `init` runs again
    _, etr = ssm.statements(o, data, ess_perc_min=0.5)
    d = sf.compare(g, o, ev, ess, etr)
    assert d is None, d
    ev, tr = g.ssm_run(ssm, data, ess_perc_min=1.0, scheme=SYST, trace=True)
    _, etr, want = ssm.statements(o, data, ess_perc_min=1.0, scheme=SYST, trace=True)
    d = sf.compare(g, o, ev, tr.ess, etr)
    assert d is None, d
    assert tt.rows_differ(tr, want, "traced after smoothed") is None
    assert g.ssm_stats()["persistent_runs"] == 3 and g.ssm_stats()["statement_runs"] == 0
    g.close()
    o.close()


# ---- 4. the batch: every filter against the single smoothed run's reference --------------------------
def check_batch(res, b, ssm, data, n, seed, ess, scheme=STRAT, steps=None, what=""):
    ref, want = tt.batch_ref(ssm, data, n, seed, ess, scheme, steps)
    tb.check_filter(res, b, ref, what)
    d = tt.rows_differ(tt.batch_trace(res, b, ssm.cols), want, f"{what} filter b={b} n={n}")
    assert d is None, d
    got = wsmc.SsmSmooth({c: res.paths[c][b] for c in ssm.cols}, {c: res.smean[c][b] for c in ssm.cols},
                         {c: res.svar[c][b] for c in ssm.cols}, res.log_weights[b])
    d = smooth_differ(got, definition(ssm, data, n, seed, ess, scheme, steps)[1], f"{what} filter b={b} n={n}")
    assert d is None, d


def run_batch(g, specs, data, n, seeds, ess, scheme=STRAT, steps=None, smooth=True):
    return g.ssm_run_batch(specs, data, n, seeds, ess_perc_min=ess, scheme=scheme, state=True, T=steps, trace=True, smooth=smooth)


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("n", [65, 1000])
def test_batch_of_one_is_the_single_smoothed_run(ctx, n, ess):
    for name in sorted(SPECS):
        ssm, data = SPECS[name]
        res = run_batch(ctx, ssm, data, n, [sf.SEED], ess)
        check_batch(res, 0, ssm, data, n, sf.SEED, ess, what=name)


@pytest.mark.parametrize("scheme", [STRAT, SYST])
@pytest.mark.parametrize("n", [65, 1000])
def test_batch_per_filter_parameters_and_seeds(ctx, n, scheme):
    try:
        for segment, ess in ((1, 0.5), (5, 1.0), (0, 0.5)):
            ctx.set_ssm_batch_segment(segment)
            res = run_batch(ctx, tb.SV_SPECS, tb.SV_DATA, n, tb.SV_SEEDS, ess, scheme)
            for b in range(5):
                check_batch(res, b, tb.SV_SPECS[b], tb.SV_DATA, n, tb.SV_SEEDS[b], ess, scheme, what=f"segment {segment}")
    finally:
        ctx.set_ssm_batch_segment(0)
    assert len({float(res.smean["h"][b][0]) for b in range(5)}) == 5   # the filters do differ


@pytest.mark.parametrize("n", [65, 1000])
def test_batch_shared_spec_and_per_filter_tables(ctx, n):
    ssm, seeds = models.local_trend(), [3, 4, 5, 6, 7]
    y = models.local_trend_data(T)
    tables = [y, models.local_trend_data(T, seed=9), y.copy(), y[::-1].copy(), models.local_trend_data(T, seed=10)]
    res = run_batch(ctx, ssm, tables, n, seeds, 0.5)
    for b in range(5):
        check_batch(res, b, ssm, tables[b], n, seeds[b], 0.5, what="tables")
    res = run_batch(ctx, ssm, y, n, seeds, 1.0)   # one spec, one table: the seeds alone differ
    for b in range(5):
        check_batch(res, b, ssm, y, n, seeds[b], 1.0, what="shared")
    assert not tb.bits_equal(res.smean["x"][0], res.smean["x"][1]).all()


def test_batch_mixed_spec_with_observes_anywhere(ctx, cases):
    c = cases["mixed-3"]
    seeds = [sf.SEED, 9, 10]
    res = run_batch(ctx, c.ssm, c.data, 65, seeds, 0.5, steps=c.T)
    for b in range(3):
        check_batch(res, b, c.ssm, c.data, 65, seeds[b], 0.5, steps=c.T, what=c.name)
    c = three_observes()
    res = run_batch(ctx, c.ssm, c.data, 1000, seeds, 1.0, steps=c.T)
    for b in range(3):
        check_batch(res, b, c.ssm, c.data, 1000, seeds[b], 1.0, steps=c.T, what=c.name)


def test_batch_more_filters_than_resident_blocks(ctx):
    """a batch larger than one round of resident workgroups: B from the residency the library reports"""
    n, steps = 65, 6
    ssm, data = models.local_trend(), models.local_trend_data(steps)
    run_batch(ctx, ssm, data, n, [1, 2], 0.5)   # (the residency is known after a batch of this shape)
    st = ctx.ssm_batch_stats()
    assert st["cus"] >= 1 and st["blocks_per_cu"] >= 1
    B = st["cus"] * st["blocks_per_cu"] + 3
    res = run_batch(ctx, ssm, data, n, list(range(B)), 0.5)
    assert res.paths["x"].shape == (B, steps, n) and res.smean["v"].shape == (B, steps)
    for b in range(B):
        check_batch(res, b, ssm, data, n, b, 0.5, what="many")


def test_batch_a_part_alone_and_without_the_trace(ctx):
    ssm, data = SPECS["sv"]
    full = run_batch(ctx, ssm, data, 1000, [1, 2], 0.5)
    for parts in (("paths",), ("mean",), ("var",)):
        res = ctx.ssm_run_batch(ssm, data, 1000, [1, 2], ess_perc_min=0.5, smooth=parts)
        assert res.mean is None and res.log_evidence_trace is None
        for p, a, f in (("paths", res.paths, full.paths), ("mean", res.smean, full.smean), ("var", res.svar, full.svar)):
            assert (a is not None) == (p in parts), p
            if a is not None:
                assert all(tb.bits_equal(a[c], f[c]).all() for c in ssm.cols), p
        assert tb.bits_equal(res.log_evidence, full.log_evidence).all()


def test_batch_refusals_are_the_batch_s(ctx, cap):
    sv, y = SPECS["sv"]
    with pytest.raises(wsmc.WSMCError, match="cap"):
        ctx.ssm_run_batch(sv, y, cap[2] + 1, [1, 2], smooth=True)
    with pytest.raises(wsmc.WSMCError, match="multinomial"):
        ctx.ssm_run_batch(sv, y, 100, [1, 2], scheme=MULT, smooth=True)
    with pytest.raises(wsmc.WSMCError, match="differs from spec 0 in shape"):
        ctx.ssm_run_batch([sv, models.local_trend()], y, 100, [1, 2], smooth=True)
    res = run_batch(ctx, sv, y, 65, [1, 2], 0.5)   # afterwards the context still runs a smoothed batch
    for b in range(2):
        check_batch(res, b, sv, y, 65, b + 1, 0.5, what="after the refusals")

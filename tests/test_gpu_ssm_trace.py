"""The per-step filtering trace of the fused scalar-SSM runs (wsmc_ssm_run_traced,
wsmc_ssm_run_batch_traced; csrc/wsmc_ssm_body.h ss_trace_row). Every row (the ESS%, each column's
weighted mean and variance, the cumulative log evidence) is compared bit for bit, NaNs by position
and -0.0 apart from 0.0, with the definition: `spec.statements(Oracle(n, seed), data, trace=True)`,
which takes `weighted_moments` and `log_evidence` between each step's last observe and its
Resample. Everything else a run leaves is compared as the untraced tests compare it.

The sizes are where the workgroup's canonical sum (tiles of 2048 items, 256 canonical threads of 8
strided items, dealt as canonical waves over 1..16 real waves) can go wrong: 1 (variance 0), 2,
63 / 64 / 65 (one particle in the second wave), 255 / 256 / 257 (a second item for one canonical
thread), 1000, 1025, 2047 / 2048 / 2049 (a second tile of one item; three particles a thread), 4097
(a third tile; specs of one or two columns), the cap of the column count, and one past the cap (the
statement route). T = 24, with segments of 1 and 5 steps so that rows cross launch boundaries.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ssmfuzz as sf
import test_gpu_ssm_batch as tb   # its references, its per-filter comparison, its sv parameter sets
import wsmc
from oracle import Oracle
from ssmfuzz import A, K, O, S, col, dat
from test_gpu_ssm_random_specs import rotated
from wsmc import abi, dsl, models
from wsmc.dsl import Col, Data
from wsmc.ssm import SSM, observe, sample

pytestmark = pytest.mark.gpu

STRAT, SYST, MULT = abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL
T = sf.T
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1025, 2047, 2048, 2049, 4097, "cap", "cap+1"]
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


def rows_differ(got, want, what=""):
    """None, or the first differing row of two SsmTrace (a part that is None on `got` was not asked for)"""
    parts = [("ess", got.ess, want.ess), ("log_evidence", got.log_evidence, want.log_evidence)]
    for kind, a, b in (("mean", got.mean, want.mean), ("var", got.var, want.var)):
        if a is not None:
            assert list(a) == list(b), (list(a), list(b))
            parts += [(f"{kind}[{c}]", a[c], b[c]) for c in b]
    for name, a, b in parts:
        if a is None:
            continue
        if a.shape != b.shape:
            return f"{what}: {name}: shape {a.shape} != {b.shape}"
        ok = tb.bits_equal(a, b)
        if not ok.all():
            t = int(np.argmin(ok))
            return f"{what}: {name} differs first at step {t}: {a[t]!r} != the oracle's {b[t]!r}"
    return None


def run_pair(ssm, data, n, ess, scheme=STRAT, segment=None, steps=None, route="persistent", foreign=False,
             seed=sf.SEED, trace=True, what=""):
    """the traced fused run on a fresh context, the traced statements on a fresh oracle of the same
    seed: the rows, everything ssmfuzz.compare compares, and the route; returns (got, want)"""
    g, o = wsmc.Context(n, seed=seed), Oracle(n, seed=seed)
    try:
        if segment is not None:
            g.set_ssm_segment(segment)
        if foreign:   # a column that is not the spec's: the library issues the statements itself
            for c in (g, o):
                c.assign(c.col_create("other", 1), [abi.Operand.const(0.3)])
        ev, got = g.ssm_run(ssm, data, ess_perc_min=ess, scheme=scheme, T=steps, trace=trace)
        _, etr, want = ssm.statements(o, data, ess_perc_min=ess, scheme=scheme, T=steps, trace=True)
        tag = f"{what} N={n} ess={ess} scheme={scheme} segment={segment}"
        d = sf.compare(g, o, ev, got.ess if got.ess is not None else etr, etr)
        assert d is None, f"{tag}: {d}"
        st = g.ssm_stats()
        took = (st["persistent_runs"], st["statement_runs"])
        assert took == ((1, 0) if route == "persistent" else (0, 1)), f"{tag}: runs {took}, expected the {route} route"
        d = rows_differ(got, want, tag)
        assert d is None, d
        return got, want
    finally:
        g.close()
        o.close()


# ---- 1. the models, at the sizes where the reduction can go wrong --------------------------------
MODEL_CASES = [(name, n) for name in sorted(SPECS) for n in SIZES if not (n == 4097 and len(SPECS[name][0].cols) > 2)]


@pytest.mark.parametrize("name, n", MODEL_CASES, ids=[f"{a}-{b}" for a, b in MODEL_CASES])
def test_models(cap, name, n):
    """both thresholds each; the scheme and the segment (1, 5, the default) rotate with the case, so
    every size meets every value of both and every model every combination"""
    ssm, data = SPECS[name]
    k = MODEL_CASES.index((name, n))
    s = len(ssm.cols)
    size = cap[s] + (n == "cap+1") if isinstance(n, str) else n
    route = "statements" if n == "cap+1" else "persistent"
    for e, ess in enumerate((1.0, 0.5)):
        got, _ = run_pair(ssm, data, size, ess, (STRAT, SYST)[(k + e) % 2], (1, 5, None)[(k // 2 + e) % 3], route=route, what=name)
        if size == 1:
            assert all((v == 0.0).all() for v in got.var.values())   # one particle: no spread
        assert np.isfinite(got.log_evidence).all() and all(np.isfinite(v).all() for v in got.mean.values())


# ---- 2. random and directed specs ----------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sf.corpus()}


MIXED = [(s, 1001, 0.5, STRAT, None) for s in sf.MIXED_SEEDS] + [(s,) + rotated(s) for s in sf.MIXED_SEEDS]


@pytest.mark.parametrize("case", MIXED, ids=lambda c: "-".join("default" if v is None else str(v) for v in c))
def test_mixed_seed(cases, case):
    seed, n, ess, scheme, segment = case
    c = cases[f"mixed-{seed}"]
    run_pair(c.ssm, c.data, n, ess, scheme, segment, steps=c.T, what=c.name)


@pytest.mark.parametrize("n", [65, 2049])
@pytest.mark.parametrize("name", ["observe_first", "init_observe", "nodata", "wide_data", "no_init", "all_xops", "partial_support"])
def test_directed(cases, name, n):
    c = cases[name]
    got, want = run_pair(c.ssm, c.data, n, 0.5, STRAT, 5, steps=c.T, what=name)
    if name == "all_xops":          # the programs' non-finite columns: rows compared by position, c0's by their bits
        bad = ~np.isfinite(np.column_stack([got.mean[k] for k in ("c1", "c2", "c3")])).all(axis=1)
        assert bad[1:].all() and not bad[0] and np.isfinite(got.mean["c0"]).all() and np.isfinite(got.var["c0"]).all()
    if name == "partial_support":   # every weight -inf from step 20 on: NaN moments, evidence and ESS%
        dead = slice(sf.PARTIAL_ALL_AT, None)
        assert np.isnan(got.mean["c0"][dead]).all() and not np.isfinite(got.log_evidence[dead]).any()
        assert np.isfinite(got.mean["c0"][:sf.PARTIAL_ALL_AT]).all()


def test_observe_first_row_is_the_third_observes():
    """the step's last OBSERVE is its third; the statements after it (a SAMPLE of x, an ASSIGN of m)
    are not in the row, so the row's mean of x is not the final column's"""
    c = sf.gen("observe_first", "directed")
    got, _ = run_pair(c.ssm, c.data, 1001, 0.5, steps=c.T, what="observe_first")
    o = Oracle(1001, seed=sf.SEED)
    c.ssm.statements(o, c.data, ess_perc_min=0.5, T=c.T)
    final, _ = o.weighted_moments([abi.Operand.column(o.col_find("c0"))])
    o.close()
    assert got.mean["c0"][-1] != final[0]


def test_full_at_the_cap(cap, cases):
    c = cases["full"]
    run_pair(c.ssm, c.data, cap[4], 0.5, steps=c.T, what="full")


def test_prog97_takes_the_statement_route(cases):
    c = cases["prog97"]
    run_pair(c.ssm, c.data, 65, 0.5, steps=c.T, route="statements", what="prog97")


def test_statement_route_multinomial_and_foreign_column(cases):
    c = cases["observe_first"]
    run_pair(c.ssm, c.data, 65, 0.5, MULT, steps=c.T, route="statements", what="multinomial")
    run_pair(c.ssm, c.data, 65, 0.5, STRAT, steps=c.T, route="statements", foreign=True, what="foreign column")


@pytest.mark.parametrize("n", [65, 2049])
def test_negative_zero_column(n):
    """a column assigned -0.0 at every step: its expression 0.0 + 1.0 * x is +0.0, so are the products
    and the sums; the row's zeros carry the oracle's signs"""
    data = np.round(np.random.default_rng(5).normal(0.0, 1.0, T), 3)
    normal = lambda mu, sc: sf.DistD(abi.FAM_NORMAL, mu, K(sc))
    c = sf.Case("negzero", 2, [S(0, normal(K(0.0), 1.0))],
                [S(0, normal(K(0.0, col(0, 0.9)), 0.5)), A(1, K(-0.0)), O(K(0.0, dat(0)), normal(K(0.0, col(0)), 1.0))],
                1, data, T, ["real", "real"])
    got, want = run_pair(c.ssm, c.data, n, 0.5, steps=c.T, what="negzero")
    o = Oracle(n, seed=sf.SEED)
    c.ssm.statements(o, c.data, ess_perc_min=0.5, T=c.T)
    assert np.signbit(o.col_download(o.col_find("c1"))).all()   # the column does hold -0.0
    o.close()
    assert (want.mean["c1"] == 0.0).all() and (want.var["c1"] == 0.0).all()
    assert tb.bits_equal(got.mean["c1"], want.mean["c1"]).all() and tb.bits_equal(got.var["c1"], want.var["c1"]).all()


# ---- 3. the trace changes nothing else, and its parts do not depend on one another ----------------
@pytest.mark.parametrize("name, n", [("sv", 1001), ("kitagawa", 2049), ("poisson_count", 65)])
def test_trace_on_and_off(name, n):
    ssm, data = SPECS[name]
    o = Oracle(n, seed=7)
    _, etr = ssm.statements(o, data, ess_perc_min=0.5)
    out = []
    for trace in (False, True):
        g = wsmc.Context(n, seed=7)
        g.set_ssm_segment(5)
        if trace:
            ev, tr = g.ssm_run(ssm, data, ess_perc_min=0.5, trace=True)
            ess = tr.ess
        else:
            ev, ess = g.ssm_run(ssm, data, ess_perc_min=0.5, ess_trace=True)
        d = sf.compare(g, o, ev, ess, etr)
        assert d is None, f"trace={trace}: {d}"
        out.append((ev, ess, g.weights_download(), g.last_ancestors(), g.get_state(),
                    [g.col_download(g.col_find(c)) for c in ssm.cols]))
        assert g.ssm_stats()["persistent_runs"] == 1 and g.ssm_stats()["segments"] == -(-T // 5)
        g.close()
    o.close()
    a, b = out
    assert tb.bits_equal(a[0], b[0]).all() and tb.bits_equal(a[1], b[1]).all() and tb.bits_equal(a[2], b[2]).all()
    assert (a[3] == b[3]).all() and a[4] == b[4]
    assert all(tb.bits_equal(x, y).all() for x, y in zip(a[5], b[5]))


@pytest.mark.parametrize("parts", [("mean",), ("log_evidence",), ("var",), ("ess", "var")])
def test_a_part_of_the_trace_alone(parts):
    ssm, data = SPECS["local_trend"]
    full, want = run_pair(ssm, data, 2049, 0.5, SYST, 5, what="full")
    got, _ = run_pair(ssm, data, 2049, 0.5, SYST, 5, trace=parts, what=str(parts))
    for p in ("ess", "mean", "var", "log_evidence"):
        assert (getattr(got, p) is not None) == (p in parts), p
    assert rows_differ(got, full) is None


def test_null_trace_is_the_untraced_run():
    """wsmc_ssm_run_traced with a NULL trace, and with every member NULL"""
    ssm, data = SPECS["sv"]
    tab = ssm.table(data)
    o = Oracle(1001, seed=3)
    ssm.statements(o, data, ess_perc_min=0.5, wait=False)
    for tr in (None, abi.SsmTraceOut()):
        g = wsmc.Context(1001, seed=3)
        ev = C.c_double()
        abi.check(g._L.wsmc_ssm_run_traced(g._h, C.byref(ssm.spec), tab.ctypes.data_as(C.POINTER(C.c_double)), len(tab), 0.5,
                                           STRAT, C.byref(ev), None if tr is None else C.byref(tr)))
        d = sf.compare(g, o, ev.value)
        assert d is None, d
        assert g.ssm_stats()["persistent_runs"] == 1
        g.close()
    o.close()


# ---- 4. the batch: every filter against its own oracle ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_trace(key, n, seed, ess, scheme, steps):
    ssm, data = BATCH_SPECS[key]
    o = Oracle(n, seed=seed)
    try:
        return ssm.statements(o, data, ess_perc_min=ess, scheme=scheme, T=steps, trace=True)[2]
    finally:
        o.close()


BATCH_SPECS = {}


def batch_ref(ssm, data, n, seed, ess, scheme=STRAT, steps=None):
    """(the untraced batch file's reference of the final state, the oracle's trace), computed once"""
    key = (id(ssm), None if data is None else np.asarray(data).tobytes())
    BATCH_SPECS.setdefault(key, (ssm, data))
    return _final_ref(key, n, seed, ess, scheme, steps), _oracle_trace(key, n, seed, ess, scheme, steps)


@functools.lru_cache(maxsize=None)
def _final_ref(key, n, seed, ess, scheme, steps):
    ssm, data = BATCH_SPECS[key]
    return tb.reference(ssm, data, n, seed, ess, scheme, steps)


def batch_trace(res, b, cols):
    return wsmc.SsmTrace(res.ess[b], {c: res.mean[c][b] for c in cols}, {c: res.var[c][b] for c in cols},
                         res.log_evidence_trace[b])


def check_batch(res, b, ssm, data, n, seed, ess, scheme=STRAT, steps=None, what=""):
    ref, want = batch_ref(ssm, data, n, seed, ess, scheme, steps)
    tb.check_filter(res, b, ref, what)
    d = rows_differ(batch_trace(res, b, ssm.cols), want, f"{what} filter b={b} n={n}")
    assert d is None, d


def run_batch(g, specs, data, n, seeds, ess, scheme=STRAT, steps=None):
    return g.ssm_run_batch(specs, data, n, seeds, ess_perc_min=ess, scheme=scheme, state=True, T=steps, trace=True)


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("name", sorted(models.SSM_MODELS))
def test_batch_of_one_is_the_traced_single_run(ctx, name, ess):
    ssm, data = SPECS[name]
    res = run_batch(ctx, ssm, data, 1000, [42], ess)
    check_batch(res, 0, ssm, data, 1000, 42, ess, what=name)
    g = wsmc.Context(1000, seed=42)
    ev, tr = g.ssm_run(ssm, data, ess_perc_min=ess, trace=True)
    g.close()
    assert tb.bits_equal(ev, res.log_evidence[0]).all()
    assert rows_differ(batch_trace(res, 0, ssm.cols), tr, name) is None


@pytest.mark.parametrize("scheme", [STRAT, SYST])
@pytest.mark.parametrize("ess", [0.5, 1.0])
@pytest.mark.parametrize("n", [1, 65, 1001, 2049])
def test_batch_per_filter_parameters_and_seeds(ctx, n, ess, scheme):
    try:
        for segment in (1, 5, 0):
            ctx.set_ssm_batch_segment(segment)
            res = run_batch(ctx, tb.SV_SPECS, tb.SV_DATA, n, tb.SV_SEEDS, ess, scheme)
            assert ctx.ssm_batch_stats()["segments"] == (-(-T // segment) if segment else 1)
            for b in range(5):
                check_batch(res, b, tb.SV_SPECS[b], tb.SV_DATA, n, tb.SV_SEEDS[b], ess, scheme, what=f"segment {segment}")
    finally:
        ctx.set_ssm_batch_segment(0)
    assert len({float(res.mean["h"][b][-1]) for b in range(5)}) == 5   # the filters do differ


def test_batch_more_filters_than_resident_blocks(ctx):
    cus = ctx.ssm_batch_stats()["cus"]
    assert cus >= 1
    n, B, steps = 65, 2 * cus + 3, 6
    ssm, data = models.local_trend(), models.local_trend_data(steps)
    res = run_batch(ctx, ssm, data, n, list(range(B)), 0.5)
    assert res.mean["x"].shape == (B, steps) and res.log_evidence_trace.shape == (B, steps)
    for b in range(B):
        check_batch(res, b, ssm, data, n, b, 0.5, what="many")


def test_batch_a_dying_filter_between_two_healthy_ones(ctx):
    case = sf.gen("partial_support", "directed")
    healthy = case.data.copy()
    healthy[sf.PARTIAL_ALL_AT] = 0.5
    tables, seeds = [healthy, case.data, healthy.copy()], [5, 6, 7]
    res = run_batch(ctx, case.ssm, tables, 1001, seeds, 1.0, steps=case.T)
    for b in range(3):
        check_batch(res, b, case.ssm, tables[b], 1001, seeds[b], 1.0, steps=case.T, what="dying")
    dead = slice(sf.PARTIAL_ALL_AT, None)
    assert np.isnan(res.mean["c0"][1][dead]).all() and np.isfinite(res.mean["c0"][1][:sf.PARTIAL_ALL_AT]).all()
    assert not np.isfinite(res.log_evidence_trace[1][dead]).any()
    for b in (0, 2):
        assert np.isfinite(res.mean["c0"][b]).all() and np.isfinite(res.var["c0"][b]).all()
        assert np.isfinite(res.log_evidence_trace[b]).all()


def test_batch_per_filter_tables(ctx):
    n, ess = 1001, 0.5
    ssm, seeds = models.local_trend(), [3, 4, 5, 6]
    y = models.local_trend_data(T)
    tables = [y, models.local_trend_data(T, seed=9), y.copy(), y[::-1].copy()]
    res = run_batch(ctx, ssm, tables, n, seeds, ess)
    for b in range(4):
        check_batch(res, b, ssm, tables[b], n, seeds[b], ess, what="tables")
    assert not tb.bits_equal(res.mean["x"][0], res.mean["x"][1]).all()


def test_batch_log_gamma_and_ext_variants(ctx):
    pois = [models.poisson_count(a, s) for a, s in ((0.9, 0.3), (0.7, 0.5), (0.95, 0.1))]
    data = models.poisson_count_data(T)
    res = run_batch(ctx, pois, data, 1001, [1, 2, 3], 0.5)
    for b in range(3):
        check_batch(res, b, pois[b], data, 1001, b + 1, 0.5, what="poisson_count")
    mk = lambda a, th, sg: (SSM(cols=["x"])
                            .init(sample("x", dsl.Laplace(0.0, 1.0)))
                            .step(sample("x", dsl.Laplace(Col("x") * a, th)),
                                  observe(Data(0), dsl.Cauchy(Col("x"), sg))))
    ext = [mk(0.9, 0.5, 0.7), mk(0.5, 1.0, 0.2), mk(0.99, 0.1, 2.0)]
    data = models.lgssm1d_data(T)
    res = run_batch(ctx, ext, data, 1001, [1, 2, 3], 1.0)
    for b in range(3):
        check_batch(res, b, ext[b], data, 1001, b + 1, 1.0, what="ext")


def test_batch_ess_goes_to_both_buffers(ctx):
    ssm, data = SPECS["sv"]
    res = ctx.ssm_run_batch(ssm, data, 65, [1, 2], ess_perc_min=0.5, ess_trace=True, trace=True)
    plain = ctx.ssm_run_batch(ssm, data, 65, [1, 2], ess_perc_min=0.5, ess_trace=True)
    assert tb.bits_equal(res.ess, plain.ess).all() and tb.bits_equal(res.log_evidence, plain.log_evidence).all()
    assert plain.mean is None and plain.log_evidence_trace is None


def _raw(g, specs, n_specs, tab, n_tables, steps, n, B, seeds, ess=0.5, scheme=STRAT, out=True):
    """wsmc_ssm_run_batch_traced with a full trace: (return code, message)"""
    arr = (abi.SsmSpec * len(specs))()
    for k, s in enumerate(specs):
        C.memmove(C.byref(arr[k]), C.byref(s.spec), C.sizeof(abi.SsmSpec))
    sd = (C.c_uint64 * max(1, len(seeds)))(*seeds) if seeds is not None else None
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    o, tr = abi.SsmBatchOut(), abi.SsmTraceOut()
    rows, s_cols = max(B, 1) * max(steps, 1), len(specs[0].cols)
    bufs = [np.empty(max(B, 1)), np.empty(rows), np.empty(rows * s_cols), np.empty(rows * s_cols), np.empty(rows)]
    o.log_evidence, tr.ess, tr.mean, tr.var, tr.log_evidence = (dp(a) for a in bufs)
    t = None if tab is None else np.ascontiguousarray(tab, dtype=np.float64)
    rc = g._L.wsmc_ssm_run_batch_traced(g._h, arr, n_specs, None if t is None else dp(t), n_tables, steps, n, B, sd, ess,
                                        scheme, C.byref(o) if out else None, C.byref(tr))
    return rc, g._L.wsmc_last_error().decode()


def test_batch_refusals_are_unchanged(ctx, cap):
    sv, y = SPECS["sv"]
    big = sf.gen("prog97", "directed")
    bad = SSM.from_spec(type(sv.spec).from_buffer_copy(bytes(sv.spec)))
    bad.spec.step[0].dist.family = 15   # the reserved family: wsmc_ssm_spec_check refuses it
    other = models.local_trend()
    refusals = [
        ("above the cap", lambda: _raw(ctx, [sv], 1, y, 1, T, cap[2] + 1, 2, [1, 2]), "cap"),
        ("multinomial", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, [1, 2], scheme=MULT), "multinomial"),
        ("unknown scheme", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, [1, 2], scheme=7), "scheme"),
        ("97 instructions", lambda: _raw(ctx, [big.ssm], 1, big.data, 1, big.T, 65, 2, [1, 2]), "program instructions"),
        ("B < 1", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 0, [1]), "B < 1"),
        ("T < 1", lambda: _raw(ctx, [sv], 1, y, 1, 0, 100, 2, [1, 2]), "T < 1"),
        ("n < 1", lambda: _raw(ctx, [sv], 1, y, 1, T, 0, 2, [1, 2]), "n < 1"),
        ("n_specs", lambda: _raw(ctx, [sv, sv], 2, y, 1, T, 100, 3, [1, 2, 3]), "n_specs"),
        ("n_tables", lambda: _raw(ctx, [sv], 1, np.concatenate([y, y]), 2, T, 100, 3, [1, 2, 3]), "n_tables"),
        ("null seeds", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, None), "seeds"),
        ("null out", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, [1, 2], out=False), "out"),
        ("null data", lambda: _raw(ctx, [sv], 1, None, 1, T, 100, 2, [1, 2]), "data"),
        ("a refused spec", lambda: _raw(ctx, [sv, sv, bad], 3, y, 1, T, 100, 3, [1, 2, 3]), "spec 2"),
        ("another shape", lambda: _raw(ctx, [sv, other], 2, y, 1, T, 100, 2, [1, 2]), "spec 1 differs from spec 0 in shape"),
    ]
    for what, call, word in refusals:
        rc, msg = call()
        assert rc == abi.WSMC_EARG, (what, rc, msg)
        assert word in msg, (what, msg)
    m = wsmc.Context.multi(128, 2, seed=1, devices=[0, 0], transport=abi.TRANSPORT_HOST)
    rc, msg = _raw(m, [sv], 1, y, 1, T, 100, 2, [1, 2])
    assert rc == abi.WSMC_EARG and "multi-device" in msg, msg
    m.close()
    res = run_batch(ctx, sv, y, 65, [1, 2], 0.5)   # afterwards the context still runs a traced batch
    for b in range(2):
        check_batch(res, b, sv, y, 65, b + 1, 0.5, what="after the refusals")

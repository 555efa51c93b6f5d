"""Backward simulation on the device (wsmc_ssm_backward, wsmc_ssm_run_backward;
csrc/wsmc_ssm_backward.hip). Every comparison is bit for bit, NaNs by position and -0.0 apart from
0.0, with the definition run on the CPU oracle: `spec.backward_definition(Oracle, record, data, M,
seed)` over the record of `spec.statements(Oracle(n, seed), data, record=True)`.

The sizes are where the workgroup's layout changes: N = 1, 65 (one particle in the second wave),
1001 (sixteen waves, one particle a thread) and 5120 (five a thread: the cap); T = 1 (the draw from
the last weights alone), 2 and 7; M = 1, 3, 64 and 130 (a third canonical wave of the moments).

Not covered: WSMC_FAM_UNIFORM as an included SAMPLE term. Its bounds are the dist's constants, so
no operand of it can read a column and the rule never includes it; it is here as an OBSERVE term.
"""
import ctypes as C

import numpy as np
import pytest

import ssmfuzz as sf
import test_gpu_ssm_batch as tb     # bits_equal
import test_gpu_ssm_trace as tt     # the filter trace's comparison
import wsmc
from oracle import Oracle
from ssmfuzz import K, O, S, col, dat
from wsmc import Col, Normal, abi, dsl, models
from wsmc.dsl import Data
from wsmc.ssm import SSM, SsmRecord, assign, observe, sample, weight

pytestmark = pytest.mark.gpu

STRAT, SYST, MULT = abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL
SHIPPED = {"lgssm1d_spec": (models.lgssm1d_spec, models.lgssm1d_data), "sv": (models.sv, models.sv_data),
           "poisson_count": (models.poisson_count, models.poisson_count_data), "kitagawa": (models.kitagawa, models.kitagawa_data),
           "local_trend": (models.local_trend, models.local_trend_data), "lgssm1d_guided": (models.lgssm1d_guided, models.lgssm1d_data)}


@pytest.fixture(scope="module")
def ctx(gpu_available):
    g = wsmc.Context(16, seed=1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cap(ctx):
    return ctx.ssm_stats()["cap"]


def backward_differ(got, want, what=""):
    """None, or the first difference of two SsmBackward"""
    if got.idx.shape != want.idx.shape or got.idx.dtype != np.int32:
        return f"{what}: idx {got.idx.dtype}{got.idx.shape} != int32{want.idx.shape}"
    if (got.idx != want.idx).any():
        at = tuple(int(v) for v in np.argwhere(got.idx != want.idx)[-1])   # the last: the pass runs backwards
        return f"{what}: idx differs (going backwards) first at {at} (step, trajectory): {got.idx[at]} != the oracle's {want.idx[at]}"
    for kind, a, b in (("paths", got.paths, want.paths), ("mean", got.mean, want.mean), ("var", got.var, want.var)):
        assert list(a) == list(b), (list(a), list(b))
        for c in b:
            x, y = np.asarray(a[c]), np.asarray(b[c])
            if x.shape != y.shape:
                return f"{what}: {kind}[{c}]: shape {x.shape} != {y.shape}"
            ok = tb.bits_equal(x, y)
            if not ok.all():
                at = tuple(int(v) for v in np.argwhere(~ok)[0])
                return f"{what}: {kind}[{c}] differs first at {at}: {x[at]!r} != the oracle's {y[at]!r}"
    return None


def oracle_record(ssm, data, n, seed=sf.SEED, ess=0.5, scheme=STRAT, steps=None, trace=False):
    o = Oracle(n, seed=seed)
    try:
        r = ssm.statements(o, data, ess_perc_min=ess, scheme=scheme, T=steps, trace=trace, record=True)
        return (r[2], r[3]) if trace else r[2]
    finally:
        o.close()


def check_pass(ctx, ssm, data, rec, M, seed, what):
    want = ssm.backward_definition(Oracle, rec, data, M, seed)
    got = ctx.ssm_backward(ssm, data, rec, M, seed)
    d = backward_differ(got, want, what)
    assert d is None, d
    return got


# ---- 1. the stand-alone pass over the oracle's record ---------------------------------------------
PASS_CASES = [("lgssm1d_spec", 1, 7, 3), ("lgssm1d_spec", 5120, 2, 130), ("lgssm1d_spec", 65, 1, 64),
              ("sv", 65, 7, 64), ("sv", 1001, 2, 1),
              ("poisson_count", 1001, 7, 3), ("poisson_count", 65, 2, 130),
              ("kitagawa", 65, 7, 3), ("kitagawa", 5120, 2, 1),
              ("local_trend", 1001, 7, 64), ("local_trend", 1, 1, 1),
              ("lgssm1d_guided", 65, 7, 130), ("lgssm1d_guided", 1001, 2, 3), ("lgssm1d_guided", 5120, 1, 3)]


@pytest.mark.parametrize("name, n, steps, M", PASS_CASES, ids=["-".join(map(str, c)) for c in PASS_CASES])
def test_pass_over_the_oracles_record(ctx, name, n, steps, M):
    make, gen = SHIPPED[name]
    ssm, data = make(), gen(steps)
    rec = oracle_record(ssm, data, n)
    before = repr(ctx.get_state())   # (repr: a fresh context's last ESS% is NaN)
    got = check_pass(ctx, ssm, data, rec, M, 1234 + n, f"{name} N={n} T={steps} M={M}")
    assert (got.idx >= 0).all() and (got.idx < n).all()
    assert all(np.isfinite(v).all() for v in list(got.mean.values()) + list(got.var.values()))
    assert repr(ctx.get_state()) == before and ctx.col_names() == []   # the context gives the device and the stream only
    st = ctx.ssm_backward_stats()
    assert st["segments_s"] == 0.0 and st["bytes"] >= 8 * steps * n * (len(ssm.cols) + 1)


# ---- 2. directed inputs ------------------------------------------------------------------------------
N, STEPS, M = 65, 4, 6


@pytest.fixture(scope="module")
def base():
    ssm, data = models.lgssm1d_spec(), models.lgssm1d_data(STEPS)
    return ssm, data, oracle_record(ssm, data, N)


def test_equal_particles(ctx, base):
    """particles equal in pairs, columns and weights: the integer weights tie, and the first index whose
    running sum exceeds the target wins, as in the oracle"""
    ssm, data, rec = base
    cols, lw = rec.cols.copy(), rec.log_weights.copy()
    cols[:, :, 1::2], lw[:, 1::2] = cols[:, :, 0:-1:2], lw[:, 0:-1:2]
    check_pass(ctx, ssm, data, SsmRecord(cols, lw), M, 5, "pairs")
    cols[:], lw[:] = 0.25, -1.0   # every particle the same: the draw is the target's position alone
    got = check_pass(ctx, ssm, data, SsmRecord(cols, lw), M, 5, "all equal")
    assert len(np.unique(got.idx)) > 1


@pytest.mark.parametrize("where", ["prefix", "suffix", "one"])
def test_inf_weights(ctx, base, where):
    ssm, data, rec = base
    lw = rec.log_weights.copy()
    if where == "prefix":
        lw[:, :40] = -np.inf
    elif where == "suffix":
        lw[:, 20:] = -np.inf
    else:
        lw[:] = -np.inf
        lw[np.arange(STEPS), [64, 0, 33, 7]] = -3.5   # one particle a step has any weight
    got = check_pass(ctx, ssm, data, SsmRecord(rec.cols, lw), M, 6, where)
    if where == "prefix":
        assert (got.idx >= 40).all()
    elif where == "suffix":
        assert (got.idx < 20).all()
    else:
        assert (got.idx == np.array([64, 0, 33, 7])[:, None]).all()


def test_nan_weights_are_estate(ctx, base):
    ssm, data, rec = base
    lw = rec.log_weights.copy()
    lw[1] = np.nan
    bad = SsmRecord(rec.cols, lw)
    with pytest.raises(abi.WSMCError) as e:
        ssm.backward_definition(Oracle, bad, data, M, 7)
    assert e.value.code == abi.WSMC_ESTATE
    with pytest.raises(abi.WSMCError) as e:
        ctx.ssm_backward(ssm, data, bad, M, 7)
    assert e.value.code == abi.WSMC_ESTATE
    check_pass(ctx, ssm, data, rec, M, 7, "after ESTATE")   # the context serves the next call


def test_nan_data_row(ctx, base):
    """a NaN data row where no included term reads it changes nothing; where one does (kitagawa's
    covariate enters m, which the transition reads) every weight is NaN: WSMC_ESTATE from both"""
    ssm, data, rec = base
    nan = data.copy()
    nan[2] = np.nan
    want = ssm.backward_definition(Oracle, rec, data, M, 8)
    got = ctx.ssm_backward(ssm, nan, rec, M, 8)
    d = backward_differ(got, want, "unread NaN")
    assert d is None, d
    kit, kd = models.kitagawa(), models.kitagawa_data(STEPS)
    krec = oracle_record(kit, kd, N)
    kd = kd.copy()
    kd[2] = np.nan
    for run in (lambda: kit.backward_definition(Oracle, krec, kd, M, 8), lambda: ctx.ssm_backward(kit, kd, krec, M, 8)):
        with pytest.raises(abi.WSMCError) as e:
            run()
        assert e.value.code == abi.WSMC_ESTATE


# ---- 3. every kind of term ---------------------------------------------------------------------------
def test_observe_and_weight_terms(ctx):
    x = Col("x")
    data = models.lgssm1d_data(5)
    two = (SSM(cols=["x"]).init(sample("x", Normal(0.0, 1.0)))
           .step(observe(Data(0), Normal(x, 2.0)), sample("x", Normal(x * 0.9, 1.0)), weight(x, Normal(0.0, 3.0)),
                 observe(Data(0), Normal(x, 0.5))))
    assert two.backward_terms() == [0, 1]
    check_pass(ctx, two, data, oracle_record(two, data, 65), 3, 11, "two observes")
    aux = (SSM(cols=["x", "p"]).init(sample("x", Normal(0.0, 1.0)))
           .step(assign("p", x * 0.5), sample("x", Normal(x * 0.9, 1.0)), weight(Col("p"), Normal(x, 1.0)),
                 observe(Data(0), Normal(x, 0.5))))
    assert aux.backward_terms() == [1, 2]
    check_pass(ctx, aux, data, oracle_record(aux, data, 1001), 3, 12, "a WEIGHT through an auxiliary column")
    prog = (SSM(cols=["x", "m", "s"]).init(sample("x", Normal(0.0, 1.0)))   # programs on both sides of the SAMPLE
            .step(assign("m", dsl.sin(x) + x / 2 + Data(0) * 0.1), sample("x", Normal(Col("m"), 1.0)),
                  assign("s", dsl.exp(x / 4)), observe(Data(0), Normal(x, Col("s")))))
    assert prog.backward_terms() == [1]
    check_pass(ctx, prog, data, oracle_record(prog, data, 65), 3, 13, "programs")


def family_case(fam, steps=4):
    """columns u (c0, in (0, 1)) and x (c1): step: v => F(u); x ~ F(u); u ~ Uniform; y => Normal(u, 0.5). The
    first OBSERVE and the SAMPLE of family F read the old u, so both terms are included. F's
    parameters by ssmfuzz's recipes for their kinds, so every particle stays in F's support"""
    rng = np.random.default_rng([fam, 99])
    mean_kind, scale_kind, value_kind = sf._FAM[fam][:3]

    def param(kind, default):
        if kind is None:
            return K(default)
        w = sf._WANT[kind]
        if "prob" in w["pool"]:
            return K(w["c0"](rng), col(0, w["pool"]["prob"][0]))
        return K(w["alone"](rng))

    if fam == abi.FAM_UNIFORM:   # constant bounds: the observed value reads u
        d = sf.DistD(fam, params=(-4.0, 4.0))
        value = K(sf._WANT["vreal"]["alone"](rng) / 2, col(0, 1.0))
    else:
        d = sf.DistD(fam, param(mean_kind, 0.0), param(scale_kind, 1.0))
        value = K(1.0 if fam == abi.FAM_BINOMIAL else sf._WANT[sf._VALUE_WANT[value_kind]]["alone"](rng))
    unit = sf.DistD(abi.FAM_UNIFORM, params=(0.05, 0.95))
    step = [O(value, d), S(1, d), S(0, unit), O(K(0.0, dat(0)), sf.DistD(abi.FAM_NORMAL, K(0.0, col(0, 1.0)), K(0.5)))]
    data = rng.uniform(0.0, 1.0, size=steps)
    return sf.Case(f"family-{fam}", 2, [S(0, unit)], step, data_dim=1, data=data, T=steps)


@pytest.mark.parametrize("fam", sf.SCALAR_FAMILIES, ids=[sf.FAMILIES[f] for f in sf.SCALAR_FAMILIES])
def test_every_family_as_a_term(ctx, fam):
    case = family_case(fam)
    want = [0] if fam == abi.FAM_UNIFORM else [0, 1]
    assert case.ssm.backward_terms() == want
    rec = oracle_record(case.ssm, case.data, 65, steps=case.T)
    assert np.isfinite(rec.log_weights).any(axis=1).all(), "the family's case lost every weight"
    got = check_pass(ctx, case.ssm, case.data, rec, 3, 40 + fam, sf.FAMILIES[fam])
    assert np.isfinite(got.mean["c0"]).all()


# ---- 4. the fused call -------------------------------------------------------------------------------
def four_columns():
    a, b, c = Col("a"), Col("b"), Col("c")
    return (SSM(cols=["a", "b", "c", "d"]).init(sample("a", Normal(0.0, 1.0)), sample("b", Normal(0.0, 1.0)))
            .step(sample("a", Normal(a * 0.9, 0.5)), sample("b", Normal(b * 0.5 + a * 0.3, 0.7)), assign("c", a + b),
                  assign("d", dsl.exp(c / 4)), observe(Data(0), Normal(c, 1.0))))


def run_fused(ssm, data, n, M, ess=0.5, scheme=STRAT, segment=None, seed=sf.SEED, bseed=321, what=""):
    """ssm_run(backward=M) on a fresh context: its record against the oracle's, its outputs against the
    definition, and everything it leaves against ssm_run(trace=True) on an identical context and
    against the plain statements on a fresh oracle"""
    g, h, o = wsmc.Context(n, seed=seed), wsmc.Context(n, seed=seed), Oracle(n, seed=seed)
    try:
        for c in (g, h):
            if segment is not None:
                c.set_ssm_segment(segment)
        ev, tr, bw = g.ssm_run(ssm, data, ess_perc_min=ess, scheme=scheme, trace=True, backward=M, backward_seed=bseed, record=True)
        ev_h, tr_h = h.ssm_run(ssm, data, ess_perc_min=ess, scheme=scheme, trace=True)
        _, etr = ssm.statements(o, data, ess_perc_min=ess, scheme=scheme)
        wtr, rec = oracle_record(ssm, data, n, seed, ess, scheme, trace=True)
        tag = f"{what} N={n} M={M} ess={ess} scheme={scheme} segment={segment}"
        assert tb.bits_equal(bw.record.cols, rec.cols).all(), f"{tag}: the record's columns"
        assert tb.bits_equal(bw.record.log_weights, rec.log_weights).all(), f"{tag}: the record's log-weights"
        d = backward_differ(bw, ssm.backward_definition(Oracle, rec, data, M, bseed), tag)
        assert d is None, d
        d = tt.rows_differ(tr, wtr, tag)
        assert d is None, d
        for other, e in ((o, ev), (h, ev)):
            d = sf.compare(g, other, e, tr.ess, etr)
            assert d is None, f"{tag}: {d}"
        assert sf.same_value(ev, ev_h) and tt.rows_differ(tr, tr_h, tag) is None
        sg, sh = g.ssm_stats(), h.ssm_stats()
        assert (sg["persistent_runs"], sg["statement_runs"], sg["segments"]) == (1, 0, sh["segments"]), f"{tag}: {sg}"
        assert (g.sample_particles(9) == h.sample_particles(9)).all()   # the backward pass drew from its own seed
        st = g.ssm_backward_stats()
        assert st["bytes"] >= 8 * len(data) * n * (len(ssm.cols) + 1) and h.ssm_backward_stats()["bytes"] == 0
        # every segment of the backward run went to the recording kernels, none of the traced run's did
        assert st["recording_segments"] == sg["segments"] and h.ssm_backward_stats()["recording_segments"] == 0
        return bw
    finally:
        g.close()
        h.close()
        o.close()


FUSED = [("lgssm1d_spec", 1001, 7, None), ("sv", 65, 3, 3), ("kitagawa", 1001, 64, 3), ("poisson_count", 257, 3, None),
         ("local_trend", 65, 130, 1), ("lgssm1d_guided", 1001, 3, 3), ("lgssm1d_guided", 65, 64, None)]


@pytest.mark.parametrize("name, n, M, segment", FUSED, ids=["-".join(map(str, c)) for c in FUSED])
def test_fused_run(name, n, M, segment):
    make, gen = SHIPPED[name]
    k = FUSED.index((name, n, M, segment))
    run_fused(make(), gen(7), n, M, ess=(0.5, 1.0, 0.0)[k % 3], scheme=(STRAT, SYST)[k % 2], segment=segment, what=name)


@pytest.mark.parametrize("S", [1, 4])
def test_fused_run_at_the_cap(cap, S):
    ssm = models.lgssm1d_spec() if S == 1 else four_columns()
    run_fused(ssm, models.lgssm1d_data(4), cap[S], 3, segment=3 if S == 4 else None, what=f"cap S={S}")


def test_fused_run_parts(ctx):
    """without the trace and without the record; the first trajectories are the draws"""
    ssm, data = models.sv(), models.sv_data(5)
    g = wsmc.Context(65, seed=3)
    try:
        ev, bw = g.ssm_run(ssm, data, ess_perc_min=0.5, backward=4, backward_seed=9)
        assert bw.record is None and np.isfinite(ev)
        rec = oracle_record(ssm, data, 65, seed=3)
        d = backward_differ(bw, ssm.backward_definition(Oracle, rec, data, 4, 9), "no trace")
        assert d is None, d
        assert all(tb.bits_equal(bw.draw(2)[c], bw.paths[c][:, :2].T).all() for c in ssm.cols)
    finally:
        g.close()


# ---- 4b. the batch ------------------------------------------------------------------------------------
def sv_set(k):
    return models.sv(mu=-1.0 + 0.3 * k, phi=0.95 - 0.05 * k, sigma=0.25 + 0.1 * k)


@pytest.mark.parametrize("which, n, M, segment", [("sv", 65, 5, None), ("sv", 1001, 64, 2), ("guided", 257, 3, None)])
def test_batch(ctx, which, n, M, segment):
    """B = 3 filters with distinct specs (of one shape), seeds and backward seeds: each is the single
    call on a fresh context, record, trace and outputs, and the lending context is not touched"""
    steps = 6
    if which == "sv":
        specs, data = [sv_set(k) for k in range(3)], models.sv_data(steps)
    else:
        specs, data = [models.lgssm1d_guided(a=0.9 - 0.1 * k, q=1.0 + 0.2 * k) for k in range(3)], models.lgssm1d_data(steps)
    seeds, bseeds = [11, 12, 13], [101, 202, 303]
    before = repr(ctx.get_state())
    launched = ctx.ssm_backward_stats()["recording_segments"]
    if segment is not None:
        ctx.set_ssm_batch_segment(segment)
    try:
        res = ctx.ssm_run_batch(specs, data, n, seeds, ess_perc_min=0.5, trace=True, state=True, backward=M, backward_seeds=bseeds,
                                record=True)
        nseg = ctx.ssm_batch_stats()["segments"]
    finally:
        ctx.set_ssm_batch_segment(0)
    assert repr(ctx.get_state()) == before and ctx.col_names() == []
    assert ctx.ssm_backward_stats()["recording_segments"] == launched + nseg
    assert len(res.backward) == 3
    for b in range(3):
        g = wsmc.Context(n, seed=seeds[b])
        try:
            ev, tr, bw = g.ssm_run(specs[b], data, ess_perc_min=0.5, trace=True, backward=M, backward_seed=bseeds[b], record=True)
            tag = f"{which} filter {b} N={n} M={M}"
            d = backward_differ(res.backward[b], bw, tag)
            assert d is None, d
            assert tb.bits_equal(res.backward[b].record.cols, bw.record.cols).all(), tag
            assert tb.bits_equal(res.backward[b].record.log_weights, bw.record.log_weights).all(), tag
            assert sf.same_value(res.log_evidence[b], ev) and sf.same_value(res.log_weights[b], g.weights_download()), tag
            for c in specs[b].cols:
                assert sf.same_value(res.cols[c][b], g.col_download(g.col_find(c))), (tag, c)
                assert sf.same_value(res.mean[c][b], tr.mean[c]) and sf.same_value(res.var[c][b], tr.var[c]), (tag, c)
            assert sf.same_value(res.ess[b], tr.ess)
        finally:
            g.close()
    # distinct filters and distinct backward seeds give distinct draws
    assert (res.backward[0].idx != res.backward[1].idx).any()


def test_batch_refusals(ctx):
    data = models.sv_data(4)
    x = Col("x")
    static = (SSM(cols=["a", "x"]).init(sample("a", Normal(0.9, 0.05)), sample("x", Normal(0.0, 1.0)))
              .step(sample("x", Normal(x * 0.5 + Col("a"), 1.0)), observe(Data(0), Normal(x, 0.5))))
    with pytest.raises(abi.WSMCError, match="spec 0: state column a"):
        ctx.ssm_run_batch(static, data, 65, [1, 2], backward=3, backward_seeds=[1, 2])
    with pytest.raises(abi.WSMCError, match="M = 100000"):
        ctx.ssm_run_batch(models.sv(), data, 65, [1, 2], backward=100000, backward_seeds=[1, 2])
    with pytest.raises(abi.WSMCError, match="multinomial"):
        ctx.ssm_run_batch(models.sv(), data, 65, [1, 2], scheme=MULT, backward=3, backward_seeds=[1, 2])
    with pytest.raises(ValueError, match="one backward seed per filter"):
        ctx.ssm_run_batch(models.sv(), data, 65, [1, 2], backward=3, backward_seeds=[1])


# ---- 5. refusals: the context is left as it was -------------------------------------------------------
def snapshot(g):
    return repr(g.get_state()), g.col_names(), g.weights_download().tobytes(), g.ssm_stats()["persistent_runs"], g.ssm_stats()["statement_runs"]


def test_refusals(cap):
    x = Col("x")
    ok, data = models.lgssm1d_spec(), models.lgssm1d_data(4)
    static = (SSM(cols=["a", "x"]).init(sample("a", Normal(0.9, 0.05)), sample("x", Normal(0.0, 1.0)))
              .step(sample("x", Normal(x * 0.5 + Col("a"), 1.0)), observe(Data(0), Normal(x, 0.5))))
    g = wsmc.Context(65, seed=2)
    big = wsmc.Context(cap[1] + 64, seed=2)
    try:
        for c, run, why in ((g, lambda c: c.ssm_run(static, data, backward=3), "state column a"),
                            (big, lambda c: c.ssm_run(ok, data, backward=3), "above the cap"),
                            (g, lambda c: c.ssm_run(ok, data, backward=cap[1] + 1), f"M = {cap[1] + 1}"),
                            (g, lambda c: c.ssm_run(ok, data, scheme=MULT, backward=3), "multinomial")):
            before = snapshot(c)
            with pytest.raises(abi.WSMCError) as e:
                run(c)
            assert e.value.code == abi.WSMC_EARG and why in str(e.value), str(e.value)
            assert snapshot(c) == before, why
        # M = 0 through the C entry point (the wrapper reads backward=0 as "no backward pass")
        with pytest.raises(ValueError, match="number of trajectories"):
            g.ssm_run(ok, data, backward=-1)
        out, ev = abi.SsmBackwardOut(), C.c_double()
        tab = ok.table(data)
        before = snapshot(g)
        rc = g._L.wsmc_ssm_run_backward(g._h, C.byref(ok.spec), tab.ctypes.data_as(C.POINTER(C.c_double)), len(tab), 1.0, STRAT,
                                        C.byref(ev), None, 0, 1, C.byref(out))
        assert rc == abi.WSMC_EARG and b"M = 0" in g._L.wsmc_last_error() and snapshot(g) == before
        # a column that is not the spec's
        g.assign(g.col_create("other", 1), [abi.Operand.const(0.3)])
        before = snapshot(g)
        with pytest.raises(abi.WSMCError) as e:
            g.ssm_run(ok, data, backward=3)
        assert e.value.code == abi.WSMC_EARG and "not the spec's" in str(e.value) and snapshot(g) == before
        # the stand-alone pass: n above its cap, M out of range
        rec = SsmRecord(np.zeros((2, 1, 5121)), np.zeros((2, 5121)))
        with pytest.raises(abi.WSMCError, match="5121 particles"):
            g.ssm_backward(ok, data[:2], rec, 3, 1)
        rec = SsmRecord(np.zeros((2, 1, 8)), np.zeros((2, 8)))
        for bad in (0, cap[1] + 1):
            with pytest.raises(abi.WSMCError, match=f"M = {bad}"):
                g.ssm_backward(ok, data[:2], rec, bad, 1)
        with pytest.raises(abi.WSMCError, match="state column a"):
            g.ssm_backward(static, data[:2], SsmRecord(np.zeros((2, 2, 8)), np.zeros((2, 8))), 3, 1)
        assert snapshot(g) == before
    finally:
        g.close()
        big.close()


# ---- 6. the other runs are what they were ------------------------------------------------------------
def test_other_runs_take_their_own_routes():
    """an untraced, a smoothed and a guided run after the feature: each the persistent route with its
    own statistics, none of them a backward pass and none of their segments launched on the
    backward-recording kernels (wsmc_debug_ssm_backward counts those launches), and bit for bit the
    statements; so is a batch of each"""
    data = models.lgssm1d_data(6)
    for ssm, kw in ((models.lgssm1d_spec(), {}), (models.lgssm1d_spec(), {"smooth": True}), (models.lgssm1d_guided(), {}),
                    (models.lgssm1d_guided(), {"smooth": True})):
        g, o = wsmc.Context(257, seed=4), Oracle(257, seed=4)
        try:
            r = g.ssm_run(ssm, data, ess_perc_min=0.5, **kw)
            ssm.statements(o, data, ess_perc_min=0.5)
            d = sf.compare(g, o, r[0] if kw else r)
            assert d is None, d
            st = g.ssm_stats()
            assert (st["persistent_runs"], st["statement_runs"], st["segments"]) == (1, 0, 1)
            assert g.ssm_backward_stats() == {"segments_s": 0.0, "backward_s": 0.0, "rows_s": 0.0, "bytes": 0, "recording_segments": 0}
            assert (g.ssm_smooth_stats()["log_bytes"] > 0) == bool(kw)
            g.ssm_run_batch(ssm, data, 65, [1, 2], **kw)
            assert g.ssm_backward_stats()["recording_segments"] == 0
        finally:
            g.close()
            o.close()

"""Conditional SMC on the device (wsmc_ssm_run_conditional; csrc/wsmc_ssm_batch_conditional.hip).
Every comparison is bit for bit, NaNs by position and -0.0 apart from 0.0, with the definition run
on the CPU oracle: `spec.conditional_definition(Oracle, data, n, seed, reference, ess)` and
`spec.backward_definition` over its record (tests/ssmcond.py `definition`).

The sizes are where the workgroup's layout changes: n = 1 (the reference particle alone), 2, 65
(one particle in the second wave), 1001 (sixteen waves) and the cap for 1 and 4 columns (several
particles a thread, the owner of particle n-1 the last thread with any); T = 1, 2, 7; segments of 1
and 2 steps, so the reference rows and the record cross launches.
"""
import ctypes as C

import numpy as np
import pytest

import ssmcond as sc
import ssmfuzz as sf
import wsmc
from wsmc import Col, Normal, abi, models
from wsmc.dsl import Data
from wsmc.ssm import SSM, observe, sample, weight

pytestmark = pytest.mark.gpu

SPECS = {name: (make, data) for name, (make, data, _) in sc.SHIPPED.items()}
SPECS["two_observes"] = (sc.two_observes, models.lgssm1d_data)
SPECS["chained_samples"] = (sc.chained_samples, models.lgssm1d_data)


@pytest.fixture(scope="module")
def ctx(gpu_available):
    g = wsmc.Context(16, seed=1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cap(ctx):
    return ctx.ssm_stats()["cap"]


def differ(res, b, want, cols, M, what):
    """None, or the first difference between filter b of a device result and the definition's
    (flags, ESS%, SsmTrace, SsmRecord, SsmFinal, SsmBackward or None)"""
    flags, ess, tr, rec, end, bw = want
    pairs = [("log_weights", res.log_weights[b], end.log_weights), ("last_ancestors", res.last_ancestors[b], end.last_ancestors),
             ("n_resamples", res.n_resamples[b], end.n_resamples), ("last_resampled", res.last_resampled[b], end.last_resampled),
             ("log_evidence", res.log_evidence[b], end.log_evidence), ("ess", res.ess[b], ess),
             ("log_evidence_trace", res.log_evidence_trace[b], tr.log_evidence)]
    for c in cols:
        pairs += [(f"cols[{c}]", res.cols[c][b], end.cols[c]), (f"mean[{c}]", res.mean[c][b], tr.mean[c]),
                  (f"var[{c}]", res.var[c][b], tr.var[c])]
    got_rec = res.backward[b].record if M else res.backward[b]
    pairs += [("record.cols", got_rec.cols, rec.cols), ("record.log_weights", got_rec.log_weights, rec.log_weights)]
    if M:
        g = res.backward[b]
        pairs.append(("idx", g.idx, bw.idx))
        for c in cols:
            pairs += [(f"paths[{c}]", g.paths[c], bw.paths[c]), (f"bmean[{c}]", g.mean[c], bw.mean[c]),
                      (f"bvar[{c}]", g.var[c], bw.var[c])]
    assert res.last_ancestors.dtype == np.int32
    for name, got, exp in pairs:
        if not sf.same_value(got, exp):
            return f"{what} filter {b}: {name}: {np.asarray(got)!r} != the definition's {np.asarray(exp)!r}"
    return None


def run_case(ctx, specs, tabs, n, seeds, refs, ess, M, segment, what):
    """the device call against the definition, filter by filter; returns the device result"""
    B = len(seeds)
    bseeds = [900 + 7 * b for b in range(B)]
    launched = ctx.ssm_conditional_stats()["conditional_segments"]
    before = repr(ctx.get_state())
    ctx.set_ssm_batch_segment(segment)
    try:
        res = ctx.ssm_run_conditional(specs if len(specs) > 1 else specs[0], tabs if len(tabs) > 1 else tabs[0], n, seeds, refs,
                                      ess_perc_min=ess, trace=True, backward=M, backward_seeds=bseeds if M else None, record=True,
                                      state=True)
        nseg = ctx.ssm_batch_stats()["segments"]
    finally:
        ctx.set_ssm_batch_segment(0)
    st = ctx.ssm_conditional_stats()
    assert st["conditional_segments"] == launched + nseg and st["bytes"] > 0
    assert repr(ctx.get_state()) == before and ctx.col_names() == []
    if segment:
        assert nseg == -(-len(tabs[0]) // segment)
    for b in range(B):
        spec, tab = specs[b % len(specs)], tabs[b % len(tabs)]
        want = sc.definition(spec, tab, n, seeds[b], refs[b], ess, M, bseeds[b], trace=True)
        d = differ(res, b, want, spec.cols, M, what)
        assert d is None, d
    return res


# (spec, n, T, B, M, ess, segment): B = 3 has distinct seeds, references and tables; n_specs is B for sv
CASES = [
    ("lgssm1d_spec", 1, 1, 1, 1, 2.0, 0), ("lgssm1d_spec", 1, 7, 1, 3, 0.5, 2), ("lgssm1d_spec", 2, 2, 1, 1, 2.0, 1),
    ("lgssm1d_spec", 2, 7, 3, 0, 0.5, 0), ("lgssm1d_spec", 65, 1, 3, 3, 2.0, 0), ("lgssm1d_spec", 65, 7, 1, 1, 0.0, 2),
    ("lgssm1d_spec", 1001, 2, 1, 0, 2.0, 1), ("lgssm1d_spec", 1001, 7, 3, 1, 0.5, 2),
    ("sv", 65, 7, 3, 3, 0.5, 1), ("sv", 1001, 7, 1, 1, 2.0, 0), ("poisson_count", 65, 7, 1, 1, 0.5, 0),
    ("poisson_count", 1001, 2, 3, 0, 2.0, 0), ("kitagawa", 2, 7, 1, 3, 2.0, 1), ("kitagawa", 1001, 7, 1, 1, 0.5, 0),
    ("local_trend", 65, 7, 3, 1, 2.0, 2), ("local_trend", 1001, 2, 1, 3, 0.5, 0),
    ("two_observes", 65, 7, 1, 3, 2.0, 1), ("two_observes", 1001, 7, 3, 1, 0.5, 0),
    ("chained_samples", 2, 7, 1, 1, 2.0, 0), ("chained_samples", 65, 2, 3, 3, 0.5, 1), ("chained_samples", 1001, 7, 1, 0, 2.0, 2),
]


def case_arguments(name, n, T, B):
    make, make_data = SPECS[name]
    if name == "sv" and B > 1:   # n_specs = B: specs of one shape whose numbers differ
        specs = [models.sv(mu=-1.0 + 0.3 * k, phi=0.95 - 0.05 * k, sigma=0.25 + 0.1 * k) for k in range(B)]
    else:
        specs = [make()]
    if name == "kitagawa":
        tabs = [specs[0].table(make_data(T)) for _ in range(1)]
    else:
        tabs = [specs[0].table(make_data(T, seed=40 + b)) for b in range(B)]
    seeds = [11, 2**63 + 5, 0][:B]
    refs = sc.reference(specs[0], T, 1000 + n + T, B=B)
    return specs, tabs, seeds, refs


@pytest.mark.parametrize("name, n, T, B, M, ess, segment", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_against_the_definition(ctx, name, n, T, B, M, ess, segment):
    specs, tabs, seeds, refs = case_arguments(name, n, T, B)
    res = run_case(ctx, specs, tabs, n, seeds, refs, ess, M, segment, f"{name} n={n} T={T}")
    if ess == 2.0:
        assert (res.n_resamples == T * (2 if name == "two_observes" else 1)).all()
        assert (res.last_ancestors[:, n - 1] == n - 1).all()
    if ess == 0.0:
        assert not res.n_resamples.any() and not res.last_ancestors.any()


@pytest.mark.parametrize("S", [1, 4])
def test_at_the_cap(ctx, cap, S):
    name = "lgssm1d_spec" if S == 1 else "chained_samples"
    specs, tabs, seeds, refs = case_arguments(name, cap[S], 2, 1)
    assert len(specs[0].cols) == S
    run_case(ctx, specs, tabs, cap[S], seeds, refs, 2.0, 1, 1, f"{name} at the cap")


@pytest.mark.parametrize("special, M", [("inf", 1), ("nan", 0)])
def test_special_values_in_the_reference_pass_through(ctx, special, M):
    """+-inf and NaN in the reference are pinned as they are. A NaN reference makes particle n-1's
    weight NaN, after which no Resample decides to run and a backward draw is WSMC_ESTATE: that
    case runs the filter alone and then checks the refusal of the draw."""
    n, T = 65, 7
    specs, tabs, seeds, refs = case_arguments("local_trend", n, T, 1)
    refs[0, 2, 0], refs[0, 4, 1] = np.inf, -np.inf
    if special == "nan":
        refs[0, 5, 1] = np.nan
    res = run_case(ctx, specs, tabs, n, seeds, refs, 2.0, M, 2, f"reference with {special}")
    rec = res.backward[0].record if M else res.backward[0]
    assert sf.same_value(rec.cols[:, :, n - 1], refs[0])
    if special == "nan":
        assert np.isnan(res.log_evidence[0])
        with pytest.raises(abi.WSMCError) as e:
            ctx.ssm_run_conditional(specs[0], tabs[0], n, seeds, refs, ess_perc_min=2.0, backward=1, backward_seeds=[3])
        assert e.value.code == abi.WSMC_ESTATE


def snapshot(g):
    return (repr(g.get_state()), g.col_names(), g.weights_download().tobytes(), g.ssm_conditional_stats()["conditional_segments"],
            g.ssm_backward_stats()["recording_segments"])


def test_refusals(ctx, cap):
    x = Col("x")
    ok, data = models.lgssm1d_spec(), models.lgssm1d_data(4)
    ref1, ref3 = np.zeros((2, 4, 1)), np.zeros((2, 4, 3))
    weighted = (SSM(cols=["x"]).init(sample("x", Normal(0.0, 1.0)))
                .step(sample("x", Normal(x * 0.9, 1.0)), weight(x, Normal(0.0, 3.0)), observe(Data(0), Normal(x, 0.5))))
    init_obs = (SSM(cols=["x"], data_dim=1).init(sample("x", Normal(0.0, 1.0)), observe(0.3, Normal(x, 1.0)))
                .step(sample("x", Normal(x * 0.9, 1.0)), observe(Data(0), Normal(x, 0.5))))
    static = (SSM(cols=["a", "x"]).init(sample("a", Normal(0.9, 0.05)), sample("x", Normal(0.0, 1.0)))
              .step(sample("x", Normal(x * 0.5 + Col("a"), 1.0)), observe(Data(0), Normal(x, 0.5))))
    kw = dict(backward=1, backward_seeds=[1, 2])
    runs = [
        (lambda: ctx.ssm_run_conditional(models.lgssm1d_guided(), data, 65, [1, 2], ref3, **kw), "spec 0: statement 2 of step is an importance SAMPLE"),
        (lambda: ctx.ssm_run_conditional(weighted, data, 65, [1, 2], ref1, **kw), "spec 0: statement 1 of step is a WEIGHT"),
        (lambda: ctx.ssm_run_conditional(init_obs, data, 65, [1, 2], ref1, **kw), "spec 0: statement 1 of init is an OBSERVE"),
        (lambda: ctx.ssm_run_conditional(static, data, 65, [1, 2], np.zeros((2, 4, 2)), **kw), "ssm backward: state column a"),
        (lambda: ctx.ssm_run_conditional([ok, models.lgssm1d_spec(a=0.5), ok], data, 65, [1, 2], ref1, **kw), None),
        (lambda: ctx.ssm_run_conditional(ok, data, cap[1] + 64, [1, 2], ref1, **kw), "above the cap"),
        (lambda: ctx.ssm_run_conditional(ok, data, 65, [1, 2], ref1, backward=cap[1] + 1, backward_seeds=[1, 2]), f"M = {cap[1] + 1}"),
    ]
    for run, why in runs:
        before = snapshot(ctx)
        if why is None:   # the wrapper's own check: one spec or one per filter
            with pytest.raises(ValueError, match="specs"):
                run()
        else:
            with pytest.raises(abi.WSMCError) as e:
                run()
            assert e.value.code == abi.WSMC_EARG and why in str(e.value), str(e.value)
        assert snapshot(ctx) == before, why
    with pytest.raises(ValueError, match="one backward seed per filter"):
        ctx.ssm_run_conditional(ok, data, 65, [1, 2], ref1, backward=1, backward_seeds=[1])
    with pytest.raises(ValueError, match="reference"):
        ctx.ssm_run_conditional(ok, data, 65, [1, 2], ref3)
    # through the C entry point: a null reference, M < 0, M = 0 with a backward output, M > 0 without bw_out or seeds
    tab = ok.table(data)
    seeds, out, bo = (C.c_uint64 * 2)(1, 2), abi.SsmBatchOut(), abi.SsmBackwardOut()
    D = C.POINTER(C.c_double)
    idx = np.zeros((2, 4, 1), dtype=np.int32)

    def call(ref, M, bseeds, bw_out):
        return ctx._L.wsmc_ssm_run_conditional(ctx._h, C.byref(ok.spec), 1, tab.ctypes.data_as(D), 1, 4, 65, 2, seeds, 0.5,
                                               None if ref is None else ref.ctypes.data_as(D), C.byref(out), None, M, bseeds, bw_out)
    before = snapshot(ctx)
    for args, why in (((None, 0, None, None), b"null reference"), ((ref1, -1, None, None), b"M < 0"),
                      ((ref1, 1, seeds, None), b"null bw_out"), ((ref1, 1, None, C.byref(bo)), b"null bw_seeds")):
        assert call(*args) == abi.WSMC_EARG and why in ctx._L.wsmc_last_error(), why
    bo.idx = idx.ctypes.data_as(C.POINTER(C.c_int32))
    assert call(ref1, 0, None, C.byref(bo)) == abi.WSMC_EARG and b"M = 0" in ctx._L.wsmc_last_error()
    assert snapshot(ctx) == before
    # M = 0 with no bw_out at all is a run
    assert call(ref1, 0, None, None) == abi.WSMC_OK


def test_other_runs_launch_none_of_the_conditional_kernels():
    data = models.lgssm1d_data(6)
    ssm = models.lgssm1d_spec()
    g = wsmc.Context(257, seed=4)
    try:
        g.ssm_run(ssm, data, ess_perc_min=0.5)
        g.ssm_run_batch(ssm, data, 65, [1, 2], ess_perc_min=0.5)
        g.ssm_run_batch(ssm, data, 65, [1, 2], ess_perc_min=0.5, backward=2, backward_seeds=[3, 4])
        assert g.ssm_conditional_stats() == {"segments_s": 0.0, "backward_s": 0.0, "rows_s": 0.0, "bytes": 0, "conditional_segments": 0}
        recording = g.ssm_backward_stats()["recording_segments"]
        g.ssm_run_conditional(ssm, data, 65, [1, 2], np.zeros((2, 6, 1)), backward=1, backward_seeds=[3, 4])
        assert g.ssm_conditional_stats()["conditional_segments"] == g.ssm_batch_stats()["segments"] == 1
        assert g.ssm_backward_stats()["recording_segments"] == recording   # nor does it launch the unconditional recording kernels
    finally:
        g.close()


def test_particle_gibbs(ctx):
    """3 sweeps of 2 chains on the device equal the loop over the definitions with pg_seeds, from an
    unconditional first sweep and from a given reference"""
    ssm, y = models.kitagawa(), models.kitagawa_data(7)
    for ref in (None, sc.reference(ssm, 7, 5, B=2)):
        traj, logev = wsmc.particle_gibbs(ctx, ssm, y, 65, 3, 77, chains=2, ess_perc_min=0.5, reference=ref)
        want_traj, want_logev = sc.definition_gibbs(ssm, y, 65, 3, 77, chains=2, ess=0.5, ref=ref)
        assert list(traj) == ssm.cols and traj["x"].shape == (3, 2, 7) and logev.shape == (3, 2)
        assert sf.same_value(traj, want_traj) and sf.same_value(logev, want_logev)
        assert not sf.same_value(traj["x"][1], traj["x"][2])

"""The fused run of a specified scalar SSM (wsmc_ssm_run) against the CPU oracle running the same
spec statement by statement (wsmc.SSM.statements), bit for bit: every column, the weights, every
state field, the last ancestors, both evidences, the per-step ESS trace and the score fold. Small
populations run on one persistent workgroup (csrc/wsmc_ssm.hip); every other shape goes through
the statements inside the library, and the counters say which route a run took.
"""
import math

import numpy as np
import pytest

import wsmc
from wsmc import abi, dsl, models
from wsmc.dsl import Col, Data, Normal
from wsmc.ssm import SSM, assign, observe, sample
from oracle import Oracle

pytestmark = pytest.mark.gpu

SEED = 42
T = 40
STATE = ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples")


def same_float(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def assert_same(g, o, ev=None, trace=None, ess=None):
    assert g.col_names() == o.col_names()
    for name in g.col_names():
        np.testing.assert_array_equal(g.col_download(g.col_find(name)), o.col_download(o.col_find(name)),
                                      err_msg=f"column {name}")
    np.testing.assert_array_equal(g.weights_download(), o.weights_download())
    sg, so = g.get_state(), o.get_state()
    for k in STATE:
        assert sg[k] == so[k], k
    assert same_float(sg["last_ess_perc"], so["last_ess_perc"])
    np.testing.assert_array_equal(g.last_ancestors(), o.last_ancestors())
    if ev is not None:
        assert same_float(ev, o.log_evidence())
    assert same_float(g.log_evidence(), o.log_evidence())
    if trace is not None:
        np.testing.assert_array_equal(trace, ess)   # NaNs equal by position
    np.testing.assert_array_equal(g.score(-1), o.score(-1))
    # ... and the fold over the whole tape (a target depth of -1 folds no term): every Sample and
    # Observe term with the step's data folded in
    np.testing.assert_array_equal(g.score(sg["depth"]), o.score(so["depth"]))


def run_both(spec, N, data, persistent=True, seed=SEED, segment=None, **kw):
    """One fused run on a fresh context, the statements on a fresh oracle, everything compared.
    Returns (context, oracle, flags, evidence)."""
    g, o = wsmc.Context(N, seed=seed), Oracle(N, seed=seed)
    if segment is not None:
        g.set_ssm_segment(segment)
    ev, trace = g.ssm_run(spec, data, ess_trace=True, **kw)
    flags, ess = spec.statements(o, data, **kw)
    assert len(trace) == len(flags)
    assert_same(g, o, ev, trace, ess)
    st = g.ssm_stats()
    assert (st["persistent_runs"], st["statement_runs"]) == ((1, 0) if persistent else (0, 1))
    return g, o, flags, ev


@pytest.fixture(scope="module")
def caps(gpu_available):
    g = wsmc.Context(1, seed=SEED)
    c = g.ssm_stats()["cap"]
    g.close()
    assert c[1] >= c[2] >= c[3] >= c[4] >= 2048
    return c


MODELS = {name: (make(), gen(T)) for name, (make, gen) in models.SSM_MODELS.items()}


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 1025, "cap", "cap+1"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_models(caps, name, N, ess):
    """One thread short of, at and past a wave, one and several particles a thread, the cap of the
    model's column count and one past it (the statement route); forced and gated resampling."""
    spec, data = MODELS[name]
    cap = caps[len(spec.cols)]
    N = cap if N == "cap" else cap + 1 if N == "cap+1" else N
    g, o, flags, _ = run_both(spec, N, data, persistent=N <= cap, ess_perc_min=ess)
    sp = spec.spec
    ns = sum(sp.step[q].kind == abi.SSM_SAMPLE for q in range(sp.n_step))
    ni = sum(sp.init[q].kind == abi.SSM_SAMPLE for q in range(sp.n_init))
    assert g.get_state()["op_counter"] == 2 * ni + (2 * ns + 1) * T
    assert g.get_state()["depth"] == sp.n_init + sp.n_step * T
    if N >= 63:
        assert all(flags) if ess == 1.0 else 0 < sum(flags) < T
    elif N == 1 or ess == 0.5:
        assert not any(flags)


LGSSM = models.lgssm1d_spec()
LGDATA = models.lgssm1d_data(T)


@pytest.mark.parametrize("N", ["cap", "cap+1"])
def test_one_column_cap(caps, N):
    N = caps[1] + (N == "cap+1")
    run_both(LGSSM, N, LGDATA, persistent=N <= caps[1], ess_perc_min=0.5)


def four_columns():
    """local_trend with an acceleration: four columns, three Samples, an affine Assign"""
    return (SSM(cols=["a", "v", "x", "m"])
            .init(sample("a", Normal(0.0, 0.01)), sample("v", Normal(0.0, 0.1)), sample("x", Normal(0.0, 1.0)))
            .step(sample("a", Normal(Col("a") * 0.9, 0.02)),
                  sample("v", Normal(Col("v") + Col("a"), 0.05)),
                  sample("x", Normal(Col("x") + Col("v"), 0.3)),
                  assign("m", 2.0 * Col("x") + 1.0),
                  observe(Data(0), Normal(Col("x"), 0.5))))


@pytest.mark.parametrize("N", [65, 1000, "cap", "cap+1"])
def test_four_columns(caps, N):
    N = caps[4] if N == "cap" else caps[4] + 1 if N == "cap+1" else N
    _, _, flags, _ = run_both(four_columns(), N, models.local_trend_data(T), persistent=N <= caps[4], ess_perc_min=0.5)
    assert 0 < sum(flags) < T


@pytest.mark.parametrize("K", [7, 1])
@pytest.mark.parametrize("name", ["local_trend", "kitagawa"])
def test_segment_hand_over(gpu_available, name, K):
    """Every column, the weights, the ancestors row and the record cross a launch boundary: any
    segment length gives the oracle's bits."""
    spec, data = MODELS[name]
    for ess in (1.0, 0.5):
        g, _, _, _ = run_both(spec, 1000, data, segment=K, ess_perc_min=ess)
        assert g.ssm_stats()["segments"] == -(-T // K)


@pytest.mark.parametrize("K", [7, 1])
def test_last_segment_without_resampling(gpu_available, K):
    """A gated run whose last segment resamples nowhere: the ancestors row of an earlier segment stays."""
    spec = models.local_trend()
    _, _, flags, _ = run_both(spec, 1000, models.local_trend_data(T, seed=7), segment=K, ess_perc_min=0.3)
    assert sum(flags) > 3 and not any(flags[35:])


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [65, 1000])
@pytest.mark.parametrize("name", ["sv", "kitagawa"])
def test_systematic(gpu_available, name, N, ess):
    spec, data = MODELS[name]
    run_both(spec, N, data, ess_perc_min=ess, scheme=abi.RESAMPLE_SYSTEMATIC)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_statement_route_multinomial(gpu_available, name):
    spec, data = MODELS[name]
    run_both(spec, 1000, data, persistent=False, ess_perc_min=0.5, scheme=abi.RESAMPLE_MULTINOMIAL)


def test_statement_route_without_trace(gpu_available):
    """No trace requested: the statement route's Resamples stay asynchronous; the same state."""
    spec, data = MODELS["kitagawa"]
    g, o = wsmc.Context(1000, seed=SEED), Oracle(1000, seed=SEED)
    ev = g.ssm_run(spec, data, ess_perc_min=0.5, scheme=abi.RESAMPLE_MULTINOMIAL)
    spec.statements(o, data, ess_perc_min=0.5, scheme=abi.RESAMPLE_MULTINOMIAL)
    assert_same(g, o, ev)


def test_statement_route_foreign_column(gpu_available):
    """A column that is not the spec's: the statement route, the oracle's bits."""
    spec, data = MODELS["sv"]
    g, o = wsmc.Context(1000, seed=SEED), Oracle(1000, seed=SEED)
    for c in (g, o):
        c.assign(c.col_create("other", 1), models._const([0.3]))
    ev, trace = g.ssm_run(spec, data, ess_perc_min=0.5, ess_trace=True)
    flags, ess = spec.statements(o, data, ess_perc_min=0.5)
    assert_same(g, o, ev, trace, ess)
    st = g.ssm_stats()
    assert (st["persistent_runs"], st["statement_runs"]) == (0, 1)


def test_statement_route_weights_changed(gpu_available):
    """weights_changed set on entry: the first auto-inserted Resample runs, so the statements do."""
    spec, data = MODELS["local_trend"]
    g, o = wsmc.Context(1000, seed=SEED), Oracle(1000, seed=SEED)
    for c in (g, o):
        cv = c.col_create("v", 1)
        c.sample(cv, Normal(0.0, 1.0).dist(models.resolver(c)))
        c.observe(Normal(Col("v"), 1.0).dist(models.resolver(c)), models._const([0.1]))
    assert g.get_state()["weights_changed"] == 1
    ev, trace = g.ssm_run(spec, data, ess_perc_min=0.5, ess_trace=True)
    flags, ess = spec.statements(o, data, ess_perc_min=0.5)
    assert_same(g, o, ev, trace, ess)
    st = g.ssm_stats()
    assert (st["persistent_runs"], st["statement_runs"]) == (0, 1)


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("name", ["kitagawa", "local_trend"])
def test_two_runs_continue(gpu_available, name, ess):
    """A second run on the same context: the columns exist, the op counter, the weights and the tape
    continue and `init` runs again, as the statements issued twice."""
    spec, data = MODELS[name]
    g, o, _, _ = run_both(spec, 1000, data, ess_perc_min=ess)
    data2 = models.SSM_MODELS[name][1](25, seed=7)
    ev, trace = g.ssm_run(spec, data2, ess_perc_min=ess, ess_trace=True)
    flags, e = spec.statements(o, data2, ess_perc_min=ess)
    assert_same(g, o, ev, trace, e)
    assert g.ssm_stats()["persistent_runs"] == 2


def test_all_weights_minus_inf(gpu_available):
    """A count of -1 has probability 0 under every rate: Q = 0, the ESS NaN, no resampling after it."""
    spec = models.poisson_count()
    data = models.poisson_count_data(12)
    data[5] = -1.0
    g, o, flags, ev = run_both(spec, 1000, data, ess_perc_min=1.0)
    assert flags == [True] * 5 + [False] * 7
    s = g.get_state()
    assert s["n_resamples"] == 5 and math.isnan(s["last_ess_perc"])
    assert np.all(np.isneginf(g.weights_download()))


@pytest.mark.parametrize("name", ["sv", "kitagawa"])
def test_nan_observation(gpu_available, name):
    spec = models.SSM_MODELS[name][0]()
    data = models.SSM_MODELS[name][1](12)
    data.reshape(12, -1)[5, 0] = math.nan
    g, o, flags, ev = run_both(spec, 1000, data, ess_perc_min=0.5)
    assert math.isnan(ev)


def gamma_spec():
    """a log-Gamma variant: a Gamma(alpha, x / alpha) transition (mean x) and a NegativeBinomial
    observation whose p comes from an expression column"""
    alpha = 20.0
    x = Col("x")
    return (SSM(cols=["x", "p"])
            .init(sample("x", dsl.Gamma(4.0, 1.0)))
            .step(sample("x", dsl.Gamma(alpha, x * (1.0 / alpha))),
                  assign("p", 5.0 / (5.0 + x)),
                  observe(Data(0), dsl.NegativeBinomial(5.0, Col("p")))))


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [65, 1000])
def test_log_gamma_variant(gpu_available, N, ess):
    rng = np.random.Generator(np.random.Philox(3))
    data = rng.poisson(4.0, T).astype(float)
    _, _, flags, ev = run_both(gamma_spec(), N, data, ess_perc_min=ess)
    assert math.isfinite(ev)
    assert all(flags) if ess == 1.0 else 0 < sum(flags) < T


def ext_spec():
    """an EXT variant: a Laplace transition with a Cauchy observation"""
    return (SSM(cols=["x"])
            .init(sample("x", dsl.Laplace(0.0, 1.0)))
            .step(sample("x", dsl.Laplace(Col("x") * 0.9, 0.5)),
                  observe(Data(0), dsl.Cauchy(Col("x"), 0.7))))


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [65, 1000])
def test_ext_variant(gpu_available, N, ess):
    _, _, flags, ev = run_both(ext_spec(), N, LGDATA, ess_perc_min=ess)
    assert math.isfinite(ev)
    assert all(flags) if ess == 1.0 else 0 < sum(flags) < T


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [65, 1000, 4096])
def test_lgssm_spec_against_lgssm1d_run(gpu_available, N, ess):
    """The new kernel against the old one: the LGSSM spec through ssm_run and lgssm1d_run on two
    fresh contexts of one seed."""
    a, b = wsmc.Context(N, seed=SEED), wsmc.Context(N, seed=SEED)
    ev_a, tr_a = a.ssm_run(LGSSM, LGDATA, ess_perc_min=ess, ess_trace=True)
    ev_b, tr_b = b.lgssm1d_run(LGDATA, ess_perc_min=ess, ess_trace=True)
    assert a.ssm_stats()["persistent_runs"] == 1 and b.lgssm_stats()["persistent_runs"] == 1
    assert ev_a == ev_b
    np.testing.assert_array_equal(tr_a, tr_b)
    np.testing.assert_array_equal(a.col_download(0), b.col_download(0))
    np.testing.assert_array_equal(a.weights_download(), b.weights_download())
    np.testing.assert_array_equal(a.last_ancestors(), b.last_ancestors())
    assert a.get_state() == b.get_state()
    np.testing.assert_array_equal(a.score(-1), b.score(-1))
    d = a.get_state()["depth"]
    np.testing.assert_array_equal(a.score(d), b.score(d))   # the whole tape


def test_state_right_after_run(gpu_available):
    """get_state() straight after ssm_run is exact: nothing is left pending."""
    spec, data = MODELS["local_trend"]
    g, o = wsmc.Context(1000, seed=SEED), Oracle(1000, seed=SEED)
    g.ssm_run(spec, data, ess_perc_min=0.5, want_evidence=False)
    sg = g.get_state()
    flags, _ = spec.statements(o, data, ess_perc_min=0.5)
    so = o.get_state()
    for k in STATE + ("last_ess_perc",):
        assert sg[k] == so[k], k
    assert sg["n_resamples"] == sum(flags)


@pytest.mark.parametrize("bad", ["scheme", "T", "dim"])
def test_argument_errors(gpu_available, bad):
    spec, data = MODELS["sv"]
    g = wsmc.Context(1000, seed=SEED)
    if bad == "dim":
        g.col_create("s", 2)
    before = ({k: g.get_state()[k] for k in STATE}, g.col_names())
    with pytest.raises(abi.WSMCError) as e:
        if bad == "scheme":
            g.ssm_run(spec, data, scheme=7)
        elif bad == "T":
            g.ssm_run(spec, data[:0])
        else:
            g.ssm_run(spec, data)
    assert e.value.code == abi.WSMC_EARG
    assert ({k: g.get_state()[k] for k in STATE}, g.col_names()) == before
    assert g.ssm_stats()["segments"] == 0

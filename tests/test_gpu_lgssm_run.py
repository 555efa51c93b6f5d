"""The fused 1D LGSSM run (wsmc_lgssm1d_run) against the CPU oracle's statement-by-statement
restatement (models.lgssm1d_statements), bit for bit: column, weights, every state field, the
last ancestors, the log evidence and the per-step ESS trace. Small populations run on one
persistent workgroup (csrc/wsmc_lgssm.hip); everything else goes through the statements inside
the library, and the counters say which route a run took.
"""
import math

import numpy as np
import pytest

import wsmc
from wsmc import abi, models
from wsmc.dsl import Col, Normal
from backends import kalman_filter_evidence
from oracle import Oracle

pytestmark = pytest.mark.gpu

SEED = 42


class Recording:
    """An oracle whose Resamples' waited returns (flag, ESS%) are kept, in issue order."""

    def __init__(self, o):
        self._o = o
        self.resamples = []

    def __getattr__(self, k):
        return getattr(self._o, k)

    def resample(self, *a, **kw):
        r = self._o.resample(*a, **kw)
        self.resamples.append(r)
        return r


def oracle_run(o, data, **kw):
    """models.lgssm1d_statements on the oracle: (flags, ESS% of each step's post-Observe Resample)."""
    rec = Recording(o)
    flags = models.lgssm1d_statements(rec, data, **kw)
    post = rec.resamples[2::2]          # [0] follows x's prior, then (after Sample, after Observe) per step
    assert [f for f, _ in post] == flags
    return flags, np.array([e for _, e in post])


def assert_same_state(g, o):
    """tests/test_gpu_parity.py's assert_same_state (bitwise)."""
    assert g.col_names() == o.col_names()
    for name in g.col_names():
        a = g.col_download(g.col_find(name))
        b = o.col_download(o.col_find(name))
        np.testing.assert_array_equal(a, b, err_msg=f"column {name}")
    np.testing.assert_array_equal(g.weights_download(), o.weights_download())
    sg, so = g.get_state(), o.get_state()
    for k in ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples"):
        assert sg[k] == so[k], k
    assert sg["last_ess_perc"] == so["last_ess_perc"] or (math.isnan(sg["last_ess_perc"]) and math.isnan(so["last_ess_perc"]))
    for d in (-1, so["depth"]):      # the tape (on the persistent route the host writes it)
        np.testing.assert_array_equal(g.score(d), o.score(d), err_msg=f"score({d})")


def same_float(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def run_both(N, data, persistent=True, seed=SEED, segment=None, **kw):
    """One fused run on a fresh context, the statements on a fresh oracle, everything compared.
    Returns (context, oracle, flags, evidence)."""
    g, o = wsmc.Context(N, seed=seed), Oracle(N, seed=seed)
    if segment is not None:
        g.set_lgssm_segment(segment)
    ev, trace = g.lgssm1d_run(data, ess_trace=True, **kw)
    flags, ess = oracle_run(o, data, **kw)
    check_pair(g, o, ev, trace, flags, ess)
    st = g.lgssm_stats()
    assert (st["persistent_runs"], st["statement_runs"]) == ((1, 0) if persistent else (0, 1))
    return g, o, flags, ev


def check_pair(g, o, ev, trace, flags, ess):
    assert_same_state(g, o)
    assert len(trace) == len(flags)
    np.testing.assert_array_equal(g.last_ancestors(), o.last_ancestors())   # (no step resampled: untouched rows)
    assert same_float(ev, o.log_evidence())
    assert same_float(g.log_evidence(), o.log_evidence())
    np.testing.assert_array_equal(trace, ess)   # NaNs equal by position


@pytest.fixture(scope="module")
def cap(gpu_available):
    g = wsmc.Context(1, seed=SEED)
    c = g.lgssm_stats()["cap"]
    g.close()
    assert c >= 4096
    return c


DATA40 = models.lgssm1d_data(40)


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 1023, 1024, 1025, 4096, "cap"])
def test_shapes_stratified(cap, N, ess):
    """One thread short of, at and past a wave and the workgroup, one and several particles a
    thread, the cap; forced and gated resampling (both branches of the step)."""
    N = cap if N == "cap" else N
    g, o, flags, _ = run_both(N, DATA40, ess_perc_min=ess)
    s = g.get_state()
    assert s["op_counter"] == 2 + 3 * 40 and s["depth"] == s["n_terms"] == 1 + 2 * 40
    if N >= 63:
        assert all(flags) if ess == 1.0 else 0 < sum(flags) < 40
    elif N == 1 or ess == 0.5:
        assert not any(flags)
    else:
        assert all(flags)


@pytest.mark.parametrize("N", [127, 128, 129, 2047, 2048, 2049])
def test_shapes_thread_layout(gpu_available, N):
    """The kernel runs two particles a thread up to a full workgroup: around the sizes where the
    wave count (128) and the particles per thread (2048) change."""
    run_both(N, DATA40, ess_perc_min=0.5)


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("N", [65, 1000])
def test_shapes_systematic(gpu_available, N, ess):
    run_both(N, DATA40, ess_perc_min=ess, scheme=abi.RESAMPLE_SYSTEMATIC)


@pytest.fixture(scope="module")
def unsegmented(gpu_available):
    g = wsmc.Context(1000, seed=SEED)
    ev, trace = g.lgssm1d_run(DATA40, ess_perc_min=0.5, ess_trace=True)
    return g.col_download(g.col_find("x")), g.weights_download(), g.last_ancestors(), ev, trace


@pytest.mark.parametrize("K", [1, 7, 40, 64])
def test_segment_boundaries(unsegmented, K):
    """The state crosses a launch boundary through the column, the weights, the ancestors row and
    the record: any segment length gives the unsegmented run and the oracle."""
    g, _, _, ev = run_both(1000, DATA40, segment=K, ess_perc_min=0.5)
    assert g.lgssm_stats()["segments"] == -(-40 // K)
    x, w, anc, ev0, trace0 = unsegmented
    np.testing.assert_array_equal(g.col_download(g.col_find("x")), x)
    np.testing.assert_array_equal(g.weights_download(), w)
    np.testing.assert_array_equal(g.last_ancestors(), anc)
    assert ev == ev0


@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_two_runs_continue(gpu_available, ess):
    """A second run on the same context continues the RNG stream, the weights, the tape and the
    counters as the statements issued twice."""
    g, o, _, _ = run_both(1000, DATA40, ess_perc_min=ess)
    data2 = models.lgssm1d_data(25, seed=7)
    ev, trace = g.lgssm1d_run(data2, ess_perc_min=ess, ess_trace=True)
    flags, e = oracle_run(o, data2, ess_perc_min=ess)
    check_pair(g, o, ev, trace, flags, e)
    assert g.lgssm_stats()["persistent_runs"] == 2


def test_after_other_statements(gpu_available):
    """Another column and changed weights before the run: the statement route, the oracle's bits."""
    g, o = wsmc.Context(1000, seed=SEED), Oracle(1000, seed=SEED)
    for c in (g, o):
        cy = c.col_create("y", 1)
        c.assign(cy, models._const([0.3]))
        c.observe(Normal(Col("y"), 1.0).dist(models.resolver(c)), models._const([0.1]))
    ev, trace = g.lgssm1d_run(DATA40, ess_perc_min=0.5, ess_trace=True)
    flags, e = oracle_run(o, DATA40, ess_perc_min=0.5)
    check_pair(g, o, ev, trace, flags, e)
    st = g.lgssm_stats()
    assert (st["persistent_runs"], st["statement_runs"]) == (0, 1)


def test_statement_route_past_cap(cap):
    run_both(cap + 1, DATA40, persistent=False, ess_perc_min=0.5)


def test_statement_route_multinomial(gpu_available):
    run_both(1000, DATA40, persistent=False, ess_perc_min=0.5, scheme=abi.RESAMPLE_MULTINOMIAL)


def test_statement_route_without_trace(gpu_available):
    """No trace requested: the statement route's Resamples stay asynchronous; the same state."""
    g, o = wsmc.Context(1000, seed=SEED), Oracle(1000, seed=SEED)
    ev = g.lgssm1d_run(DATA40, ess_perc_min=0.5, scheme=abi.RESAMPLE_MULTINOMIAL)
    flags, _ = oracle_run(o, DATA40, ess_perc_min=0.5, scheme=abi.RESAMPLE_MULTINOMIAL)
    assert_same_state(g, o)
    np.testing.assert_array_equal(g.last_ancestors(), o.last_ancestors())
    assert ev == o.log_evidence()


def test_outlier(gpu_available):
    data = models.lgssm1d_data(12)
    data[5] = 40.0
    g, o, flags, _ = run_both(1000, data, ess_perc_min=0.5)
    assert sum(flags) == 9 == g.get_state()["n_resamples"]
    assert g.get_state()["last_ess_perc"] == 0.5438822010205497


def test_degenerate_weights(gpu_available):
    """Every weight -inf from step 6 on: Q = 0, ESS NaN, no resampling, NaN evidence."""
    data = models.lgssm1d_data(12)
    data[5] = 1e200
    g, o, flags, ev = run_both(1000, data, ess_perc_min=1.0)
    assert flags == [True] * 5 + [False] * 7
    s = g.get_state()
    assert s["n_resamples"] == 5 and math.isnan(s["last_ess_perc"]) and math.isnan(ev)
    assert np.all(np.isneginf(g.weights_download()))


def test_horizon(gpu_available):
    """Several segments at the default length, the observations streamed from one upload."""
    data = models.lgssm1d_data(5000)
    g, o, flags, ev = run_both(1000, data, ess_perc_min=1.0)
    assert ev == -7977.36031044567
    assert g.get_state()["n_resamples"] == 5000
    assert g.lgssm_stats()["segments"] > 1


def test_kalman(gpu_available):
    """The evidence against the exact filter, within test_reference_ports.test_lgssm1d_kalman's bound."""
    data = models.lgssm1d_data(200)
    _, exact_ev = kalman_filter_evidence(data, 0.9, 1.0, 0.5)
    g = wsmc.Context(4096, seed=SEED)
    ev = g.lgssm1d_run(data, ess_perc_min=1.0)
    assert g.lgssm_stats()["persistent_runs"] == 1
    assert abs(ev - exact_ev) < 1.0


@pytest.mark.parametrize("bad", [dict(data=[]), dict(q=0.0), dict(scheme=7)])
def test_argument_errors(gpu_available, bad):
    g = wsmc.Context(1000, seed=SEED)
    g.lgssm1d_run(DATA40[:5], ess_perc_min=0.5)
    before = (g.get_state(), g.col_names(), g.weights_download(), g.col_download(0), g.lgssm_stats()["segments"])
    kw = dict(data=DATA40[:5], ess_perc_min=0.5)
    kw.update(bad)
    with pytest.raises(abi.WSMCError) as e:
        g.lgssm1d_run(**kw)
    assert e.value.code == abi.WSMC_EARG
    s = g.get_state()
    assert {k: v for k, v in s.items() if k != "last_ess_perc"} == {k: v for k, v in before[0].items() if k != "last_ess_perc"}
    assert same_float(s["last_ess_perc"], before[0]["last_ess_perc"])
    assert g.col_names() == before[1]
    np.testing.assert_array_equal(g.weights_download(), before[2])
    np.testing.assert_array_equal(g.col_download(0), before[3])
    assert g.lgssm_stats()["segments"] == before[4]

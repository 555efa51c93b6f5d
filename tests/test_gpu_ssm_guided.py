"""The guided fused scalar-SSM runs: specs with importance Samples (WSMC_SSM_SAMPLE_IMPORTANCE) and
WEIGHTs (WSMC_SSM_WEIGHT) through wsmc_ssm_run, its traced, smoothed and batch forms, against the
CPU oracle issuing the same spec statement by statement, bit for bit (tests/ssmguidedfuzz.py; what
its corpus covers and how its runs come out is asserted on the CPU by tests/test_ssm_guided.py).

N = 1 is a lone particle, 65 two particles a thread with one in the second wave's first thread,
1001 two a thread over 8 waves, 2049 three a thread (five of the log-Gamma variant's 512 threads)
with waves that own nothing; T = 12 with segments of 1, 5 and the default, so that steps, rows of
the history and slots of the log cross launch boundaries. Every random seed runs at (1001, ess 0.5,
stratified, the default segment) and once more with the four axes rotated by the seed; every
directed case at 65 and 2049 with two of the three thresholds each.
"""
import numpy as np
import pytest

import ssmfuzz as sf
import ssmguidedfuzz as gf
import test_gpu_ssm_batch as tb     # bits_equal
import test_gpu_ssm_smooth as ts    # the smoothed run against its definition
import test_gpu_ssm_trace as tt     # the traced run against the traced statements
import wsmc
from oracle import Oracle
from wsmc import abi, importance_kernel, models
from wsmc.dsl import Col, Data, Normal
from wsmc.ssm import SSM, assign, observe, sample, weight

pytestmark = pytest.mark.gpu

STRAT, SYST, MULT = abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL
ESS = (1.0, 0.5, 0.0)


def rotated(seed):
    """(N, ess, scheme, segment) of a seed's second run: over the 24 seeds every value of every axis
    is met six times or more"""
    return ((1, 65, 2049)[(seed // 2) % 3], ESS[(seed // 3) % 3], (STRAT, SYST)[(seed + seed // 4) % 2],
            (1, 5, None)[(seed + seed // 3) % 3])


RANDOM = [(s, 1001, 0.5, STRAT, None) for s in gf.SEEDS] + [(s,) + rotated(s) for s in gf.SEEDS]
DIRECTED = [(name, n, ESS[(k + j) % 3], (STRAT, SYST)[(k + j + (n > 65)) % 2])
            for k, name in enumerate(gf.DIRECTED) for n in (65, 2049) for j in (0, 1)]


def _id(c):
    return "-".join("default" if v is None else str(v) for v in c)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in gf.corpus()}


@pytest.fixture(scope="module")
def cap(gpu_available):
    g = wsmc.Context(1, seed=sf.SEED)
    c = g.ssm_stats()["cap"]
    g.close()
    assert c[1] >= c[2] >= c[3] >= c[4] == 3008
    return c


def test_axes_are_each_met(cases):
    met = {}
    for seed in gf.SEEDS:
        for axis, v in zip(("N", "ess", "scheme", "segment"), rotated(seed)):
            met.setdefault((axis, v), set()).add(seed)
    assert len(met) == 3 + 3 + 2 + 3 and min(len(v) for v in met.values()) >= 6, {k: len(v) for k, v in met.items()}
    assert {e for _, _, e, _ in DIRECTED} == set(ESS) and {s for _, _, _, s in DIRECTED} == {STRAT, SYST}


# ---- 1. the corpus through ssm_run: differential asserts the persistent route from wsmc_debug_ssm ----
@pytest.mark.parametrize("case", RANDOM, ids=_id)
def test_random_seed(cap, cases, case):
    seed, n, ess, scheme, segment = case
    gf.differential(cases[f"random-{seed}"], n, ess, scheme, segment, "persistent")


@pytest.mark.parametrize("case", DIRECTED, ids=_id)
def test_directed(cap, cases, case):
    name, n, ess, scheme = case
    c = cases[name]
    flags, state = gf.differential(c, n, ess, scheme, 5, "persistent")
    if name == "init_importance" and ess == 1.0:
        assert state["n_resamples"] == 1 + gf.T and all(flags)
    if name == "all_neg_inf" and ess > 0.0:
        assert not any(flags[gf.ALL_NEG_INF_AT + 1:]) and np.isnan(state["last_ess_perc"])
    if name == "nan_weights":
        assert state["n_resamples"] == 0


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("n", ["cap", "cap+1"])
def test_four_columns_at_the_cap(cap, cases, n, ess):
    n = cap[4] + (n == "cap+1")
    gf.differential(cases["four_columns"], n, ess, STRAT, None, "persistent" if n <= cap[4] else "statements")


def test_statement_route_multinomial(cap, cases):
    gf.differential(cases["eight_statements"], 65, 0.5, MULT, None, "statements")


@pytest.mark.parametrize("name", ["after_last_observe", "log_gamma", "random-3"])
def test_statement_route_foreign_column(cap, cases, name):
    gf.differential(cases[name], 65, 0.5, STRAT, None, "statements")


# ---- 2. the trace and the smoothing ---------------------------------------------------------------
TRACED = [("after_last_observe", 65, 1.0, 1), ("after_last_observe", 2049, 0.5, 5), ("eight_statements", 1001, 1.0, 5),
          ("four_columns", 1001, 0.5, None), ("log_gamma", 2049, 1.0, 5), ("extended_families", 65, 0.5, 1),
          ("lgssm1d_guided", 1001, 0.5, None), ("all_neg_inf", 65, 1.0, 5), ("init_importance", 1, 1.0, 1)] + \
         [(f"random-{s}", (65, 1001, 2049)[s % 3], ESS[s % 2], (1, 5, None)[(s // 2) % 3]) for s in (1, 3, 7, 12, 16, 21)]


@pytest.mark.parametrize("case", TRACED, ids=_id)
def test_traced(cap, cases, case):
    """trace=True, all four parts, from the guided kernel with its trace pointers set"""
    name, n, ess, segment = case
    c = cases[name]
    got, want = tt.run_pair(c.ssm, c.data, n, ess, (STRAT, SYST)[n % 2], segment, steps=c.T, what=name)
    assert got.ess is not None and got.mean is not None and got.var is not None and got.log_evidence is not None


@pytest.mark.parametrize("case", TRACED, ids=_id)
def test_smoothed(cap, cases, case):
    """smooth=True (paths, mean, var) with the trace, from the recording guided kernel: the cases
    whose trace slot is not the step's last slot walk back through the slots behind it"""
    name, n, ess, segment = case
    c = cases[name]
    ts.run_pair(c.ssm, c.data, n, ess, (STRAT, SYST)[n % 2], segment, steps=c.T, what=name)


def test_traced_cases_have_late_and_last_trace_slots(cases):
    late = [n for n, _, _, _ in TRACED if cases[n].trace_slot[1] != cases[n].trace_slot[0] - 1]
    assert "after_last_observe" in late and len(set(late)) >= 4 and len(set(late)) < len({n for n, _, _, _ in TRACED}), late


def test_smoothed_row_is_the_trace_points_not_the_steps_end(cap, cases):
    c = cases["after_last_observe"]
    _, sm = ts.run_pair(c.ssm, c.data, 1001, 1.0, STRAT, 5, steps=c.T, what=c.name)
    g = wsmc.Context(1001, seed=sf.SEED)
    g.ssm_run(c.ssm, c.data, ess_perc_min=1.0, T=c.T)
    final = g.col_download(g.col_find("c0"))
    g.close()
    assert not tb.bits_equal(sm.paths["c0"][-1], final).all()   # the importance Sample after the trace point


# ---- 3. the batch: filter b against ssm_run on a fresh context of its seed ---------------------------
GUIDED_PARAMS = [dict(), dict(a=0.8, q=0.7, r=1.0), dict(a=0.95, q=1.2, r=0.4, gain=0.6, prop_std=0.6)]
SEEDS3 = [42, 2**63 + 5, 0]


def _weighted_spec(k):
    """a shape with a WEIGHT and a log-Gamma target, numbers by k"""
    return (SSM(cols=["x", "s"])
            .init(sample("x", Normal(0.0, 1.0 + 0.1 * k)), sample("s", wsmc.Gamma(3.0 + k, 0.4)))
            .step(sample("s", importance_kernel(wsmc.Gamma(3.0, (0.25 + 0.05 * k) * Col("s") + 0.2), wsmc.InverseGamma(3.0 + k, 2.5))),
                  weight(Col("s"), wsmc.Exponential(1.0 + k)),
                  sample("x", Normal((0.9 - 0.1 * k) * Col("x"), Col("s"))),
                  observe(Data(0), Normal(Col("x"), 0.5 + 0.25 * k)),
                  weight(Data(0), wsmc.Laplace(Col("x"), 2.0))))


BATCHES = {"lgssm1d_guided": [models.lgssm1d_guided(**p) for p in GUIDED_PARAMS], "weighted": [_weighted_spec(k) for k in range(3)]}


def _single(spec, data, n, seed, ess, scheme, trace, smooth):
    g = wsmc.Context(n, seed=seed)
    try:
        r = g.ssm_run(spec, data, ess_perc_min=ess, scheme=scheme, trace=trace, smooth=smooth,
                      ess_trace=not (trace or smooth))
        st = g.ssm_stats()
        assert (st["persistent_runs"], st["statement_runs"]) == (1, 0), st
        state = g.get_state()
        return dict(r=r, cols={c: g.col_download(g.col_find(c)) for c in spec.cols}, w=g.weights_download(),
                    anc=g.last_ancestors(), nres=state["n_resamples"], last=bool(state["resampled"]))
    finally:
        g.close()


def _same(what, a, b):
    ok = tb.bits_equal(a, b)
    assert ok.all(), f"{what}: differs first at {tuple(int(v) for v in np.argwhere(~np.atleast_1d(ok))[0])}"


@pytest.mark.parametrize("mode", ["plain", "traced", "smoothed"])
@pytest.mark.parametrize("n", [65, 1001])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batch(cap, name, n, mode):
    specs = BATCHES[name]
    assert all(specs[0].same_shape(s) for s in specs[1:])
    data = models.lgssm1d_data(gf.T) + 1.0 if name == "weighted" else models.lgssm1d_data(gf.T)
    ess, scheme = (0.5, STRAT) if n == 65 else (1.0, SYST)
    trace, smooth = mode != "plain", mode == "smoothed"
    g = wsmc.Context(16, seed=1)
    try:
        g.set_ssm_batch_segment(5)
        res = g.ssm_run_batch(specs, data, n, SEEDS3, ess_perc_min=ess, scheme=scheme, ess_trace=True, state=True,
                              trace=trace, smooth=smooth)
        assert g.ssm_batch_stats()["segments"] == 3
    finally:
        g.close()
    for b, (spec, seed) in enumerate(zip(specs, SEEDS3)):
        one = _single(spec, data, n, seed, ess, scheme, trace, smooth)
        tag = f"{name} N={n} {mode} filter {b}"
        _same(f"{tag}: log evidence", res.log_evidence[b], one["r"][0])
        for c in spec.cols:
            _same(f"{tag}: column {c}", res.cols[c][b], one["cols"][c])
        _same(f"{tag}: log-weights", res.log_weights[b], one["w"])
        assert (res.last_ancestors[b] == one["anc"]).all(), f"{tag}: last ancestors"
        assert (int(res.n_resamples[b]), bool(res.last_resampled[b])) == (one["nres"], one["last"]), tag
        if not trace:
            _same(f"{tag}: ESS trace", res.ess[b], one["r"][1])
            continue
        tr = one["r"][1]
        _same(f"{tag}: trace ess", res.ess[b], tr.ess)
        _same(f"{tag}: trace log evidence", res.log_evidence_trace[b], tr.log_evidence)
        for c in spec.cols:
            _same(f"{tag}: trace mean {c}", res.mean[c][b], tr.mean[c])
            _same(f"{tag}: trace var {c}", res.var[c][b], tr.var[c])
        if smooth:
            sm = one["r"][2]
            for c in spec.cols:
                _same(f"{tag}: paths {c}", res.paths[c][b], sm.paths[c])
                _same(f"{tag}: smoothed mean {c}", res.smean[c][b], sm.mean[c])
                _same(f"{tag}: smoothed var {c}", res.svar[c][b], sm.var[c])
    assert len({float(v) for v in res.log_evidence}) == 3   # the filters do differ


def test_batch_single_runs_match_the_oracle(cap):
    """the single runs the batch is compared with are themselves the oracle's statements"""
    for spec in BATCHES["weighted"][:2]:
        data = models.lgssm1d_data(gf.T) + 1.0
        g, o = wsmc.Context(1001, seed=42), Oracle(1001, seed=42)
        try:
            ev, trace = g.ssm_run(spec, data, ess_perc_min=1.0, scheme=SYST, ess_trace=True)
            _, etr = spec.statements(o, data, ess_perc_min=1.0, scheme=SYST)
            d = sf.compare(g, o, ev, trace, etr)
            assert d is None, d
            assert g.ssm_stats()["persistent_runs"] == 1
        finally:
            g.close()
            o.close()


# ---- 4. an unguided spec around a guided run ---------------------------------------------------------
def test_unguided_spec_before_and_after_a_guided_run(cap):
    """models.sv() before and after a guided run on one context, against a context on which the
    guided spec went through the operators instead (it never launched a guided kernel)"""
    sv, y = models.sv(), models.sv_data(gf.T)
    guided = (SSM(cols=["h", "s"])
              .step(assign("s", Col("h")),
                    sample("h", importance_kernel(Normal(Data(0) + 0.9 * Col("s"), 0.3), Normal(0.95 * Col("s"), 0.25))),
                    weight(Col("h"), Normal(0.0, 3.0)),
                    observe(Data(0), Normal(Col("h"), 1.0))))
    a, b = wsmc.Context(1001, seed=5), wsmc.Context(1001, seed=5)
    try:
        for k in range(2):
            eva = a.ssm_run(sv, y, ess_perc_min=0.5)
            evb = b.ssm_run(sv, y, ess_perc_min=0.5)
            d = sf.compare(a, b, eva)
            assert d is None and tb.bits_equal(eva, evb).all(), (k, d)
            if k == 0:
                a.ssm_run(guided, y, ess_perc_min=0.5)
                guided.statements(b, y, ess_perc_min=0.5)
                d = sf.compare(a, b)
                assert d is None, d
        sa, sb = a.ssm_stats(), b.ssm_stats()
        assert (sa["persistent_runs"], sa["statement_runs"]) == (3, 0) and (sb["persistent_runs"], sb["statement_runs"]) == (2, 0)
    finally:
        a.close()
        b.close()
    # and the first of those runs is a fresh context's
    c = wsmc.Context(1001, seed=5)
    o = Oracle(1001, seed=5)
    try:
        ev, tr = c.ssm_run(sv, y, ess_perc_min=0.5, ess_trace=True)
        _, etr = sv.statements(o, y, ess_perc_min=0.5)
        assert sf.compare(c, o, ev, tr, etr) is None
    finally:
        c.close()
        o.close()

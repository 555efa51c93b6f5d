"""The random fused 2D-SSM corpus (tests/ssm2dfuzz.py) on the CPU: what tests/test_gpu_ssm2d_random_runs.py
holds the device to is two CPU statements that agree bit for bit (the statement oracle and the port
that restates the fused formula, oracle/wsmc_port_mt.c), is right by arithmetic that shares no
header with them (tests/test_independent_math.py), and reaches what the corpus is for (asserted
below: sizes, horizons, thresholds, gates that go both ways, guessed reference points that miss and
that hold)."""
import numpy as np
import pytest

import oracle
import ssm2dfuzz as sf
from oracle import Oracle
from progfuzz import same_value
from wsmc import abi, models

MIXED = [f"mixed-{s}" for s in sf.MIXED_SEEDS]
INDEPENDENT_SEEDS = (4, 8, 22, 23)      # N = 65, 2049, 1025, 2049; forced and gated; both schemes


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sf.corpus()}


def _trace(name):
    return sf._trace_of(name)    # (one oracle pass a case, shared by the tests below)


# ---- the two CPU statements of the result agree ------------------------------------------------
@pytest.mark.parametrize("name", MIXED + sf.DIRECTED)
def test_port_restates_the_statements(cases, name):
    """Every run of every case: oracle.ssm2d_run_mt (fed the op counter and the weights the run
    starts from) equals the statement oracle bit for bit: every column, the weights, the flags and
    the evidence. (The port states the stratified and systematic schemes only: `multinomial` has
    the statement oracle alone, as tests/test_gpu_parity.py's multinomial runs have.)"""
    c = cases[name]
    if any(r.scheme == abi.RESAMPLE_MULTINOMIAL for r in c.runs):
        assert name == "multinomial"
        with pytest.raises(ValueError):
            oracle.ssm2d_run_mt(c.N, c.runs[0].obs, seed=c.ctx_seed, **c.runs[0].kw())
        return
    o = Oracle(c.N, seed=c.ctx_seed)
    try:
        for k, run in enumerate(c.runs):
            op, w0 = o.get_state()["op_counter"], o.weights_download()
            flags = models.ssm2d_statements(o, run.obs, **run.kw())
            r = oracle.ssm2d_run_mt(c.N, run.obs, seed=c.ctx_seed, threads=4, op_base=op, weights=w0 if k else None,
                                    **run.kw())
            assert list(r["flags"]) == [bool(f) for f in flags], f"run {k}"
            for col in [f"x_{t}" for t in range(1, run.T + 2)] + ["v", "dv"]:
                assert same_value(r[col], o.col_download(o.col_find(col))), f"run {k} column {col}"
            assert same_value(r["weights"], o.weights_download()), f"run {k} weights"
            assert same_value(r["log_evidence"], o.log_evidence()), f"run {k} evidence"
    finally:
        o.close()


# ---- q_var and r_var are variances, by arithmetic that shares no header ------------------------------
@pytest.mark.parametrize("name", ["recip", "lpmax_positive"] + [f"mixed-{s}" for s in INDEPENDENT_SEEDS])
def test_parameters_match_reference_math(cases, name):
    from test_independent_math import run_ssm2d_checked
    c = cases[name]
    run = c.runs[0]
    n_rs = run_ssm2d_checked("oracle", min(c.N, 5001), run.T, run.ess, run.scheme, obs=run.obs, x0=run.x0, v0=run.v0,
                             q_var=run.q_var, r_var=run.r_var)
    assert n_rs >= 1


# ---- the corpus reaches what it is for -----------------------------------------------------------
def test_corpus_covers_sizes_horizons_schemes_and_thresholds(cases):
    mixed = [cases[n] for n in MIXED]
    ns = [c.N for c in mixed]
    assert set(ns) == set(sf.NS)
    assert sum(n in sf.LARGE_NS for n in ns) <= len(mixed) // 4
    runs = [r for c in mixed for r in c.runs]
    assert {r.T for r in runs} == set(range(1, sf.T_MAX + 1))
    assert {r.scheme for r in runs} == {abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC}
    assert {r.ess for r in runs} == set(sf.ESS)
    assert {len(c.runs) for c in mixed} == {1, 2, 3}
    assert {c.keep_history for c in mixed} == {True, False}
    for r in runs:
        assert 1e-2 <= r.q_var <= 10.0 and -0.5 - 1e-9 <= np.log10(r.r_var / r.q_var) <= 1.5 + 1e-9
        assert not sf._pow2(r.q_var) and not sf._pow2(r.r_var)
    outliers = [c for c in mixed if int(c.name[6:]) % 5 == 0]
    assert len(outliers) == 7
    # the directed list is the issue's
    for name in ([f"t{T}_{N}_{g}" for T in (1, 2, 3) for N in (1025, 16385) for g in ("forced", "gated")] +
                 ["recip", "recip_inexact", "lpmax_positive", "loose", "collapse_5001", "collapse_70001", "far_start", "still", "inf_obs",
                  "huge_obs", "nan_obs", "grow_T", "shorter_run_after_longer", "param_switch", "async_mix", "multinomial", "qstat_edge_2999999",
                  "qstat_edge_3000000"]):
        assert name in cases, name
    assert [r.T for r in cases["grow_T"].runs] == [3, 9, 2]
    assert cases["grow_T"].routes() == ["fused", "fused", "statements"]
    assert cases["shorter_run_after_longer"].routes() == ["fused", "statements"]
    assert cases["async_mix"].routes() == ["fused"] * 5          # (no history: x, v and dv whatever T)
    routes = [r for n in MIXED for r in cases[n].routes()]
    assert routes.count("statements") >= 3 and routes.count("fused") >= 50
    ps = cases["param_switch"].runs          # A, B, A, A, B: both sets at both buffer parities
    assert [r.kw() == ps[0].kw() for r in ps] == [True, False, True, True, False] and ps[1].kw() == ps[4].kw()
    assert all(r.obs is ps[0].obs for r in ps) and cases["param_switch"].routes() == ["fused"] * 5
    mix = cases["async_mix"].runs
    assert len(mix) == 5 and not any(r.want_evidence for r in mix) and len({r.T for r in mix}) == 5
    assert (cases["recip"].runs[0].q_var, cases["recip"].runs[0].r_var) == (0.07, 0.3)
    assert cases["far_start"].runs[0].x0 == (1e8, -1e8) and cases["still"].runs[0].v0 == (0.0, 0.0)
    assert all(r.r_var == 1e-3 * r.q_var for n in ("collapse_5001", "collapse_70001") for r in cases[n].runs)


def test_gated_runs_go_both_ways(cases):
    """Among the mixed profile's gated runs with N >= 65 and T >= 4, at least 80 % have both a
    resampled and a non-resampled step after step 1. (Drawn with r_var / q_var from the whole of
    10^U(-0.5, 1.5) whatever the threshold, 17 of 26 had: ssm2dfuzz.RATIO_LOG10 narrows the range by
    threshold; the condition is the issue's.)"""
    both = []
    for name in MIXED:
        for run, tr in zip(cases[name].runs, _trace(name)):
            if run.ess < 1.0 and cases[name].N >= 65 and run.T >= 4:
                both.append(any(tr.flags[1:]) and not all(tr.flags[1:]))
    print(f"gated runs going both ways: {sum(both)} of {len(both)}")
    assert len(both) >= 10
    assert sum(both) >= 0.8 * len(both)


def test_predicted_misses_and_holds(cases):
    """Over the corpus at least 10 % of the steps t >= 2 are predicted to miss their guessed
    reference point and at least 30 % to hold; at most 2 % are undetermined."""
    n = {"miss": 0, "hold": 0, "undetermined": 0}
    for c in cases.values():
        for p in sf.predict_misses(c):
            for k in n:
                n[k] += len(p[k])
    total = sum(n.values())
    print(f"steps t >= 2: {total}: {n}")
    assert total == sum(r.T - 1 for c in cases.values() for r in c.runs)
    assert n["miss"] >= 0.10 * total
    assert n["hold"] >= 0.30 * total
    assert n["undetermined"] <= 0.02 * total
    # both happen away from the outliers and the degenerate cases too, and lpmax takes both signs
    plain = [p for name in MIXED if int(name[6:]) % 5 for p in sf.predict_misses(cases[name])]
    assert sum(len(p["miss"]) for p in plain) >= 10 and sum(len(p["hold"]) for p in plain) >= 10
    assert any(r.r_var < 1 / (2 * np.pi) for c in cases.values() for r in c.runs)
    assert any(r.r_var > 1 / (2 * np.pi) for c in cases.values() for r in c.runs)


def test_reciprocal_differs_from_division_where_the_corpus_says():
    """What makes a kernel that multiplies by 1 / r_var differ from one that divides: the rounding of
    the reciprocal. At r_var = 0.5 it is exact; at the doubles 0.3 and 0.6 the product equals the
    quotient for every s all the same (so `recip`, whose parameters are fixed, cannot see such a
    kernel); at recip_inexact's 0.445, and at most of the mixed profile's variances, it does not."""
    s = np.random.default_rng(5).uniform(0.0, 40.0, 1_000_000)
    differ = lambda r: float(np.mean(s / r != s * (1.0 / r)))
    assert differ(0.5) == 0.0 and differ(0.3) == 0.0 and differ(0.6) == 0.0
    assert differ(sf.gen("recip_inexact", "directed").runs[0].r_var) > 0.5
    mixed = [differ(r.r_var) for n in sf.MIXED_SEEDS for r in sf.gen(n).runs]
    assert sum(d > 0.1 for d in mixed) >= 0.7 * len(mixed)


def test_counter_bounds_follow_the_prediction():
    """counter_bounds: (missed_steps' growth, replays' growth) from one run's prediction"""
    run = sf.Run(np.zeros((6, 2)))
    none = {"miss": [], "hold": [2, 3, 4, 5, 6], "undetermined": []}
    assert sf.counter_bounds(run, none) == ((0, 0), (0, 0))
    assert sf.counter_bounds(run, {"miss": [6], "hold": [2, 3, 4, 5], "undetermined": []}) == ((1, 1), (1, 1))
    assert sf.counter_bounds(run, {"miss": [3, 5], "hold": [2, 4, 6], "undetermined": []}) == ((1, 4), (1, 1))
    assert sf.counter_bounds(run, {"miss": [5], "hold": [2, 3, 6], "undetermined": [4]}) == ((0, 3), (0, 1))
    assert sf.counter_bounds(run, {"miss": [3], "hold": [2, 4, 6], "undetermined": [5]}) == ((1, 4), (1, 1))
    multinomial = sf.Run(np.zeros((6, 2)), scheme=abi.RESAMPLE_MULTINOMIAL)
    assert sf.counter_bounds(multinomial, {"miss": [3], "hold": [2, 4, 5, 6], "undetermined": []}) == ((0, 0), (0, 0))


def test_directed_cases_are_what_their_names_say(cases):
    for name in ("collapse_5001", "collapse_70001"):
        assert max(_trace(name)[0].top) > 0.5, name          # one particle holds more than half the weight
    a, b, c = (tr.flags for tr in _trace("recip_inexact"))
    assert not any(a) and all(b[1:]) and c[-2] and not c[-1]      # raw weights after runs 0 and 2
    assert cases["recip_inexact"].routes() == ["fused"] * 3 and cases["recip"].routes() == ["fused"] * 2
    assert cases["loose"].runs[0].ess == 0.5 and not any(_trace("loose")[0].flags)
    assert max(_trace("loose")[0].top) < 2.0 / cases["loose"].N     # nearly flat
    ev = _trace("huge_obs")[0].log_evidence
    assert ev == -np.inf or np.isnan(ev)
    for name in ("inf_obs", "huge_obs", "nan_obs"):
        tr = _trace(name)[0]
        assert any(tr.flags[:4]) and not any(tr.flags[4:]), name    # no Resample from the degenerate step on
    r = cases["lpmax_positive"].runs[0]
    assert -(2 * np.log(2 * np.pi) + 2 * np.log(r.r_var)) * 0.5 > 0
    for T in (1, 2, 3):
        for N in (1025, 16385):
            assert [cases[f"t{T}_{N}_{g}"].runs[0].T for g in ("forced", "gated")] == [T, T]


# ---- the comparer and the replay ---------------------------------------------------------------
def _planted(at_run, column):
    """an oracle behind ssm2d_run that moves one value of one column by one ulp after run `at_run`"""
    class Planted(sf.oracle_context()):
        done = 0

        def ssm2d_run(self, obs, *a, **kw):
            ev = super().ssm2d_run(obs, *a, **kw)
            if self.done == at_run:
                cid = self.col_find(column)
                if cid >= 0:        # (a horizon too short to have the column: nothing planted)
                    v = self.col_download(cid)
                    v[1, self.n // 2] = np.nextafter(v[1, self.n // 2], np.inf)
                    self.col_upload(cid, v)
            self.done += 1
            return ev

    return Planted


@pytest.mark.parametrize("drive", ["sync", "async"])
def test_comparer_reports_a_planted_ulp_at_its_run(cases, drive, capsys):
    c = cases["grow_T"]
    assert sf.differential(c, "oracle", drive)                      # the oracle against itself: no difference
    with pytest.raises(sf.Mismatch) as e:
        sf.differential(c, _planted(1, "x_7"), drive)
    msg = str(e.value)
    assert "after run 1: column x_7: 1 of" in msg if drive == "sync" else "column x_7: 1 of" in msg
    assert "first differing step of run 1: 6:" in msg               # x_7 exists from horizon 6 on
    assert sf.replay(c, drive) in msg and sf.replay(c, drive) in capsys.readouterr().out


def test_comparer_sees_weights_state_and_evidence(cases):
    c = cases["param_switch"]

    class Reweighted(sf.oracle_context()):
        def ssm2d_run(self, obs, *a, **kw):
            ev = super().ssm2d_run(obs, *a, **kw)
            w = self.weights_download()
            w[0] = np.nextafter(w[0], -np.inf)
            self.weights_upload(w)
            return ev

    with pytest.raises(sf.Mismatch, match="after run 0: weights: 1 of 4097"):
        sf.differential(c, Reweighted, "sync")

    class WrongEvidence(sf.oracle_context()):
        def ssm2d_run(self, obs, *a, **kw):
            ev = super().ssm2d_run(obs, *a, **kw)
            return None if ev is None else np.nextafter(ev, 0.0)

    with pytest.raises(sf.Mismatch, match="after run 0: the run's log evidence"):
        sf.differential(c, WrongEvidence, "sync")


@pytest.mark.parametrize("argv", [["--name", "recip"], ["--seed", "3", "--profile", "mixed", "--drive", "async"],
                                  ["--name", "param_switch", "--drive", "island2"]])
def test_replay_line_runs_on_the_oracle(argv, capsys):
    assert sf.main(argv + ["--backend", "oracle"]) == 0
    out = capsys.readouterr().out
    assert "same as the oracle" in out and "python tests/ssm2dfuzz.py" in out

"""The random fused 1D-LGSSM corpus (tests/lgssmfuzz.py) on the CPU: what
tests/test_gpu_lgssm_random_runs.py holds the device to is right by arithmetic that shares no header
with it (tests/test_independent_math.py, case (f)), and the corpus reaches what it is for (asserted
below: sizes, horizons, thresholds, parameters that are no powers of two, gates that go both ways,
collapsed and degenerate weights, the routes of the sequences)."""
import math
import pathlib
import re

import numpy as np
import pytest

import lgssmfuzz as lf
from progfuzz import same_value
from wsmc import abi

MIXED = [f"mixed-{s}" for s in lf.MIXED_SEEDS]
# run 0 of: N = 129 forced stratified; 4096 forced systematic; 4097 gated (0.3) systematic; 1000 gated (0.3) stratified
INDEPENDENT_SEEDS = (7, 15, 16, 20)
INDEPENDENT = ["recip_inexact", "neg_a", "collapse_1025"] + [f"mixed-{s}" for s in INDEPENDENT_SEEDS]


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in lf.corpus()}


def _trace(name):
    return lf.trace_of(name)    # (one oracle pass a case, shared by the tests below)


def independent_args(case, **par):
    """run_lgssm_checked's arguments for a case's first run (its first six steps)"""
    run = case.runs[0]
    kw = dict(a=run.a, q=run.q, r=run.r, x0_std=run.x0_std)
    kw.update(par)
    return dict(n=case.n(), data=run.data[:6], ess_min=run.ess, scheme=run.scheme, seed=case.ctx_seed, **kw)


# ---- q, r and x0_std are standard deviations, a the multiplier, by arithmetic that shares no header ----
@pytest.mark.parametrize("name", INDEPENDENT)
def test_parameters_match_reference_math(cases, name):
    from test_independent_math import run_lgssm_checked
    n_rs, ties = run_lgssm_checked("oracle", **independent_args(cases[name]))
    print(f"{name}: {n_rs} steps resampled, {ties} ancestor ties")
    assert n_rs >= 1 and ties <= 2       # (a step's own allowance: test_resample_reference.check_against_reference)


def test_independent_cases_cover_forced_gated_and_both_schemes(cases):
    runs = [cases[f"mixed-{s}"].runs[0] for s in INDEPENDENT_SEEDS]
    assert {r.scheme for r in runs} == {abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC}
    assert any(r.ess == 1.0 for r in runs) and any(r.ess < 1.0 for r in runs)
    for s, r in zip(INDEPENDENT_SEEDS, runs):
        flags = _trace(f"mixed-{s}")[0].flags[:6]
        assert all(flags) if r.ess == 1.0 else (any(flags) and not all(flags)), s


# ---- the corpus reaches what it is for -----------------------------------------------------------
def test_constants_are_the_librarys():
    src = (pathlib.Path(__file__).resolve().parents[1] / "weightedsampling.jl_amd/csrc/wsmc_internal.h").read_text()
    assert int(re.search(r"constexpr int kLgCap = (\d+);", src).group(1)) == lf.CAP
    assert int(re.search(r"constexpr int kLgSegmentSteps = (\d+);", src).group(1)) == lf.DEFAULT_SEGMENT


def _particles_a_thread(n):
    """wsmc_lgssm1d_run's layout: threads = max(64, min(1024, ceil(N / 128) 64)), P = ceil(N / threads)"""
    threads = max(64, min(1024, -(-n // 128) * 64))
    return -(-n // threads)


def test_corpus_covers_sizes_horizons_schemes_thresholds_and_options(cases):
    mixed = [cases[n] for n in MIXED]
    assert {c.N for c in mixed} >= set(lf.NS) and all(c.n() <= lf.CAP for c in mixed)
    assert {_particles_a_thread(c.n()) for c in mixed} == {1, 2, 3, 4, 5}
    runs = [r for c in mixed for r in c.runs]
    assert {r.T for r in runs} == set(range(1, lf.T_MAX + 1))
    assert {r.scheme for r in runs} == {abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC}
    assert {r.ess for r in runs} == set(lf.ESS)
    assert {len(c.runs) for c in mixed} == {1, 2, 3}
    assert sum(c.lazy for c in mixed) == len(mixed) // 2
    segs = set()
    for r in runs:
        segs |= {r.segment} & {None, 1, 2, 3, 7}
        segs |= {"T"} if r.segment == r.T else {"T+1"} if r.segment == r.T + 1 else set()
    assert segs == {None, 1, 2, 3, 7, "T", "T+1"}
    for what in ("want_evidence", "ess_trace"):
        off = sum(not getattr(r, what) for r in runs)
        assert 0.1 * len(runs) <= off <= 0.4 * len(runs), (what, off, len(runs))
    for r in runs:
        assert 0.0 < abs(r.a) < 1.1 and 10 ** -1.5 <= r.q <= 10.0 and 0.1 <= r.x0_std <= 10.0
        lo, hi = lf.RATIO_LOG10[r.ess]
        assert lo - 1e-9 <= np.log10(r.r / r.q) <= hi + 1e-9
        assert not any(lf._pow2(v) for v in (r.q, r.r, r.x0_std)) and not lf._dyadic(r.a)
    assert any(r.a < 0 for r in runs) and any(r.a > 0 for r in runs) and any(abs(r.a) > 1 for r in runs)
    assert len([c for c in mixed if int(c.name[6:]) % 5 == 0]) == 7          # the outliers
    seeds = [c.ctx_seed for c in mixed]
    assert len(set(seeds)) == len(seeds) and all(0 <= s < 2 ** 64 for s in seeds)
    assert sum(s >= 2 ** 63 for s in seeds) >= 1 and sum(s >= 2 ** 32 for s in seeds) >= 30
    assert all(route == "persistent" for c in mixed for route in c.routes())


def test_directed_list_is_the_issues(cases):
    want = ([f"p_boundaries_{N}_{g}" for N in (2048, 2049, 3072, 3073, 4096, 4097) for g in ("forced", "gated")] +
            ["cap", "cap+1", "recip_inexact", "unit_a", "zero_a", "negzero_a", "neg_a", "explosive", "collapse_1025",
             "collapse_4097", "loose", "nan_obs", "inf_obs", "neginf_obs_mid", "huge_obs", "param_switch", "grow_shrink_T",
             "route_flip", "own_x", "own_x_eager", "foreign_column", "multinomial", "then_statements", "seg_every_step"] +
            list(lf.THRESHOLDS) + list(lf.NONFINITE))
    assert sorted(want) == sorted(lf.DIRECTED)
    assert all(c.n(lf.CAP) <= lf.CAP + 1 and all(r.T <= lf.T_MAX for r in c.runs) for c in cases.values())


def test_directed_cases_are_what_their_names_say(cases):
    one = lambda name: cases[name].runs[0]
    for N, P in ((2048, 2), (2049, 3), (3072, 3), (3073, 4), (4096, 4), (4097, 5)):
        assert _particles_a_thread(N) == P
        for tag, ess in (("forced", 1.0), ("gated", 0.5)):
            c = cases[f"p_boundaries_{N}_{tag}"]
            assert (c.N, one(c.name).T, one(c.name).ess) == (N, 3, ess)
    for name in ("cap", "cap+1"):
        assert cases[name].N == name and [r.ess for r in cases[name].runs] == [1.0, 0.5]
    assert cases["cap"].n(4096) == 4096 and cases["cap+1"].n(4096) == 4097
    assert (one("recip_inexact").r, one("recip_inexact").q) == (0.3, 0.07)
    assert one("unit_a").a == 1.0 and one("neg_a").a == -0.95
    assert (one("explosive").a, one("explosive").T) == (1.1, 12)
    z, nz = one("zero_a"), one("negzero_a")
    assert z.a == 0.0 and nz.a == 0.0 and math.copysign(1.0, z.a) == 1.0 and math.copysign(1.0, nz.a) == -1.0
    assert np.array_equal(z.data, nz.data)
    for name in ("collapse_1025", "collapse_4097"):
        assert one(name).r == 1e-3 * one(name).q and one(name).ess == 1.0
    assert one("loose").r == 1e3 * one("loose").q and one("loose").ess == 0.5
    assert [one(n).ess for n in lf.THRESHOLDS][:4] == [0.0, -1.0, 2.0, math.inf] and math.isnan(one("thresholds_nan").ess)
    at = lf.DEGENERATE_AT
    assert math.isnan(one("nan_obs").data[at]) and one("inf_obs").data[at] == math.inf and one("huge_obs").data[at] == 1e308
    assert one("neginf_obs_mid").data[one("neginf_obs_mid").T // 2] == -math.inf
    nf = {n: one(n) for n in lf.NONFINITE}
    assert math.isnan(nf["nonfinite_a_nan"].a) and nf["nonfinite_a_inf"].a == math.inf and nf["nonfinite_r_inf"].r == math.inf
    assert nf["nonfinite_r_denormal"].r == 5e-324 and nf["nonfinite_q_inf"].q == math.inf and nf["nonfinite_x0_huge"].x0_std == 1e300
    assert all(np.all(np.isfinite(r.data)) for r in nf.values())
    ps = cases["param_switch"].runs          # A, B, A, A, B
    assert [r.kw() == ps[0].kw() for r in ps] == [True, False, True, True, False] and ps[1].kw() == ps[4].kw()
    assert all(r.data is ps[0].data for r in ps)
    assert [r.T for r in cases["grow_shrink_T"].runs] == [3, 9, 2]
    flip = cases["route_flip"].runs
    assert [st[0] for st in flip[1].before] == ["weight"] and flip[3].before == (("resample", 2.0, abi.RESAMPLE_STRATIFIED),)
    assert not flip[0].before and not flip[2].before
    for name, lazy in (("own_x", True), ("own_x_eager", False)):
        c = cases[name]
        assert c.lazy is lazy and [st[0] for st in c.prelude] == ["col", "sample", "observe", "resample"]
        assert c.prelude[0] == ("col", "x", 1) and c.prelude[3][1] == 2.0
    assert cases["foreign_column"].prelude[0] == ("col", "y", 1)
    assert one("multinomial").scheme == abi.RESAMPLE_MULTINOMIAL
    assert [st[0] for st in cases["then_statements"].tail] == ["move", "move", "col", "sample", "observe", "resample", "moments",
                                                               "median", "sample_particles"]
    assert [st[1] for st in cases["then_statements"].tail[:2]] == ["rw", "autorw"]
    s = one("seg_every_step")
    assert (s.segment, s.T, s.ess) == (1, 12, 0.5)
    f = _trace("seg_every_step")[0].flags
    assert any(f) and not all(f) and any(a and not b for a, b in zip(f, f[1:]))      # a row that crosses a quiet segment


def test_routes(cases):
    assert cases["route_flip"].routes() == ["persistent", "statements", "persistent", "persistent"]
    assert cases["foreign_column"].routes() == ["statements", "statements"]
    assert cases["cap"].routes() == ["persistent", "persistent"] and cases["cap+1"].routes() == ["statements", "statements"]
    assert cases["cap"].routes(4096) == ["persistent", "persistent"] and cases["cap+1"].routes(4096) == ["statements"] * 2
    assert cases["multinomial"].routes() == ["statements"] == cases["nonfinite_a_inf_statements"].routes()
    assert all(cases[n].routes() == ["persistent"] for n in lf.NONFINITE if n != "nonfinite_a_inf_statements")
    assert cases["grow_shrink_T"].routes() == ["persistent"] * 3 and cases["param_switch"].routes() == ["persistent"] * 5
    assert cases["own_x"].routes() == ["persistent"] and cases["then_statements"].routes() == ["persistent"]
    # the rule's other clauses, one at a time
    run = cases["own_x"].runs[0]
    assert lf.Case("c", 100, (run,), prelude=(("col", "x", 2),)).routes() == ["statements"]
    assert lf.Case("c", 100, (run,), prelude=lf.OWN_X_PRELUDE[:3]).routes() == ["statements"]     # no Resample after the Observe


def test_own_x_prelude_resamples():
    """the prelude's Resample at 2.0 runs, so a lazy store enters the run with a logged Resample on x"""
    o = lf._recording()(1025, seed=42)
    for st in lf.OWN_X_PRELUDE:
        lf.issue(o, st)
    assert o.resamples == [(True, o.resamples[0][1])] and o.get_state()["n_resamples"] == 1
    o.close()


def test_gated_runs_go_both_ways(cases):
    """Among the mixed profile's gated runs with N >= 65 and T >= 4, at least 10 exist and at least
    80 % have both a resampled and a non-resampled step (lgssmfuzz.RATIO_LOG10 draws r / q by
    threshold for this; the condition is the issue's)."""
    both = []
    for name in MIXED:
        for run, tr in zip(cases[name].runs, _trace(name)):
            if run.ess < 1.0 and cases[name].n() >= 65 and run.T >= 4:
                both.append(any(tr.flags) and not all(tr.flags))
    print(f"gated runs going both ways: {sum(both)} of {len(both)}")
    assert len(both) >= 10
    assert sum(both) >= 0.8 * len(both)


def test_collapse_cases_collapse(cases):
    for name in ("collapse_1025", "collapse_4097"):
        tr = _trace(name)[0]
        assert all(tr.flags) and float(np.min(tr.ess)) * cases[name].n() < 2.0, name     # one particle takes nearly all weight
    tr = _trace("loose")[0]
    assert not any(tr.flags) and float(np.min(tr.ess)) > 0.99


def test_zero_and_negative_zero_a_give_the_same_bits():
    a, b = _trace("zero_a")[0], _trace("negzero_a")[0]
    assert a.flags == b.flags and same_value(a.ess, b.ess) and same_value(a.log_evidence, b.log_evidence)
    assert same_value(a.weights, b.weights) and same_value(a.x, b.x)


# the oracle's flags, written down from its run
DEGENERATE_FLAGS = {
    "thresholds_0": [False] * 6, "thresholds_neg1": [False] * 6, "thresholds_2": [True] * 6, "thresholds_inf": [True] * 6,
    "thresholds_nan": [False] * 6,
    "nan_obs": [True] * 4 + [False] * 4, "inf_obs": [True] * 4 + [False] * 4, "huge_obs": [True] * 4 + [False] * 4,
    "neginf_obs_mid": [True, False, False, True] + [False] * 5,
    **{n: [False] * 4 for n in lf.NONFINITE},
}


@pytest.mark.parametrize("name", list(DEGENERATE_FLAGS))
def test_degenerate_cases_give_the_expected_flags(cases, name):
    tr = _trace(name)[0]
    assert tr.flags == DEGENERATE_FLAGS[name]
    if name.startswith("thresholds"):
        assert math.isfinite(tr.log_evidence) and np.all(np.isfinite(tr.ess))
        return
    # from the degenerate step on every weight is -inf or NaN, the ESS% NaN, the evidence NaN, and no
    # step resamples (Q = 0)
    first = {"neginf_obs_mid": 4}.get(name, lf.DEGENERATE_AT if name.endswith("_obs") else 0)
    assert np.all(np.isfinite(tr.ess[:first])) and np.all(np.isnan(tr.ess[first:]))
    assert math.isnan(tr.log_evidence)
    assert np.all(np.isnan(tr.weights) | np.isneginf(tr.weights))
    if name in ("nan_obs", "nonfinite_a_nan"):
        assert np.all(np.isnan(tr.weights))


def test_infinite_multiplier_is_inf_times_x_in_the_statements():
    """Found by nonfinite_a_inf on the device: `Col("x") * inf` scaled the operand's absent constant too
    (0.0 * inf), so models.lgssm1d_statements drew NaN where a x is +-inf (the library's own
    operand, csrc lg_normal, has the constant 0.0, on both of its routes). The product of a
    column and a non-finite constant keeps the constant 0.0."""
    from wsmc.dsl import Col, Normal
    for a in (math.inf, -math.inf, math.nan):
        d = Normal(Col("x") * a, 0.45).dist(lambda name: 0)
        assert d.mu[0].c0 == 0.0 and d.mu[0].col[0] == 0 and same_value(d.mu[0].coef[0], a)
        assert same_value((Col("x") * a + 1.5).c0, 1.5)
    assert same_value((Col("x") * -2.0).c0, -0.0) and same_value(((Col("x") + 1.5) * math.inf).c0, math.inf)   # as before
    for name in ("nonfinite_a_inf", "nonfinite_a_inf_statements"):
        x = _trace(name)[0].x
        assert np.all(np.isinf(x)) and np.any(x > 0) and np.any(x < 0)
    assert np.all(np.isnan(_trace("nonfinite_a_nan")[0].x))


def test_reciprocal_differs_from_division_in_the_mixed_profile():
    """What makes a kernel that multiplies by 1 / r differ from one that divides: the rounding of the
    reciprocal. At 0.5 (the only r the earlier tests sent) it is exact, and at the double 0.3
    (recip_inexact) the product equals the quotient for every s all the same; at most of the mixed
    profile's r it does not."""
    s = np.random.default_rng(5).uniform(0.0, 40.0, 200_000)
    differ = lambda r: float(np.mean(s / r != s * (1.0 / r)))
    assert differ(0.5) == 0.0
    mixed = [differ(r.r) for n in lf.MIXED_SEEDS for r in lf.gen(n).runs]
    assert sum(d > 0.1 for d in mixed) >= 0.7 * len(mixed)


# ---- the comparer and the replay ---------------------------------------------------------------
def _planted(at_run):
    """an oracle behind lgssm1d_run that moves one value of x by one ulp after run `at_run`"""
    class Planted(lf.oracle_context()):
        done = 0

        def lgssm1d_run(self, data, *a, **kw):
            out = super().lgssm1d_run(data, *a, **kw)
            if self.done == at_run and len(data) >= 6:
                cid = self.col_find("x")
                v = self.col_download(cid)
                v[self.n // 2] = np.nextafter(v[self.n // 2], np.inf)
                self.col_upload(cid, v)
            self.done += 1
            return out

    return Planted


def test_comparer_reports_a_planted_ulp_at_its_run(cases, capsys):
    c = cases["grow_shrink_T"]
    assert lf.differential(c, "oracle") == [tr.flags for tr in _trace(c.name)]      # the oracle against itself
    with pytest.raises(lf.Mismatch) as e:
        lf.differential(c, _planted(1))
    msg = str(e.value)
    assert "after run 1: column x: 1 of 4097" in msg
    assert "first differing step of run 1: 6:" in msg               # planted from horizon 6 on
    assert lf.replay(c) in msg and lf.replay(c) in capsys.readouterr().out


def test_comparer_sees_weights_evidence_trace_tape_and_returns(cases):
    c = cases["then_statements"]

    class Reweighted(lf.oracle_context()):
        def lgssm1d_run(self, data, *a, **kw):
            out = super().lgssm1d_run(data, *a, **kw)
            w = self.weights_download()
            w[0] = np.nextafter(w[0], -np.inf)
            self.weights_upload(w)
            return out

    with pytest.raises(lf.Mismatch, match="after run 0: weights: 1 of 1025"):
        lf.differential(c, Reweighted)

    class WrongEvidence(lf.oracle_context()):
        def lgssm1d_run(self, data, *a, **kw):
            ev, tr = super().lgssm1d_run(data, *a, **kw)
            return np.nextafter(ev, 0.0), tr

    with pytest.raises(lf.Mismatch, match="after run 0: the run's log evidence"):
        lf.differential(c, WrongEvidence)

    class WrongTrace(lf.oracle_context()):
        def lgssm1d_run(self, data, *a, **kw):
            ev, tr = super().lgssm1d_run(data, *a, **kw)
            tr[-1] = np.nextafter(tr[-1], 0.0)
            return ev, tr

    with pytest.raises(lf.Mismatch, match=r"after run 0: ESS trace \(by step\): 1 of"):
        lf.differential(c, WrongTrace)

    class WrongTape(lf.oracle_context()):
        def score(self, d):
            s = super().score(d)
            if d == 6:           # the run's mid depth (13 terms: the prior and six steps of two)
                s[3] = np.nextafter(s[3], 0.0)
            return s

    with pytest.raises(lf.Mismatch, match=r"after run 0: score\(6\): 1 of 1025"):
        lf.differential(c, WrongTape)

    class WrongMedian(lf.oracle_context()):
        def weighted_median(self, *a):
            return np.nextafter(super().weighted_median(*a), np.inf)

    with pytest.raises(lf.Mismatch, match=r"after run 1: tail \('median', 'x'\) returned"):
        lf.differential(c, WrongMedian)


def test_exchanged_parameters_show_in_the_corpus_and_not_at_the_old_point(cases):
    """At q = x0_std = 1 (all that tests/test_gpu_lgssm_run.py sends) a run that exchanged q and x0_std
    is the same run. The mixed cases tell the exchange apart, and a run that took r for a variance."""
    class Exchanged(lf.oracle_context()):
        def lgssm1d_run(self, data, a=0.9, q=1.0, r=0.5, x0_std=1.0, **kw):
            return super().lgssm1d_run(data, a=a, q=x0_std, r=r, x0_std=q, **kw)

    class Variance(lf.oracle_context()):
        def lgssm1d_run(self, data, a=0.9, q=1.0, r=0.5, x0_std=1.0, **kw):
            return super().lgssm1d_run(data, a=a, q=q, r=math.sqrt(r), x0_std=x0_std, **kw)

    old = lf.Case("old_point", 1000, (lf.Run(cases["seg_every_step"].runs[0].data, 0.9, 1.0, 0.5, 1.0, 0.5),))
    assert lf.differential(old, Exchanged)
    for seed in lf.MIXED_SEEDS[1::4]:
        for planted in (Exchanged, Variance):
            with pytest.raises(lf.Mismatch, match="after run 0"):
                lf.differential(cases[f"mixed-{seed}"], planted)


@pytest.mark.parametrize("argv", [["--seed", "3", "--profile", "mixed"], ["--name", "route_flip"], ["--name", "then_statements"],
                                  ["--name", "own_x"]])
def test_replay_line_runs_on_the_oracle(argv, capsys):
    assert lf.main(argv + ["--backend", "oracle"]) == 0
    out = capsys.readouterr().out
    assert "same as the oracle" in out and "python tests/lgssmfuzz.py" in out

"""The random-spec corpus of the fused run on the CPU (tests/ssmfuzz.py): that every spec is one
wsmc_ssm_spec_check takes, what the seed lists of tests/test_gpu_ssm_random_specs.py cover and how
their runs come out on the oracle, so that the GPU file cannot quietly go vacuous; the generator's
determinism; the comparer's and the locator's teeth; a raw struct against the builder."""
import ctypes as C
import math

import numpy as np
import pytest

import ssmfuzz as sf
import wsmc
from oracle import Oracle
from wsmc import abi, dsl
from wsmc.dsl import Col, Data, Normal
from wsmc.ssm import SSM, assign, observe, sample

N = 1001


oracle_context = sf.oracle_context   # the oracle behind Context.ssm_run's interface


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sf.corpus()}


@pytest.fixture(scope="module")
def mixed_runs(cases):
    """every `mixed` case once on the oracle at ess 0.5: name -> (flags, trace, evidence, weights, state)"""
    out = {}
    for s in sf.MIXED_SEEDS:
        c = cases[f"mixed-{s}"]
        o = Oracle(N, seed=sf.SEED)
        flags, trace = c.ssm.statements(o, c.data, ess_perc_min=0.5, T=c.T)
        out[c.name] = (flags, trace, o.log_evidence(), o.weights_download(), o.get_state())
        o.close()
    return out


# ---- validity and determinism -----------------------------------------------------------------
def test_every_spec_passes_the_checker(cases):
    L = wsmc.load_library()
    assert len(cases) == len(sf.MIXED_SEEDS) + len(sf.DIRECTED)
    for c in cases.values():
        assert L.wsmc_ssm_spec_check(C.byref(c.spec)) == abi.WSMC_OK, (c.name, L.wsmc_last_error().decode(), c.text())
        assert c.T == sf.T == 24
        assert (c.data is None) == (c.data_dim == 0) and (c.data is None or c.data.shape == (c.T, c.data_dim))
        # the program instructions counted as wsmc_ssm_run counts them: prog97 alone is past the limit
        assert (c.n_prog > abi.XPROG_MAX) == (c.name == "prog97"), (c.name, c.n_prog)
    assert cases["prog96"].n_prog == 96 and cases["prog97"].n_prog == 97
    # ... and past that limit alone: its longest program is one the kernel takes
    sp = cases["prog97"].spec
    assert max(sp.step[q].prog_len for q in range(sp.n_step)) == abi.SSM_XPROG_MAX


def test_generator_is_deterministic():
    for a, b in zip(sf.corpus(), sf.corpus()):
        assert a.name == b.name and a.lines == b.lines
        assert bytes(a.spec) == bytes(b.spec), a.name
        assert (a.data is None and b.data is None) or a.data.tobytes() == b.data.tobytes(), a.name


# ---- coverage ---------------------------------------------------------------------------------
def _operands(c):
    """(position, Opnd, where) of every operand of a case"""
    for where, k, s in c.statements():
        if s[0] in ("sample", "observe"):
            yield "mean", s[2].mu, where
            yield "scale", s[2].scale, where
        if s[0] == "observe":
            yield "value", s[1], where
        if s[0] == "assign":
            yield "assign", s[2], where


def test_corpus_covers_the_vocabulary(cases):
    sampled, observed, xops, forms, slot1_alone = set(), set(), set(), set(), 0
    n_cols, data_dim, n_init, n_step, n_obs = set(), set(), set(), set(), set()
    feats = {0: 0, 1: 0, 2: 0}
    first_obs = last_other = init_obs = 0
    for c in cases.values():
        feats[c.feat()] += 1
        n_cols.add(c.n_cols), data_dim.add(c.data_dim), n_init.add(len(c.init)), n_step.add(len(c.step))
        n_obs.add(sum(s[0] == "observe" for s in c.step))
        first_obs += c.step[0][0] == "observe"
        last_other += c.step[-1][0] != "observe"
        init_obs += any(s[0] == "observe" for s in c.init)
        for where, k, s in c.statements():
            if s[0] == "sample":
                sampled.add(s[2].fam)
            elif s[0] == "observe":
                observed.add(s[2].fam)
            elif s[0] == "expr":
                xops |= sf.tree_ops(s[2])
        for position, o, where in _operands(c):
            forms.add((position, o.form))
            slot1_alone += o.slots[0] is None and o.slots[1] is not None and o.slots[1][0] == "data"
    fams = set(sf.SCALAR_FAMILIES)
    assert len(fams) == 21
    assert not fams - sampled, f"families in no SAMPLE: {[sf.FAMILIES[f] for f in sorted(fams - sampled)]}"
    assert not fams - observed, f"families in no OBSERVE: {[sf.FAMILIES[f] for f in sorted(fams - observed)]}"
    assert min(feats.values()) >= 4, f"specs by kernel variant (plain, extended, log-Gamma): {feats}"
    missing = set(sf.pf.XOPS_ALL) - xops
    assert not missing, f"WSMC_X_* opcodes in no program: {sorted(missing)}"
    missing = {(p, f) for p in sf.POSITIONS for f in sf.FORMS} - forms
    assert not missing, f"operand forms by position never built: {sorted(missing)}"
    assert slot1_alone > 0, "no operand with its data in slot 1 and slot 0 empty"
    assert n_cols >= {1, 2, 3, 4}, n_cols
    assert data_dim >= {0, 1, 2, 3, 4}, data_dim
    assert n_init >= {0, 4}, n_init
    assert 8 in n_step, n_step
    assert n_obs >= {1, 2, 3}, n_obs
    assert first_obs > 0, "no step starts with an OBSERVE"
    assert last_other > 0, "no step ends with a non-OBSERVE"
    assert init_obs > 0, "no init holds an OBSERVE"


def test_mixed_profile_alone_covers_the_shapes(cases):
    """the seeds' forced choices: what the `mixed` specs cover without the directed ones"""
    mixed = [cases[f"mixed-{s}"] for s in sf.MIXED_SEEDS]
    assert {c.n_cols for c in mixed} == {1, 2, 3, 4}
    assert {c.data_dim for c in mixed} == {0, 1, 2, 3, 4}
    assert {len(c.init) for c in mixed} == {0, 1, 2, 3, 4}
    assert {len(c.step) for c in mixed} >= {3, 8}
    assert {sum(s[0] == "observe" for s in c.step) for c in mixed} == {1, 2, 3}
    assert any(c.step[0][0] == "observe" for c in mixed) and any(c.step[-1][0] != "observe" for c in mixed)
    assert any(s[0] == "observe" for c in mixed for s in c.init)
    assert all(c.n_prog <= abi.XPROG_MAX for c in mixed)
    # data_dim larger than what is read
    def read(c):
        js = {s[1] for _, o, _ in _operands(c) for s in o.slots if s is not None and s[0] == "data"}
        for _, _, s in c.statements():
            if s[0] == "expr":
                js |= {j for n, j in _leaves(s[2]) if n == sf.DATA}
        return js
    assert any(c.data_dim > 0 and max(read(c), default=-1) + 1 < c.data_dim for c in mixed)


def _leaves(t):
    if t[0] == "col":
        yield t[1], t[2]
    elif t[0] != "c":
        for x in (t[2:] if t[0] == abi.X_POWI else t[1:]):
            yield from _leaves(x)


def test_directed_cases_are_what_their_names_say(cases):
    kinds = lambda c: [s[0] for s in c.step]
    c = cases["full"]
    assert (c.n_cols, len(c.init), len(c.step), c.data_dim) == (4, 4, 8, 4)
    lens = [c.spec.step[q].prog_len for q in range(8)]
    assert 32 in lens
    assert max(sf.to_fx(s[2])._need() for s in c.step if s[0] == "expr") == abi.XSTACK_MAX
    assert kinds(cases["observe_first"]) == ["observe", "sample", "observe", "expr", "observe", "sample", "assign"]
    c = cases["nodata"]
    assert c.data_dim == 0 and c.data is None and {o.form for p, o, _ in _operands(c) if p == "value"} == {"const", "col"}
    c = cases["wide_data"]
    assert c.data_dim == 4
    assert [s[1] for p, o, _ in _operands(c) for s in o.slots if s is not None and s[0] == "data"] == [3]
    assert [j for _, _, s in c.statements() if s[0] == "expr" for n, j in _leaves(s[2]) if n == sf.DATA] == [1]
    assert len(cases["no_init"].init) == 0 and len(cases["pre_state"].init) == 0
    assert [s[0] for s in cases["init_observe"].init].count("observe") == 2
    ops = set()
    for s in cases["all_xops"].step:
        if s[0] == "expr":
            ops |= sf.tree_ops(s[2])
    assert ops == set(sf.pf.XOPS_ALL), sorted(set(sf.pf.XOPS_ALL) - ops)


def test_gpu_axes_are_each_met_four_times():
    import test_gpu_ssm_random_specs as gpu
    met = {}
    for seed in sf.MIXED_SEEDS:
        n, ess, scheme, segment = gpu.rotated(seed)
        for axis, v in (("N", n), ("ess", ess), ("scheme", scheme), ("segment", segment)):
            met.setdefault((axis, v), set()).add(seed)
    want = ({("N", v) for v in (1, 65, 2049)} | {("ess", v) for v in (1.0, 0.5)} |
            {("scheme", v) for v in (abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC)} |
            {("segment", v) for v in (1, 5, None)})
    assert set(met) == want
    assert min(len(v) for v in met.values()) >= 4, {k: len(v) for k, v in met.items()}


# ---- outcomes on the oracle -------------------------------------------------------------------
def test_mixed_outcomes(mixed_runs):
    flags_all, both = [], 0
    for name, (flags, trace, ev, w, state) in mixed_runs.items():
        assert len(flags) == sf.T and len(trace) == sf.T
        assert math.isfinite(ev), (name, ev)
        assert not np.all(np.isneginf(w)), name
        assert not np.any(np.isnan(w)), name
        flags_all += flags
        both += 0 < sum(flags) < len(flags)
    frac = sum(flags_all) / len(flags_all)
    assert 0.2 <= frac <= 0.8, f"{frac:.3f} of the traced Resamples resample"
    assert both >= 18, f"{both} of {len(mixed_runs)} specs show both outcomes"


def test_init_observe_resamples_in_init(cases):
    c = cases["init_observe"]
    for ess in (1.0, 0.5):
        o = Oracle(N, seed=sf.SEED)
        flags, _ = c.ssm.statements(o, c.data[:1], ess_perc_min=ess, T=1)
        assert o.get_state()["n_resamples"] - int(flags[0]) >= 1, ess
        o.close()


@pytest.mark.parametrize("name", sf.THRESHOLDS)
def test_thresholds_draws_from_every_branch(cases, name):
    """neighbouring particles take different sampler branches: at every step every named parameter
    value is chosen for many particles (n / 4 or n / 2 expected), interleaved"""
    class Spy(Oracle):
        def assign_expr(self, out, prog, lens):
            super().assign_expr(out, prog, lens)
            chosen.append(self.col_download(out))

    c = cases[name]
    for n in (65, 2049):
        chosen = []
        o = Spy(n, seed=sf.SEED)
        c.ssm.statements(o, c.data, ess_perc_min=0.5, T=c.T)
        o.close()
        assert len(chosen) == c.T
        for t, p in enumerate(chosen):
            for v in set(sf.THRESHOLD_VALUES[name]):
                assert np.sum(p == v) >= n // 16, (name, n, t, v, int(np.sum(p == v)))
            # ... some thread's consecutive particles (P = 2, 3) differ
            assert np.sum(p[1:] != p[:-1]) >= n // 4


def test_all_xops_reaches_nan_and_both_infinities(cases):
    c = cases["all_xops"]
    o = Oracle(N, seed=sf.SEED)
    c.ssm.statements(o, c.data, ess_perc_min=0.5, T=c.T)
    w = np.concatenate([o.col_download(k) for k in (1, 2, 3)])
    o.close()
    assert np.any(np.isnan(w)) and np.any(np.isposinf(w)) and np.any(np.isneginf(w)) and np.any(np.isfinite(w))


def test_partial_support_outcomes(cases):
    c = cases["partial_support"]
    for ess in (1.0, 0.5):
        o = Oracle(N, seed=sf.SEED)
        flags, trace = c.ssm.statements(o, c.data[:sf.PARTIAL_ALL_AT], ess_perc_min=ess, T=sf.PARTIAL_ALL_AT)
        assert np.all(np.isfinite(trace)) and 0 < sum(flags)
        o.close()
        # a step's OBSERVE alone (no Resample after it would show the zeros): -inf for a subset
        o = Oracle(N, seed=sf.SEED)
        o.sample(o.col_create("x", 1), Normal(0.0, 1.0).dist(lambda n: 0))
        o.observe(dsl.Exponential(1.0).dist(lambda n: 0), [abi.Operand.column(0, c0=float(c.data[0, 0]))])
        w = o.weights_download()
        assert 0 < np.sum(np.isneginf(w)) < N
        o.close()
        o = Oracle(N, seed=sf.SEED)
        flags, trace = c.ssm.statements(o, c.data, ess_perc_min=ess, T=c.T)
        assert np.all(np.isnan(trace[sf.PARTIAL_ALL_AT:])) and np.all(np.isfinite(trace[:sf.PARTIAL_ALL_AT]))
        assert not any(flags[sf.PARTIAL_ALL_AT:]) and np.all(np.isneginf(o.weights_download()))
        o.close()


def test_pre_state_on_the_oracle():
    """the driver's own conditions: its first Resample resamples (lazy genealogy on the device), the
    Move accepts, the second run continues the first"""
    for n in (65, 2049):
        out = sf.run_pre_state(n, 0.5, context=oracle_context)
        assert out["first_resample"][0] is True
        assert 0 < out["accepted"] < n
        assert len(out["flags1"]) == sf.T and len(out["flags2"]) == 10
        assert 0 < sum(out["flags1"]) < sf.T
        assert out["state"]["weights_changed"] == 0


# ---- teeth ------------------------------------------------------------------------------------
def _run(case, n=N, ess=0.5, extra=None):
    o = oracle_context(n)
    ev, trace = o.ssm_run(case.ssm, case.data, ess_perc_min=ess, ess_trace=True, T=case.T)
    if extra:
        extra(o)
    return o, ev, trace


def _replace(case, **kw):
    a = dict(name=case.name, n_cols=case.n_cols, init=case.init, step=case.step, data_dim=case.data_dim, data=case.data, T=case.T)
    a.update(kw)
    return sf.Case(**a)


def test_comparer_sees_nothing_between_two_runs_of_one_case(cases):
    for name in ("mixed-3", "observe_first", "all_xops", "partial_support"):
        (a, ev, tr), (b, _, tr_b) = _run(cases[name]), _run(cases[name])
        assert sf.compare(a, b, ev, tr, tr_b) is None, name


def test_comparer_sees_one_data_value_of_the_last_step(cases):
    c = cases["observe_first"]
    data = c.data.copy()
    data[-1, 1] += 0.125
    (a, ev, tr), (b, _, tr_b) = _run(c), _run(_replace(c, data=data))
    assert sf.compare(a, b, ev, tr, tr_b) is not None
    # ... and the locator finds the step
    other = _replace(c, data=data)

    class Swapped(type(a)):   # the context's side runs the changed data
        def ssm_run(self, spec, d, **kw):
            return super().ssm_run(other.ssm, other.data[:len(d)], **kw)

    step, why = sf.locate(c, 65, 0.5, abi.RESAMPLE_STRATIFIED, None, "persistent", context=lambda n: Swapped(n, seed=sf.SEED))
    assert step == c.T - 1 and why, (step, why)
    with pytest.raises(sf.Mismatch, match=f"first differing step: {c.T - 1}"):
        sf.differential(c, 65, 0.5, context=lambda n: Swapped(n, seed=sf.SEED))


def test_comparer_sees_a_coefficient_moved_by_an_ulp(cases):
    c = cases["observe_first"]
    step = list(c.step)
    kind, col_, d = step[1]
    mu = sf.K(d.mu.c0, sf.col(0, np.nextafter(0.9, 1.0)))
    step[1] = (kind, col_, sf.DistD(d.fam, mu, d.scale))
    (a, ev, tr), (b, _, tr_b) = _run(c), _run(_replace(c, step=step))
    d = sf.compare(a, b, ev, tr, tr_b)
    assert d is not None and d.startswith("column c0"), d


def test_comparer_sees_the_ancestors_of_one_more_resample(cases):
    c = cases["observe_first"]

    def extra(o):
        o.observe(Normal(Col("c0"), 1.0).dist(lambda n: 0), [abi.Operand.const(0.1)])
        o.resample(1.0)

    a, ev, tr = _run(c)
    b, _, tr_b = _run(c, extra=extra)
    assert not sf.same_value(a.last_ancestors(), b.last_ancestors())
    assert sf.compare(a, b, ev, tr, tr_b) is not None
    # the ancestors alone: two runs that differ in nothing else the comparer reads before them
    class SameButAncestors:
        def __init__(self, o, anc):
            self.o, self.anc = o, anc

        def __getattr__(self, k):
            return getattr(self.o, k)

        def last_ancestors(self):
            return self.anc

    anc = a.last_ancestors().copy()
    anc[7] ^= 1
    d = sf.compare(SameButAncestors(a, anc), a, ev, tr, tr)
    assert d is not None and d.startswith("last_ancestors"), d


def test_comparer_tells_signed_zeros_apart_and_matches_nans(cases):
    class Patched:
        def __init__(self, o, w):
            self.o, self.w = o, w

        def __getattr__(self, k):
            return getattr(self.o, k)

        def weights_download(self):
            return self.w

    a, ev, tr = _run(cases["partial_support"])
    assert np.all(np.isnan(tr[sf.PARTIAL_ALL_AT:]))
    assert sf.compare(a, a, ev, tr, tr.copy()) is None          # NaNs equal by position
    tr2 = tr.copy()
    tr2[3], tr2[-1] = math.nan, tr[3]
    assert sf.compare(a, a, ev, tr, tr2) is not None
    b, ev_b, tr_b = _run(cases["nodata"])
    w = b.weights_download()
    assert sf.compare(Patched(b, np.zeros_like(w)), Patched(b, np.zeros_like(w)), ev_b, tr_b, tr_b) is None
    d = sf.compare(Patched(b, np.zeros_like(w)), Patched(b, -np.zeros_like(w)), ev_b, tr_b, tr_b)
    assert d is not None and d.startswith("weights"), d


# ---- a raw struct against the builder ---------------------------------------------------------
def observe_first_by_the_builder():
    x = Col("c0")
    return (SSM(cols=["c0", "c1", "c2"])
            .init(sample("c0", Normal(0.0, 1.0)))
            .step(observe(Data(0), Normal(x, 1.0)),
                  sample("c0", Normal(0.9 * x, 0.5)),
                  observe(Data(1), Normal(0.5 * x, 0.8)),
                  assign("c1", x ** 2 / 20),
                  observe(Data(0), Normal(Col("c1"), 1.5)),
                  sample("c0", Normal(0.95 * x, 0.3)),
                  assign("c2", 2.0 * x + 1.0)))


def test_raw_spec_equals_the_builders(cases):
    c = cases["observe_first"]
    b = observe_first_by_the_builder()
    assert b.spec.data_dim == 2 and bytes(b.spec) == bytes(c.spec)
    assert c.ssm.cols == b.cols and c.ssm.spec.data_dim == b.spec.data_dim
    np.testing.assert_array_equal(c.ssm.table(c.data), b.table(c.data))
    for ess in (1.0, 0.5):
        oa, ob = Oracle(N, seed=sf.SEED), Oracle(N, seed=sf.SEED)
        fa, ta = c.ssm.statements(oa, c.data, ess_perc_min=ess)
        fb, tb = b.statements(ob, c.data, ess_perc_min=ess)
        assert fa == fb
        assert sf.compare(oa, ob, oa.log_evidence(), ta, tb) is None
        assert np.any(oa.score(oa.get_state()["depth"]) != 0.0)
        oa.close(), ob.close()

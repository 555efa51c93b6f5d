"""CPU checks of the two weighting statements of a scalar-SSM spec, the importance Sample
(WSMC_SSM_SAMPLE_IMPORTANCE) and WEIGHT (WSMC_SSM_WEIGHT): what the host-only checker takes and
refuses, the layout of `target`, the builder's lowering, the expansion into statements against the
same statements issued by hand on the oracle, what the corpus of tests/ssmguidedfuzz.py covers (so
that tests/test_gpu_ssm_guided.py cannot quietly go vacuous), and the guided LGSSM's evidence
against the Kalman filter's.
"""
import ctypes as C
import math

import numpy as np
import pytest

import ssmfuzz as sf
import ssmguidedfuzz as gf
import wsmc
from backends import kalman_filter_evidence
from oracle import Oracle
from wsmc import abi, dsl, importance_kernel, models
from wsmc.dsl import Col, Data, Fx, Normal
from wsmc.ssm import SSM, assign, observe, sample, weight

STRAT = abi.RESAMPLE_STRATIFIED


def L():
    return wsmc.load_library()


def check_code(spec) -> int:
    return L().wsmc_ssm_spec_check(C.byref(spec))


def reason() -> str:
    return L().wsmc_last_error().decode()


def clone(spec: abi.SsmSpec) -> abi.SsmSpec:
    r = abi.SsmSpec()
    C.memmove(C.byref(r), C.byref(spec), C.sizeof(abi.SsmSpec))
    return r


def guided() -> abi.SsmSpec:
    """models.lgssm1d_guided(): step[2] is the importance Sample"""
    s = clone(models.lgssm1d_guided().spec)
    assert s.step[2].kind == abi.SSM_SAMPLE_IMPORTANCE
    return s


def refused(spec, word):
    assert check_code(spec) == abi.WSMC_EARG
    assert word in reason(), reason()


# ---- the checker ------------------------------------------------------------------------------
def test_guided_model_passes():
    assert check_code(guided()) == abi.WSMC_OK, reason()
    models.lgssm1d_guided().check()
    models.lgssm1d_guided(gain=0.6, prop_std=0.6).check()


def test_a_spec_of_new_kinds_up_to_the_limits_passes():
    """no cap on the new kinds beyond WSMC_SSM_MAX_INIT / WSMC_SSM_MAX_STMTS"""
    ik = importance_kernel(Normal(Col("x"), 1.0), Normal(0.0, 2.0))
    m = (SSM(cols=["x"]).init(*[sample("x", ik)] * 4)
         .step(*([sample("x", ik)] * 4 + [weight(Col("x"), Normal(0.0, 1.0))] * 3 + [observe(Data(0), Normal(Col("x"), 1.0))])))
    m.check()


@pytest.mark.parametrize("family", [abi.FAM_MVNORMAL_ISO, abi.FAM_MVNORMAL, 15, 24, -1])
def test_refuses_target_family(family):
    s = guided()
    s.step[2].target.family = family
    refused(s, "family")


def test_refuses_target_dim():
    s = guided()
    s.step[2].target.dim = 2
    refused(s, "dim")


def test_refuses_target_mean_function():
    s = guided()
    s.step[2].target.mean_fn = abi.MEAN_OSCILLATOR
    refused(s, "mean")


def test_refuses_target_column_past_n_cols():
    s = guided()
    s.step[2].target.mu[0].col[0] = 3
    refused(s, "past n_cols")
    s = guided()
    s.step[2].target.scale.col[1] = 7
    refused(s, "past n_cols")


def test_refuses_init_reading_data_through_target():
    m = SSM(cols=["x"]).init(sample("x", importance_kernel(Normal(0.0, 1.0), Normal(0.0, 2.0)))) \
        .step(observe(Data(0), Normal(Col("x"), 1.0)))
    s = clone(m.spec)
    assert check_code(s) == abi.WSMC_OK, reason()
    o = s.init[0].target.mu[0]
    o.col[0], o.comp[0], o.coef[0] = abi.OPERAND_DATA, 0, 1.0
    refused(s, "init reads data")


def test_target_operand_rules_are_sample_s():
    s = guided()
    o = s.step[2].target.scale
    o.c0, o.col[0], o.comp[0], o.coef[0] = 0.0, abi.OPERAND_DATA, 0, 2.0
    refused(s, "coef == 1")
    s = guided()
    o = s.step[2].target.mu[0]
    o.col[1], o.comp[1], o.coef[1] = abi.OPERAND_DATA, 5, 1.0
    refused(s, "past data_dim")


def test_weight_takes_observe_s_rules():
    m = SSM(cols=["x"]).init(sample("x", Normal(0.0, 1.0))).step(weight(Col("x"), Normal(0.0, 1.0)), observe(Data(0), Normal(Col("x"), 1.0)))
    s = clone(m.spec)
    assert s.step[0].kind == abi.SSM_WEIGHT and s.step[0].col == -1
    assert check_code(s) == abi.WSMC_OK, reason()
    s.step[0].value.col[0] = 2
    refused(s, "past n_cols")
    s = clone(m.spec)
    s.step[0].dist.family = abi.FAM_MVNORMAL
    refused(s, "family")
    # a WEIGHT is not the OBSERVE a step needs
    s = clone(m.spec)
    s.n_step = 1
    refused(s, "OBSERVE")
    s = clone(m.spec)
    s.step[1].kind = 6
    refused(s, "unknown statement kind")


def test_same_shape_names_the_target():
    a, b = models.lgssm1d_guided(), models.lgssm1d_guided(a=0.7, q=0.4, r=1.5, gain=0.3, prop_std=2.0)
    assert a.same_shape(b)
    for field, setter in (("target.family", lambda t: setattr(t, "family", abi.FAM_LAPLACE)),
                          ("target.mu[0].col[0]", lambda t: t.mu[0].col.__setitem__(0, 0)),
                          ("target.scale.col[1]", lambda t: t.scale.col.__setitem__(1, 2))):
        s = clone(b.spec)
        setter(s.step[2].target)
        assert L().wsmc_ssm_spec_same_shape(C.byref(a.spec), C.byref(s)) == abi.WSMC_EARG
        assert f"step[2].{field}" in reason(), reason()
    # a WEIGHT against an OBSERVE of the same fields: the kind
    s = clone(a.spec)
    s.step[3].kind = abi.SSM_WEIGHT
    assert L().wsmc_ssm_spec_same_shape(C.byref(a.spec), C.byref(s)) == abi.WSMC_EARG
    assert "step[3].kind" in reason(), reason()


def test_layout():
    assert (abi.SSM_SAMPLE_IMPORTANCE, abi.SSM_WEIGHT) == (4, 5)
    assert abi.SsmStmt.target.offset == abi.SsmStmt.prog.offset + C.sizeof(abi.XInst * abi.SSM_XPROG_MAX)
    assert abi.SsmStmt.target.offset + C.sizeof(abi.Dist) == C.sizeof(abi.SsmStmt)
    stmt, spec = C.c_int64(), C.c_int64()
    assert L().wsmc_ssm_spec_sizeof(C.byref(stmt), C.byref(spec)) == abi.WSMC_OK
    assert (stmt.value, spec.value) == (C.sizeof(abi.SsmStmt), C.sizeof(abi.SsmSpec))


# ---- the builder ------------------------------------------------------------------------------
def test_builder_lowering():
    m = models.lgssm1d_guided(a=0.9, q=1.0, r=0.5)
    sp = m.spec
    assert m.cols == ["x", "xp", "m"] and (sp.n_init, sp.n_step, sp.data_dim) == (1, 4, 1)
    assert [sp.step[q].kind for q in range(4)] == [abi.SSM_ASSIGN, abi.SSM_ASSIGN_EXPR, abi.SSM_SAMPLE_IMPORTANCE, abi.SSM_OBSERVE]
    st = sp.step[2]
    gain, std = 1.0 / 1.25, math.sqrt(0.25 / 1.25)
    assert st.col == 0
    assert (st.dist.family, st.dist.mu[0].col[0], st.dist.mu[0].coef[0], st.dist.scale.c0) == (abi.FAM_NORMAL, 2, 1.0, std)
    assert (st.target.family, st.target.mu[0].col[0], st.target.mu[0].coef[0], st.target.scale.c0) == (abi.FAM_NORMAL, 1, 0.9, 1.0)
    assert (st.target.dim, st.target.mean_fn) == (1, abi.MEAN_AFFINE)
    # m .= xp ((1 - gain) a) + gain Data(0): the scaled data read is a leaf of a program
    prog = [(sp.step[1].prog[k].op, sp.step[1].prog[k].col, sp.step[1].prog[k].c) for k in range(sp.step[1].prog_len)]
    assert prog == [(abi.X_CONST, prog[0][1], (1 - gain) * 0.9), (abi.X_COL, 1, 0.0), (abi.X_MUL, prog[2][1], 0.0),
                    (abi.X_CONST, prog[3][1], gain), (abi.X_COL, abi.OPERAND_DATA, 0.0), (abi.X_MUL, prog[5][1], 0.0),
                    (abi.X_ADD, prog[6][1], 0.0)]
    w = SSM(cols=["x"]).step(weight(2 * Col("x") + 1, Normal(0.0, 1.0)), observe(Data(0), Normal(Col("x"), 1.0))).spec.step[0]
    assert (w.kind, w.col, w.value.c0, w.value.col[0], w.value.coef[0]) == (abi.SSM_WEIGHT, -1, 1.0, 0, 2.0)
    # a plain kernel still lowers to SAMPLE
    assert SSM(cols=["x"]).init(sample("x", Normal(0.0, 1.0))).spec.init[0].kind == abi.SSM_SAMPLE


def test_data_dimension_scan_covers_the_target():
    ik = importance_kernel(Normal(Col("x"), 1.0), Normal(Data(2) + 0.5 * Col("x"), 1.0))
    m = SSM(cols=["x"]).step(sample("x", ik), observe(Data(0), Normal(Col("x"), 1.0)))
    assert m.spec.data_dim == 3
    ik = importance_kernel(Normal(Col("x"), 1.0), Normal(0.0, Data(3)))
    assert SSM(cols=["x"]).step(sample("x", ik), observe(Data(0), Normal(Col("x"), 1.0))).spec.data_dim == 4


# ---- the executable definition against the statements issued by hand ---------------------------
def _state(o, cols):
    st = o.get_state()
    return ({c: o.col_download(o.col_find(c)) for c in cols}, o.weights_download(), o.log_evidence(),
            {k: st[k] for k in ("n_terms", "op_counter", "depth", "n_resamples", "resampled", "weights_changed")})


def _same(a, b):
    for c in a[0]:
        assert sf.same_value(a[0][c], b[0][c]), f"column {c}: " + sf._where(a[0][c], b[0][c])
    assert sf.same_value(a[1], b[1]), "weights: " + sf._where(a[1], b[1])
    assert sf.same_value(a[2], b[2]), (a[2], b[2])
    assert a[3] == b[3], (a[3], b[3])


@pytest.mark.parametrize("ess", [0.5, 1.0])
def test_statements_are_the_operators_issued_by_hand(ess):
    a, q, r, n, T = 0.9, 1.0, 0.5, 257, 12
    gain, std = q * q / (q * q + r * r), math.sqrt(q * q * r * r / (q * q + r * r))
    y = models.lgssm1d_data(T)
    m = models.lgssm1d_guided(a, q, r)
    o = Oracle(n, seed=7)
    flags, trace = m.statements(o, y, ess_perc_min=ess)
    got = _state(o, m.cols)
    o.close()

    h = Oracle(n, seed=7)
    x, xp, mm = (h.col_create(c, 1) for c in ("x", "xp", "m"))
    ids = {"x": x, "xp": xp, "m": mm}
    R = ids.__getitem__
    h.sample(x, Normal(0.0, 1.0).dist(R))
    h.resample(ess, STRAT, wait=False)
    hflags, hess = [], []
    for t in range(T):
        h.assign(xp, [Col("x").operand(R)])
        fx = Fx(abi.X_ADD, (Fx(abi.X_MUL, (Fx(abi.X_CONST, c=(1 - gain) * a), Fx(abi.X_COL, col="xp"))),
                            Fx(abi.X_MUL, (Fx(abi.X_CONST, c=gain), Fx(abi.X_CONST, c=float(y[t]))))))
        prog, lens = dsl.xprogram([fx], R)
        h.assign_expr(mm, prog, lens)
        h.sample_importance(x, Normal(Col("m"), std).dist(R), Normal(Col("xp") * a, q).dist(R))
        h.resample(ess, STRAT, wait=False)
        h.observe(Normal(Col("x"), r).dist(R), [abi.Operand.const(float(y[t]))])
        f, e = h.resample(ess, STRAT)
        hflags.append(f), hess.append(e)
    want = _state(h, m.cols)
    h.close()
    _same(got, want)
    assert flags == hflags and sf.same_value(np.asarray(trace), np.asarray(hess))
    # 1 Sample + T (2 Assigns, an importance Sample, an Observe): depth; the Sample kinds take 2 op counters
    assert got[3]["depth"] == 1 + 4 * T and got[3]["op_counter"] == 2 + 3 * T and got[3]["n_terms"] == 1 + 2 * T


def test_statements_with_a_weight_by_hand():
    n, T, ess = 65, 8, 0.5
    y = models.lgssm1d_data(T)
    m = (SSM(cols=["x", "xp"]).init(sample("x", Normal(0.0, 1.0)), weight(Col("x"), Normal(0.5, 2.0)))
         .step(assign("xp", Col("x")),
               sample("x", importance_kernel(Normal(Data(0) + 0.5 * Col("xp"), 0.8), Normal(0.9 * Col("xp"), 1.0))),
               weight(Data(0) - Col("x"), dsl.Laplace(0.0, 1.5)),
               observe(Data(0), Normal(Col("x"), 0.7))))
    m.check()
    o = Oracle(n, seed=3)
    m.statements(o, y, ess_perc_min=ess)
    got = _state(o, m.cols)
    o.close()
    h = Oracle(n, seed=3)
    ids = {c: h.col_create(c, 1) for c in m.cols}
    R = ids.__getitem__
    h.sample(ids["x"], Normal(0.0, 1.0).dist(R))
    h.resample(ess, STRAT, wait=False)
    h.weight(Normal(0.5, 2.0).dist(R), [Col("x").operand(R)])
    h.resample(ess, STRAT, wait=False)
    for t in range(T):
        yt = float(y[t])
        h.assign(ids["xp"], [Col("x").operand(R)])
        h.sample_importance(ids["x"], Normal(yt + 0.5 * Col("xp"), 0.8).dist(R), Normal(0.9 * Col("xp"), 1.0).dist(R))
        h.resample(ess, STRAT, wait=False)
        v = abi.Operand.const(yt)   # the fold: the step's value in c0, the column with its coefficient
        v.col[0], v.coef[0] = ids["x"], -1.0
        h.weight(dsl.Laplace(0.0, 1.5).dist(R), [v])
        h.resample(ess, STRAT, wait=False)
        h.observe(Normal(Col("x"), 0.7).dist(R), [abi.Operand.const(yt)])
        h.resample(ess, STRAT)
    want = _state(h, m.cols)
    h.close()
    _same(got, want)
    assert got[3]["n_terms"] == 2 + 3 * T and got[3]["op_counter"] == 3 + 4 * T


# ---- the corpus -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in gf.corpus()}


def test_every_spec_passes_the_checker(cases):
    assert len(cases) == len(gf.SEEDS) + len(gf.DIRECTED)
    for c in cases.values():
        assert check_code(c.spec) == abi.WSMC_OK, (c.name, reason(), c.text())
        assert c.T == gf.T == 12 and c.guided and c.n_prog <= abi.XPROG_MAX
        assert c.data.shape == (c.T, c.data_dim)


def test_generator_is_deterministic():
    for a, b in zip(gf.corpus(), gf.corpus()):
        assert a.name == b.name and a.lines == b.lines and bytes(a.spec) == bytes(b.spec) and a.data.tobytes() == b.data.tobytes()


def test_corpus_covers_the_vocabulary(cases):
    props, targs, weighed, forms = set(), set(), set(), set()
    n_is, n_w, n_obs, feats = set(), set(), set(), {0: 0, 1: 0, 2: 0}
    init_is = init_w = 0
    random = [c for c in cases.values() if c.name.startswith("random-")]
    for c in cases.values():
        feats[c.feat()] += 1
        for where, k, s in c.statements():
            if s[0] == "isample":
                props.add(s[2].fam), targs.add(s[3].fam)
                for p, o in zip(gf.IS_POSITIONS, (s[2].mu, s[2].scale, s[3].mu, s[3].scale)):
                    forms.add((p, o.form))
                init_is += where == "init"
            if s[0] == "weight":
                weighed.add(s[2].fam)
                init_w += where == "init"
    for c in random:
        kinds = [s[0] for _, _, s in c.statements()]
        n_is.add(kinds.count("isample")), n_w.add(kinds.count("weight"))
        n_obs.add(sum(s[0] == "observe" for s in c.step))
    fams = set(sf.SCALAR_FAMILIES)
    assert len(fams) == 21
    assert not fams - props, f"families in no proposal: {[gf.FAMILIES[f] for f in sorted(fams - props)]}"
    assert not fams - targs, f"families in no target: {[gf.FAMILIES[f] for f in sorted(fams - targs)]}"
    assert len(weighed) >= 8, weighed
    missing = {(p, f) for p in gf.IS_POSITIONS for f in sf.FORMS} - forms
    assert not missing, f"operand forms by importance-Sample position never built: {sorted(missing)}"
    assert n_is == {0, 1, 2} and n_w == {0, 1, 2} and n_obs == {1, 2, 3}, (n_is, n_w, n_obs)
    assert init_is >= 2 and init_w >= 2, (init_is, init_w)
    assert min(feats.values()) >= 4, f"specs by kernel variant (plain, extended, log-Gamma): {feats}"


def test_directed_cases_are_what_their_names_say(cases):
    kinds = lambda c: [s[0] for s in c.step]
    c = cases["self_reading"]
    assert all(any(s is not None and s[0] == "col" and s[1] == c.step[0][1] for s in d.mu.slots) for d in c.step[0][2:4])
    c = cases["data_slots"]
    st = c.step[1]
    assert st[2].mu.form == "data_col" and st[3].mu.form == "col_data" and st[2].scale.form == "data" and st[3].scale.form == "data"
    assert st[3].scale.slots[0] is None
    assert [s[0] for s in cases["init_importance"].init] == ["sample", "isample"]
    c = cases["after_last_observe"]
    assert kinds(c) == ["weight", "observe", "assign", "isample", "weight"] and c.trace_slot == (4, 1)
    c = cases["eight_statements"]
    assert len(c.step) == 8 and kinds(c).count("isample") == 2 and kinds(c).count("weight") == 1 and kinds(c).count("observe") == 2
    assert c.trace_slot == (5, 4)
    c = cases["uniform_in_normal"]
    assert (c.step[0][2].fam, c.step[0][3].fam) == (abi.FAM_NORMAL, abi.FAM_UNIFORM)
    assert (cases["base_families"].feat(), cases["extended_families"].feat(), cases["log_gamma"].feat()) == (0, 1, 2)
    assert {d.fam for d in cases["base_families"].dists()} == {abi.FAM_NORMAL, abi.FAM_HALFNORMAL, abi.FAM_UNIFORM}
    c = cases["log_gamma"]
    assert (c.step[0][2].fam, c.step[0][3].fam) == (abi.FAM_GAMMA, abi.FAM_INVERSEGAMMA)
    assert cases["four_columns"].n_cols == 4 and len(cases["four_columns"].init) == 4
    assert bytes(cases["lgssm1d_guided"].spec) == bytes(models.lgssm1d_guided().spec)
    # trace slots that are not the step's last slot, and ones that are
    late = [c.name for c in cases.values() if c.trace_slot[1] != c.trace_slot[0] - 1]
    assert "after_last_observe" in late and len(late) >= 6 and len(late) < len(cases) - 6, late


@pytest.fixture(scope="module")
def outcomes(cases):
    """every case on the oracle at ess 1.0 and 0.5: name -> {ess: (flags, trace, evidence, weights, state)}"""
    out = {}
    for c in cases.values():
        out[c.name] = {}
        for ess in (1.0, 0.5):
            o = Oracle(1001, seed=sf.SEED)
            flags, trace = c.ssm.statements(o, c.data, ess_perc_min=ess, T=c.T)
            out[c.name][ess] = (flags, np.asarray(trace), o.log_evidence(), o.weights_download(), o.get_state())
            o.close()
    return out


def test_outcomes_on_the_oracle(cases, outcomes):
    degenerate = ("all_neg_inf", "nan_weights")
    for name, by in outcomes.items():
        for ess, (flags, trace, ev, w, state) in by.items():
            if name in degenerate:
                continue
            assert math.isfinite(ev), (name, ess, ev)
            assert not np.isnan(w).any() and not np.isneginf(w).all(), (name, ess)
            if ess == 1.0:
                assert all(flags), (name, flags)
    # init_importance: the importance Sample's Resample runs in `init` (one more than the steps')
    flags, _, _, _, state = outcomes["init_importance"][1.0]
    assert state["n_resamples"] == 1 + sum(flags) == 1 + gf.T
    # uniform_in_normal: draws outside the target's support carry -inf into the step's OBSERVE
    # (seen where no Resample takes them away: threshold 0)
    o = Oracle(1001, seed=sf.SEED)
    c = cases["uniform_in_normal"]
    c.ssm.statements(o, c.data, ess_perc_min=0.0, T=c.T)
    w, ev = o.weights_download(), o.log_evidence()
    o.close()
    assert np.isneginf(w).any() and not np.isneginf(w).all() and math.isfinite(ev)
    # all_neg_inf: its WEIGHT stands after the step's OBSERVE, so from the next step's trace point on
    # no Resample runs, the ESS% is NaN and the evidence is lost
    flags, trace, ev, w, state = outcomes["all_neg_inf"][1.0]
    k = gf.ALL_NEG_INF_AT + 1
    assert np.isneginf(w).all() and np.isnan(trace[k:]).all() and not any(flags[k:]) and math.isnan(ev)
    assert all(flags[:k]) and np.isfinite(trace[:k]).all()
    # nan_weights: a NaN weight from the first step: never a Resample
    flags, trace, ev, w, state = outcomes["nan_weights"][1.0]
    assert np.isnan(w).any() and np.isnan(trace).all() and state["n_resamples"] == 0
    # the new statements' Resamples do run at the gated threshold too: more resamples than the traced ones
    more = [n for n, by in outcomes.items() if by[0.5][4]["n_resamples"] > sum(by[0.5][0])]
    assert len(more) >= 8, more


# ---- the guided LGSSM against the Kalman filter -------------------------------------------------
def test_guided_evidence_against_kalman():
    """N = 1001, T = 50, ess 0.5, stratified, seeds 0..19; sd over the seeds with the divisor 20.
    Measured on the oracle with the spec's own bits (m from the program (k xp) + (gain y_t), not
    from a host product): guided max |err| 0.320, sd 0.174; bootstrap max |err| 0.631, sd 0.346,
    the figures of the hand-issued Oracle.sample_importance runs that set the bound: 1.0 is 3x their
    maximum of 0.320."""
    a, q, r = 0.9, 1.0, 0.5
    y = models.lgssm1d_data(50)
    _, exact = kalman_filter_evidence(y, a, q, r)
    errs = {}
    for name, make in (("guided", models.lgssm1d_guided), ("bootstrap", models.lgssm1d_spec)):
        e = []
        for seed in range(20):
            o = Oracle(1001, seed=seed)
            make().statements(o, y, ess_perc_min=0.5, scheme=STRAT)
            e.append(o.log_evidence() - exact)
            o.close()
        errs[name] = np.asarray(e)
        print(f"{name}: max |err| {np.abs(errs[name]).max():.3f} sd {errs[name].std():.3f}")
    assert np.abs(errs["guided"]).max() < 1.0, errs["guided"]
    assert errs["guided"].std() < errs["bootstrap"].std(), (errs["guided"].std(), errs["bootstrap"].std())

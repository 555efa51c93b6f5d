"""CPU checks of the specified scalar SSM (include/wsmc.h wsmc_ssm_spec): what the host-only checker
refuses, the ctypes layout against the library's, and the expansion of a spec into statements
(wsmc.SSM.statements) against the hand-written models.lgssm1d_statements on the oracle alone.
"""
import ctypes as C

import numpy as np
import pytest

import wsmc
from wsmc import abi, dsl, models
from wsmc.dsl import Col, Data, Normal
from wsmc.ssm import SSM, assign, observe, sample
from oracle import Oracle


def check_code(spec: abi.SsmSpec) -> int:
    return wsmc.load_library().wsmc_ssm_spec_check(C.byref(spec))


def reason() -> str:
    return wsmc.load_library().wsmc_last_error().decode()


def clone(spec: abi.SsmSpec) -> abi.SsmSpec:
    r = abi.SsmSpec()
    C.memmove(C.byref(r), C.byref(spec), C.sizeof(abi.SsmSpec))
    return r


def lgssm() -> abi.SsmSpec:
    return clone(models.lgssm1d_spec().spec)


@pytest.mark.parametrize("name", sorted(models.SSM_MODELS))
def test_models_pass(name):
    spec = models.SSM_MODELS[name][0]()
    assert check_code(spec.spec) == abi.WSMC_OK, reason()
    spec.check()
    assert spec.spec.data_dim == (2 if name == "kitagawa" else 1)


def test_lgssm_spec_passes():
    assert check_code(lgssm()) == abi.WSMC_OK, reason()


def refused(spec, word):
    assert check_code(spec) == abi.WSMC_EARG
    assert word in reason(), reason()


def test_refuses_vector_dist():
    s = lgssm()
    s.step[0].dist.dim = 2
    refused(s, "dim")


@pytest.mark.parametrize("family", [abi.FAM_MVNORMAL_ISO, abi.FAM_MVNORMAL, 15, 24, -1])
def test_refuses_family(family):
    s = lgssm()
    s.step[1].dist.family = family
    refused(s, "family")


def test_refuses_oscillator_mean():
    s = lgssm()
    s.step[1].dist.mean_fn = abi.MEAN_OSCILLATOR
    refused(s, "mean")


def test_refuses_step_without_observe():
    s = lgssm()
    s.n_step = 1
    refused(s, "OBSERVE")


def test_refuses_two_data_slots():
    s = lgssm()
    o = s.step[1].value
    o.col[1], o.comp[1], o.coef[1] = abi.OPERAND_DATA, 0, 1.0
    refused(s, "two data slots")


@pytest.mark.parametrize("field, value, word", [("c0", 0.5, "c0 == 0"), ("coef", 2.0, "coef == 1")])
def test_refuses_inexact_data_operand(field, value, word):
    s = lgssm()
    if field == "c0":
        s.step[1].value.c0 = value
    else:
        s.step[1].value.coef[0] = value
    refused(s, word)


def test_refuses_data_past_data_dim():
    s = lgssm()
    s.step[1].value.comp[0] = 1
    refused(s, "data_dim")


def test_refuses_data_in_init():
    s = lgssm()
    s.init[0].dist.mu[0] = s.step[1].value
    refused(s, "init reads data")
    spec = SSM(cols=["x"]).init(assign("x", dsl.exp(Data(0)))).step(observe(Data(0), Normal(Col("x"), 1.0)))
    refused(spec.spec, "init reads data")


def test_refuses_column_past_n_cols():
    s = lgssm()
    s.step[0].dist.mu[0].col[0] = 1
    refused(s, "n_cols")
    s = lgssm()
    s.step[0].col = 1
    refused(s, "n_cols")
    s = clone(models.sv().spec)
    s.step[1].prog[0].col = 2   # the program's read of h
    assert s.step[1].prog[0].op == abi.X_COL
    refused(s, "n_cols")


def test_refuses_bad_program():
    s = clone(models.sv().spec)
    assert s.step[1].kind == abi.SSM_ASSIGN_EXPR
    s.step[1].prog[s.step[1].prog_len - 1].op = 99   # an unknown operator
    refused(s, "program")
    s = clone(models.sv().spec)
    s.step[1].prog_len -= 2   # h, 2: leaves two values
    refused(s, "program")
    s = clone(models.sv().spec)
    s.step[1].prog_len = abi.SSM_XPROG_MAX + 1
    refused(s, "program")


@pytest.mark.parametrize("field, value", [("n_cols", 0), ("n_cols", 5), ("n_init", 5), ("n_step", 9), ("n_step", 0),
                                          ("data_dim", 5)])
def test_refuses_counts(field, value):
    s = lgssm()
    setattr(s, field, value)
    refused(s, field)


def test_refuses_names():
    s = clone(models.sv().spec)
    s.col_names[1].value = b"h"
    refused(s, "one name")
    s = lgssm()
    s.col_names[0].value = b""
    refused(s, "name")


def test_null_spec():
    assert wsmc.load_library().wsmc_ssm_spec_check(None) == abi.WSMC_EARG


def test_builder_limits():
    with pytest.raises(ValueError):
        SSM(cols=list("abcde")).step(observe(Data(0), Normal(Col("a"), 1.0))).spec
    with pytest.raises(KeyError):
        SSM(cols=["x"]).step(observe(Data(0), Normal(Col("y"), 1.0))).spec


def test_builder_lowering():
    """affine right-hand sides are operands, everything else a program; data reads keep their index"""
    sp = models.kitagawa().spec
    kinds = [sp.step[k].kind for k in range(sp.n_step)]
    assert kinds == [abi.SSM_ASSIGN_EXPR, abi.SSM_SAMPLE, abi.SSM_ASSIGN_EXPR, abi.SSM_OBSERVE]
    reads = [(i.col, i.comp) for i in sp.step[0].prog[:sp.step[0].prog_len] if i.op == abi.X_COL]
    assert (abi.OPERAND_DATA, 1) in reads and (0, 0) in reads
    v = sp.step[3].value
    assert (v.col[0], v.comp[0], v.coef[0], v.c0, v.col[1]) == (abi.OPERAND_DATA, 0, 1.0, 0.0, -1)
    sp = SSM(cols=["x", "y"]).step(assign("y", 2.0 * Col("x") + 1.0), observe(Data(0), Normal(Col("y"), 1.0))).spec
    assert sp.step[0].kind == abi.SSM_ASSIGN and sp.step[0].value.coef[0] == 2.0 and sp.step[0].value.c0 == 1.0


def test_struct_layouts_match_c():
    a, b = C.c_int64(), C.c_int64()
    assert wsmc.load_library().wsmc_ssm_spec_sizeof(C.byref(a), C.byref(b)) == abi.WSMC_OK
    assert C.sizeof(abi.SsmStmt) == a.value
    assert C.sizeof(abi.SsmSpec) == b.value
    assert abi.SsmStmt.prog.offset == 16 + C.sizeof(abi.Dist) + C.sizeof(abi.Operand)


STATE = ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples", "last_ess_perc")


@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_expansion_equals_hand_written_statements(ess):
    """spec.statements for the LGSSM spec against models.lgssm1d_statements, on the oracle alone."""
    N, T = 65, 12
    data = models.lgssm1d_data(T)
    kw = dict(a=0.9, q=1.0, r=0.5, x0_std=1.0)
    a, b = Oracle(N, seed=42), Oracle(N, seed=42)
    flags = models.lgssm1d_statements(a, data, ess_perc_min=ess, **kw)
    flags_b, trace = models.lgssm1d_spec(**kw).statements(b, data, ess_perc_min=ess)
    assert flags == flags_b and len(trace) == T
    if ess == 0.5:
        assert 0 < sum(flags) < T
    assert a.col_names() == b.col_names() == ["x"]
    np.testing.assert_array_equal(a.col_download(0), b.col_download(0))
    np.testing.assert_array_equal(a.weights_download(), b.weights_download())
    np.testing.assert_array_equal(a.last_ancestors(), b.last_ancestors())
    sa, sb = a.get_state(), b.get_state()
    for k in STATE:
        assert sa[k] == sb[k], k
    assert sa["op_counter"] == 2 + 3 * T
    assert a.log_evidence() == b.log_evidence()
    np.testing.assert_array_equal(a.score(-1), b.score(-1))
    np.testing.assert_array_equal(a.score(sa["depth"]), b.score(sb["depth"]))   # the whole tape
    assert np.any(a.score(sa["depth"]) != 0.0)


@pytest.mark.parametrize("name", sorted(models.SSM_MODELS))
def test_models_run_on_the_oracle(name):
    """Each model's statements run on the oracle and give a finite evidence on its own data; with
    ess 0.5 the flags are mixed (what the GPU cases rely on)."""
    make, gen = models.SSM_MODELS[name]
    data = gen(40)
    o = Oracle(63, seed=42)
    flags, trace = make().statements(o, data, ess_perc_min=0.5)
    assert len(flags) == 40 and 0 < sum(flags) < 40
    assert np.isfinite(o.log_evidence())
    assert o.col_names() == make().cols

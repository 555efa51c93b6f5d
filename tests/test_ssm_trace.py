"""The per-step filtering trace of the scalar-SSM runs (wsmc_ssm_run_traced,
wsmc_ssm_run_batch_traced), on the host: the symbols and the struct's layout, the wrappers' argument
checks, and the definition itself, `SSM.statements(..., trace=True)` on the CPU oracle: that it is
a filter's (against a Kalman filter written here), that the rows the GPU file compares by position
are finite where they should be, and that the last evidence row is the run's evidence.
tests/test_gpu_ssm_trace.py compares the fused runs with this definition bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest

import ssmfuzz as sf   # (puts the package and the oracle on sys.path)
import wsmc
from oracle import Oracle
from wsmc import abi, models
from wsmc.ssm import SsmTrace

T = sf.T


def test_symbols_and_trace_struct():
    lib = wsmc.load_library()
    for name in ("wsmc_ssm_trace_sizeof", "wsmc_ssm_run_traced", "wsmc_ssm_run_batch_traced"):
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    n = C.c_int64()
    assert lib.wsmc_ssm_trace_sizeof(C.byref(n)) == abi.WSMC_OK
    assert n.value == C.sizeof(abi.SsmTraceOut) == 4 * C.sizeof(C.c_void_p)
    assert [f for f, _ in abi.SsmTraceOut._fields_] == ["ess", "mean", "var", "log_evidence"]
    assert lib.wsmc_ssm_trace_sizeof(None) == abi.WSMC_EARG
    # the batch's result struct is what it was
    assert lib.wsmc_ssm_batch_out_sizeof(C.byref(n)) == abi.WSMC_OK and n.value == 7 * C.sizeof(C.c_void_p)


def test_library_refuses_before_the_device():
    """the traced entry points have the untraced ones' argument checks (a null context first)"""
    lib = wsmc.load_library()
    sv = models.sv()
    seeds = (C.c_uint64 * 2)(1, 2)
    out, tr = abi.SsmBatchOut(), abi.SsmTraceOut()
    rc = lib.wsmc_ssm_run_batch_traced(None, C.byref(sv.spec), 1, None, 1, 4, 100, 2, seeds, 1.0, abi.RESAMPLE_STRATIFIED,
                                       C.byref(out), C.byref(tr))
    assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    rc = lib.wsmc_ssm_run_traced(None, C.byref(sv.spec), None, 4, 1.0, abi.RESAMPLE_STRATIFIED, None, C.byref(tr))
    assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    rc = lib.wsmc_ssm_run_traced(None, C.byref(sv.spec), None, 4, 1.0, abi.RESAMPLE_STRATIFIED, None, None)
    assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()


def test_wrapper_checks():
    sv, y = models.sv(), models.sv_data(8)
    g = object.__new__(wsmc.Context)   # no library handle behind the object: refused before any call
    with pytest.raises(ValueError, match="ess_trace and trace"):
        wsmc.Context.ssm_run(g, sv, y, ess_trace=True, trace=True)
    with pytest.raises(ValueError, match="unknown part"):
        wsmc.Context.ssm_run(g, sv, y, trace=("mean", "median"))
    with pytest.raises(ValueError, match="specs"):
        wsmc.Context.ssm_run_batch(g, [sv, sv], y, 100, [1, 2, 3], trace=True)
    with pytest.raises(ValueError, match="wait=True"):
        sv.statements(Oracle(8, seed=1), y, wait=False, trace=True)


def test_statements_without_trace_are_unchanged():
    """trace=False returns what it always has, and the trace changes nothing the run leaves"""
    case = sf.gen(5)
    a, b = Oracle(65, seed=sf.SEED), Oracle(65, seed=sf.SEED)
    r = case.ssm.statements(a, case.data, ess_perc_min=0.5, T=case.T)
    assert isinstance(r, tuple) and len(r) == 2
    assert case.ssm.statements(Oracle(65, seed=sf.SEED), case.data, ess_perc_min=0.5, T=case.T, wait=False) is None
    flags, ess, tr = case.ssm.statements(b, case.data, ess_perc_min=0.5, T=case.T, trace=True)
    assert isinstance(tr, SsmTrace)
    assert flags == r[0] and sf.same_value(ess, r[1]) and sf.same_value(tr.ess, r[1])
    assert sorted(tr.mean) == sorted(tr.var) == sorted(case.ssm.cols)
    assert all(v.shape == (case.T,) for v in list(tr.mean.values()) + list(tr.var.values()) + [tr.log_evidence])
    assert sf.compare(a, b) is None
    assert tr.predictive_loglik().shape == (case.T,) and tr.predictive_loglik()[0] == tr.log_evidence[0]


def kalman(y, a=0.9, q=1.0, r=0.5, x0_std=1.0):
    """the filtered mean and variance of models.lgssm1d_spec (q, r and x0_std are standard deviations)"""
    m, P = 0.0, x0_std * x0_std
    ms, Ps = [], []
    for yt in y:
        m, P = a * m, a * a * P + q * q
        k = P / (P + r * r)
        m, P = m + k * (yt - m), (1.0 - k) * P
        ms.append(m)
        Ps.append(P)
    return np.array(ms), np.array(Ps)


@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_the_definition_is_a_filter(ess):
    """N = 4096 particles against the exact filter. The bars are the issue's: the mean within 8
    standard errors sqrt(P_t / N) (5.41 measured at worst over these 16 seeded runs: resampling and
    the weights' spread cost a few plain standard errors), the variance within 25 % (0.14 measured)."""
    n, y = 4096, models.lgssm1d_data(50)
    m, P = kalman(y)
    worst_m = worst_v = 0.0
    for seed in range(1, 9):
        o = Oracle(n, seed=seed)
        _, _, tr = models.lgssm1d_spec().statements(o, y, ess_perc_min=ess, trace=True)
        o.close()
        worst_m = max(worst_m, float(np.max(np.abs(tr.mean["x"] - m) / np.sqrt(P / n))))
        worst_v = max(worst_v, float(np.max(np.abs(tr.var["x"] / P - 1.0))))
    print(f"ess {ess}: worst |mean - m_t| / sqrt(P_t / N) = {worst_m:.3f}, worst |var / P_t - 1| = {worst_v:.3f}")
    assert worst_m <= 8.0
    assert worst_v <= 0.25


def bad_rows(tr):
    """the rows with a non-finite mean, variance or evidence"""
    m = np.column_stack([tr.mean[c] for c in tr.mean] + [tr.var[c] for c in tr.var] + [tr.log_evidence])
    return ~np.isfinite(m).all(axis=1)


def oracle_trace(case, n, ess=0.5):
    o = Oracle(n, seed=sf.SEED)
    try:
        return case.ssm.statements(o, case.data, ess_perc_min=ess, T=case.T, trace=True)[2]
    finally:
        o.close()


@pytest.mark.parametrize("n", [65, 1001])
def test_reference_rows_are_finite_where_the_gpu_file_needs_them(n):
    """NaN rows compare equal by position, so an all-NaN trace must not pass unseen: every mixed
    spec's rows are finite, and the two directed cases have exactly the NaN rows they are there for"""
    for seed in sf.MIXED_SEEDS:
        tr = oracle_trace(sf.gen(seed), n)
        assert not bad_rows(tr).any() and np.isfinite(tr.ess).all(), seed
    tr = oracle_trace(sf.gen("all_xops", "directed"), n)
    assert bad_rows(tr).sum() == 23 and list(np.where(~bad_rows(tr))[0]) == [0]
    assert np.isfinite(tr.log_evidence).all()            # (the programs' NaN columns, not the weights)
    tr = oracle_trace(sf.gen("partial_support", "directed"), n)
    assert bad_rows(tr).sum() == 4 and list(np.where(bad_rows(tr))[0]) == list(range(sf.PARTIAL_ALL_AT, T))
    assert (~np.isfinite(tr.log_evidence)).sum() == 4    # evidence included


@pytest.mark.parametrize("name", sorted(models.SSM_MODELS))
@pytest.mark.parametrize("ess", [0.0, 0.5, 1.0])
def test_last_evidence_row_is_the_evidence(name, ess):
    """the models' last statement is the OBSERVE: the weights the last row sees are the final ones
    when that Resample does not run, and a Resample's reset to the log-mean keeps the evidence"""
    mk, data = models.SSM_MODELS[name]
    o = Oracle(1001, seed=3)
    _, _, tr = mk().statements(o, data(T), ess_perc_min=ess, trace=True)
    assert sf.same_value(tr.log_evidence[-1], o.log_evidence())
    assert math.isfinite(tr.log_evidence[-1])
    o.close()

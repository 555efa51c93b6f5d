"""Sampled trajectories and smoothed moments of the scalar-SSM runs (wsmc_ssm_run_smoothed,
wsmc_ssm_run_batch_smoothed), on the host: the symbols and the struct's layout, the wrappers'
argument checks, and the definition itself, `SSM.statements(..., smooth=True)` on the CPU oracle:
that without resampling its rows are the columns the run passed through, that it is a smoother's
(against a Rauch-Tung-Striebel smoother written here), and that the rows the GPU file compares by
position are finite where they should be. tests/test_gpu_ssm_smooth.py compares the fused runs with
this definition bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import ssmfuzz as sf   # (puts the package and the oracle on sys.path)
import wsmc
from oracle import Oracle
from wsmc import abi, models
from wsmc.ssm import SsmSmooth, SsmTrace

T = sf.T


def test_symbols_and_smooth_struct():
    lib = wsmc.load_library()
    for name in ("wsmc_ssm_smooth_sizeof", "wsmc_ssm_run_smoothed", "wsmc_ssm_run_batch_smoothed"):
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    n = C.c_int64()
    assert lib.wsmc_ssm_smooth_sizeof(C.byref(n)) == abi.WSMC_OK
    assert n.value == C.sizeof(abi.SsmSmoothOut) == 3 * C.sizeof(C.c_void_p)
    assert [f for f, _ in abi.SsmSmoothOut._fields_] == ["paths", "mean", "var"]
    assert lib.wsmc_ssm_smooth_sizeof(None) == abi.WSMC_EARG
    # the trace's and the batch's structs are what they were
    assert lib.wsmc_ssm_trace_sizeof(C.byref(n)) == abi.WSMC_OK and n.value == 4 * C.sizeof(C.c_void_p)
    assert lib.wsmc_ssm_batch_out_sizeof(C.byref(n)) == abi.WSMC_OK and n.value == 7 * C.sizeof(C.c_void_p)
    assert wsmc.SsmSmooth is SsmSmooth


def test_library_refuses_before_the_device():
    """the smoothed entry points have the other ones' argument checks (a null context first)"""
    lib = wsmc.load_library()
    sv = models.sv()
    seeds = (C.c_uint64 * 2)(1, 2)
    out, tr, sm = abi.SsmBatchOut(), abi.SsmTraceOut(), abi.SsmSmoothOut()
    rc = lib.wsmc_ssm_run_batch_smoothed(None, C.byref(sv.spec), 1, None, 1, 4, 100, 2, seeds, 1.0, abi.RESAMPLE_STRATIFIED,
                                         C.byref(out), C.byref(tr), C.byref(sm))
    assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    st = (C.c_int64 * 4)()
    assert "wsmc_debug_ssm_smooth" in abi.SIGNATURES
    assert lib.wsmc_debug_ssm_smooth(None, st) == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    for t, s in ((C.byref(tr), C.byref(sm)), (None, C.byref(sm)), (None, None)):
        rc = lib.wsmc_ssm_run_smoothed(None, C.byref(sv.spec), None, 4, 1.0, abi.RESAMPLE_STRATIFIED, None, t, s)
        assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()


def test_wrapper_checks():
    sv, y = models.sv(), models.sv_data(8)
    g = object.__new__(wsmc.Context)   # no library handle behind the object: refused before any call
    with pytest.raises(ValueError, match="ess_trace and smooth"):
        wsmc.Context.ssm_run(g, sv, y, ess_trace=True, smooth=True)
    with pytest.raises(ValueError, match="unknown part"):
        wsmc.Context.ssm_run(g, sv, y, smooth=("mean", "median"))
    with pytest.raises(ValueError, match="unknown part"):
        wsmc.Context.ssm_run_batch(g, sv, y, 100, [1, 2], smooth=("path",))
    with pytest.raises(ValueError, match="specs"):
        wsmc.Context.ssm_run_batch(g, [sv, sv], y, 100, [1, 2, 3], smooth=True)
    with pytest.raises(ValueError, match="wait=True"):
        sv.statements(Oracle(8, seed=1), y, wait=False, smooth=True)
    # the history columns beside the spec's own must fit the store: T n_cols + n_cols <= 4096
    o = Oracle(8, seed=1)
    with pytest.raises(ValueError, match="store columns"):
        sv.statements(o, models.sv_data(2048), smooth=True)
    assert o.col_names() == []   # refused before a column was made
    o.close()


def test_draw_picks_rows_by_the_final_weights():
    paths = {"x": np.arange(12.0).reshape(3, 4)}   # T = 3, N = 4
    sm = SsmSmooth(paths, None, None, np.log(np.array([0.0, 1.0, 0.0, 0.0]) + 1e-300))
    d = sm.draw(5, np.random.default_rng(0))
    assert d["x"].shape == (5, 3) and (d["x"] == paths["x"][:, 1]).all()
    sm = SsmSmooth(paths, None, None, np.zeros(4))
    d = sm.draw(400, np.random.default_rng(0))
    assert sorted(set(d["x"][:, 0])) == [0.0, 1.0, 2.0, 3.0]
    assert all((row == paths["x"][:, int(row[0])]).all() for row in d["x"])   # whole trajectories
    with pytest.raises(ValueError, match="paths"):
        SsmSmooth(None, None, None, np.zeros(4)).draw(1)


def test_statements_without_smooth_are_unchanged():
    """smooth=False returns what it always has, and smoothing changes nothing of the spec's own columns,
    the weights, the decisions or the filtering trace"""
    case = sf.gen(5)
    a, b, c = (Oracle(65, seed=sf.SEED) for _ in range(3))
    r = case.ssm.statements(a, case.data, ess_perc_min=0.5, T=case.T)
    assert isinstance(r, tuple) and len(r) == 2
    assert case.ssm.statements(Oracle(65, seed=sf.SEED), case.data, ess_perc_min=0.5, T=case.T, wait=False) is None
    rt = case.ssm.statements(b, case.data, ess_perc_min=0.5, T=case.T, trace=True)
    assert len(rt) == 3 and isinstance(rt[2], SsmTrace)
    assert sf.compare(a, b) is None
    flags, ess, sm = case.ssm.statements(c, case.data, ess_perc_min=0.5, T=case.T, smooth=True)
    assert isinstance(sm, SsmSmooth)
    assert flags == r[0] and sf.same_value(ess, r[1])
    assert sorted(sm.paths) == sorted(sm.mean) == sorted(sm.var) == sorted(case.ssm.cols)
    assert all(v.shape == (case.T, 65) for v in sm.paths.values())
    assert all(v.shape == (case.T,) for v in list(sm.mean.values()) + list(sm.var.values()))
    assert c.col_names() == case.ssm.cols + [f"{n}@{t}" for t in range(case.T) for n in case.ssm.cols]
    for name in case.ssm.cols:
        assert sf.same_value(c.col_download(c.col_find(name)), a.col_download(a.col_find(name))), name
    assert sf.same_value(c.weights_download(), a.weights_download()) and sf.same_value(sm.log_weights, a.weights_download())
    assert sf.same_value(c.last_ancestors(), a.last_ancestors())
    assert c.get_state()["op_counter"] == a.get_state()["op_counter"] and c.log_evidence() == a.log_evidence()
    d = Oracle(65, seed=sf.SEED)
    four = case.ssm.statements(d, case.data, ess_perc_min=0.5, T=case.T, trace=True, smooth=True)
    assert len(four) == 4 and isinstance(four[2], SsmTrace) and isinstance(four[3], SsmSmooth)
    assert sf.same_value(four[2].log_evidence, rt[2].log_evidence)
    assert all(sf.same_value(four[2].mean[n], rt[2].mean[n]) and sf.same_value(four[3].paths[n], sm.paths[n]) for n in case.ssm.cols)
    for o in (a, b, c, d):
        o.close()


SPECS = {name: (make(), gen(12)) for name, (make, gen) in models.SSM_MODELS.items()}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_without_resampling_the_rows_are_the_run(name):
    """ess 0.0 never resamples and the models' last step statement is the OBSERVE, so row t is the
    column a run stopped after step t leaves, the last row is the final column, and the last smoothed
    moments are the filter's last row"""
    ssm, data = SPECS[name]
    steps, n = len(data), 65
    o = Oracle(n, seed=9)
    _, _, tr, sm = ssm.statements(o, data, ess_perc_min=0.0, trace=True, smooth=True)
    for c in ssm.cols:
        assert sf.same_value(sm.paths[c][steps - 1], o.col_download(o.col_find(c))), c
        assert sf.same_value(sm.mean[c][steps - 1], tr.mean[c][steps - 1]) and sf.same_value(sm.var[c][steps - 1], tr.var[c][steps - 1])
        assert np.isfinite(sm.mean[c]).all() and np.isfinite(sm.var[c]).all()
    assert o.get_state()["n_resamples"] == 0
    o.close()
    for t in range(steps):
        s = Oracle(n, seed=9)
        ssm.statements(s, data[:t + 1], ess_perc_min=0.0)
        for c in ssm.cols:
            assert sf.same_value(sm.paths[c][t], s.col_download(s.col_find(c))), (c, t)
        s.close()


def rts(y, a=0.9, q=1.0, r=0.5, x0_std=1.0):
    """the smoothed mean and variance of models.lgssm1d_spec (q, r and x0_std are standard deviations):
    a Kalman filter forward, Rauch-Tung-Striebel backward"""
    m, P = 0.0, x0_std * x0_std
    mf, Pf, mp, Pp = [], [], [], []
    for yt in y:
        m, P = a * m, a * a * P + q * q
        mp.append(m)
        Pp.append(P)
        k = P / (P + r * r)
        m, P = m + k * (yt - m), (1.0 - k) * P
        mf.append(m)
        Pf.append(P)
    ms, Ps = list(mf), list(Pf)
    for t in range(len(y) - 2, -1, -1):
        g = a * Pf[t] / Pp[t + 1]
        ms[t] = mf[t] + g * (ms[t + 1] - mp[t + 1])
        Ps[t] = Pf[t] + g * g * (Ps[t + 1] - Pp[t + 1])
    return np.array(ms), np.array(Ps)


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("steps", [12, 24])
def test_the_definition_is_a_smoother(steps, ess):
    """N = 4096 particles against the exact smoother. The genealogy coalesces, so row t holds U_t
    distinct values and the standard error is sqrt(P_t^s / U_t). The bars are the issue's: the mean
    within 8 of these standard errors (4.6 measured at worst over the 32 seeded runs, U_t as low as
    106), the variance within 15 % of P_t^s at the steps with U_t >= 1000 (6 % measured)."""
    n, y = 4096, models.lgssm1d_data(steps)
    m, P = rts(y)
    worst_m = worst_v = 0.0
    least_u, wide = n, 0
    for seed in range(1, 9):
        o = Oracle(n, seed=seed)
        sm = models.lgssm1d_spec().statements(o, y, ess_perc_min=ess, smooth=True)[2]
        o.close()
        u = np.array([len(np.unique(row)) for row in sm.paths["x"]])
        least_u = min(least_u, int(u.min()))
        worst_m = max(worst_m, float(np.max(np.abs(sm.mean["x"] - m) / np.sqrt(P / u))))
        many = u >= 1000
        wide += int(many.sum())
        if many.any():
            worst_v = max(worst_v, float(np.max(np.abs(sm.var["x"][many] / P[many] - 1.0))))
    print(f"T {steps} ess {ess}: worst |mean - m_t^s| / sqrt(P_t^s / U_t) = {worst_m:.3f}, worst |var / P_t^s - 1| = {worst_v:.3f} "
          f"over {wide} rows with U_t >= 1000, least U_t = {least_u}")
    assert wide > 0   # (the last rows: the variance bar is not vacuous)
    assert worst_m <= 8.0
    assert worst_v <= 0.15


def bad_rows(sm):
    """the rows with a non-finite smoothed mean or variance"""
    m = np.column_stack([sm.mean[c] for c in sm.mean] + [sm.var[c] for c in sm.var])
    return ~np.isfinite(m).all(axis=1)


def oracle_smooth(case, n, ess=0.5):
    o = Oracle(n, seed=sf.SEED)
    try:
        return case.ssm.statements(o, case.data, ess_perc_min=ess, T=case.T, smooth=True)[2]
    finally:
        o.close()


@pytest.mark.parametrize("n", [65, 1001])
def test_reference_rows_are_finite_where_the_gpu_file_needs_them(n):
    """NaN rows compare equal by position, so all-NaN rows must not pass unseen: every mixed spec's
    smoothed rows are finite, and the two directed cases have exactly the NaN rows they are there for"""
    for seed in sf.MIXED_SEEDS:
        sm = oracle_smooth(sf.gen(seed), n)
        assert not bad_rows(sm).any(), seed
        assert all(np.isfinite(p).all() for p in sm.paths.values()), seed
    sm = oracle_smooth(sf.gen("all_xops", "directed"), n)   # the programs' NaN columns from step 1 on
    assert list(np.where(~bad_rows(sm))[0]) == [0]
    assert np.isfinite(sm.mean["c0"]).all() and np.isfinite(sm.paths["c0"]).all() and np.isfinite(sm.log_weights).all()
    sm = oracle_smooth(sf.gen("partial_support", "directed"), n)   # every final weight is -inf: no row has moments
    assert bad_rows(sm).all() and np.isneginf(sm.log_weights).all()
    assert np.isfinite(sm.paths["c0"]).all()                # ... but the trajectories are there

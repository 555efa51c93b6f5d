"""Conditional SMC for the scalar-SSM runs (wsmc_ssm_spec_conditional, wsmc_ssm_run_conditional), on
the host: the eligibility rule in the library and its restatement in Python, properties of the
definition itself, `SSM.conditional_definition` on the CPU oracle, the invariance of the particle
Gibbs kernel it builds (against a Rauch-Tung-Striebel smoother), and the sweeps' seeds.
tests/test_gpu_ssm_conditional.py compares the device with this definition bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import ssmcond as sc   # (puts the package and the oracle on sys.path)
import test_ssm_backward as tb   # its refused specs and its RTS smoother
import wsmc
from oracle import Oracle
from wsmc import Col, Normal, abi, models
from wsmc.dsl import Data
from wsmc.ssm import SSM, assign, observe, sample, weight


def library_pinned(ssm):
    """(code, pinned column names or the reason) of wsmc_ssm_spec_conditional"""
    lib = wsmc.load_library()
    pin = (C.c_int32 * abi.SSM_MAX_COLS)(*([7] * abi.SSM_MAX_COLS))
    rc = lib.wsmc_ssm_spec_conditional(C.byref(ssm.spec), pin)
    if rc != abi.WSMC_OK:
        return rc, lib.wsmc_last_error().decode()
    assert all(v in (0, 1) for v in pin)
    return rc, [c for k, c in enumerate(ssm.cols) if pin[k]]


def test_symbols():
    lib = wsmc.load_library()
    for name in ("wsmc_ssm_spec_conditional", "wsmc_ssm_run_conditional", "wsmc_debug_ssm_conditional"):
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    pin = (C.c_int32 * abi.SSM_MAX_COLS)()
    sv = models.sv()
    assert lib.wsmc_ssm_spec_conditional(C.byref(sv.spec), None) == abi.WSMC_EARG
    assert lib.wsmc_ssm_spec_conditional(None, pin) == abi.WSMC_EARG and b"null spec" in lib.wsmc_last_error()
    st = (C.c_int64 * 5)()
    assert lib.wsmc_debug_ssm_conditional(None, st) == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    seeds, out = (C.c_uint64 * 2)(1, 2), abi.SsmBatchOut()
    ref = np.zeros((2, 4, 2))
    rc = lib.wsmc_ssm_run_conditional(None, C.byref(sv.spec), 1, None, 1, 4, 100, 2, seeds, 1.0, ref.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(out), None, 0, None, None)
    assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    rc = lib.wsmc_ssm_run_conditional(None, C.byref(sv.spec), 1, None, 1, 4, 100, 2, seeds, 1.0, None, C.byref(out), None, 0, None, None)
    assert rc == abi.WSMC_EARG and b"null reference" in lib.wsmc_last_error()


@pytest.mark.parametrize("name", sorted(sc.SHIPPED))
def test_shipped_specs_are_eligible(name):
    make, _, want = sc.SHIPPED[name]
    ssm = make()
    assert library_pinned(ssm) == (abi.WSMC_OK, want)
    assert ssm.conditional_terms() == want


def test_the_tests_own_specs_are_eligible():
    assert sc.two_observes().conditional_terms() == ["x"] == library_pinned(sc.two_observes())[1]
    assert sc.chained_samples().conditional_terms() == ["v", "x", "u"] == library_pinned(sc.chained_samples())[1]


def refused_specs():
    x = Col("x")
    own = {
        "importance": (models.lgssm1d_guided(), "statement 2 of step is an importance SAMPLE"),
        "weight": (SSM(cols=["x"]).init(sample("x", Normal(0.0, 1.0)))
                   .step(sample("x", Normal(x * 0.9, 1.0)), weight(x, Normal(0.0, 3.0)), observe(Data(0), Normal(x, 0.5))),
                   "statement 1 of step is a WEIGHT"),
        "observe_in_init": (SSM(cols=["x"], data_dim=1).init(sample("x", Normal(0.0, 1.0)), observe(0.3, Normal(x, 1.0)))
                            .step(sample("x", Normal(x * 0.9, 1.0)), observe(Data(0), Normal(x, 0.5))),
                            "statement 1 of init is an OBSERVE"),
    }
    # each of backward_terms' refusals, with the reason it gives (weight_last holds a WEIGHT: refused for that first)
    for name, (ssm, reason) in tb.refused_specs().items():
        own["backward_" + name] = (ssm, "statement 2 of step is a WEIGHT" if name == "weight_last" else reason)
    return own


@pytest.mark.parametrize("name", sorted(refused_specs()))
def test_refusals_carry_their_reason(name):
    ssm, reason = refused_specs()[name]
    ssm.check()   # a spec the run itself takes
    rc, why = library_pinned(ssm)
    assert rc == abi.WSMC_EARG and why.startswith("ssm conditional: ") and reason in why, why
    if name.startswith("backward_") and name != "backward_weight_last":
        assert why.startswith("ssm conditional: ssm backward: "), why
    with pytest.raises(ValueError) as e:
        ssm.conditional_terms()
    assert str(e.value) == why   # the library's reason, word for word


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


PROPERTY_SPECS = ("lgssm1d_spec", "kitagawa", "local_trend")


@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 2, 65])
@pytest.mark.parametrize("name", PROPERTY_SPECS)
def test_properties_of_the_definition(name, n, T):
    make, make_data, pinned = sc.SHIPPED[name]
    ssm, y, seed = make(), make_data(T), 100 + n + T
    ref = sc.reference(ssm, T, seed)
    pin = [ssm.cols.index(c) for c in pinned]
    for ess in (0.0, 0.5, 2.0):
        flags, _, _, rec, end, bw = sc.definition(ssm, y, n, seed, ref, ess, M=1, bw_seed=9)
        # row n-1 of the record is the reference at the pinned columns, bit for bit, at every step
        assert np.array_equal(bits(rec.cols[:, pin, n - 1]), bits(ref[:, pin])), ess
        assert end.n_resamples == sum(flags)
        if end.n_resamples:
            assert end.last_ancestors[n - 1] == n - 1 and np.all((0 <= end.last_ancestors) & (end.last_ancestors < n))
        else:
            assert not end.last_ancestors.any()
        if ess == 0.0:
            assert not any(flags)
        if ess == 2.0:
            assert all(flags)
        if n == 1:   # the only particle is the reference particle: the backward path is the reference
            for c, k in zip(pinned, pin):
                assert np.array_equal(bits(bw.paths[c][:, 0]), bits(ref[:, k]))
        # the unconditional run of the same seed
        o = Oracle(n, seed=seed)
        _, _, urec = ssm.statements(o, y, ess, record=True)
        o.close()
        # step 0, before the first Resample: particles 0 .. n-2 are the unconditional run's
        assert np.array_equal(bits(rec.cols[0][:, :n - 1]), bits(urec.cols[0][:, :n - 1]))
        assert np.array_equal(bits(rec.log_weights[0][:n - 1]), bits(urec.log_weights[0][:n - 1]))
        if ess == 0.0:   # never resamples: so is the whole record
            assert np.array_equal(bits(rec.cols[:, :, :n - 1]), bits(urec.cols[:, :, :n - 1]))
            assert np.array_equal(bits(rec.log_weights[:, :n - 1]), bits(urec.log_weights[:, :n - 1]))


def test_unpinned_reference_entries_are_ignored_and_init_is_free():
    ssm, y = models.kitagawa(), models.kitagawa_data(5)
    ref = sc.reference(ssm, 5, 3)
    other = ref.copy()
    other[:, 1:] = np.nan   # m and z are assigned, not pinned
    a = sc.definition(ssm, y, 9, 4, ref, 0.5)
    b = sc.definition(ssm, y, 9, 4, other, 0.5)
    assert np.array_equal(bits(a[3].cols), bits(b[3].cols)) and np.array_equal(bits(a[3].log_weights), bits(b[3].log_weights))
    # the assigned columns of row n-1 are recomputed from the pinned x: z = x^2 / 20
    assert np.array_equal(bits(a[3].cols[:, 2, 8]), bits(ref[:, 0] ** 2 / 20))


def test_pg_seeds():
    s0, b0 = wsmc.pg_seeds(7, 0, 4)
    assert s0.dtype == b0.dtype == np.uint64 and s0.shape == b0.shape == (4,)
    again = wsmc.pg_seeds(7, 0, 4)
    assert np.array_equal(s0, again[0]) and np.array_equal(b0, again[1])
    seen = set()
    for j in range(50):
        s, b = wsmc.pg_seeds(7, j, 4)
        seen |= {int(v) for v in s} | {int(v) for v in b}
    assert len(seen) == 50 * 4 * 2
    assert not seen & {int(v) for v in np.concatenate(wsmc.pg_seeds(8, 0, 4))}
    # the documented function, restated
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2**64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2**64
        return z ^ (z >> 31)
    s, b = wsmc.pg_seeds(7, 3, 4)
    for c in range(4):
        i = 2 * (3 * 4 + c)
        assert int(s[c]) == mix((7 + (i + 1) * 0x9E3779B97F4A7C15) % 2**64)
        assert int(b[c]) == mix((7 + (i + 2) * 0x9E3779B97F4A7C15) % 2**64)


def test_particle_gibbs_wrapper_checks():
    with pytest.raises(ValueError):
        wsmc.particle_gibbs(None, models.lgssm1d_spec(), models.lgssm1d_data(4), 8, 0, 1)
    with pytest.raises(ValueError):
        wsmc.particle_gibbs(None, models.lgssm1d_spec(), models.lgssm1d_data(4), 8, 2, 1, chains=0)


GIBBS_SWEEPS = 1200


def test_invariance_against_the_rts_smoother():
    """A guard against gross errors only (its power is low; the bit-exact device tests are the
    check of the kernel). Particle Gibbs with backward sampling as a loop over the definitions on
    the oracle: lgssm1d_spec, n = 8, T = 8, ess_perc_min = 2 (every Resample runs), 8 chains of
    GIBBS_SWEEPS sweeps, the first fifth dropped. The per-step smoothed mean over the kept sweeps,
    averaged over the chains, against the RTS smoother of the model with `init` integrated out, in
    units of the across-chain standard error: every |z| <= 5.
    Measured: the largest |z| is 2.95 at 1200 sweeps (20 s), 2.72 at 600 and 2.10 at 2400 (40 s)."""
    n, T, chains = 8, 8, 8
    y = models.lgssm1d_data(T)
    ms, _ = tb.rts(y)
    traj, logev = sc.definition_gibbs(models.lgssm1d_spec(), y, n, GIBBS_SWEEPS, 2024, chains=chains, ess=2.0)
    kept = traj["x"][GIBBS_SWEEPS // 5:]          # [sweeps kept, chains, T]
    per_chain = kept.mean(axis=0)                 # [chains, T]
    se = per_chain.std(axis=0, ddof=1) / np.sqrt(chains)
    z = (per_chain.mean(axis=0) - ms) / se
    print("largest |z|:", np.abs(z).max(), "z:", z)
    assert np.all(np.isfinite(logev))
    assert np.all(np.abs(z) <= 5.0), z

"""Host-side checks of the batched scalar-SSM run (wsmc_ssm_run_batch): the symbols and the result
struct's layout, the shape rule a batch's specs obey (wsmc_ssm_spec_same_shape, on the host alone),
and the wrapper's argument checks, which come before any device call. No compute without a GPU;
tests/test_gpu_ssm_batch.py compares the filters with the oracle.
"""
import ctypes as C

import numpy as np
import pytest

import wsmc
from wsmc import abi, dsl, models
from wsmc.dsl import Col, Data, Normal
from wsmc.ssm import SSM, assign, batch_arguments, observe, sample


def test_symbols_and_out_struct():
    lib = wsmc.load_library()
    for name in ("wsmc_ssm_run_batch", "wsmc_ssm_spec_same_shape", "wsmc_debug_ssm_batch", "wsmc_ssm_batch_out_sizeof"):
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    n = C.c_int64()
    assert lib.wsmc_ssm_batch_out_sizeof(C.byref(n)) == abi.WSMC_OK
    assert n.value == C.sizeof(abi.SsmBatchOut) == 7 * C.sizeof(C.c_void_p)
    assert [f for f, _ in abi.SsmBatchOut._fields_] == ["log_evidence", "ess_trace", "cols", "log_weights",
                                                        "last_ancestors", "n_resamples", "last_resampled"]


def clone(spec: SSM) -> SSM:
    """the spec's struct copied, to be changed by hand"""
    sp = abi.SsmSpec()
    C.memmove(C.byref(sp), C.byref(spec.spec), C.sizeof(abi.SsmSpec))
    return SSM.from_spec(sp)


@pytest.mark.parametrize("name", sorted(models.SSM_MODELS))
def test_same_shape_with_itself(name):
    spec = models.SSM_MODELS[name][0]()
    assert spec.same_shape(spec)
    assert spec.same_shape(clone(spec))
    assert spec.shape_difference(spec) is None


def test_same_shape_numbers_may_differ():
    a, b = models.sv(phi=0.9), models.sv(phi=0.97)
    assert a.same_shape(b) and b.same_shape(a)
    assert models.sv(mu=-1.0, sigma=0.2).same_shape(models.sv(mu=0.5, sigma=0.4))
    # a dist's param (Uniform's bounds) and a program's constants
    u = lambda lo, hi, k: (SSM(cols=["x", "y"])
                           .init(sample("x", dsl.Uniform(lo, hi)))
                           .step(assign("y", dsl.exp(Col("x") * k) + k),
                                 observe(Data(0), Normal(Col("y"), 1.0))))
    assert u(0.0, 1.0, 2.0).same_shape(u(-1.0, 3.0, 0.25))
    assert models.kitagawa(q=1.0).same_shape(models.kitagawa(q=2.0, r=0.3))


def _other_family():
    return (SSM(cols=["h", "s"])
            .init(sample("h", Normal(0.0, 0.8)))
            .step(sample("h", dsl.Laplace(Col("h") * 0.95 - 0.05, 0.25)),
                  assign("s", dsl.exp(Col("h") / 2)),
                  observe(Data(0), Normal(0.0, Col("s")))))


def _other_column():
    b = clone(models.sv())
    b.spec.step[0].dist.mu[0].col[0] = 1   # the transition reads s, not h
    return b


def _other_opcode():
    b = clone(models.sv())
    st = b.spec.step[1]
    assert st.kind == abi.SSM_ASSIGN_EXPR
    k = next(q for q in range(st.prog_len) if st.prog[q].op == abi.X_EXP)
    st.prog[k].op = abi.X_SIN
    return b


def _other_data_reference():
    a = (SSM(cols=["x"], data_dim=2)
         .init(sample("x", Normal(0.0, 1.0)))
         .step(sample("x", Normal(Col("x") * 0.9, 1.0)), observe(Data(0), Normal(Col("x"), 0.5))))
    b = clone(a)
    b.spec.step[1].value.comp[0] = 1   # observes data column 1
    return a, b


def _other_count():
    return (SSM(cols=["h", "s"])
            .init(sample("h", Normal(0.0, 0.8)))
            .step(sample("h", Normal(Col("h") * 0.95 - 0.05, 0.25)),
                  assign("s", dsl.exp(Col("h") / 2)),
                  observe(Data(0), Normal(0.0, Col("s"))),
                  observe(Data(0), Normal(0.0, Col("s")))))


def _other_name():
    b = clone(models.sv())
    b.spec.col_names[1].value = b"vol"
    return b


@pytest.mark.parametrize("case, field", [("family", "step[0].dist.family"), ("column", "step[0].dist.mu[0].col[0]"),
                                         ("opcode", "step[1].prog["), ("data", "step[1].value.comp[0]"),
                                         ("count", "n_step"), ("name", "col_names[1]")])
def test_different_shape_names_the_field(case, field):
    a = models.sv()
    if case == "data":
        a, b = _other_data_reference()
    else:
        b = {"family": _other_family, "column": _other_column, "opcode": _other_opcode, "count": _other_count,
             "name": _other_name}[case]()
    a.check()
    b.check()   # each a valid spec on its own
    assert not a.same_shape(b) and not b.same_shape(a)
    why = a.shape_difference(b)
    assert "differ in shape" in why and field in why, why
    if case == "opcode":
        assert why.rstrip().endswith(".op"), why
    lib = wsmc.load_library()
    assert lib.wsmc_ssm_spec_same_shape(C.byref(a.spec), C.byref(b.spec)) == abi.WSMC_EARG
    assert lib.wsmc_ssm_spec_same_shape(None, C.byref(b.spec)) == abi.WSMC_EARG


def test_powi_exponent_is_shape():
    mk = lambda p: (SSM(cols=["x", "z"])
                    .init(sample("x", Normal(0.0, 1.0)))
                    .step(assign("z", Col("x") ** p / 20), observe(Data(0), Normal(Col("z"), 1.0))))
    assert mk(2).same_shape(mk(2))
    why = mk(2).shape_difference(mk(3))
    assert why is not None and "prog[" in why


def test_wrapper_checks_come_before_the_device():
    """list lengths, the seeds, the tables: refused on the host (no context is needed to ask)"""
    sv, y = models.sv(), models.sv_data(8)
    specs, tabs, seeds = batch_arguments(sv, y, 100, [1, 2, 3])
    assert len(specs) == 1 and len(tabs) == 1 and tabs[0].shape == (8, 1) and seeds.dtype == np.uint64
    specs, tabs, seeds = batch_arguments([sv] * 3, [y, y + 1, y], 100, [1, 2, 2**64 - 1])
    assert len(specs) == 3 and len(tabs) == 3 and int(seeds[2]) == 2**64 - 1
    assert len(batch_arguments(sv, np.stack([y, y]).reshape(2, 8, 1), 100, [5, 6])[1]) == 2
    with pytest.raises(ValueError, match="specs"):
        batch_arguments([sv, sv], y, 100, [1, 2, 3])
    with pytest.raises(ValueError, match="seeds"):
        batch_arguments(sv, y, 100, [])
    with pytest.raises(ValueError, match="data"):
        batch_arguments(sv, [y, y], 100, [1, 2, 3])      # n_tables = 2, B = 3
    with pytest.raises(ValueError, match="one length"):
        batch_arguments(sv, [y, y[:5]], 100, [1, 2])
    with pytest.raises(ValueError, match="n:"):
        batch_arguments(sv, y, 0, [1])
    with pytest.raises(ValueError, match="step"):
        batch_arguments(sv, y[:0], 100, [1])
    # the method itself: the same refusals with no library handle behind the object
    g = object.__new__(wsmc.Context)
    with pytest.raises(ValueError, match="specs"):
        wsmc.Context.ssm_run_batch(g, [sv, sv], y, 100, [1, 2, 3])
    with pytest.raises(ValueError, match="data"):
        wsmc.Context.ssm_run_batch(g, sv, [y, y], 100, [1, 2, 3])


def test_library_refuses_before_the_device():
    """the C entry point's own argument checks need no device either (a null context first)"""
    lib = wsmc.load_library()
    sv = models.sv()
    seeds = (C.c_uint64 * 2)(1, 2)
    out = abi.SsmBatchOut()
    rc = lib.wsmc_ssm_run_batch(None, C.byref(sv.spec), 1, None, 1, 4, 100, 2, seeds, 1.0, abi.RESAMPLE_STRATIFIED,
                                C.byref(out))
    assert rc == abi.WSMC_EARG and b"null context" in lib.wsmc_last_error()
    assert lib.wsmc_debug_ssm_batch(None, -1, None) == abi.WSMC_EARG

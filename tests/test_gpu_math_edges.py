"""The shared math at its edges on the GPU (tests/mathedge.py's corpus) against the CPU oracle, bit
for bit through `view(np.uint64)`: a NaN matches any NaN (an invalid operation's default NaN is
negative on x86 and positive on the GPU), -0.0 is distinct from 0.0, and there is no tolerance
anywhere in this file. tests/test_math_edges.py holds the oracle itself to mpmath.

include/wsmc_math.h and include/wsmc_terms.h are compiled for the device several ways, and each
test asserts which one it ran on:
  (a) an expression operator as one Assign alone, then a download: the library's k_assign_expr (an
      expression Assign is never part of a statement batch, so the run-time compiler's counters
      stand still);
  (b) every operator of one arity issued back to back, downloaded at the end: the same kernel, the
      launches queued behind one another;
  (c) (a), (b), the log-densities and the draws in a child process under WSMC_DIAG_NO_JIT=1: the
      library's own k_weigh / k_sample for a statement alone and the interpreter k_ew_batch for
      several (`launched == 0 and interpreted > 0`);
  (d) the persistent scalar-SSM workgroup (csrc/wsmc_ssm_body.h): a spec whose step evaluates the
      operator on a data column, one corpus point per step, read back as the smoothed paths;
  (e) a family's log-density with both parameters and the value from columns, as one Observe alone
      and as two back to back: statement batches compiled for their shape at run time (`launched`
      rises, `interpreted` does not), then the same term through the Moves' fold, score(depth);
  (f) draws with the parameters from columns at every sampler threshold, then the draw observed
      under the same distribution: one compiled batch.
A difference is reported by mathedge.first_difference: the operator or family, the arrangement, the
index, the input value(s) and both bit patterns (`python tests/mathedge.py --op NAME --backend hip`
replays one entry)."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import mathedge as me
import wsmc
from oracle import Oracle
from wsmc import abi, models
from wsmc.dsl import Col

pytestmark = pytest.mark.gpu

SSM_N, SSM_STEPS = 65, 256      # one particle in the second wave; steps per persistent run
ARITIES = {1: me.UNARY, 2: me.BINARY, 3: ["ifelse"]}
FAMILIES = [n for n in me.LOGPDFS]


def jit_counts():
    st = abi.jit_stats()
    return st["launched"], st["interpreted"]


# ---- (a), (b): the operators through Assign -----------------------------------------------------------
def operator_alone(name):
    e = me.OPERATORS[name]
    want = me.oracle_operator(name)
    g = wsmc.Context(2 * e.n, seed=1)
    try:
        got = me.run_operator(g, e, each=True)
        depth = g.get_state()["depth"]
    finally:
        g.close()
    assert depth == 2 * len(e.variants), depth   # every Assign ran
    ins = me.operator_inputs(e)
    for (w, v), y in want.items():
        d = me.first_difference(e.label(e.variants[v]), w, ins[w], got[(w, v)], y)
        assert d is None, d


def _issue_arity(ctx, names, n):
    for name in names:
        e = me.OPERATORS[name]
        me.upload(ctx, {k: np.resize(v, n) for k, v in me.operator_columns(e, name + "_").items()})
    count = 0
    for name in names:
        for out, _, _, tree in me.operator_statements(me.OPERATORS[name], name + "_"):
            me.assign_tree(ctx, out, tree)
            count += 1
    return count


def operators_back_to_back(arity):
    """every operator of the arity on one context (each entry's columns repeated up to the longest
    entry's length), nothing read until the last Assign has been issued"""
    names = ARITIES[arity]
    n = max(2 * me.OPERATORS[name].n for name in names)
    g, o = wsmc.Context(n, seed=1), Oracle(n, seed=1)
    try:
        count = _issue_arity(g, names, n)
        assert _issue_arity(o, names, n) == count
        assert g.get_state()["depth"] == count
        for name in names:
            e = me.OPERATORS[name]
            cols = me.operator_columns(e, name + "_")
            for out, w, v, _ in me.operator_statements(e, name + "_"):
                ins = tuple(np.resize(cols[f"{name}_{w}{k}"], n) for k in range(e.arity))
                d = me.first_difference(e.label(e.variants[v]), w + ", back to back", ins,
                                        g.col_download(g.col_find(out)), o.col_download(o.col_find(out)))
                assert d is None, d
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("name", list(me.OPERATORS))
def test_operator_alone(gpu_available, name):
    before = jit_counts()
    operator_alone(name)
    assert jit_counts() == before   # k_assign_expr: no statement batch, compiled or interpreted


@pytest.mark.parametrize("arity", sorted(ARITIES))
def test_operators_back_to_back(gpu_available, arity):
    before = jit_counts()
    operators_back_to_back(arity)
    assert jit_counts() == before


# ---- (d): the persistent scalar-SSM workgroup ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(me.OPERATORS))
def test_operator_in_the_ssm_workgroup(gpu_available, name):
    """N = 65 and a threshold of 0.0 (no Resample), so paths[c][t] is the operator at point t for
    every particle: against the definition (SSM.statements on the oracle, smooth=True) through
    test_gpu_ssm_smooth.run_pair, which also compares everything else the run leaves with
    ssmfuzz.compare and asserts one persistent run and no statement run; and against the oracle's
    value of the same point through Assign"""
    import test_gpu_ssm_smooth as tsm
    e = me.OPERATORS[name]
    want = me.oracle_operator(name)
    for variants, lo, hi in me.ssm_runs(e, SSM_STEPS):
        case = me.ssm_case(e, variants, lo, hi)
        _, sm = tsm.run_pair(case.ssm, case.data, SSM_N, 0.0, trace=False, smooth=("paths",), what=case.name)
        for c, v in enumerate(variants):
            paths = np.asarray(sm.paths[f"c{c}"])
            assert paths.shape == (hi - lo, SSM_N)
            direct = np.repeat(want[("built", v)][lo:hi, None], SSM_N, axis=1)
            ins = tuple(np.repeat(a[lo:hi], SSM_N) for a in e.args)
            d = me.first_difference(e.label(e.variants[v]), f"ssm steps {lo}:{hi}, (step, particle) flattened", ins, paths, direct)
            assert d is None, d


# ---- (e): the log-densities ---------------------------------------------------------------------------------
def logpdf_alone(name):
    """one Observe with its parameters and value from columns, the weights downloaded (a batch of one
    statement), then the same term through the fold"""
    e = me.LOGPDFS[name]
    for w in me.ARRANGEMENTS:
        g, o = wsmc.Context(2 * e.n, seed=1), Oracle(2 * e.n, seed=1)
        try:
            (gw, gs), (ow, os_) = me.run_logpdf(g, e, w), me.run_logpdf(o, e, w)
        finally:
            g.close()
            o.close()
        ins = e.inputs()[w]
        d = me.first_difference(f"logpdf:{name}", w, ins, gw, ow) or \
            me.first_difference(f"logpdf:{name} score(depth)", w, ins, gs, os_)
        assert d is None, d


def logpdf_batched(name):
    """both arrangements as columns of one context and their two Observes back to back (one
    statement batch): the summed weights, then score(depth)"""
    e = me.LOGPDFS[name]
    res = []
    ins = e.inputs()
    for ctx in (wsmc.Context(2 * e.n, seed=1), Oracle(2 * e.n, seed=1)):
        try:
            for k, w in enumerate(me.ARRANGEMENTS):
                a, b, x = ins[w]
                me.upload(ctx, {f"a{k}": a, f"b{k}": b, f"x{k}": x})
            R = models.resolver(ctx)
            for k in range(2):
                ctx.observe(e.kernel(f"a{k}", f"b{k}").dist(R), [Col(f"x{k}").operand(R)])
            res.append((ctx.weights_download(), ctx.score(ctx.get_state()["depth"])))
        finally:
            ctx.close()
    both = ins["built"] + ins["mixed"]
    d = me.first_difference(f"logpdf:{name}", "built + mixed, one batch", both, res[0][0], res[1][0]) or \
        me.first_difference(f"logpdf:{name} score(depth)", "built + mixed, one batch", both, res[0][1], res[1][1])
    assert d is None, d


@pytest.mark.parametrize("name", FAMILIES)
def test_logpdf_alone(gpu_available, name):
    launched, interpreted = jit_counts()
    logpdf_alone(name)
    after = jit_counts()
    assert after[0] >= launched + 2 and after[1] == interpreted, (launched, interpreted, after)


@pytest.mark.parametrize("name", FAMILIES)
def test_logpdf_batched(gpu_available, name):
    launched, interpreted = jit_counts()
    logpdf_batched(name)
    after = jit_counts()
    assert after[0] >= launched + 1 and after[1] == interpreted, (launched, interpreted, after)


# ---- (f): the draws -----------------------------------------------------------------------------------------
def draws(name):
    e = me.DRAWS[name]
    for w in me.ARRANGEMENTS:
        g, o = wsmc.Context(2 * e.n, seed=1), Oracle(2 * e.n, seed=1)
        try:
            (gx, gw), (ox, ow) = me.run_draw(g, e, w), me.run_draw(o, e, w)
        finally:
            g.close()
            o.close()
        ins = e.inputs()[w]
        d = me.first_difference(f"draw:{name}", w, ins, gx, ox) or \
            me.first_difference(f"draw:{name} (the draw's log-density)", w, ins + (ox,), gw, ow)
        assert d is None, d


@pytest.mark.parametrize("name", list(me.DRAWS))
def test_draws(gpu_available, name):
    launched, interpreted = jit_counts()
    draws(name)
    after = jit_counts()
    assert after[0] >= launched + 2 and after[1] == interpreted, (launched, interpreted, after)


# ---- (c): the library's own kernels ------------------------------------------------------------------------
# WSMC_DIAG_NO_JIT is read once per process, so the library kernels run in a child process (as in
# tests/test_gpu_gamma_families.py): k_weigh / k_sample for a statement alone, k_ew_batch for several
CHILD = r"""
import sys
sys.path[:0] = [{pkg!r}, {orc!r}, {tests!r}]
from wsmc import abi
import test_gpu_math_edges as t

for name in t.me.OPERATORS:
    t.operator_alone(name)
for arity in t.ARITIES:
    t.operators_back_to_back(arity)
for name in t.FAMILIES:
    t.logpdf_alone(name)
    t.logpdf_batched(name)
for name in t.me.DRAWS:
    t.draws(name)
st = abi.jit_stats()
print("EWJIT", st["launched"], st["interpreted"])
"""


def test_library_kernels_without_the_runtime_compiler(gpu_available):
    repo = pathlib.Path(__file__).resolve().parents[1]
    code = CHILD.format(pkg=str(repo / "weightedsampling.jl_amd"), orc=str(repo / "oracle"), tests=str(repo / "tests"))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "WSMC_DIAG_NO_JIT": "1"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("EWJIT")][0]
    launched, interpreted = map(int, line.split()[1:])
    assert launched == 0 and interpreted > 0, line

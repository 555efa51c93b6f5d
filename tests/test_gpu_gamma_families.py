"""The log-Gamma families (WSMC_FAM_GAMMA .. WSMC_FAM_NEGBINOMIAL) on the GPU against the oracle,
bit for bit: draws and log-densities through compiled statement batches and single statements,
every sampler branch, parameters from a column that straddles every sampler threshold within one
wave (the rejection loops' trip counts then differ between neighbouring lanes), the importance
path, Moves whose score fold holds the new families' terms, and the library's own (not run-time
compiled) kernels in a child process with the run-time compiler switched off."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import wsmc
from oracle import Oracle
from wsmc import abi, models
from wsmc.dsl import Col

pytestmark = pytest.mark.gpu

# every family, one case per sampler branch (tests/test_gamma_families.py DRAW_CASES)
KERNELS = {
    "gamma-0.3": lambda: wsmc.Gamma(0.3, 2.0),
    "gamma-1": lambda: wsmc.Gamma(1.0, 2.0),
    "gamma-7.5": lambda: wsmc.Gamma(7.5, 0.5),
    "invgamma": lambda: wsmc.InverseGamma(3.0, 2.0),
    "chisq": lambda: wsmc.Chisq(5.0),
    "beta-0.5-0.5": lambda: wsmc.Beta(0.5, 0.5),
    "beta-2-5": lambda: wsmc.Beta(2.0, 5.0),
    "tdist-1.5": lambda: wsmc.TDist(1.5),
    "tdist-30": lambda: wsmc.TDist(30.0),
    "poisson-0.7": lambda: wsmc.Poisson(0.7),
    "poisson-9.99": lambda: wsmc.Poisson(9.99),
    "poisson-10": lambda: wsmc.Poisson(10.0),
    "poisson-250": lambda: wsmc.Poisson(250.0),
    "binomial-20-0.1": lambda: wsmc.Binomial(20, 0.1),
    "binomial-40-0.5": lambda: wsmc.Binomial(40, 0.5),
    "binomial-1000-0.3": lambda: wsmc.Binomial(1000, 0.3),
    "binomial-1000-0.97": lambda: wsmc.Binomial(1000, 0.97),
    "negbinomial-0.5": lambda: wsmc.NegativeBinomial(0.5, 0.3),
    "negbinomial-12": lambda: wsmc.NegativeBinomial(12.0, 0.4),
}
# the second Observe's point: inside the support of each family (an integer for the discrete ones)
SHIFT = {"beta": 0.0, "poisson": 1.0, "binomial": 0.0, "negbinomial": 1.0}


def same(g, o, names):
    for n in names:
        a = g.col_download(g.col_find(n))
        b = o.col_download(o.col_find(n))
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=n)
    np.testing.assert_array_equal(g.weights_download().view(np.uint64), o.weights_download().view(np.uint64))


def draw_and_score(ctx, kern, shift):
    """x ~ D; y ~ D (one batch: Sample, Sample, Observe, Observe); the weights are
    logpdf(D, x) + logpdf(D, y + shift)"""
    R = models.resolver(ctx)
    d = kern.dist(R)
    cx, cy = ctx.col_create("x"), ctx.col_create("y")
    ctx.sample(cx, d)
    ctx.sample(cy, d)
    ctx.observe(d, Col("x").operand(R))
    ctx.observe(d, (Col("y") + shift).operand(R))


@pytest.mark.parametrize("name", sorted(KERNELS))
@pytest.mark.parametrize("N", [4096, 1001])
def test_family_draws_and_logpdf_match_the_oracle(gpu_available, name, N):
    g, o = wsmc.Context(N, seed=31), Oracle(N, seed=31)
    for ctx in (g, o):
        draw_and_score(ctx, KERNELS[name](), SHIFT.get(name.split("-")[0], 0.25))
    same(g, o, ["x", "y"])
    g.close()


# parameters from columns that straddle every sampler threshold within 64 consecutive particles
def _poisson(N):
    return {"a": np.tile([0.5, 9.99, 10.0, 300.0], N)[:N]}, lambda: wsmc.Poisson(Col("a"))


def _gamma(N):
    return {"a": np.tile([0.2, 1.0, 50.0], N)[:N]}, lambda: wsmc.Gamma(Col("a"), 1.5)


def _binomial(N):
    # n p = 9 / 11 (p < 1/2), n (1 - p) = 9 / 11 (p > 1/2), a small n, p at 1/2
    n = np.tile([30.0, 110.0, 30.0, 110.0, 7.0, 64.0], N)[:N]
    p = np.tile([0.3, 0.1, 0.7, 0.9, 0.45, 0.5], N)[:N]
    return {"a": n, "b": p}, lambda: wsmc.Binomial(Col("a"), Col("b"))


def _negbinomial(N):
    return {"a": np.tile([0.4, 3.0, 40.0], N)[:N], "b": np.tile([0.5, 0.05], N)[:N]}, \
        lambda: wsmc.NegativeBinomial(Col("a"), Col("b"))


def divergent(make, N=1001):
    g, o = wsmc.Context(N, seed=17), Oracle(N, seed=17)
    for ctx in (g, o):
        cols, kern = make(N)
        R = models.resolver(ctx)
        for name, v in cols.items():
            ctx.col_upload(ctx.col_create(name), v)
        d = kern().dist(R)
        cx = ctx.col_create("x")
        ctx.sample(cx, d)
        ctx.observe(d, Col("x").operand(R))
    same(g, o, ["x"])
    g.close()


@pytest.mark.parametrize("make", [_poisson, _gamma, _binomial, _negbinomial], ids=lambda f: f.__name__[1:])
def test_divergent_parameters_within_a_wave(gpu_available, make):
    divergent(make)


SINGLES = ["gamma-0.3", "invgamma", "beta-2-5", "tdist-1.5", "poisson-250", "binomial-1000-0.97", "negbinomial-12"]


def single_statements(name, N=1001):
    g, o = wsmc.Context(N, seed=5), Oracle(N, seed=5)
    for ctx in (g, o):
        R = models.resolver(ctx)
        d = KERNELS[name]().dist(R)
        cx = ctx.col_create("x")
        ctx.sample(cx, d)
        ctx.col_download(cx)
        ctx.observe(d, Col("x").operand(R))
        ctx.weights_download()
    same(g, o, ["x"])
    g.close()


@pytest.mark.parametrize("name", SINGLES)
def test_single_statements(gpu_available, name):
    """wsmc_sample / wsmc_observe issued alone (a download in between closes the batch): batches of
    one statement, each compiled for its shape at run time like any other batch"""
    single_statements(name)


# The kernels a batch runs on when its shape does not compile at run time: k_sample<GAM> and
# k_weigh<GAM> for a statement alone, the interpreter k_ew_batch<ALL> for several. WSMC_DIAG_NO_JIT
# selects them and is read once per process, so they run in a child process (as
# tests/test_gpu_interp.py does for the Moves).
CHILD = r"""
import sys
sys.path[:0] = [{pkg!r}, {orc!r}, {tests!r}]
import wsmc
from oracle import Oracle
from wsmc import abi
import test_gpu_gamma_families as t

for name in t.SINGLES:
    t.single_statements(name)
for make in (t._poisson, t._gamma, t._binomial, t._negbinomial):
    t.divergent(make)
for name in ("beta-0.5-0.5", "tdist-30", "gamma-7.5"):
    g, o = wsmc.Context(1001, seed=31), Oracle(1001, seed=31)
    for ctx in (g, o):
        t.draw_and_score(ctx, t.KERNELS[name](), t.SHIFT.get(name.split("-")[0], 0.25))
    t.same(g, o, ["x", "y"])
    g.close()
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


def test_sample_importance(gpu_available):
    """a Gamma proposal for an InverseGamma target (src/default_kernels.jl:69-73)"""
    N = 4096 + 37
    g, o = wsmc.Context(N, seed=8), Oracle(N, seed=8)
    for ctx in (g, o):
        R = models.resolver(ctx)
        cx = ctx.col_create("x")
        ctx.sample_importance(cx, wsmc.Gamma(2.0, 0.7).dist(R), wsmc.InverseGamma(3.0, 2.0).dist(R))
    same(g, o, ["x"])
    g.close()


def count_model(ctx, ys):
    """s2 ~ InverseGamma(2, 1); lam ~ Gamma(2, 1.5); y_k => Poisson(lam); a Normal(0, sqrt s2) term;
    Resample(1.0); bounded autoRW Moves on lam and s2 — the Moves fold the InverseGamma, Gamma and
    Poisson terms (generic fold)"""
    R = models.resolver(ctx)
    cs, cl = ctx.col_create("s2"), ctx.col_create("lam")
    ctx.sample(cs, wsmc.InverseGamma(2.0, 1.0).dist(R))
    ctx.sample(cl, wsmc.Gamma(2.0, 1.5).dist(R))
    csd = ctx.col_create("sd")
    prog, lens = wsmc.dsl.xprogram([wsmc.dsl.sqrt(Col("s2"))], R)
    acc = []
    for k, y in enumerate(ys):
        ctx.observe(wsmc.Poisson(Col("lam")).dist(R), models._const([y]))
        if k == 2:
            ctx.assign_expr(csd, prog, lens)
            ctx.observe(wsmc.Normal(0.0, Col("sd")).dist(R), models._const([0.8]))
        rs, _ = ctx.resample(1.0)
        if rs:
            acc.append((ctx.move(abi.PROPOSAL_AUTORW, [cl], 1e-3, lo=[0.0], hi=[np.inf]),
                        ctx.move(abi.PROPOSAL_AUTORW, [cs], 1e-3, lo=[0.0], hi=[np.inf])))
    return acc


def test_moves_over_the_new_families_match_the_oracle(gpu_available):
    N = 8192
    ys = [3.0, 1.0, 4.0, 2.0, 6.0, 3.0]
    g, o = wsmc.Context(N, seed=9), Oracle(N, seed=9)
    ag, ao = count_model(g, ys), count_model(o, ys)
    assert ag == ao and len(ag) > 0
    g.store_materialize()
    same(g, o, ["lam", "s2"])
    g.close()


def test_family_argument_checks(gpu_available):
    g = wsmc.Context(64, seed=1)
    c = g.col_create("x")
    d = wsmc.Gamma(1.0, 1.0).dist(models.resolver(g))
    d.family = 24
    with pytest.raises(wsmc.WSMCError):
        g.sample(c, d)
    for fam in range(16, 24):
        d = wsmc.Gamma(1.0, 1.0).dist(models.resolver(g))
        d.family = fam
        d.dim = 2
        with pytest.raises(wsmc.WSMCError):
            g.sample(c, d)
    g.close()

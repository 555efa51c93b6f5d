"""The log-Gamma families (WSMC_FAM_GAMMA .. WSMC_FAM_NEGBINOMIAL; the reference's
default_kernels, src/default_kernels.jl:83-102) on the CPU oracle: wsmc_lgamma against
mpmath.loggamma at 50 digits, every logpdf against scipy.stats (mpmath where scipy is the less
accurate side) at interior points, support edges and parameter edges, the draws' distribution
for every sampler branch, and two conjugate models against their closed forms (the `hip` leg of
those runs under -m gpu). The HIP kernels are compared with the oracle bit for bit in
tests/test_gpu_gamma_families.py. Parity with Julia's draws is not claimed: the streams are
Philox (include/wsmc_math.h)."""
import ctypes as C
import pathlib
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest
from scipy import special, stats

import wsmc
from backends import BACKENDS, make_ctx
from oracle import Oracle
from wsmc import abi, models
from wsmc.dsl import Col

REPO = pathlib.Path(__file__).resolve().parents[1]


# ---- wsmc_lgamma ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    """tests/hooks/wsmc_math_hook.c built with the oracle's flags (oracle/Makefile)"""
    so = tmp_path_factory.mktemp("hook") / "libwsmc_math_hook.so"
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-mfma", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                           "-I", str(REPO / "include"), "-shared", str(REPO / "tests" / "hooks" / "wsmc_math_hook.c"),
                           "-o", str(so)])
    return C.CDLL(str(so))


def _lgamma(hook, x):
    x = np.ascontiguousarray(x, float)
    out = np.empty_like(x)
    hook.hook_lgamma(x.ctypes.data_as(C.c_void_p), C.c_int64(len(x)), out.ctypes.data_as(C.c_void_p))
    return out


def _around(v, k=4):
    out, a, b = [v], v, v
    for _ in range(k):
        a, b = np.nextafter(a, -np.inf), np.nextafter(b, np.inf)
        out += [a, b]
    return out


# the boundaries between the scheme's pieces (include/wsmc_math.h wsmc_lgamma)
PIECES = [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.0]
LGAMMA_ABS = 1.09e-16   # measured: the largest absolute error inside [0.5, 3] (at x = 2.794)
LGAMMA_ULP = 1.52       # measured: the largest error outside, in ulps of the result (x just below 0.5)


def test_lgamma_against_mpmath(hook):
    """Measured on this grid: absolute error 1.085e-16 inside [0.5, 3] (the result there is below
    1 in magnitude and goes through 0 at 1 and 2, so ulps of it mean nothing), 1.512 ulp of the
    result elsewhere (a denser scan of 140 000 random arguments over (0, 100) found 1.19e-16 and
    1.78 ulp, the latter at x = 11.25 in the Stirling piece: inside the margin, under 2 ulp). The
    assertion is twice each: the margin is for the arguments not on the grid."""
    mp.mp.dps = 50
    rs = np.random.default_rng(5)
    xs = list(np.logspace(-300, 300, 2401)) + list(np.linspace(0.5, 3.0, 2501))
    xs += _around(1.0) + _around(2.0) + _around(3.0) + list(np.arange(1, 401) / 2.0)
    for b in PIECES:
        xs += _around(b)
    xs += list(rs.uniform(0.0, 0.5, 800)) + list(rs.uniform(3.0, 8.0, 800)) + list(rs.uniform(8.0, 200.0, 800))
    xs = np.array(xs)
    got = _lgamma(hook, xs)
    worst_abs = worst_ulp = mp.mpf(0)
    for x, g in zip(xs, got):
        want = mp.loggamma(mp.mpf(float(x)))
        err = abs(mp.mpf(float(g)) - want)
        if 0.5 <= x <= 3.0:
            worst_abs = max(worst_abs, err)
        else:
            worst_ulp = max(worst_ulp, err / mp.mpf(float(np.spacing(abs(float(want))))))
    print(f"lgamma: abs error {float(worst_abs):.3e} in [0.5, 3], {float(worst_ulp):.3f} ulp outside")
    assert float(worst_abs) <= 2 * LGAMMA_ABS
    assert float(worst_ulp) <= 2 * LGAMMA_ULP


def test_lgamma_edges(hook):
    got = _lgamma(hook, [0.0, np.inf, 1.0, 2.0, -1.0, np.nan])
    assert got[0] == np.inf and got[1] == np.inf
    assert got[2] == 0.0 and got[3] == 0.0
    assert np.isnan(got[4]) and np.isnan(got[5])


def test_lbeta_and_lchoose(hook):
    """the three-lgamma combinations: a few ulp of the largest term"""
    mp.mp.dps = 50
    a = np.array([0.5, 2.0, 7.5, 120.0, 0.01])
    b = np.array([0.5, 5.0, 0.3, 340.0, 30.0])
    out = np.empty_like(a)
    hook.hook_lbeta(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.c_int64(len(a)),
                    out.ctypes.data_as(C.c_void_p))
    for x, y, g in zip(a, b, out):
        big = max(abs(special.gammaln(x)), abs(special.gammaln(y)), abs(special.gammaln(x + y)))
        want = mp.loggamma(x) + mp.loggamma(y) - mp.loggamma(mp.mpf(x) + mp.mpf(y))
        assert abs(mp.mpf(float(g)) - want) <= 6 * np.spacing(big), (x, y)
    n = np.array([5.0, 40.0, 1000.0, 1000.0])
    k = np.array([2.0, 20.0, 0.0, 300.0])
    hook.hook_lchoose(n.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), C.c_int64(len(n)),
                      out.ctypes.data_as(C.c_void_p))
    for x, y, g in zip(n, k, out[:4]):
        want = mp.log(mp.binomial(int(x), int(y)))
        assert abs(mp.mpf(float(g)) - want) <= 6 * np.spacing(special.gammaln(x + 1)), (x, y)


# ---- logpdf -----------------------------------------------------------------------------
def observe_at(kernel, xs):
    o = Oracle(len(xs), seed=1)
    cx = o.col_create("x")
    o.col_upload(cx, np.asarray(xs, float))
    o.observe(kernel.dist(models.resolver(o)), Col("x").operand(models.resolver(o)))
    return o.weights_download()


def _lg(x):
    return abs(float(special.gammaln(x)))


def _log(x):
    return abs(float(np.log(x))) if x > 0 else 0.0


# per family: the summed magnitudes of the textbook formula's terms at (parameters, x), and the
# formula itself in mpmath
MAG = {
    "gamma": lambda a, t, x: abs(a - 1) * _log(x) + x / t + _lg(a) + abs(a) * _log(t),
    "invgamma": lambda a, t, x: abs(a) * _log(t) + _lg(a) + (a + 1) * _log(x) + t / x,
    "chisq": lambda n, _, x: abs(n / 2 - 1) * _log(x) + x / 2 + _lg(n / 2) + n / 2 * np.log(2),
    "beta": lambda a, b, x: (abs(float(special.xlogy(a - 1, x))) + abs(float(special.xlog1py(b - 1, -x)))
                             + _lg(a) + _lg(b) + _lg(a + b)),
    "tdist": lambda n, _, x: _lg((n + 1) / 2) + _lg(n / 2) + 0.5 * _log(n * np.pi) + (n + 1) / 2 * float(np.log1p(x * x / n)),
    "poisson": lambda l, _, x: x * _log(l) + l + _lg(x + 1),
    "binomial": lambda n, p, x: _lg(n + 1) + _lg(x + 1) + _lg(n - x + 1) + x * _log(p) + abs(float(special.xlog1py(n - x, -p))),
    "negbinomial": lambda r, p, x: _lg(r + x) + _lg(r) + _lg(x + 1) + r * _log(p) + abs(float(special.xlog1py(x, -p))),
}
_M = mp.mpf
MPF = {
    "gamma": lambda a, t, x: (_M(a) - 1) * mp.log(x) - _M(x) / t - mp.loggamma(a) - _M(a) * mp.log(t),
    "invgamma": lambda a, t, x: _M(a) * mp.log(t) - mp.loggamma(a) - (_M(a) + 1) * mp.log(x) - _M(t) / x,
    "chisq": lambda n, _, x: (_M(n) / 2 - 1) * mp.log(x) - _M(x) / 2 - mp.loggamma(_M(n) / 2) - _M(n) / 2 * mp.log(2),
    "beta": lambda a, b, x: ((_M(a) - 1) * mp.log(x) + (_M(b) - 1) * mp.log1p(-_M(x))
                             - (mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(_M(a) + _M(b)))),
    "tdist": lambda n, _, x: (mp.loggamma((_M(n) + 1) / 2) - mp.loggamma(_M(n) / 2) - mp.log(_M(n) * mp.pi) / 2
                              - (_M(n) + 1) / 2 * mp.log1p(_M(x) ** 2 / n)),
    "poisson": lambda l, _, x: _M(x) * mp.log(l) - l - mp.loggamma(_M(x) + 1),
    "binomial": lambda n, p, x: (mp.loggamma(_M(n) + 1) - mp.loggamma(_M(x) + 1) - mp.loggamma(_M(n) - x + 1)
                                 + _M(x) * mp.log(p) + (_M(n) - x) * mp.log1p(-_M(p))),
    "negbinomial": lambda r, p, x: (mp.loggamma(_M(r) + x) - mp.loggamma(r) - mp.loggamma(_M(x) + 1)
                                    + _M(r) * mp.log(p) + _M(x) * mp.log1p(-_M(p))),
}
KERNEL = {
    "gamma": lambda a, b: wsmc.Gamma(a, b), "invgamma": lambda a, b: wsmc.InverseGamma(a, b),
    "chisq": lambda a, b: wsmc.Chisq(a), "beta": lambda a, b: wsmc.Beta(a, b), "tdist": lambda a, b: wsmc.TDist(a),
    "poisson": lambda a, b: wsmc.Poisson(a), "binomial": lambda a, b: wsmc.Binomial(a, b),
    "negbinomial": lambda a, b: wsmc.NegativeBinomial(a, b),
}
SCIPY = {
    "gamma": lambda a, b: stats.gamma(a, scale=b), "invgamma": lambda a, b: stats.invgamma(a, scale=b),
    "chisq": lambda a, b: stats.chi2(a), "beta": lambda a, b: stats.beta(a, b), "tdist": lambda a, b: stats.t(a),
    "poisson": lambda a, b: stats.poisson(a), "binomial": lambda a, b: stats.binom(a, b),
    "negbinomial": lambda a, b: stats.nbinom(a, b),
}
DISCRETE = ("poisson", "binomial", "negbinomial")
# (family, a, b, test points, reference, {x: value scipy does not give}): interior points, every
# support edge, outside the support, the parameter edges. "mpmath": large arguments, where
# scipy's gammaln differences are the less accurate side
LOGPDF_CASES = [
    ("gamma", 0.3, 2.0, [0.0, 1e-8, 0.4, 3.0, 60.0, -1.0], "scipy", {}),
    ("gamma", 1.0, 2.5, [0.0, 0.4, 3.0, -0.5], "scipy", {}),
    ("gamma", 7.5, 0.5, [0.0, 0.4, 3.0, 60.0, -1.0], "scipy", {}),
    ("gamma", 350.0, 1.5, [400.0, 525.0, 700.0], "mpmath", {}),
    ("invgamma", 2.0, 1.0, [0.0, 1e-3, 0.4, 3.0, 1e4, -1.0], "scipy", {0.0: -np.inf}),
    ("invgamma", 0.4, 3.0, [0.2, 5.0], "scipy", {}),
    ("chisq", 1.0, 1.0, [0.0, 0.3, 5.0, -1.0], "scipy", {}),
    ("chisq", 2.0, 1.0, [0.0, 0.3, 5.0], "scipy", {}),
    ("chisq", 9.0, 1.0, [0.0, 0.3, 5.0, 40.0], "scipy", {}),
    ("beta", 0.5, 0.5, [0.0, 1e-9, 0.3, 0.999, 1.0, -0.1, 1.1], "scipy", {}),
    ("beta", 2.0, 5.0, [0.0, 0.3, 0.999, 1.0, 1.5], "scipy", {}),
    ("beta", 1.0, 1.0, [0.0, 0.5, 1.0], "scipy", {}),
    ("beta", 300.0, 700.0, [0.25, 0.3, 0.35], "mpmath", {}),
    ("tdist", 1.5, 1.0, [0.0, -0.7, 3.0, 1e6], "scipy", {}),
    ("tdist", 30.0, 1.0, [0.0, -0.7, 3.0, 50.0], "scipy", {}),
    ("poisson", 0.7, 1.0, [0.0, 1.0, 5.0, 2.5, -1.0], "scipy", {}),
    ("poisson", 0.0, 1.0, [0.0, 1.0, 0.5], "scipy", {}),
    ("poisson", 250.0, 1.0, [0.0, 200.0, 250.0, 330.0], "mpmath", {}),
    ("binomial", 20.0, 0.1, [0.0, 2.0, 20.0, 21.0, 2.5, -1.0], "scipy", {}),
    ("binomial", 20.0, 0.0, [0.0, 1.0, 20.0], "scipy", {}),
    ("binomial", 20.0, 1.0, [0.0, 19.0, 20.0], "scipy", {}),
    ("binomial", 1000.0, 0.3, [0.0, 280.0, 300.0, 1000.0], "mpmath", {}),
    ("negbinomial", 0.5, 0.3, [0.0, 1.0, 9.0, 2.5, -1.0], "scipy", {}),
    ("negbinomial", 12.0, 0.4, [0.0, 18.0, 60.0], "scipy", {}),
    ("negbinomial", 3.0, 1.0, [0.0, 1.0], "scipy", {0.0: 0.0, 1.0: -np.inf}),
    ("negbinomial", 400.0, 0.5, [300.0, 400.0, 520.0], "mpmath", {}),
]


@pytest.mark.parametrize("case", LOGPDF_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_logpdf_matches_scipy(case):
    """Non-finite values agree exactly (-Inf outside the support and at the edges, +Inf at the
    poles of Gamma / Chisq / Beta). Finite ones are within 8 ulp of the summed magnitudes of the
    formula's terms (the bound of test_families.py's decimal test): each term is rounded at its own
    scale, wsmc_lgamma is good to 1.6 ulp of its value and wsmc_log to under 1, and at most three
    lgamma and three log terms enter a formula."""
    fam, a, b, xs, ref, given = case
    mp.mp.dps = 50
    got = observe_at(KERNEL[fam](a, b), xs)
    d = SCIPY[fam](a, b)
    with np.errstate(all="ignore"):
        want = np.array(d.logpmf(xs) if fam in DISCRETE else d.logpdf(xs), float)
    for k, x in enumerate(xs):
        if x in given:
            want[k] = given[x]
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), (got, want)
    assert np.array_equal(got[~finite], want[~finite]), (got, want)
    for x, g, w, f in zip(xs, got, want, finite):
        if not f:
            continue
        tol = 8 * np.spacing(max(MAG[fam](a, b, x), 1e-300))
        if ref == "mpmath":
            assert abs(mp.mpf(float(g)) - MPF[fam](a, b, x)) <= tol, (fam, a, b, x, g)
        else:
            assert abs(g - w) <= tol, (fam, a, b, x, g, w)


def test_logpdf_at_extreme_arguments():
    """Gamma / Chisq at x = +Inf are -Inf for every shape (not (alpha - 1) Inf - Inf); TDist where
    x^2 passes the largest double stays finite: against the formula in mpmath, 8 ulp of its
    terms' summed magnitudes as above."""
    for kern in (wsmc.Gamma(0.3, 2.0), wsmc.Gamma(1.0, 2.0), wsmc.Gamma(7.5, 0.5), wsmc.Chisq(1.0), wsmc.Chisq(9.0),
                 wsmc.InverseGamma(2.0, 1.0)):
        assert observe_at(kern, [np.inf])[0] == -np.inf
    mp.mp.dps = 50
    for nu in (1.5, 30.0):
        xs = [1e154, 1.4e154, 1e160, -1e200, 1e308]
        got = observe_at(wsmc.TDist(nu), xs)
        for x, g in zip(xs, got):
            want = MPF["tdist"](nu, 1.0, x)
            mag = _lg((nu + 1) / 2) + _lg(nu / 2) + 0.5 * _log(nu * np.pi) + abs(float((nu + 1) / 2 * mp.log1p(_M(x) ** 2 / nu)))
            assert np.isfinite(g) and abs(mp.mpf(float(g)) - want) <= 8 * np.spacing(mag), (nu, x, g)


# ---- draws ------------------------------------------------------------------------------
# one case per sampler branch
DRAW_CASES = [
    ("gamma", 0.3, 2.0), ("gamma", 1.0, 2.0), ("gamma", 7.5, 0.5),
    ("invgamma", 3.0, 2.0), ("chisq", 5.0, 1.0),
    ("beta", 0.5, 0.5), ("beta", 2.0, 5.0),
    ("tdist", 1.5, 1.0), ("tdist", 30.0, 1.0),
    ("poisson", 0.7, 1.0), ("poisson", 9.99, 1.0), ("poisson", 10.0, 1.0), ("poisson", 250.0, 1.0),
    ("binomial", 20.0, 0.1), ("binomial", 40.0, 0.5), ("binomial", 1000.0, 0.3), ("binomial", 1000.0, 0.97),
    ("negbinomial", 0.5, 0.3), ("negbinomial", 12.0, 0.4),
]
SUPPORT = {
    "gamma": lambda x, a, b: x > 0, "invgamma": lambda x, a, b: x > 0, "chisq": lambda x, a, b: x > 0,
    "beta": lambda x, a, b: (x >= 0) & (x <= 1), "tdist": lambda x, a, b: np.isfinite(x),
    "poisson": lambda x, a, b: x >= 0, "binomial": lambda x, a, b: (x >= 0) & (x <= a),
    "negbinomial": lambda x, a, b: x >= 0,
}


@pytest.mark.parametrize("case", DRAW_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_draws_follow_the_distribution(case):
    fam, a, b = case
    N = 40_000
    o = Oracle(N, seed=7)
    cx = o.col_create("x")
    o.sample(cx, KERNEL[fam](a, b).dist(models.resolver(o)))
    x = o.col_download(cx)
    ref = SCIPY[fam](a, b)
    assert np.all(np.isfinite(x))
    assert np.all(SUPPORT[fam](x, a, b))
    if fam in DISCRETE:
        assert np.all(x == np.floor(x))
        m, s = ref.mean(), ref.std()
        ks = np.arange(max(0, int(m - 5 * s)), int(m + 5 * s) + 2)
        freq = np.array([(x == k).mean() for k in ks])
        np.testing.assert_allclose(freq, ref.pmf(ks), atol=4.5 * np.sqrt(0.25 / N))
        # the frequencies bound each pmf value loosely where it is small: the mean as well, to
        # 4.5 standard errors
        assert abs(x.mean() - m) <= 4.5 * s / np.sqrt(N)
    else:
        d, p = stats.kstest(x, ref.cdf)
        assert p > 1e-4, (d, p)


def test_beta_draws_when_both_gamma_stages_underflow():
    """Beta(0.002, 0.002): each Gamma stage underflows to 0 in about a fifth of the draws, both in
    about 5 %. Whenever a stage is below 2^-1000 the ratio is taken from the logarithms: it stays
    a number in [0, 1] (never 0 / 0) and keeps the right distribution where one stage is 0 and
    the other merely tiny (the CDF at thresholds down to 1e-200, frequencies as for the pmfs)."""
    N = 40_000
    o = Oracle(N, seed=7)
    cx = o.col_create("x")
    o.sample(cx, wsmc.Beta(0.002, 0.002).dist(models.resolver(o)))
    x = o.col_download(cx)
    assert np.all(np.isfinite(x)) and np.all((x >= 0) & (x <= 1))
    ref = stats.beta(0.002, 0.002)
    ts = np.array([1e-200, 1e-50, 1e-3, 0.5, 1 - 1e-3, 1 - 1e-12])
    freq = np.array([(x <= t).mean() for t in ts])
    np.testing.assert_allclose(freq, ref.cdf(ts), atol=4.5 * np.sqrt(0.25 / N))


def test_parameters_from_a_column_straddle_the_sampler_thresholds():
    """lambda alternating across the inversion / PTRS threshold within consecutive particles:
    each particle's draw is that of its own parameter (a function of (seed, op, idx))"""
    N = 40_000
    lam = np.tile([0.5, 9.99, 10.0, 300.0], N // 4)
    o = Oracle(N, seed=7)
    R = models.resolver(o)
    cl, cx = o.col_create("lam"), o.col_create("x")
    o.col_upload(cl, lam)
    o.sample(cx, wsmc.Poisson(Col("lam")).dist(R))
    x = o.col_download(cx)
    for l in (0.5, 9.99, 10.0, 300.0):
        xs = x[lam == l]
        assert abs(xs.mean() - l) <= 4.5 * np.sqrt(l / len(xs))
        assert abs(xs.var() - l) <= 0.1 * l


# ---- conjugate pins ---------------------------------------------------------------------
def _is_stats(ctx, col):
    lw = ctx.weights_download()
    w = np.exp(lw - lw.max())
    W = w / w.sum()
    ess = 1.0 / np.sum(W * W)
    v = ctx.col_download(col)
    mean = float(np.sum(W * v))
    se_mean = float(np.sqrt(np.sum(W * W * (v - mean) ** 2)))
    # the evidence is a plain average of N weights: relative variance 1/ESS - 1/N
    se_logz = float(np.sqrt(max(1.0 / ess - 1.0 / len(w), 0.0)))
    return mean, se_mean, se_logz


@pytest.mark.parametrize("backend", BACKENDS)
def test_gamma_poisson_conjugacy(backend):
    """lambda ~ Gamma(a, theta); y_1..y_5 => Poisson(lambda): the evidence is a product of
    negative-binomial predictives, the posterior Gamma(a + sum y, 1 / (1/theta + n)). Tolerance:
    5 Monte-Carlo standard errors, from the run's own weights (ESS)."""
    N, a, theta = 20_000, 3.0, 1.5
    ys = [2.0, 5.0, 3.0, 4.0, 1.0]
    ctx = make_ctx(backend, N, seed=11)
    R = models.resolver(ctx)
    cl = ctx.col_create("lam")
    ctx.sample(cl, wsmc.Gamma(a, theta).dist(R))
    for y in ys:
        ctx.observe(wsmc.Poisson(Col("lam")).dist(R), models._const([y]))
    ak, bk, ev = a, 1.0 / theta, 0.0
    for y in ys:
        ev += stats.nbinom(ak, bk / (bk + 1.0)).logpmf(y)
        ak, bk = ak + y, bk + 1.0
    mean, se_mean, se_logz = _is_stats(ctx, cl)
    assert abs(ctx.log_evidence() - ev) <= 5 * se_logz, (ctx.log_evidence(), ev, se_logz)
    assert abs(mean - ak / bk) <= 5 * se_mean, (mean, ak / bk, se_mean)


@pytest.mark.parametrize("backend", BACKENDS)
def test_beta_binomial_conjugacy(backend):
    """p ~ Beta(a, b); k => Binomial(n, p): log evidence = log C(n, k) + lbeta(a + k, b + n - k)
    - lbeta(a, b). Tolerance as above."""
    N, a, b, n, k = 20_000, 2.0, 3.0, 30.0, 11.0
    ctx = make_ctx(backend, N, seed=12)
    R = models.resolver(ctx)
    cp = ctx.col_create("p")
    ctx.sample(cp, wsmc.Beta(a, b).dist(R))
    ctx.observe(wsmc.Binomial(n, Col("p")).dist(R), models._const([k]))
    ev = (special.gammaln(n + 1) - special.gammaln(k + 1) - special.gammaln(n - k + 1)
          + special.betaln(a + k, b + n - k) - special.betaln(a, b))
    mean, se_mean, se_logz = _is_stats(ctx, cp)
    assert abs(ctx.log_evidence() - ev) <= 5 * se_logz, (ctx.log_evidence(), ev, se_logz)
    assert abs(mean - (a + k) / (a + b + n)) <= 5 * se_mean


# ---- family numbers ---------------------------------------------------------------------
def test_family_numbers():
    header = (REPO / "include" / "wsmc.h").read_text()
    nums = {m.group(1): int(m.group(2)) for m in re.finditer(r"WSMC_FAM_(\w+)\s*=\s*(\d+)", header)}
    names = ["GAMMA", "INVERSEGAMMA", "CHISQ", "BETA", "TDIST", "POISSON", "BINOMIAL", "NEGBINOMIAL"]
    assert [nums[n] for n in names] == list(range(16, 24))
    assert [getattr(abi, "FAM_" + n) for n in names] == list(range(16, 24))
    assert 15 not in nums.values()
    o = Oracle(64, seed=2)
    R = models.resolver(o)
    for fam in range(16, 24):   # the oracle path takes every one of them
        d = wsmc.Gamma(2.0, 0.5).dist(R)
        d.family = fam
        c = o.col_create(f"x{fam}")
        o.sample(c, d)
        o.observe(d, Col(f"x{fam}").operand(R))
    assert np.all(np.isfinite(o.weights_download()))

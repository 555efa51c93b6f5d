"""The shared math at its edges on the CPU oracle (tests/mathedge.py's corpus): every expression
operator against mpmath at 50 digits or against its exact expected value, every scalar family's
log-density over the cross of its parameters' and its support's edges, the samplers at their branch
thresholds and valid extremes, and the corpus' own claims (the neighbours it names, the comparer).

The bounds are the project's own statements or are derived, none is fitted to what the oracle gives:
    log      0.75 ulp (tests/test_oracle_math.py test_log_table_accuracy_against_decimal)
    exp      0.55 ulp for |x| < 512, 1 ulp beyond; one unit of 5e-324 where the result is subnormal
    sqrt     the correctly rounded value
    sin cos  1 ulp (the fdlibm kernels' stated bound)
    log1p    2 ulp (the log's 0.75 and the roundings of Goldberg's quotient and product)
    pow      a non-integer exponent: relative 2^-53 (2 + 2 |b ln a|); the special values: Julia's table
    powi     1 ulp for |n| <= 1024 where the result is normal, parity beyond
Two cases miss what was asked of powi and are recorded in DESIGN.md section 6 (mathedge._ref_powi
holds them to what is derived for them): x^-2, Base.literal_pow's inv(x)^2 (1.12 ulp at 10.0^-2),
and the sign of a zero that Base.pow_body reaches from a negative zero.
The device is held to the oracle, bit for bit, in tests/test_gpu_math_edges.py."""
import math

import mpmath as mp
import numpy as np
import pytest

import mathedge as me
import test_gamma_families as tgf
from mathedge import INF, NAN
from oracle import Oracle
from test_families import LOGPDF_ATOL, LOGPDF_RTOL
from wsmc import abi


# ---- the operators -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(me.OPERATORS))
def test_operator_against_its_reference(name):
    """every point of the entry, in both arrangements and under every constant the instruction
    carries, against its reference: bit for bit where the expected value is exact (the special
    values, the arithmetic, the comparisons, min / max by Julia's rules), within the bound above
    where mpmath gives it"""
    e = me.OPERATORS[name]
    values = me.oracle_operator(name)
    bad, worst = me.check_operator(e, values)
    print(name, "worst error per constant:", {e.label(e.variants[v]): round(x, 3) for v, x in worst.items()})
    shown = [(w, e.label(e.variants[v]), [float(a[i]) for a in e.args], why) for w, v, i, why in bad[:8]]
    assert not bad, (len(bad), shown)
    for v in range(len(e.variants)):   # the ordinary values are the same numbers in both arrangements
        b, m = values[("built", v)][e.n:], values[("mixed", v)][1::2]
        assert me.first_difference(name, "ordinary", (), m, b) is None


def test_every_operator_has_an_entry():
    ops = {v for k, v in vars(abi).items() if k.startswith("X_") and isinstance(v, int)}
    assert ops == {e.op for e in me.OPERATORS.values()}
    for e in me.OPERATORS.values():
        assert 20 <= e.n and 2 * e.n <= 4200, (e.name, e.n)
        assert len({len(a) for a in e.args}) == 1
    assert any(2 * e.n % 64 for e in me.OPERATORS.values())   # nothing is padded to the wave


def test_domain_masks():
    """a finite reference exists exactly where the operator's real value is finite"""
    e = me.OPERATORS["log"]
    x = e.args[0]
    assert np.array_equal(e.domain(), (x > 0) & np.isfinite(x) & (x != 1.0))
    e = me.OPERATORS["sqrt"]
    assert np.array_equal(e.domain(), (e.args[0] > 0) & np.isfinite(e.args[0]))
    e = me.OPERATORS["sin"]
    assert np.array_equal(e.domain(), np.isfinite(e.args[0]) & (e.args[0] != 0.0))
    assert not me.OPERATORS["min"].domain().any()


def _at(e, *point):
    hit = np.ones(e.n, bool)
    for a, p in zip(e.args, point):
        hit &= (a.view(np.uint64) == np.float64(p).view(np.uint64)) | (np.isnan(a) & math.isnan(p))
    assert hit.any(), (e.name, point)
    return int(np.flatnonzero(hit)[0])


def _same(got, want):
    return (math.isnan(got) and math.isnan(want)) or me.bits(got) == me.bits(want)


# Base.^(::Float64, ::Float64), as include/wsmc_math.h's comment describes it: (x, y, x^y)
JULIA_POW = [
    (1.0, NAN, 1.0), (1.0, INF, 1.0), (NAN, 0.0, 1.0), (NAN, -0.0, 1.0), (NAN, 1.0, NAN), (2.0, NAN, NAN),
    (-INF, 0.5, NAN), (-2.0, 0.5, NAN), (-2.0, 0.1, NAN), (-0.0, 0.5, 0.0), (-0.0, -0.5, INF), (0.0, 0.5, 0.0),
    (0.0, -1.0, INF), (-0.0, -1.0, -INF), (-0.0, 3.0, -0.0), (-0.0, 2.0, 0.0), (0.0, INF, 0.0), (0.0, -INF, INF),
    (INF, 0.5, INF), (INF, -0.5, 0.0), (INF, -INF, 0.0), (INF, INF, INF), (-INF, 3.0, -INF), (-INF, 2.0, INF),
    (-INF, -2.0, 0.0), (-INF, -1.0, -0.0), (-INF, INF, INF), (-INF, -INF, 0.0),
    (-2.0, 1e19, INF), (-2.0, -1e19, 0.0), (-2.0, INF, INF), (-2.0, -INF, 0.0), (-0.5, 2.0 ** 53, 0.0), (-0.5, INF, 0.0),
    (-0.5, -INF, INF), (2.0, INF, INF), (0.5, INF, 0.0), (2.0, -INF, 0.0), (0.5, -INF, INF),
    (-1.0, INF, 1.0), (-1.0, -INF, 1.0), (-1.0, 2.0 ** 53 + 2.0, 1.0), (-1.0, 1e18 + 128.0, 1.0), (-1.0, 9.3e18, 1.0),
    (-1.0, 3.0, -1.0), (-1.0, 0.5, NAN), (10.0, 2.0, 100.0), (10.0, -2.0, 0.010000000000000002),
    (10.0, 0.0, 1.0), (-INF, 0.0, 1.0), (0.0, 0.0, 1.0), (0.5, -1.0, 2.0), (2.0, 7.0, 128.0), (1e300, 2.0, INF),
    (5e-324, 2.0, 0.0), (5e-324, -1.0, INF),
]
# Base.min / Base.max: (a, b, min, max)
JULIA_MINMAX = [
    (-0.0, 0.0, -0.0, 0.0), (0.0, -0.0, -0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (-0.0, -0.0, -0.0, -0.0),
    (NAN, 1.0, NAN, NAN), (1.0, NAN, NAN, NAN), (NAN, INF, NAN, NAN), (-INF, NAN, NAN, NAN), (NAN, NAN, NAN, NAN),
    (-INF, INF, -INF, INF), (INF, -INF, -INF, INF), (INF, INF, INF, INF), (1.0, -1.0, -1.0, 1.0),
    (5e-324, 0.0, 0.0, 5e-324), (-5e-324, -0.0, -5e-324, -0.0), (me.DBL_MAX, INF, me.DBL_MAX, INF),
]


def test_pow_special_values_are_julias():
    e, values = me.OPERATORS["pow"], me.oracle_operator("pow")[("built", 0)]
    for a, b, want in JULIA_POW:
        i = _at(e, a, b)
        assert _same(float(values[i]), want), (a, b, float(values[i]), want)
        assert me.judge(e.refs()[i], want)[0] is None, (a, b, want)   # the table and the reference agree


def test_min_max_follow_julia():
    for name, k in (("min", 2), ("max", 3)):
        e, values = me.OPERATORS[name], me.oracle_operator(name)[("built", 0)]
        for row in JULIA_MINMAX:
            i = _at(e, row[0], row[1])
            assert _same(float(values[i]), row[k]), (name, row, float(values[i]))


def test_comparisons_and_logic_on_nan_and_signed_zeros():
    def val(name, *p):
        e = me.OPERATORS[name]
        return float(me.oracle_operator(name)[("built", 0)][_at(e, *p)])
    for name, nan_any, zeros in (("lt", 0.0, 0.0), ("le", 0.0, 1.0), ("gt", 0.0, 0.0), ("ge", 0.0, 1.0), ("eq", 0.0, 1.0),
                                 ("ne", 1.0, 0.0)):
        assert val(name, NAN, 1.0) == val(name, 1.0, NAN) == val(name, NAN, NAN) == nan_any, name
        assert val(name, -0.0, 0.0) == val(name, 0.0, -0.0) == zeros, name
    # a NaN is not zero, so it is true; -0.0 is zero
    assert val("and", NAN, 1.0) == 1.0 and val("and", -0.0, 1.0) == 0.0 and val("or", -0.0, 0.0) == 0.0
    assert val("or", NAN, 0.0) == 1.0 and val("not", NAN) == 0.0 and val("not", -0.0) == 1.0
    assert val("ifelse", NAN, 1.0, -1.0) == 1.0 and val("ifelse", -0.0, 1.0, -1.0) == -1.0
    assert me.bits(val("neg", 0.0)) == me.bits(-0.0) and me.bits(val("abs", -0.0)) == me.bits(0.0)
    assert me.bits(val("sub", 0.0, 0.0)) == me.bits(0.0) and me.bits(val("add", -0.0, -0.0)) == me.bits(-0.0)
    assert math.isnan(val("mul", 0.0, INF)) and math.isnan(val("div", 0.0, -0.0)) and val("div", 1.0, -0.0) == -INF
    assert val("div", 5e-324, me.DBL_MAX) == 0.0 and val("mul", 5e-324, me.DBL_MAX) == 5e-324 * me.DBL_MAX > 0.0


# ---- the corpus' own claims ------------------------------------------------------------------------------
NAMED = {
    "exp": [512.0, -512.0, 709.782712893384, -708.3964185322641, -745.1332191019411, 2.0 ** -28, 0.5 * me.LN2,
            64 * me.LN2 / 128.0, 1.0],
    "log": [1.0],
    "log1p": [-1.0, -0.5, 2.0 ** -53],
    "sqrt": [4.0, 9.0, 2.0 ** 52],
    "sin": [math.pi / 4.0, 16 * math.pi / 4.0, me.PIO2_LARGE, -me.PIO2_LARGE],
    "cos": [math.pi / 2.0, 7 * math.pi / 4.0, me.PIO2_LARGE],
    "neg": [1.0, -1.0],
}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_entries_hold_the_neighbours_they_claim(name):
    x = set(me.OPERATORS[name].args[0].view(np.uint64).tolist())
    for p in NAMED[name]:
        lo1, hi1 = np.nextafter(p, -INF), np.nextafter(p, INF)
        for v in (p, lo1, hi1, np.nextafter(lo1, -INF), np.nextafter(hi1, INF)):
            assert me.bits(v) in x, (name, p, float(v))
    assert me.bits(hi1) != me.bits(p) and float(hi1) > p > float(lo1)


def test_named_points_of_the_rest():
    x = me.OPERATORS["log"].args[0]
    for k in range(1, 5):
        assert 1.0 + k * 2.0 ** -52 in x and 1.0 - k * 2.0 ** -53 in x
    assert len(me.log_table_edges()) == 384 and set(me.log_table_edges()) <= set(x.tolist())
    assert {5e-324, me.SUB_MAX, me.TINY, me.DBL_MAX, 2.0 ** -1074, 2.0 ** 1023} <= set(x.tolist())
    for name in me.UNARY:
        if name not in ("const", "powi"):
            a = me.OPERATORS[name].args[0]
            assert {5e-324, -5e-324, me.SUB_MAX, me.TINY, me.DBL_MAX, -me.DBL_MAX, INF, -INF} <= set(a.tolist()), name
            assert np.isnan(a).any() and np.signbit(a[a == 0.0]).any() and not np.signbit(a[a == 0.0]).all(), name
    t = me.OPERATORS["sin"].args[0]
    assert {1e22, 2.0 ** 1023, 6381956970095103.0 * 2.0 ** 797} <= set(t.tolist())
    assert me.PIO2_LARGE == 823549.0   # what the header reads today: the corpus follows it when it moves
    assert set(me.POWI_N) >= {0, 1, -1, 2, -2, 3, -3, 4, -4, 7, -5, 63, 64, -64, 1023, -1074}
    b = set(me.OPERATORS["pow"].args[1].tolist())
    assert {2.0 ** 53, 2.0 ** 53 + 2.0, 1e18 + 128.0, 1e19, -1e19, 9.3e18, 1e-300, 0.1} <= b


def test_arrangements():
    for e in list(me.OPERATORS.values())[:8] + [me.OPERATORS["pow"], me.OPERATORS["ifelse"]]:
        ins = me.operator_inputs(e)
        at = me.place(e.n, e.index, "mixed")
        assert sorted(at.tolist()) == list(range(0, 2 * e.n, 2))
        assert not np.array_equal(at, 2 * np.arange(e.n))   # a permutation, not the built order
        for k in range(e.arity):
            b, m = ins["built"][k], ins["mixed"][k]
            assert len(b) == len(m) == 2 * e.n
            assert me.first_difference(e.name, "points", (), m[at], e.args[k]) is None
            assert me.first_difference(e.name, "ordinary", (), m[1::2], b[e.n:]) is None
            assert np.isfinite(b[e.n:]).all()
        again = me.operator_inputs(e)   # fixed: the same arrays at every call
        assert all(np.array_equal(x, y, equal_nan=True) for w in ins for x, y in zip(ins[w], again[w]))


def test_comparer_reports_a_planted_difference():
    """two arrays that differ by one ulp at one position: the operator, the arrangement, the index,
    the input value and both bit patterns"""
    e = me.OPERATORS["exp"]
    want = me.oracle_operator("exp")[("mixed", 0)]
    x = me.operator_inputs(e)["mixed"]
    assert me.first_difference("exp", "mixed", x, want.copy(), want) is None
    i = int(me.place(e.n, e.index, "mixed")[_at(e, 512.0)])
    got = want.copy()
    got[i] = np.nextafter(got[i], INF)
    d = me.first_difference("exp", "mixed", x, got, want)
    assert d is not None and d.startswith("exp [mixed]: 1 of %d differ, first at index %d:" % (len(want), i)), d
    assert "input 512.0 (0x4080000000000000)" in d and f"0x{me.bits(got[i]):016x}" in d and f"0x{me.bits(want[i]):016x}" in d
    # -0.0 is not 0.0; a NaN is any NaN
    assert me.first_difference("neg", "built", (np.zeros(1),), np.array([-0.0]), np.array([0.0])) is not None
    other_nan = np.array([me.from_bits(0xfff8000000000000)])
    assert me.first_difference("log", "built", (np.zeros(1),), other_nan, np.array([NAN])) is None


def test_command_line_replays_an_entry(capsys):
    assert me.main(["--op", "pow", "--backend", "oracle"]) == 0
    assert "pow: 396 points, 0 outside" in capsys.readouterr().out


def test_the_smoothing_definition_copies_a_negative_zero():
    """What tests/test_gpu_math_edges.py found on the device: the persistent workgroup stores a
    trace point's columns as they are, and SSM.statements(smooth=True), the definition, copied them
    through the affine Assign 0.0 + 1.0 x, which turns a -0.0 into 0.0. include/wsmc.h says
    "copied": the definition now copies bit for bit. Every operator entry's paths are the operator's
    own values (threshold 0.0: no Resample moves a particle)."""
    for name in ("neg", "col", "mul", "sin"):
        e = me.OPERATORS[name]
        want = me.oracle_operator(name)[("built", 0)]
        assert (np.signbit(want[:e.n]) & (want[:e.n] == 0.0)).any(), name   # the entry does produce a -0.0
        for variants, lo, hi in me.ssm_runs(e):
            case = me.ssm_case(e, variants, lo, hi)
            o = Oracle(5, seed=3)
            sm = case.ssm.statements(o, case.data, ess_perc_min=0.0, T=hi - lo, smooth=True)[-1]
            o.close()
            d = me.first_difference(name, f"paths of steps {lo}:{hi}", (), np.asarray(sm.paths["c0"]),
                                    np.repeat(want[lo:hi, None], 5, axis=1))
            assert d is None, d


# ---- the log-densities ---------------------------------------------------------------------------------
_M = mp.mpf


def _z(m, s, x):
    return (_M(x) - _M(m)) / _M(s)


def _normal(m, s, x):
    return -_z(m, s, x) ** 2 / 2 - mp.log(2 * mp.pi) / 2 - mp.log(s)


# the textbook formulas in mpmath (first parameter, second parameter, observed value); the log-Gamma
# families' are tests/test_gamma_families.py's MPF
FORMULA = {
    "normal": _normal,
    "halfnormal": lambda m, s, x: _normal(0, s, x) + mp.log(2),
    "uniform": lambda m, s, x: -mp.log(_M(2.0) - _M(0.25)),
    "bernoulli": lambda p, s, x: mp.log(p) if x == 1.0 else mp.log1p(-_M(p)),
    "bernoulli_logit": lambda m, s, x: -mp.log1p(mp.exp(-_M(m) if x == 1.0 else _M(m))),
    "exponential": lambda m, s, x: -mp.log(s) - _M(x) / s,
    "lognormal": lambda m, s, x: _normal(m, s, mp.log(x)) - mp.log(x),
    "laplace": lambda m, s, x: -(abs(_M(x) - m) / s + mp.log(2 * _M(s))),
    "cauchy": lambda m, s, x: -(mp.log1p(_z(m, s, x) ** 2) + mp.log(mp.pi) + mp.log(s)),
    "logistic": lambda m, s, x: -abs(_z(m, s, x)) - 2 * mp.log1p(mp.exp(-abs(_z(m, s, x)))) - mp.log(s),
    "gumbel": lambda m, s, x: -(_z(m, s, x) + mp.exp(-_z(m, s, x)) + mp.log(s)),
    "rayleigh": lambda m, s, x: mp.log(_M(x) / _M(s) ** 2) - _M(x) ** 2 / (2 * _M(s) ** 2),
    "geometric": lambda p, s, x: mp.log(p) + _M(x) * mp.log1p(-_M(p)),
}


def _pole(e, a, b, x):
    """where the density truly is +Inf (parameters inside the domain): Gamma (Chisq) at 0 below a
    shape of 1 (2 degrees), Beta at 0 below a first shape of 1 and at 1 below a second shape of 1"""
    if e.fam == abi.FAM_GAMMA:
        return (x == 0.0) & (a < 1.0)
    if e.fam == abi.FAM_CHISQ:
        return (x == 0.0) & (a < 2.0)
    if e.fam == abi.FAM_BETA:
        return ((x == 0.0) & (a < 1.0)) | ((x == 1.0) & (b < 1.0))
    return np.zeros(len(x), bool)


def _plus_inf_outside_the_domain(e, a, b, x):
    """The points with a parameter outside the family's domain (the reference refuses those when the
    distribution is built; the library evaluates the formula) at which the value is +Inf, every one
    of them (DESIGN.md section 6 has the same list):
      Gamma        at x = 0 with a shape below 1, whatever the scale is (NaN, 0, negative, Inf: the
                   branch at x = 0 returns before it reads the scale) and a shape <= 0 included; and
                   at x = 0 with a shape of exactly 1 and a scale of 0 (-log 0)
      Chisq        at x = 0 with nu <= 0 (the same branch, the shape nu / 2)
      Bernoulli    p = +Inf at x = 1 (log p)
      Binomial     p = +Inf at x = n, n a positive integer (x log p)
      NegBinomial  p = +Inf at x = 0 with 0 < r < Inf (r log p)
    and no other family at any point."""
    if e.fam == abi.FAM_GAMMA:
        return (x == 0.0) & ((a < 1.0) | ((a == 1.0) & (b == 0.0)))
    if e.fam == abi.FAM_CHISQ:
        return (x == 0.0) & (a < 2.0)
    if e.fam == abi.FAM_BERNOULLI:
        return (x == 1.0) & (a == INF)
    if e.fam == abi.FAM_BINOMIAL:
        return (b == INF) & (x == a) & (x > 0.0) & np.isfinite(x) & (x == np.floor(x))
    if e.fam == abi.FAM_NEGBINOMIAL:
        return (b == INF) & (x == 0.0) & (a > 0.0) & (a < INF)
    return np.zeros(len(x), bool)


@pytest.mark.parametrize("name", [n for n in me.LOGPDFS if n != "lgamma"])
def test_logpdf_corpus(name):
    """Over the whole corpus a log-density is finite, -Inf or NaN, and +Inf at exactly two sets of
    points: under parameters the family accepts, the true poles _pole names; under a parameter
    outside the domain, the points _plus_inf_outside_the_domain enumerates (recorded, not endorsed:
    a NaN scale of a Gamma among them) and no other. The interior points agree with the formula in mpmath within the tolerances of
    tests/test_families.py (rtol, atol) and tests/test_gamma_families.py (8 ulp of the summed
    magnitudes of the formula's terms). The Moves' fold reads the same term back bit for bit, and
    the two arrangements hold the same values."""
    mp.mp.dps = 50
    e = me.LOGPDFS[name]
    res = {}
    for w in me.ARRANGEMENTS:
        o = Oracle(2 * e.n, seed=1)
        res[w], score = me.run_logpdf(o, e, w)
        o.close()
        assert me.first_difference(name, w + " score(depth)", e.inputs()[w], score, res[w]) is None
    lw = res["built"][:e.n]
    assert me.first_difference(name, "mixed", (e.a, e.b, e.x), res["mixed"][me.place(e.n, 200 + e.index, "mixed")], lw) is None
    assert me.first_difference(name, "ordinary", (), res["mixed"][1::2], res["built"][e.n:]) is None
    assert np.isfinite(res["built"][e.n:]).all()   # the ordinary values are interior ones
    plus = np.isposinf(lw)
    want = np.where(e.valid, _pole(e, e.a, e.b, e.x), _plus_inf_outside_the_domain(e, e.a, e.b, e.x))
    assert np.array_equal(plus, want), [(e.a[i], e.b[i], e.x[i], lw[i]) for i in np.flatnonzero(plus != want)[:6]]
    assert (~e.valid).any() or name == "uniform"   # every entry does hold invalid parameters
    assert e.interior.sum() >= 4 and not (e.interior & ~e.valid).any()
    for i in np.flatnonzero(e.interior):
        a, b, x, g = float(e.a[i]), float(e.b[i]), float(e.x[i]), float(lw[i])
        assert math.isfinite(g), (name, a, b, x, g)
        if name in tgf.MPF:
            tol = 8 * np.spacing(max(tgf.MAG[name](a, b, x), 1e-300))
            assert abs(_M(g) - tgf.MPF[name](a, b, x)) <= tol, (name, a, b, x, g)
        else:
            want = FORMULA[name](a, b, x)
            assert abs(_M(g) - want) <= LOGPDF_ATOL + LOGPDF_RTOL * abs(want), (name, a, b, x, g, float(want))


def test_lgamma_through_the_gamma_density():
    """Gamma(a, 1) observed at 1 is -1 - lgamma(a): against mpmath.loggamma within the bound
    test_lgamma_against_mpmath asserts (twice LGAMMA_ABS inside [0.5, 3], twice LGAMMA_ULP ulp of
    lgamma outside) and the half ulp of the one rounding that adds the -1; the edges exactly"""
    mp.mp.dps = 50
    e = me.LOGPDFS["lgamma"]
    o = Oracle(2 * e.n, seed=1)
    lw = me.run_logpdf(o, e, "built", score=False)[0][:e.n]
    o.close()
    for h in tgf.PIECES + [1.0, 2.0]:
        for v in me.nb(h, 2):
            assert v in e.a, v
    worst = 0.0
    for a, g in zip(e.a.tolist(), lw.tolist()):
        if a == 0.0:
            assert g == -INF
        elif not (0.0 < a < INF):
            assert math.isnan(g), (a, g)
        else:
            lg = mp.loggamma(_M(a))
            want = -1 - lg
            inner = 2 * tgf.LGAMMA_ABS if 0.5 <= a <= 3.0 else 2 * tgf.LGAMMA_ULP * float(np.spacing(abs(float(lg))))
            tol = inner + 0.5 * float(np.spacing(abs(float(want))))
            worst = max(worst, float(abs(_M(g) - want) / tol))
            assert abs(_M(g) - want) <= tol, (a, g, float(want), tol)
    print("lgamma entry: worst error / bound", worst)
    assert lw[list(e.a).index(1.0)] == -1.0 and lw[list(e.a).index(2.0)] == -1.0


# ---- the draws -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(me.DRAWS))
def test_draws_stay_in_the_support(name):
    """parameters at every sampler threshold (read from include/wsmc_terms.h) with their neighbours
    and at the valid extremes: every draw lies in the family's support, and its own log-density
    there is neither NaN nor -Inf"""
    e = me.DRAWS[name]
    for w in me.ARRANGEMENTS:
        o = Oracle(2 * e.n, seed=1)
        x, lw = me.run_draw(o, e, w)
        o.close()
        a, b = e.inputs()[w]
        ok = e.in_support(a, b, x)
        assert ok.all(), (name, w, [(a[i], b[i], x[i]) for i in np.flatnonzero(~ok)[:6]])
        bad = np.isnan(lw) | np.isneginf(lw)
        assert not bad.any(), (name, w, [(a[i], b[i], x[i], lw[i]) for i in np.flatnonzero(bad)[:6]])


def test_draw_corpus_sits_on_the_thresholds():
    assert (me.GAMMA_SMALL, me.POISSON_PTRS, me.BINOMIAL_BTRS, me.BINOMIAL_FLIP) == (1.0, 10.0, 10.0, 0.5)
    assert (me.GAMMA_ROUNDS, me.INV_STEPS, me.TRS_ROUNDS) == (24, 96, 60)   # the caps the corpus' comments quote
    for name, t in (("gamma", me.GAMMA_SMALL), ("invgamma", me.GAMMA_SMALL), ("beta", me.GAMMA_SMALL),
                    ("negbinomial", me.GAMMA_SMALL), ("poisson", me.POISSON_PTRS), ("chisq", 2 * me.GAMMA_SMALL),
                    ("tdist", 2 * me.GAMMA_SMALL)):
        a = set(me.DRAWS[name].a.tolist())
        assert {t, float(np.nextafter(t, -INF)), float(np.nextafter(t, INF))} <= a, name
    e = me.DRAWS["binomial"]
    nq = e.a * np.minimum(e.b, 1.0 - e.b)
    assert (nq == me.BINOMIAL_BTRS).any() and ((nq < 10.0) & (nq > 9.999999)).any()
    assert {me.BINOMIAL_FLIP, float(np.nextafter(0.5, 1.0)), float(np.nextafter(0.5, 0.0)), 5e-324, me.ONE_M} <= set(e.b.tolist())
    assert 2.0 ** 31 in e.a and 1e6 in me.DRAWS["gamma"].a and 1e-300 in me.DRAWS["gamma"].a and 1e-15 in me.DRAWS["gamma"].b

"""Directed inputs for the shared math (include/wsmc_math.h, include/wsmc_terms.h): the corpus.

TEST INFRASTRUCTURE, the companion of tests/progfuzz.py and tests/ssmfuzz.py for the arguments of
the math itself. Nothing here is sampled for coverage: every entry is a list of named points with
their `np.nextafter` neighbours, and the one RNG (`default_rng([SEED, k])`) only draws the ordinary
values an arrangement interleaves with them and the arrangement's fixed permutation.

    OPERATORS   one entry per expression operator of wsmc/abi.py's X_* list: the argument arrays, an
                independent reference per point (`Entry.ref`: an exact expected value, or an mpmath
                value with the bound it is held to; `Entry.domain()` is the mask of the latter)
    LOGPDFS     one entry per scalar family (ssmfuzz.SCALAR_FAMILIES with Normal, HalfNormal and
                Uniform among them) and `lgamma`: Gamma(a, 1) observed at 1, which is -1 - lgamma(a)
    DRAWS       one entry per family whose sampler branches, its parameters at each branch threshold

Every entry is used in two arrangements of one length (`arranged`): `built`, the points in order
followed by as many ordinary values (waves mostly uniform in their branch), and `mixed`, the points
under a fixed permutation interleaved one to one with the same ordinary values (neighbouring lanes
take different branches). tests/test_math_edges.py holds the oracle to the references;
tests/test_gpu_math_edges.py holds the device to the oracle, bit for bit.

    python tests/mathedge.py --op pow --backend oracle     the oracle against the reference
    python tests/mathedge.py --op pow --backend hip        the device against the oracle

print agreement, or the first differing input with both bit patterns (`--op logpdf:gamma` and
`--op draw:binomial` replay a family's entry).
"""
from __future__ import annotations

import argparse
import functools
import math
import pathlib
import re
import struct
import sys
from dataclasses import dataclass

import numpy as np

import progfuzz as pf   # (puts the package and the oracle on sys.path)
from progfuzz import _FAM, FAMILIES

from wsmc import abi, dsl, models  # noqa: E402
from wsmc.dsl import Col  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parents[1]
SEED = 7321                      # the ordinary values and the permutation: default_rng([SEED, k])
INF, NAN = math.inf, math.nan
DBL_MAX = float(np.finfo(float).max)
TINY = float(np.finfo(float).tiny)          # the smallest normal
SUB_MIN = 5e-324                            # the smallest subnormal
SUB_MAX = float(np.nextafter(TINY, 0.0))    # the largest subnormal
ONE_M = float(np.nextafter(1.0, 0.0))       # 1 - 2^-53
ARRANGEMENTS = ("built", "mixed")


def bits(v) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def from_bits(b) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


def nb(v, k=2):
    """v with its neighbours at 1 .. k ulp on both sides: [v, v-1ulp, v+1ulp, v-2ulp, v+2ulp, ...]"""
    out, lo, hi = [float(v)], float(v), float(v)
    for _ in range(k):
        lo, hi = float(np.nextafter(lo, -INF)), float(np.nextafter(hi, INF))
        out += [lo, hi]
    return out


def _header(name) -> str:
    return (REPO / "include" / name).read_text()


def _read(text, pattern, what):
    m = re.search(pattern, text)
    if not m:
        raise RuntimeError(f"mathedge: {what} not found in the header (pattern {pattern!r})")
    return float(m.group(1))


_MATH_H, _TERMS_H = _header("wsmc_math.h"), _header("wsmc_terms.h")
PIO2_LARGE = _read(_MATH_H, r"#define WSMC_PIO2_LARGE\s+([0-9.eE+-]+)", "WSMC_PIO2_LARGE")
# the samplers' branch thresholds and loop caps, as wsmc_terms.h writes them
GAMMA_SMALL = _read(_TERMS_H, r"const int small = al < ([0-9.]+);", "the Gamma boost's threshold")
POISSON_PTRS = _read(_TERMS_H, r"if \(!\(lam >= ([0-9.]+)\)\)", "the Poisson inversion / PTRS threshold")
BINOMIAL_BTRS = _read(_TERMS_H, r"if \(!\(n \* q >= ([0-9.]+)\)\)", "the Binomial inversion / BTRS threshold")
BINOMIAL_FLIP = _read(_TERMS_H, r"const int flip = p > ([0-9.]+);", "the Binomial mirror threshold")
# (the Beta draw's switch to the ratio from logarithms is on the two drawn Gamma stages, not on a
# parameter, so no parameter can sit 1 ulp from it: the entry's shapes of 1e-300 always cross it,
# both boosts underflowing, and 0.01 crosses it in some draws; the value is read only to be quoted)
BETA_LOGFORM = _read(_TERMS_H, r"if \(g1 >= ([0-9.eE+-]+) &&", "the Beta draw's switch to logarithms")
GAMMA_ROUNDS = int(_read(_TERMS_H, r"#define WSMC_GAMMA_ROUNDS (\d+)", "WSMC_GAMMA_ROUNDS"))
INV_STEPS = int(_read(_TERMS_H, r"#define WSMC_INV_STEPS (\d+)", "WSMC_INV_STEPS"))
TRS_ROUNDS = int(_read(_TERMS_H, r"#define WSMC_TRS_ROUNDS (\d+)", "WSMC_TRS_ROUNDS"))


def _rng(k):
    return np.random.default_rng([SEED, int(k)])


def _ordinary(kind, n, k):
    g = _rng(k)
    if kind == "pos":
        return g.uniform(0.1, 3.0, n)
    if kind == "trig":
        return g.normal(0.0, 30.0, n)
    return g.normal(0.0, 2.0, n)


# ---- references -----------------------------------------------------------------------------------
# A reference of one point is one of
#   ("exact", v)          the value, bit for bit (a NaN: any NaN)
#   ("ulp", want, k)      an mpmath value: within k ulp of it (ulps of the result; a subnormal result's
#                         ulp is 5e-324, an infinite answer counts as 2^1024)
#   ("abs", want, tol)    an mpmath value: within tol of it
#   ("zero",)             a zero of either sign (the one case DESIGN.md section 6 records: _ref_powi)
#   ("sign", want)        parity only: the sign of want, an infinity where |want| >= 2^1025, a zero
#                         where |want| <= 2^-1076
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def ulp_of(want):
    """the spacing of doubles at the mpmath value `want` (5e-324 at and below the subnormals)"""
    mp = _mp()
    if want == 0:
        return mp.mpf(2) ** -1074
    e = mp.frexp(abs(want))[1] - 1
    return mp.mpf(2) ** (min(max(int(e), -1022), 1023) - 52)


def as_mpf(got, want):
    """`got` as an mpmath number; an infinity counts as 2^1024, or as `want` itself past that (where
    the infinity is the rounded answer)"""
    mp = _mp()
    if math.isinf(got):
        big = max(mp.mpf(2) ** 1024, abs(want)) if (want > 0) == (got > 0) else mp.mpf(2) ** 1024
        return big if got > 0 else -big
    return mp.mpf(float(got))


def judge(ref, got):
    """None, or why `got` misses the reference of its point; (error in the reference's unit) too"""
    mp = _mp()
    kind = ref[0]
    got = float(got)
    if kind == "exact":
        want = float(ref[1])
        if math.isnan(want):
            return (None if math.isnan(got) else f"expected NaN"), 0.0
        return (None if bits(got) == bits(want) else f"expected {want!r} (0x{bits(want):016x})"), 0.0
    if kind == "zero":
        return (None if got == 0.0 else "expected a zero"), 0.0
    want = ref[1]
    if math.isnan(got):
        return f"expected about {mp.nstr(want, 20)}, got NaN", INF
    if kind == "sign":
        neg = math.copysign(1.0, got) < 0
        if want != 0 and neg != (want < 0):
            return f"expected the sign of {mp.nstr(want, 8)}", INF
        if abs(want) >= mp.mpf(2) ** 1025 and not math.isinf(got):
            return "expected an infinity", INF
        if abs(want) <= mp.mpf(2) ** -1076 and got != 0.0:
            return "expected a zero", INF
        return None, 0.0
    err = abs(as_mpf(got, want) - want)
    if kind == "ulp":
        u = err / ulp_of(want)
        return (None if u <= ref[2] else f"{mp.nstr(u, 5)} ulp from {mp.nstr(want, 20)} (bound {ref[2]})"), float(u)
    return (None if err <= ref[2] else f"error {mp.nstr(err, 5)} from {mp.nstr(want, 20)} (bound {mp.nstr(ref[2], 5)})"), \
        float(err / ref[2]) if ref[2] else 0.0


def _ref_exp(_, x):
    """0.55 ulp on the table path (|x| < 512), 1 ulp on the fdlibm path beyond it; the same bound in
    units of 5e-324 where the result is subnormal (tests/test_oracle_math.py states both)"""
    if math.isnan(x):
        return ("exact", NAN)
    if x > 711.0:     # e^711 > 2^1025
        return ("exact", INF)
    if x < -747.0:    # e^-747 < 2^-1077
        return ("exact", 0.0)
    return ("ulp", _mp().exp(_mp().mpf(x)), 0.55 if abs(x) < 512.0 else 1.0)


def _ref_log(_, x):
    if math.isnan(x) or x < 0.0:
        return ("exact", NAN)
    if x == 0.0:
        return ("exact", -INF)
    if x == INF or x == 1.0:
        return ("exact", INF if x == INF else 0.0)
    return ("ulp", _mp().log(_mp().mpf(x)), 0.75)


def _ref_log1p(_, x):
    """2 ulp: the log's 0.75, and the roundings of the quotient and of the product in Goldberg's form"""
    if math.isnan(x) or x < -1.0:
        return ("exact", NAN)
    if x == -1.0:
        return ("exact", -INF)
    if x == INF or x == 0.0:
        return ("exact", x)
    return ("ulp", _mp().log1p(_mp().mpf(x)), 2.0)


def _ref_sqrt(_, x):
    if math.isnan(x) or x < 0.0:
        return ("exact", NAN)
    if x == 0.0 or x == INF:
        return ("exact", x)   # sqrt(-0.0) = -0.0
    return ("ulp", _mp().sqrt(_mp().mpf(x)), 0.5)   # correctly rounded: never a tie, so exactly the nearest


def _ref_trig(fn):
    def ref(_, x):
        if not math.isfinite(x):
            return ("exact", NAN)
        if x == 0.0:
            return ("exact", x if fn == "sin" else 1.0)
        mp = _mp()
        return ("ulp", getattr(mp, fn)(mp.mpf(x)), 1.0)   # the fdlibm kernels' stated bound
    return ref


def _ref_powi(n, x):
    """Base.literal_pow / pow_body: 1 ulp for |n| <= 1024 where the result is normal (compensated
    squaring), parity beyond; the signed zeros and infinities by the exponent's parity. Two cases
    are recorded in DESIGN.md section 6 and held to what is derived for them, not to that bound:
    n = -2 is literal_pow's inv(x)^2: the reciprocal's rounding (relative u = 2^-53) is squared
    (2 u + u^2) and the product rounded once more (half an ulp of the result), so the error is at
    most (2 u + u^2) |x^-2| + ulp / 2, which lies between 1.5 and 2.5 ulp by where the result sits in
    its binade (1.12 ulp measured at 10.0^-2, which is Julia's 0.010000000000000002); and a negative zero that pow_body (every odd n but 1, 3 and -1) reaches
    comes out of its last fma(x, y, +0.0) as +0.0, so there only a zero is asserted."""
    n = int(n)
    if n == 0:
        return ("exact", 1.0)
    if math.isnan(x):
        return ("exact", NAN)
    if x == 0.0 or math.isinf(x):
        neg = math.copysign(1.0, x) < 0 and n % 2 != 0
        big = math.isinf(x) == (n > 0)
        if neg and not big and n not in (1, 3, -1):
            return ("zero",)
        return ("exact", (-1.0 if neg else 1.0) * (INF if big else 0.0))
    mp = _mp()
    want = mp.mpf(x) ** n
    if n == -2 and mp.mpf(TINY) <= abs(want) <= mp.mpf(DBL_MAX):
        u = mp.mpf(2) ** -53
        return ("abs", want, abs(want) * (2 * u + u * u) + ulp_of(want) / 2)
    if abs(n) <= 1024 and mp.mpf(TINY) <= abs(want) <= mp.mpf(DBL_MAX):
        return ("ulp", want, 1.0)
    return ("sign", want)


POW_CLAMP = 6917529027641081856.0   # 0x1.8p62: Base.^ clamps |y| to it (every power past it over- or underflows)


def _ref_pow(_, a, b):
    """Base.^(::Float64, ::Float64): 1 for x == 1, NaN for a NaN y, |y| clamped to 1.5 2^62, an integer
    y as the integer power, 0^y and Inf^y by the sign of y, a negative base with a non-integer y a
    DomainError (NaN here), else exp(y log x): relative error 2^-53 (2 + 2 |y log x|) (the header's
    statement of its conditioning, with the log's and the exp's bounds), or one unit of 5e-324 where
    the result is subnormal"""
    if a == 1.0:
        return ("exact", 1.0)
    if math.isnan(b):
        return ("exact", NAN)
    if not abs(b) < POW_CLAMP:
        b = math.copysign(POW_CLAMP, b)
    if b == math.floor(b):
        return _ref_powi(int(b), a)
    if math.isnan(a) or a < 0.0:
        return ("exact", NAN)
    if a == 0.0:
        return ("exact", 0.0 if b > 0.0 else INF)
    if a == INF:
        return ("exact", INF if b > 0.0 else 0.0)
    mp = _mp()
    want = mp.power(mp.mpf(a), mp.mpf(b))
    if not (mp.mpf(2) ** -1076 < want < mp.mpf(2) ** 1025):
        return ("sign", want)
    rel = mp.mpf(2) ** -53 * (2 + 2 * abs(mp.mpf(b) * mp.log(mp.mpf(a))))
    return ("abs", want, max(want * rel, mp.mpf(2) ** -1074))


def _np2(f):
    def ref(_, a, b):
        with np.errstate(all="ignore"):
            return ("exact", float(f(np.float64(a), np.float64(b))))
    return ref


def jl_min(a, b):
    """Base.min: a NaN operand gives NaN, min(-0.0, 0.0) = min(0.0, -0.0) = -0.0"""
    if math.isnan(a) or math.isnan(b):
        return NAN
    if a == b:
        return a if math.copysign(1.0, a) < 0 else b
    return a if a < b else b


def jl_max(a, b):
    """Base.max: a NaN operand gives NaN, max(-0.0, 0.0) = max(0.0, -0.0) = 0.0"""
    if math.isnan(a) or math.isnan(b):
        return NAN
    if a == b:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a > b else b


def _truth(f):
    return lambda _, *xs: ("exact", 1.0 if f(*xs) else 0.0)


# ---- operator entries -----------------------------------------------------------------------------
@dataclass
class Entry:
    """one operator: `args` the points (one array per operand), `variants` the constants an
    instruction carries (POWI's exponent, CONST's value; (None,) otherwise), `ref(c, *point)` the
    reference of one point, `kinds` what an ordinary value of each operand is"""
    name: str
    op: int
    args: tuple
    ref: object
    kinds: tuple
    variants: tuple = (None,)
    index: int = 0

    @property
    def n(self) -> int:
        return len(self.args[0])

    @property
    def arity(self) -> int:
        return len(self.args)

    def label(self, c) -> str:
        return self.name if c is None else f"{self.name}[{c!r}]"

    def tree(self, c, leaves):
        """progfuzz's expression tree of the operator over `leaves` (one per operand)"""
        if self.op == abi.X_CONST:
            return ("c", float(c))
        if self.op == abi.X_COL:
            return leaves[0]
        if self.op == abi.X_POWI:
            return (abi.X_POWI, int(c), leaves[0])
        return (self.op,) + tuple(leaves[:self.arity])

    def ordinary(self):
        return tuple(_ordinary(kind, self.n, 16 * self.index + k) for k, kind in enumerate(self.kinds))

    def refs(self, v=0):
        """the reference of every point under variant number v"""
        return _refs(self.name, v)

    def domain(self, v=0):
        """where a finite mpmath reference exists (everywhere else the expected value is exact)"""
        return np.array([r[0] in ("ulp", "abs") for r in self.refs(v)])


@functools.lru_cache(maxsize=None)
def _refs(name, v):
    e = OPERATORS[name]
    return [e.ref(e.variants[v], *(float(a[i]) for a in e.args)) for i in range(e.n)]


def arranged(points, ordinary, index, which):
    """`built`: the points, then the ordinary values. `mixed`: the points under the entry's fixed
    permutation at the even places, the ordinary values at the odd ones. Both of length 2 n."""
    n = len(points[0])
    if which == "built":
        return tuple(np.concatenate([np.asarray(p, float), np.asarray(o, float)]) for p, o in zip(points, ordinary))
    perm = _rng(1000 + index).permutation(n)
    out = []
    for p, o in zip(points, ordinary):
        z = np.empty(2 * n)
        z[0::2], z[1::2] = np.asarray(p, float)[perm], o
        out.append(z)
    return tuple(out)


def place(n, index, which):
    """where point i of an entry sits in an arrangement: an index array of length n"""
    if which == "built":
        return np.arange(n)
    at = np.empty(n, dtype=np.int64)
    at[_rng(1000 + index).permutation(n)] = 2 * np.arange(n)
    return at


COMMON = [0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, TINY, -TINY] + nb(1.0) + nb(-1.0) + \
    [DBL_MAX, -DBL_MAX, INF, -INF, NAN]
LN2 = 0.6931471805599453
CROSS = [0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, SUB_MIN, -SUB_MIN, DBL_MAX, -DBL_MAX]


def _exp_points():
    xs = COMMON + nb(512.0) + nb(-512.0) + nb(709.782712893384) + nb(-708.3964185322641) + nb(-745.1332191019411)
    xs += nb(2.0 ** -28) + nb(-2.0 ** -28) + nb(0.5 * LN2) + nb(-0.5 * LN2)
    for k in (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, -1, -64, -127, -128, 1000):   # table index boundaries
        xs += nb(k * LN2 / 128.0)
    return xs


def log_table_edges():
    """the 128 interval edges, as tests/test_oracle_math.py test_log_table_accuracy_against_decimal builds them"""
    return [from_bits(0x3fe6000000000000 + (i << 45) + d) for i in range(128) for d in (0, 1, (1 << 45) - 1)]


def _log_points():
    xs = COMMON + log_table_edges()
    for k in range(1, 5):
        xs += [1.0 + k * 2.0 ** -52, 1.0 - k * 2.0 ** -53]
    xs += [2.0 ** k for k in range(-1074, 1024, 7)] + [2.0 ** -1022, 2.0 ** 1023, 2.0 ** -1023, 2.0 ** -1074]
    xs += [3 * SUB_MIN, 1e-310, 1e-320, float(np.nextafter(SUB_MAX, 0.0))]
    return xs


def _log1p_points():
    return COMMON + nb(-1.0) + [-1.0 + 2.0 ** -53, -0.5, 2.0 ** -53, -2.0 ** -53, 2.0 ** -54, -2.0 ** -54, 1e-300, -1e-300,
                                -1.5, -2.0, -1e300, 1e300] + nb(-0.5) + nb(2.0 ** -53) + nb(-2.0 ** -53)


def _sqrt_points():
    xs = COMMON + [-2.0, -1e-300, 3 * SUB_MIN, 1e-310, 1e-320]
    xs += [2.0 ** k for k in (-1074, -1073, -1023, -1022, -1021, -2, -1, 1, 2, 3, 52, 53, 1022, 1023)]
    for q in (4.0, 9.0, 25.0, 2.0 ** 52, 3.0 ** 30, 1e300, 4.0 ** -500):   # perfect squares, and 1e300
        xs += nb(q)
    return xs


def _trig_points():
    xs = list(COMMON)
    for k in range(17):
        xs += nb(k * math.pi / 4.0)
        xs += nb(-k * math.pi / 4.0, 1)
    xs += nb(PIO2_LARGE) + nb(-PIO2_LARGE) + [1e22, -1e22, 2.0 ** 1023, 6381956970095103.0 * 2.0 ** 797,
                                               -6381956970095103.0 * 2.0 ** 797]
    return xs


POWI_N = (0, 1, -1, 2, -2, 3, -3, 4, -4, 7, -5, 63, 64, -64, 1023, -1074)
POWI_X = [0.0, -0.0, 0.5, -0.5, 2.0, -2.0] + nb(1.0) + nb(-1.0) + [SUB_MIN, 1e-310, 1e300, INF, -INF, NAN]
POW_A = [0.0, -0.0, 1.0, -1.0] + nb(1.0)[1:] + [0.5, -0.5, 2.0, -2.0, 10.0, SUB_MIN, 1e300, INF, -INF, NAN]
POW_B = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, 3.0, -2.0, 7.0, 0.1, 2.0 ** 53, 2.0 ** 53 + 2.0, 1e18 + 128.0, 1e19, -1e19,
         9.3e18, 4503599627370496.5, 1e-300, INF, -INF, NAN]


def _cross(*sets):
    grid = np.meshgrid(*[np.asarray(s, float) for s in sets], indexing="ij")
    return tuple(g.ravel() for g in grid)


def _entries():
    out = []

    def add(name, op, args, ref, kinds, variants=(None,)):
        args = tuple(np.asarray(a, float) for a in (args if isinstance(args, tuple) else (args,)))
        out.append(Entry(name, op, args, ref, kinds, tuple(variants), len(out)))

    add("const", abi.X_CONST, COMMON, lambda c, x: ("exact", c), ("real",), tuple(CROSS))
    add("col", abi.X_COL, COMMON, lambda c, x: ("exact", x), ("real",))
    add("neg", abi.X_NEG, COMMON, lambda c, x: ("exact", -x), ("real",))
    add("abs", abi.X_ABS, COMMON, lambda c, x: ("exact", math.fabs(x)), ("real",))
    add("sqrt", abi.X_SQRT, _sqrt_points(), _ref_sqrt, ("pos",))
    add("exp", abi.X_EXP, _exp_points(), _ref_exp, ("real",))
    add("log", abi.X_LOG, _log_points(), _ref_log, ("pos",))
    add("log1p", abi.X_LOG1P, _log1p_points(), _ref_log1p, ("pos",))
    add("sin", abi.X_SIN, _trig_points(), _ref_trig("sin"), ("trig",))
    add("cos", abi.X_COS, _trig_points(), _ref_trig("cos"), ("trig",))
    add("powi", abi.X_POWI, POWI_X, _ref_powi, ("real",), POWI_N)
    add("not", abi.X_NOT, COMMON, _truth(lambda x: x == 0.0), ("real",))
    two, rr = _cross(CROSS, CROSS), ("real", "real")
    add("add", abi.X_ADD, two, _np2(lambda a, b: a + b), rr)
    add("sub", abi.X_SUB, two, _np2(lambda a, b: a - b), rr)
    add("mul", abi.X_MUL, two, _np2(lambda a, b: a * b), rr)
    add("div", abi.X_DIV, two, _np2(lambda a, b: a / b), rr)
    add("min", abi.X_MIN, two, lambda c, a, b: ("exact", jl_min(a, b)), rr)
    add("max", abi.X_MAX, two, lambda c, a, b: ("exact", jl_max(a, b)), rr)
    add("pow", abi.X_POW, _cross(POW_A, POW_B), _ref_pow, ("pos", "real"))
    add("lt", abi.X_LT, two, _truth(lambda a, b: a < b), rr)
    add("le", abi.X_LE, two, _truth(lambda a, b: a <= b), rr)
    add("gt", abi.X_GT, two, _truth(lambda a, b: a > b), rr)
    add("ge", abi.X_GE, two, _truth(lambda a, b: a >= b), rr)
    add("eq", abi.X_EQ, two, _truth(lambda a, b: a == b), rr)
    add("ne", abi.X_NE, two, _truth(lambda a, b: a != b), rr)
    add("and", abi.X_AND, two, _truth(lambda a, b: a != 0.0 and b != 0.0), rr)
    add("or", abi.X_OR, two, _truth(lambda a, b: a != 0.0 or b != 0.0), rr)
    add("ifelse", abi.X_IFELSE, _cross(CROSS, CROSS, CROSS), lambda c, k, t, f: ("exact", t if k != 0.0 else f),
        ("real", "real", "real"))
    return {e.name: e for e in out}


OPERATORS = _entries()
UNARY = [n for n, e in OPERATORS.items() if e.arity == 1]
BINARY = [n for n, e in OPERATORS.items() if e.arity == 2]


# ---- running an operator entry on a backend -----------------------------------------------------------
def upload(ctx, cols):
    for name, v in cols.items():
        ctx.col_upload(ctx.col_create(name), np.ascontiguousarray(v, float))


def assign_tree(ctx, out, tree):
    c = ctx.col_find(out)
    if c < 0:
        c = ctx.col_create(out)
    prog, lens = dsl.xprogram([pf.to_fx(tree)], models.resolver(ctx))
    ctx.assign_expr(c, prog, lens)
    return c


def operator_inputs(e: Entry):
    """{arrangement: the operand arrays}"""
    ordinary = e.ordinary()
    return {w: arranged(e.args, ordinary, e.index, w) for w in ARRANGEMENTS}


def operator_columns(e: Entry, prefix=""):
    """the context columns of both arrangements, `<prefix>built0`, `<prefix>mixed1`, ..."""
    return {f"{prefix}{w}{k}": a for w, arrs in operator_inputs(e).items() for k, a in enumerate(arrs)}


def operator_statements(e: Entry, prefix=""):
    """[(output column, arrangement, variant number, tree)] over operator_columns' names"""
    out = []
    for w in ARRANGEMENTS:
        leaves = [("col", f"{prefix}{w}{k}", 0) for k in range(e.arity)]
        for v, c in enumerate(e.variants):
            out.append((f"{prefix}out_{w}_{v}", w, v, e.tree(c, leaves)))
    return out


def run_operator(ctx, e: Entry, each=True):
    """both arrangements of `e` through Assigns on `ctx` (a context of 2 e.n particles): each=True
    downloads after every Assign (the statement alone), else after the last. {(arrangement, variant
    number): values}"""
    upload(ctx, operator_columns(e))
    res, stmts = {}, operator_statements(e)
    for out, w, v, tree in stmts:
        col = assign_tree(ctx, out, tree)
        if each:
            res[(w, v)] = ctx.col_download(col)
    if not each:
        for out, w, v, _ in stmts:
            res[(w, v)] = ctx.col_download(ctx.col_find(out))
    return res


@functools.lru_cache(maxsize=None)
def _oracle_operator(name):
    from oracle import Oracle
    e = OPERATORS[name]
    o = Oracle(2 * e.n, seed=1)
    try:
        return run_operator(o, e)
    finally:
        o.close()


def oracle_operator(name):
    """the oracle's values of an operator entry, computed once (left unchanged by every user)"""
    return _oracle_operator(name)


# ---- an operator entry as a scalar-SSM spec ------------------------------------------------------------
def ssm_case(e: Entry, variants, lo, hi):
    """an ssmfuzz.Case whose step assigns the operator (under up to three of its constants, by
    variant number) of the step's data to a column each, then observes a constant under a fixed
    Normal; the data table holds the entry's points lo .. hi, one per step"""
    import ssmfuzz as sf
    leaves = [sf.dl(k) for k in range(e.arity)]
    step = [sf.X(c, e.tree(e.variants[v], leaves)) for c, v in enumerate(variants)]
    step.append(sf.O(sf.K(0.3), sf.DistD(abi.FAM_NORMAL, sf.K(0.0), sf.K(1.0))))
    data = np.stack([a[lo:hi] for a in e.args], axis=1)
    return sf.Case(f"{e.name}{list(variants)}[{lo}:{hi}]", len(variants), [], step, e.arity, data, hi - lo)


def ssm_runs(e: Entry, steps=256):
    """(variant numbers, lo, hi) of the runs that cover an entry: three constants and `steps` points a run"""
    for v0 in range(0, len(e.variants), 3):
        variants = list(range(v0, min(v0 + 3, len(e.variants))))
        for lo in range(0, e.n, steps):
            yield variants, lo, min(lo + steps, e.n)


# ---- the comparer -------------------------------------------------------------------------------------
def first_difference(what, arrangement, inputs, got, want):
    """None, or the first place two results differ: `what` (the operator or family), the arrangement,
    the index, the input value(s) and both bit patterns. Bit for bit; a NaN matches any NaN (the
    default NaN's sign differs between x86 and the GPU); -0.0 differs from 0.0."""
    got, want = np.asarray(got, float).ravel(), np.asarray(want, float).ravel()
    if got.shape != want.shape:
        return f"{what} [{arrangement}]: {got.shape[0]} values against {want.shape[0]}"
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if ok.all():
        return None
    i = int(np.flatnonzero(~ok)[0])
    xs = ", ".join(f"{float(a[i])!r} (0x{bits(a[i]):016x})" for a in inputs)
    return (f"{what} [{arrangement}]: {int((~ok).sum())} of {len(ok)} differ, first at index {i}: input {xs}: "
            f"{got[i]!r} (0x{bits(got[i]):016x}) != {want[i]!r} (0x{bits(want[i]):016x})")


# ---- log-density entries ------------------------------------------------------------------------------
# what a parameter or an observed value of each kind runs over: the edge of its domain with
# neighbours, tiny, huge, and invalid values; MODERATE marks the interior the references cover
LOC = [0.0, -0.0, 1.0, -2.5, 1e-300, 1e15, -1e15, 1e300, NAN, INF, -INF]
POS = [SUB_MIN, 1e-300, 0.5, 1.0, 3.0, 1e15, 1e300, 0.0, -1.0, NAN, INF]
PROB = [0.0, SUB_MIN, 1e-300, 0.25, 0.5, ONE_M, 1.0, float(np.nextafter(1.0, 2.0)), -0.25, 1.5, NAN, INF]
SHAPE = [SUB_MIN, 1e-300, 0.5] + nb(1.0, 1) + [2.5, 1e15, 1e300, 0.0, -1.0, NAN, INF]
NINT = [0.0, 1.0, 20.0, 2.0 ** 31, 1e15, 1e300, 2.5, -1.0, NAN, INF]
PARAM = {"real": LOC, "small": LOC, "pos": POS, "small_pos": POS, "prob": PROB, "shape": SHAPE, "nint": NINT}
MODERATE = {"real": [0.0, 1.0, -2.5], "small": [0.0, 1.0, -2.5], "pos": [0.5, 1.0, 3.0], "small_pos": [0.5, 1.0, 3.0],
            "prob": [0.25, 0.5], "shape": [0.5, 1.0, 2.5], "nint": [1.0, 20.0]}
VALID = {"real": lambda v: math.isfinite(v), "small": lambda v: math.isfinite(v), "pos": lambda v: 0.0 < v < INF,
         "small_pos": lambda v: 0.0 < v < INF, "prob": lambda v: 0.0 <= v <= 1.0, "shape": lambda v: 0.0 < v < INF,
         "nint": lambda v: 0.0 <= v < INF and v == math.floor(v)}
OBSERVED = {
    "real": [0.0, -0.0, 1.0, -1.0, 0.5, 1e-300, -1e-300, 1e300, -1e300, INF, -INF, NAN],
    "pos": [-SUB_MIN, -0.0, 0.0, SUB_MIN, 2 * SUB_MIN, 1e-300, 0.5, 1.0, 3.0, 1e300, INF, -1.0, NAN],
    "prob": nb(0.0) + [-0.0, 0.25, 0.5] + nb(1.0) + [-0.1, 1.5, NAN],
    "count": [0.0, -0.0, 1.0, 7.0, 20.0, 2.5, 2.0 ** 53, -1.0, float(np.nextafter(1.0, 2.0)), ONE_M, INF, NAN],
    "bit": [0.0, -0.0, 1.0, 0.5, 2.0, -1.0, ONE_M, float(np.nextafter(1.0, 2.0)), SUB_MIN, NAN],
}
INTERIOR_X = {"real": [0.0, 1.0, -1.0, 0.5], "pos": [0.5, 1.0, 3.0], "prob": [0.25, 0.5], "count": [0.0, 1.0, 7.0, 20.0],
              "bit": [0.0, 1.0]}
SHORT = {abi.FAM_INVERSEGAMMA: "invgamma", abi.FAM_NEGBINOMIAL: "negbinomial", abi.FAM_BERNOULLI_LOGIT: "bernoulli_logit"}


def family_name(fam) -> str:
    return SHORT.get(fam, FAMILIES[fam].lower())


@dataclass
class PdfEntry:
    """one family's log-density: parameter columns a (mu[0]) and b (scale) and the observed x, the
    cross of their kinds' lists; a parameter the family does not have is the constant 0 / 1
    (kinds[k] None); `interior` marks the points the references of tests/test_math_edges.py cover"""
    name: str
    fam: int
    kinds: tuple          # (first parameter's kind or None, second's or None, the observed value's)
    a: np.ndarray
    b: np.ndarray
    x: np.ndarray
    interior: np.ndarray
    valid: np.ndarray     # both parameters inside the family's domain
    params: tuple = (0.0, 0.0)
    index: int = 0

    @property
    def n(self) -> int:
        return len(self.x)

    def kernel(self, a_col, b_col):
        loc = Col(a_col) if self.kinds[0] else 0.0
        scale = Col(b_col) if self.kinds[1] else 1.0
        return dsl.Kernel(self.fam, 1, (dsl.Expr.lift(loc),), scale, self.params)

    def ordinary(self):
        g = _rng(5000 + self.index)
        ka, kb, kx = self.kinds
        pick = lambda vals: g.choice(np.asarray(vals, float), self.n)
        x = pick(INTERIOR_X[kx])
        if self.fam == abi.FAM_BINOMIAL:
            x = np.minimum(x, 1.0)
        if self.fam == abi.FAM_UNIFORM:
            x = pick([0.5, 1.0, 1.5])
        return (pick(MODERATE[ka]) if ka else np.zeros(self.n), pick(MODERATE[kb]) if kb else np.ones(self.n), x)

    def inputs(self):
        o = self.ordinary()
        return {w: arranged((self.a, self.b, self.x), o, 200 + self.index, w) for w in ARRANGEMENTS}


def _among(v, vals):
    """v is one of vals (and is not the -0.0 that compares equal to a 0.0 among them)"""
    return np.isin(v, vals) & ~((v == 0.0) & np.signbit(v))


def _pdf_entries():
    out = {}
    fams = dict(_FAM)
    for fam in sorted(fams):
        ka, kb, kx = fams[fam][0], fams[fam][1], fams[fam][2]
        if fam == abi.FAM_UNIFORM:   # its bounds are constants of the dist (param[0..1]), not operands
            xs = nb(0.25) + nb(2.0) + [1.0, 0.0, -0.0, -1.0, 3.0, INF, -INF, NAN]
            a, b, x = np.zeros(len(xs)), np.ones(len(xs)), np.asarray(xs, float)
            interior = np.array([0.25 < v < 2.0 for v in xs])
            valid = np.ones(len(xs), bool)
            e = PdfEntry("uniform", fam, (None, None, "real"), a, b, x, interior, valid, (0.25, 2.0))
        else:
            A = PARAM[ka] if ka else [0.0]
            B = PARAM[kb] if kb else [1.0]
            a, b, x = _cross(A, B, OBSERVED[kx])
            ia = _among(a, MODERATE[ka]) if ka else np.ones(len(a), bool)
            ib = _among(b, MODERATE[kb]) if kb else np.ones(len(a), bool)
            ix = _among(x, INTERIOR_X[kx])
            if fam == abi.FAM_BINOMIAL:
                ix &= x <= a
            if fam in (abi.FAM_LOGNORMAL, abi.FAM_EXPONENTIAL, abi.FAM_RAYLEIGH, abi.FAM_HALFNORMAL):
                ix &= x > 0.0
            va = np.array([VALID[ka](v) for v in a]) if ka else np.ones(len(a), bool)
            vb = np.array([VALID[kb](v) for v in b]) if kb else np.ones(len(a), bool)
            e = PdfEntry(family_name(fam), fam, (ka, kb, kx), a, b, x, ia & ib & ix, va & vb)
        e.index = len(out)
        out[e.name] = e
    # wsmc_lgamma alone: Gamma(a, 1) observed at 1 is -1 - lgamma(a)
    a = []
    for h in (0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.0):
        a += nb(h)
    a += nb(1.0, 4) + nb(2.0, 4) + [1e-300, SUB_MIN, 170.5, 1e15, 1e305, 0.0, -1.0, INF, NAN]
    a = np.asarray(a, float)
    out["lgamma"] = PdfEntry("lgamma", abi.FAM_GAMMA, ("shape", "pos", "pos"), a, np.ones(len(a)), np.ones(len(a)),
                             (a > 0) & (a < INF), (a > 0) & (a < INF), index=len(out))
    return out


LOGPDFS = _pdf_entries()


def run_logpdf(ctx, e: PdfEntry, which, score=True):
    """one Observe of the entry's family with parameters and value from columns (a context of 2 e.n
    particles): (the weights, score(depth))"""
    a, b, x = e.inputs()[which]
    upload(ctx, {"a": a, "b": b, "x": x})
    R = models.resolver(ctx)
    ctx.observe(e.kernel("a", "b").dist(R), [Col("x").operand(R)])
    w = ctx.weights_download()
    return w, (ctx.score(ctx.get_state()["depth"]) if score else None)


# ---- draw entries -----------------------------------------------------------------------------------------
# Every loop of a sampler is capped (include/wsmc_terms.h): a Gamma stage runs at most
# WSMC_GAMMA_ROUNDS = 24 rounds and then returns d, the inversion at most WSMC_INV_STEPS = 96 steps,
# PTRS / BTRS at most WSMC_TRS_ROUNDS = 60 rounds and then return floor(lambda) / the mode. The bound
# beside an entry is the sum of the caps of the stages its parameters reach.
REPEAT = 8   # each parameter point stands REPEAT times (the draws are a function of the particle index)


@dataclass
class DrawEntry:
    name: str
    fam: int
    kinds: tuple
    a: np.ndarray
    b: np.ndarray
    ordinary_ab: tuple    # (valid ordinary a values, valid ordinary b values)
    index: int = 0

    @property
    def n(self) -> int:
        return len(self.a)

    def kernel(self, a_col, b_col):
        loc = Col(a_col) if self.kinds[0] else 0.0
        scale = Col(b_col) if self.kinds[1] else 1.0
        return dsl.Kernel(self.fam, 1, (dsl.Expr.lift(loc),), scale)

    def inputs(self):
        g = _rng(9000 + self.index)
        o = tuple(g.choice(np.asarray(v, float), self.n) for v in self.ordinary_ab)
        return {w: arranged((self.a, self.b), o, 400 + self.index, w) for w in ARRANGEMENTS}

    def in_support(self, a, b, x):
        fin = np.isfinite(x)
        if self.fam in (abi.FAM_GAMMA, abi.FAM_CHISQ):
            return fin & (x >= 0.0)
        if self.fam == abi.FAM_INVERSEGAMMA:
            return fin & (x > 0.0)
        if self.fam == abi.FAM_BETA:
            return (x >= 0.0) & (x <= 1.0)
        if self.fam == abi.FAM_TDIST:
            return fin
        ok = fin & (x >= 0.0) & (x == np.floor(x))
        return ok & (x <= a) if self.fam == abi.FAM_BINOMIAL else ok


def _draw_entries():
    out = {}

    def add(name, fam, kinds, pairs, oa, ob):
        a = np.repeat(np.asarray([p[0] for p in pairs], float), REPEAT)
        b = np.repeat(np.asarray([p[1] for p in pairs], float), REPEAT)
        out[name] = DrawEntry(name, fam, kinds, a, b, (oa, ob), len(out))

    one = nb(GAMMA_SMALL, 1)        # the boost below a shape of 1
    # Gamma(shape, scale): one stage, <= 24 rounds (+ the boost's one uniform below a shape of 1).
    #   shape 1e-300: 24 rounds, the boost exp(log u / 1e-300) underflows to 0 (a draw of 0); shape 1e6:
    #   24 rounds; scale 1e-15 (a rate of 1e15) only multiplies
    add("gamma", abi.FAM_GAMMA, ("shape", "pos"),
        [(s, t) for s in one + [1e-300, 1e6] for t in (1.0, 1e-15)], [0.3, 2.0, 7.5], [0.5, 2.0])
    # InverseGamma(shape, scale) = scale / Gamma(shape): <= 24 rounds
    add("invgamma", abi.FAM_INVERSEGAMMA, ("shape", "pos"),
        [(s, t) for s in one + [1e6] for t in (1.0, 1e15)], [3.0, 1.5], [2.0])
    # Chisq(nu) = 2 Gamma(nu / 2): the boost below nu = 2; <= 24 rounds
    add("chisq", abi.FAM_CHISQ, ("shape", None), [(v, 1.0) for v in nb(2.0 * GAMMA_SMALL, 1) + [1e-300, 1e6]], [5.0, 1.0], [1.0])
    # Beta(a, b): two Gamma stages, <= 24 rounds each; shapes of 1e-300 make both boosts underflow
    # (below the switch BETA_LOGFORM to the ratio from logarithms), 0.01 reaches it now and then
    add("beta", abi.FAM_BETA, ("shape", "shape"),
        [(s, t) for s in one + [0.01, 1e-300, 1e6] for t in one + [0.01, 1e-300]], [0.5, 2.0, 5.0], [0.5, 2.0, 5.0])
    # TDist(nu): one normal and Chisq(nu): <= 24 rounds
    add("tdist", abi.FAM_TDIST, ("shape", None), [(v, 1.0) for v in nb(2.0 * GAMMA_SMALL, 1) + [0.5, 1e6]], [1.5, 30.0], [1.0])
    # Poisson(lambda): inversion below 10 (<= 96 steps; lambda = 0 and 1e-300 stop at the first
    # comparison), PTRS from 10 on (<= 60 rounds at 10, 1e6 and 1e15 alike)
    add("poisson", abi.FAM_POISSON, ("shape", None), [(v, 1.0) for v in nb(POISSON_PTRS, 1) + [0.0, 1e-300, 1e6, 1e15]],
        [0.7, 4.0, 250.0], [1.0])
    # Binomial(n, p): q = min(p, 1 - p); inversion while n q < 10 (<= min(96, n) steps), BTRS from 10
    # on (<= 60 rounds). n q = 10 at (20, 1/2), (40, 1/4), (40, 3/4); p = 1/2 +- 1 ulp is the mirror's
    # switch. n = 2^31 with p = 5e-324 and p = 1 - 2^-53: n q < 10, inversion, <= 96 steps; with
    # p = 1/2: BTRS, <= 60 rounds. p = 0 and p = 1: q = 0, the search stops at its first comparison.
    add("binomial", abi.FAM_BINOMIAL, ("nint", "prob"),
        [(20.0, p) for p in nb(BINOMIAL_FLIP, 1)] + [(40.0, p) for p in nb(BINOMIAL_BTRS / 40.0, 1)] +
        [(40.0, p) for p in nb(1.0 - BINOMIAL_BTRS / 40.0, 1)] +
        [(2.0 ** 31, p) for p in (SUB_MIN, ONE_M, 0.5)] + [(20.0, 0.0), (20.0, 1.0), (0.0, 0.3), (1.0, 0.5)],
        [7.0, 30.0, 110.0], [0.1, 0.45, 0.9])
    # NegativeBinomial(r, p) = Poisson(Gamma(r) (1 - p) / p): the Gamma stage (<= 24 rounds, the boost
    # below r = 1) and then the Poisson's inversion (<= 96) or PTRS (<= 60) as the drawn rate falls
    # below or above 10: p = 1/2 keeps it below, 0.05 mostly above, 1 - 2^-53 and 1 make it ~0 / 0
    add("negbinomial", abi.FAM_NEGBINOMIAL, ("shape", "prob"),
        [(r, p) for r in one + [1e-300, 1e6] for p in (0.5, 0.05, ONE_M, 1.0)], [0.4, 3.0, 40.0], [0.5, 0.05])
    return out


DRAWS = _draw_entries()


def run_draw(ctx, e: DrawEntry, which):
    """x ~ D(a, b) with the parameters from columns, then x observed under the same D (a context of
    2 e.n particles): (the draws, the weights)"""
    a, b = e.inputs()[which]
    upload(ctx, {"a": a, "b": b})
    R = models.resolver(ctx)
    d = e.kernel("a", "b").dist(R)
    cx = ctx.col_create("x")
    ctx.sample(cx, d)
    ctx.observe(d, [Col("x").operand(R)])
    return ctx.col_download(cx), ctx.weights_download()


# ---- command line -------------------------------------------------------------------------------------
def check_operator(e: Entry, values):
    """[(arrangement, variant number, index, why)] of the points where `values` (run_operator's) miss
    the reference, and the worst error met per variant (in the reference's unit); the ordinary
    values of an arrangement are held to nothing here"""
    bad, worst = [], {}
    for v in range(len(e.variants)):
        refs = e.refs(v)
        for w in ARRANGEMENTS:
            at = place(e.n, e.index, w)
            got = values[(w, v)]
            for i, r in enumerate(refs):
                why, err = judge(r, got[at[i]])
                worst[v] = max(worst.get(v, 0.0), err if math.isfinite(err) else 0.0)
                if why:
                    bad.append((w, v, i, why))
    return bad, worst


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--op", required=True, help="an operator (%s), logpdf:FAMILY or draw:FAMILY" % ", ".join(OPERATORS))
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    a = ap.parse_args(argv)
    from oracle import Oracle
    kind, _, name = a.op.rpartition(":")
    if kind == "":
        e = OPERATORS[name]
        want = oracle_operator(name)
        if a.backend == "oracle":
            bad, worst = check_operator(e, want)
            for w, v, i, why in bad[:1]:
                xs = ", ".join(f"{float(arg[i])!r} (0x{bits(arg[i]):016x})" for arg in e.args)
                y = want[(w, v)][place(e.n, e.index, w)[i]]
                print(f"MISMATCH {e.label(e.variants[v])} [{w}] point {i}: input {xs}: {y!r} (0x{bits(y):016x}): {why}")
            print(f"{name}: {e.n} points, {len(bad)} outside the reference's bound; worst error "
                  + ", ".join(f"{e.label(e.variants[v])} {x:.3f}" for v, x in worst.items()))
            return 1 if bad else 0
        import wsmc
        g = wsmc.Context(2 * e.n, seed=1)
        got = run_operator(g, e)
        g.close()
        ins = operator_inputs(e)
        diffs = [d for (w, v) in want
                 if (d := first_difference(e.label(e.variants[v]), w, ins[w], got[(w, v)], want[(w, v)]))]
    else:
        e = (LOGPDFS if kind == "logpdf" else DRAWS)[name]
        run = (lambda ctx, w: run_logpdf(ctx, e, w)) if kind == "logpdf" else (lambda ctx, w: run_draw(ctx, e, w))
        diffs = []
        for w in ARRANGEMENTS:
            o = Oracle(2 * e.n, seed=1)
            want = run(o, w)
            if a.backend == "oracle":
                print(f"{a.op} [{w}]: {2 * e.n} particles;", " ".join(
                    f"{np.isnan(v).sum()} NaN, {np.isposinf(v).sum()} +inf, {np.isneginf(v).sum()} -inf" for v in want))
                continue
            import wsmc
            g = wsmc.Context(2 * e.n, seed=1)
            got = run(g, w)
            g.close()
            for part, x, y in zip(("first", "second"), got, want):
                d = first_difference(f"{a.op} ({part} result)", w, e.inputs()[w], x, y)
                if d:
                    diffs.append(d)
        if a.backend == "oracle":
            return 0
    for d in diffs[:1]:
        print("MISMATCH", d)
    if not diffs:
        print(f"{a.op}: the device and the oracle agree bit for bit on both arrangements")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())

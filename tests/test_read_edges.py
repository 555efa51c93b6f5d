"""The calls that read the state, on the CPU oracle, against the definitions (tests/readedge.py's
corpus): an independent restatement in Python of what src/utils.jl and src/resampling.jl compute and
of StatsBase's weighted quantile (as tests/test_analysis.py restates it), in `fractions.Fraction`
and mpmath only; nothing here comes from include/.

    min, max, diversity     exact: Base.minimum / maximum (a NaN propagates, -0.0 < 0.0), isequal
    median, histogram       on the integer weights q_i = floor(exp(lw_i - ceil(M)) 2^K), the
                            exponential from mpmath. wsmc_expw is good to ~2 ulp only, so a q_i of
                            the oracle may differ from these by one unit; every pair is therefore
                            evaluated at q and at q with every nonzero unit moved down by one, up by
                            one, and up by one with the weights that round to zero from above 1/2
                            made 1. The histogram's levels must be the same four times. The median
                            must walk to the same pair of values (vkold, vk) four times; its
                            interpolation weight f = (Q + q1 - 2 S_{k-1}) / (2 w_k) then moves by at
                            most (3 N + 3) / (2 w_k) (N + 1 + 2 N units in the numerator, 2 in the
                            denominator, f <= 1), which with w_k >= 2^20 (asserted) is the bound the
                            oracle's median is held to, plus 2 ulp for the three roundings of
                            vkold + f (vk - vkold). A pair that fails this is a corpus error, unless a
                            weight of one or two units sits on the smallest value (StatsBase takes w1
                            from that pair, so its rule is that sensitive itself): those medians are
                            counted and held to the oracle on the device only.
    moments                 exact rational sums of e_i z_i, e_i = exp(lw_i - M) from mpmath (kept to
                            2^-300): a sum of N terms in any order is within (N - 1) eps sum|t_i| of
                            the exact one (progfuzz._moments_close's bound); with the terms' own
                            roundings (the exponential's ulp, two products, two differences) a mean,
                            two sums and a quotient, is within 2 (N + 4) eps A1 / S0 of the exact one
                            (A1 = sum e_i |z_i|, S0 = sum e_i, both exact), and a centred second
                            moment within 2 (N + 8) eps A2 / S0 + d_a d_b (A2 the exact sum of the
                            centred terms' magnitudes, d the means' bounds: the means' errors enter
                            at second order only, sum e_i (z_i - mean) being 0); where terms are
                            subnormal (`subnormal`) each of the N + 2 operations may also be off by
                            one unit of 5e-324, which both bounds add (S0 >= 1). Pairs outside this
                            reference's domain (readedge.moments_domain) are pinned on the device
                            only, by "NaN / inf exactly as the oracle says".
    ESS%, log-evidence      mpmath values, 1e-12 relative (tests/test_resample_reference.py,
                            DESIGN.md section 2); the largest error per weight kind is printed
    sample                  without replacement a permutation prefix with every live particle before
                            every dead one, with replacement live indices only
The device is held to the oracle, bit for bit, in tests/test_gpu_read_edges.py."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import readedge as rd
from oracle import Oracle
from wsmc import abi

CPU_SIZES = (1, 2, 63, 64, 65, 257, 1025, 2049)
MOMENT_SIZES = {1: 3, 2: 3, 63: 3, 64: 3, 65: 3, 257: 3, 1025: 1}   # N -> how many of readedge.MOMENT_READS
EPS = 2.0 ** -52
ESCALE = 300          # e_i as an integer multiple of 2^-300
WORST = {}            # weight kind -> [largest ESS error, largest evidence error] (relative), printed


def setup_module(module):
    mp.mp.dps = 50


# ---- the restatement ------------------------------------------------------------------------------------
def jl_minimum(xs):
    """Base.minimum: NaN if any, -0.0 below 0.0"""
    if any(math.isnan(x) for x in xs):
        return math.nan
    return min(xs, key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1))


def jl_maximum(xs):
    if any(math.isnan(x) for x in xs):
        return math.nan
    return max(xs, key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1))


def isequal_key(x):
    return ("nan",) if math.isnan(x) else (x, math.copysign(1.0, x))


def same(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def ref_point(lw):
    """(max, R): the max (NaN if any NaN) and ceil of it where finite"""
    M = math.nan if any(math.isnan(w) for w in lw) else max(lw)
    return M, (float(math.ceil(M)) if math.isfinite(M) else M)


_QCACHE = {}


def scaled(wname, n):
    """exp(lw_i - R) 2^K for every particle as mpmath numbers (None: zero by definition), and K"""
    if (wname, n) not in _QCACHE:
        lw = [float(w) for w in rd.weights(wname, n)]
        K = rd.qbits(n)
        _, R = ref_point(lw)
        out = []
        for w in lw:
            x = w - R                                    # the difference as the code takes it
            out.append(None if not (x == x) or x < -80.0 else mp.exp(mp.mpf(x)) * mp.mpf(2) ** K)
        _QCACHE[(wname, n)] = (out, K)
    return _QCACHE[(wname, n)]


def q_variants(wname, n):
    """the integer weights, and the three perturbations by one unit"""
    s, _ = scaled(wname, n)
    q = [0 if v is None else int(mp.floor(v)) for v in s]
    down = [x - 1 if x else 0 for x in q]
    up = [x + 1 if x else 0 for x in q]
    up_all = [x + 1 if x else (1 if (v is not None and v >= 0.5) else 0) for x, v in zip(q, s)]
    return [q, down, up, up_all]


def ref_median(vals, q):
    """StatsBase.quantile(v, Weights(q), 0.5) on integer weights: ("nan",), ("refuse",),
    ("largest", v) or ("walk", vkold, vk, f as a Fraction, w_k)"""
    if any(math.isnan(v) for v in vals):
        return ("nan",)
    vw = sorted(((v, 0 if math.copysign(1.0, v) < 0 else 1, w) for v, w in zip(vals, q) if w != 0))
    if not vw:
        return ("refuse",)
    Q, q1 = sum(w for _, _, w in vw), vw[0][2]
    Sk = Skold = 0
    vk = vkold = 0.0
    k = wk = 0
    while 2 * Sk <= Q + q1:
        if k == len(vw):
            return ("largest", vw[-1][0])
        Skold, vkold = Sk, vk
        vk, _, wk = vw[k]
        Sk += wk
        k += 1
    return ("walk", vkold, vk, Fraction(Q + q1 - 2 * Skold, 2 * wk), wk)


def median_value(m):
    """the walk's answer: exact where finite (a Fraction), else as the doubles give it"""
    _, vkold, vk, f, _ = m
    if math.isfinite(vkold) and math.isfinite(vk) and math.isfinite(vk - vkold):
        return Fraction(vkold) + f * (Fraction(vk) - Fraction(vkold))
    with np.errstate(all="ignore"):
        return float(np.float64(vkold) + np.float64(float(f)) * (np.float64(vk) - np.float64(vkold)))


def ref_histogram(vals, q):
    """_histogram(values, weights) on integer weights: the 8 levels or ("refuse",). Where an extreme
    is not finite the reference's range() throws; the library's stated choice is
    inner edges of NaN between the two extremes, which no value reaches: searchsortedlast counts the
    edges <= v, so every value lands in the first bin, the value at a +inf upper end in the second."""
    lo, hi = jl_minimum(vals), jl_maximum(vals)
    if lo == hi:
        return [8] * 8
    if sum(q) == 0:
        return ("refuse",)
    if math.isfinite(lo) and math.isfinite(hi):
        edges = [float(Fraction(lo) + (Fraction(hi) - Fraction(lo)) * k / 8) for k in range(9)]
    else:
        edges = [lo] + [math.nan] * 7 + [hi]
    counts = [0] * 8
    for v, w in zip(vals, q):
        counts[min(max(sum(e <= v for e in edges), 1), 8) - 1] += w
    mx = max(counts)
    return [min(max(-((-8 * c) // mx), 1), 8) for c in counts]


def first_pair_is_a_unit(vals, wname, n):
    """StatsBase's h = (W - w1) / 2 + w1 takes w1 from the first pair, the smallest value's smallest
    weight. Where a particle whose weight is a unit or two (0.5 <= exp(lw - R) 2^K < 3: `q_boundary`)
    holds the smallest value among the particles that may be live, one unit of q decides whether w1 is
    that unit or a weight of ~2^K, and the median moves with it: no reference of q +- 1 can pin such a
    pair, so the median of these is held to the oracle on the device only."""
    if any(math.isnan(v) for v in vals):
        return False
    s, _ = scaled(wname, n)
    key = lambda v: (v, 0 if math.copysign(1.0, v) < 0 else 1)
    alive = [i for i, x in enumerate(s) if x is not None and x >= 0.5]
    if not alive:
        return False
    vmin = min(key(vals[i]) for i in alive)
    return any(s[i] < 3 and key(vals[i]) == vmin for i in alive)


def ulp(x):
    return float(np.spacing(np.float64(abs(float(x))))) if math.isfinite(float(x)) else 0.0


# ---- the oracle's outcomes of a size, computed once ------------------------------------------------------
_RUNS = {}


def oracle_runs(n):
    """{(values, weights): {read name: outcome}} of every pair at size n"""
    if n not in _RUNS:
        o = Oracle(n, seed=1)
        rd.prepare(o)
        out = {}
        for wname in rd.weight_entries(n):
            for vname in rd.value_entries(n, wname):
                res = rd.run_cell(o, vname, wname, n)
                out[(vname, wname)] = {r.name: (oc, op) for r, oc, op in res}
        o.close()
        _RUNS[n] = out
    return _RUNS[n]


def pairs(n):
    return [(v, w) for w in rd.weight_entries(n) for v in rd.value_entries(n, w)]


# ---- exact reads ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CPU_SIZES)
def test_minmax_and_diversity_are_exact(n):
    runs = oracle_runs(n)
    b = [float(x) for x in rd.ordinary(n, 32)]
    for (vname, wname), res in runs.items():
        a = [float(x) for x in rd.values(vname, n)]
        for name in ("minmax(a)", "minmax(v3[1])"):
            (kind, (mn, mx)), _ = res[name]
            assert kind == "ok" and same(mn, jl_minimum(a)) and same(mx, jl_maximum(a)), (vname, wname, name, mn, mx)
        ua, ub = len({isequal_key(x) for x in a}), len({isequal_key(x) for x in b})
        assert res["diversity[a]"][0] == ("ok", ua / n), (vname, res["diversity[a]"], ua)
        assert res["diversity[a,b]"][0] == ("ok", min(ua, ub) / n), (vname, res["diversity[a,b]"])
    if n >= 2:   # {0.0, -0.0} alone: min -0.0, max 0.0 and a diversity of 2 / N
        (_, (mn, mx)), _ = runs[("neg_zero", "flat")]["minmax(a)"]
        assert same(mn, -0.0) and same(mx, 0.0) and runs[("neg_zero", "flat")]["diversity[a]"][0][1] == 2 / n


def median_sensitivity(meds, n):
    """None where the four evaluations of a pair (q and its three perturbations) give the same answer:
    the same kind, for a walk the same pair of values, and where it interpolates between two distinct
    finite values a weight w_k >= 2^20 and answers within the bound (3 N + 3) / (2 w_k) |vk - vkold|
    + 2 ulp of each other; else what differs"""
    m = meds[0]
    for x in meds[1:]:
        if x[0] != m[0]:
            return f"the walk ends as {x[0]} and as {m[0]}"
        if m[0] == "largest" and not same(x[1], m[1]):
            return "the largest live value changes"
        if m[0] == "walk" and not (same(x[1], m[1]) and same(x[2], m[2])):
            return "the walk reaches another pair of values"
    if m[0] != "walk" or (m[1] == m[2] and math.isfinite(m[1])):
        return None
    want = median_value(m)
    if not isinstance(want, Fraction):
        return None if all(same(median_value(x), want) for x in meds) else "the doubles' answer changes"
    if m[4] < 2 ** 20:
        return f"the median interpolates on a weight of {m[4]} units"
    tol = median_tol(m, n)
    return None if all(abs(median_value(x) - want) <= tol for x in meds) else "the interpolation weight moves past its bound"


def median_tol(m, n):
    return Fraction(3 * n + 3, 2 * m[4]) * abs(Fraction(m[2]) - Fraction(m[1])) + 2 * Fraction(ulp(median_value(m)))


@pytest.mark.parametrize("n", CPU_SIZES)
def test_median_and_histogram_follow_the_restatement(n):
    """and the corpus is insensitive to one unit of q (the module docstring), and at least 90 % of
    the medians and histograms are compared with an answer. A median that one unit of q moves is a
    corpus error unless a weight of one or two units sits on the smallest value (first_pair_is_a_unit:
    then StatsBase's rule itself is that sensitive); those pairs are counted, and left to the device
    test."""
    runs = oracle_runs(n)
    compared = total = 0
    unit_moved = []
    for (vname, wname), res in runs.items():
        a = [float(x) for x in rd.values(vname, n)]
        qs = q_variants(wname, n)
        meds = [ref_median(a, q) for q in qs]
        hists = [ref_histogram(a, q) for q in qs]
        what = f"{vname} x {wname} at N = {n}"
        moved = median_sensitivity(meds, n)
        assert moved is None or first_pair_is_a_unit(a, wname, n), f"corpus error, {moved}: {what}: {meds}"
        assert all(h == hists[0] for h in hists), f"corpus error, the levels depend on one unit of q: {what}: {hists}"
        for name in ("median(a)", "median(v3[1])"):
            oc, _ = res[name]
            total += 1
            m = meds[0]
            if moved:
                assert oc[0] == "ok", (what, oc)
                unit_moved.append(what)
                continue
            if m[0] == "refuse":
                assert oc == ("err", abi.WSMC_ESTATE), (what, oc)
                continue
            compared += 1
            assert oc[0] == "ok", (what, oc)
            if m[0] == "nan":
                assert math.isnan(oc[1]), (what, oc)
            elif m[0] == "largest":
                assert same(oc[1], m[1]), (what, oc, m)
            elif m[1] == m[2] and math.isfinite(m[1]):
                # a tie: vkold + f * (+-0.0) whatever f is: vkold itself, or +0.0 between zeros
                # (-0.0 + 0.0 is +0.0 in the reference's doubles as well)
                assert same(oc[1], m[1] + 0.5 * (m[2] - m[1])), (what, oc, m)
            else:
                want = median_value(m)
                if not isinstance(want, Fraction):
                    assert same(oc[1], want), (what, oc, want)
                else:
                    tol = median_tol(m, n)
                    assert abs(Fraction(oc[1]) - want) <= tol, (what, oc, float(want), float(tol))
        for name in ("histogram(a)", "histogram(v3[1])"):
            oc, _ = res[name]
            total += 1
            h = hists[0]
            if h == ("refuse",):
                assert oc == ("err", abi.WSMC_ESTATE), (what, oc)
                continue
            compared += 1
            assert oc[0] == "ok" and list(oc[1]) == h, (what, oc, h)
    print(f"N = {n}: {compared} of {total} medians and histograms compared with an answer; {len(unit_moved)} medians that a "
          f"unit weight on the smallest value moves")
    assert compared >= 0.9 * total, (compared, total)


def test_known_answers():
    """fixed inputs with answers that can be read off: adjacent doubles, one live weight, no live weight"""
    o = Oracle(8, seed=1)
    c = o.col_create("a")
    o.col_upload(c, np.array([1.0, rd.UP1] * 4))
    assert list(o.histogram(c)) == [1, 1, 1, 1, 8, 1, 1, 8]   # the edges round to 1.0 five times, then to the other
    o.col_upload(c, np.arange(8.0))
    w = np.full(8, -np.inf)
    w[5] = 0.0
    o.weights_upload(w)
    assert o.weighted_median(c) == 5.0                        # one live weight: that particle's value
    o.weights_upload(np.full(8, -np.inf))
    for f in (lambda: o.weighted_median(c), lambda: o.histogram(c), lambda: o.sample_particles(3, True)):
        with pytest.raises(RuntimeError, match=r"\(5\)"):     # WSMC_ESTATE
            f()
    assert math.isnan(o.ess()) and math.isnan(o.log_evidence())
    assert math.isnan(o.weighted_moments([abi.Operand.column(c)])[0][0])
    o.close()


# ---- moments ------------------------------------------------------------------------------------------------
def _as_int(x, scale):
    f = Fraction(x) * (1 << scale)
    assert f.denominator == 1
    return f.numerator


ZSCALE = 1074   # every finite double is an integer multiple of 2^-1074
TINY_UNIT = Fraction(1, 1 << 1074)   # a product or a sum that is subnormal is off by up to one of these, not by eps


def exact_moments(cols, lw, read, n):
    """(means, their bounds, cov or None, its bounds): Fractions, the sums taken in integers"""
    M = max(lw)
    E = [0 if w == -math.inf else int(mp.floor(mp.exp(mp.mpf(w - M)) * mp.mpf(2) ** ESCALE)) for w in lw]
    S0 = sum(E)
    Z = []
    for o in read.exprs:
        z = [Fraction(o.c0)] * n
        for name, comp, coef in o.terms:
            col = cols[name] if cols[name].ndim == 1 else cols[name][comp]
            # the operand's value as the code forms it: c0 + coef * x in doubles
            z = [Fraction(float(np.float64(o.c0) + np.float64(coef) * np.float64(x))) for x in col]
        Z.append([_as_int(v, ZSCALE) for v in z])
    means, dm = [], []
    for z in Z:
        S1 = sum(e * v for e, v in zip(E, z))
        A1 = sum(e * abs(v) for e, v in zip(E, z))
        means.append(Fraction(S1, S0) / (1 << ZSCALE))
        dm.append(2 * (n + 4) * Fraction(EPS) * Fraction(A1, S0) / (1 << ZSCALE) + (n + 2) * TINY_UNIT)
    if not read.cov:
        return means, dm, None, None
    d = len(Z)
    cov, dc = [[None] * d for _ in range(d)], [[None] * d for _ in range(d)]
    for a in range(d):
        ma = means[a] * (1 << ZSCALE)
        ca = [v - ma for v in Z[a]]
        for b in range(a, d):
            mb = means[b] * (1 << ZSCALE)
            cb = ca if b == a else [v - mb for v in Z[b]]
            S2 = sum(e * x * y for e, x, y in zip(E, ca, cb))
            A2 = sum(e * abs(x * y) for e, x, y in zip(E, ca, cb))
            cov[a][b] = cov[b][a] = S2 / S0 / (1 << (2 * ZSCALE))
            dc[a][b] = dc[b][a] = 2 * (n + 8) * Fraction(EPS) * A2 / S0 / (1 << (2 * ZSCALE)) + dm[a] * dm[b] + (n + 2) * TINY_UNIT
    return means, dm, cov, dc


@pytest.mark.parametrize("n", sorted(MOMENT_SIZES))
def test_moments_against_exact_rational_sums(n):
    runs = oracle_runs(n)
    outside = {}
    checked = 0
    for (vname, wname), res in runs.items():
        why = rd.moments_domain(vname, wname, n)
        if why:
            outside[(vname, wname)] = why
            continue
        cols, lw = rd.columns(vname, n), [float(w) for w in rd.weights(wname, n)]
        for read in rd.MOMENT_READS[:MOMENT_SIZES[n]]:
            (kind, (mean, cov)), _ = res[read.name]
            assert kind == "ok"
            means, dm, ecov, dc = exact_moments(cols, lw, read, n)
            for k, (m, d) in enumerate(zip(means, dm)):
                assert abs(Fraction(float(mean[k])) - m) <= d, (vname, wname, read.name, k, float(mean[k]), float(m), float(d))
            if ecov is not None:
                for a in range(len(means)):
                    for b in range(len(means)):
                        assert abs(Fraction(float(cov[a][b])) - ecov[a][b]) <= dc[a][b], \
                            (vname, wname, read.name, a, b, float(cov[a][b]), float(ecov[a][b]), float(dc[a][b]))
            checked += 1
    print(f"N = {n}: {checked} moment reads inside the reference's domain, {len(outside)} pairs outside it:",
          sorted(set(outside.values())))
    assert checked and (n < 2 or outside)
    for (vname, wname), why in outside.items():   # pinned on the device only; here: they answer, and not finitely
        (kind, (mean, _)), _ = runs[(vname, wname)]["moments[a]"]
        assert kind == "ok", (vname, wname)
        if rd.moments_domain("ordinary", wname, n):
            assert math.isnan(mean[0]), (vname, wname, mean)


# ---- ESS% and log-evidence ----------------------------------------------------------------------------------
def mp_ess_evidence(lw, n):
    if any(math.isnan(w) for w in lw) or max(lw) == math.inf or max(lw) == -math.inf:
        return None
    M = mp.mpf(max(lw))
    e = [mp.exp(mp.mpf(w) - M) if w != -math.inf else mp.mpf(0) for w in lw]
    s1, s2 = mp.fsum(e), mp.fsum(x * x for x in e)
    return s1 * s1 / (n * s2), M + mp.log(s1) - mp.log(n)


@pytest.mark.parametrize("n", CPU_SIZES)
def test_ess_and_log_evidence_against_mpmath(n):
    runs = oracle_runs(n)
    for wname in rd.weight_entries(n):
        res = runs[(rd.value_entries(n, wname)[0], wname)]
        (k1, ess), _ = res["ess"]
        (k2, ev), _ = res["log_evidence"]
        assert k1 == k2 == "ok"
        want = mp_ess_evidence([float(w) for w in rd.weights(wname, n)], n)
        if want is None:
            assert math.isnan(ess) and math.isnan(ev), (wname, ess, ev)
            continue
        e1 = float(abs(mp.mpf(ess) - want[0]) / want[0])
        e2 = float(abs(mp.mpf(ev) - want[1]) / max(abs(want[1]), 1))
        w = WORST.setdefault(wname, [0.0, 0.0])
        w[0], w[1] = max(w[0], e1), max(w[1], e2)
        assert e1 <= 1e-12 and e2 <= 1e-12, (wname, n, ess, ev, e1, e2)
    print(f"largest relative error up to N = {n} (ESS%, log-evidence):",
          {k: (f"{v[0]:.2e}", f"{v[1]:.2e}") for k, v in WORST.items()})


# ---- sampling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CPU_SIZES)
def test_samples_are_live_and_ordered(n):
    runs = oracle_runs(n)
    for wname in rd.weight_entries(n):
        vname = rd.value_entries(n, wname)[0]
        res = runs[(vname, wname)]
        s, _ = scaled(wname, n)
        live = np.array([v is not None and v >= 2 for v in s])      # surely q >= 1
        dead = np.array([v is None or v < 0.5 for v in s])          # surely q == 0
        cols = rd.columns(vname, n)
        ops = []
        for m in rd.sample_sizes(n):
            for replace in (True, False):
                oc, op = res[f"sample({m},replace={replace})+gather"]
                ops.append(op)
                if not live.any() and dead.all():
                    assert oc == ("err", abi.WSMC_ESTATE), (wname, oc)
                    continue
                assert oc[0] == "ok", (wname, oc)
                idx, ga, gv = oc[1]
                assert idx.shape == (m,) and ((0 <= idx) & (idx < n)).all()
                assert np.array_equal(ga.view(np.uint64), cols["a"][idx].view(np.uint64))
                assert np.array_equal(gv.view(np.uint64), cols["v3"][:, idx].view(np.uint64))
                if replace:
                    assert not dead[idx].any(), (wname, m)
                else:
                    assert len(set(idx.tolist())) == m, (wname, m)
                    first_dead = np.flatnonzero(dead[idx])
                    if len(first_dead):   # a dead particle is drawn only once every live one has been
                        assert live[idx[:first_dead[0]]].sum() == live.sum(), (wname, m)
        # one op counter per draw, the Q == 0 refusals included; none for the argument refusals
        assert ops == list(range(ops[0], ops[0] + len(ops))), (wname, ops)
        assert res["sample(N+1,replace=False)"] == (("err", abi.WSMC_EARG), ops[-1])
        assert res["sample(0)"] == (("err", abi.WSMC_EARG), ops[-1])
        assert res["sample(-3)"] == (("err", abi.WSMC_EARG), ops[-1])


# ---- coverage -------------------------------------------------------------------------------------------------
def test_the_corpus_covers_every_axis():
    vk, wk, pl, sc, rk = set(), set(), set(), set(), set()
    for n in rd.SIZES:
        sc.add(rd.size_class(n))
        for w in rd.weight_entries(n):
            wk.add(w.partition("@")[0])
            for v in rd.value_entries(n, w):
                vk.add(v.partition("@")[0])
                if "@" in v:
                    pl.add(v.partition("@")[2])
        rk |= {r.kind for r in rd.reads(n)}
    small = {v.partition("@")[0] for n in rd.SIZES if n < rd.LARGE for v in rd.value_entries(n)}
    assert small == set(rd.VALUE_KINDS) and vk == small
    assert wk == set(rd.WEIGHT_KINDS)
    assert pl == {"0", "last", "1023", "1024", "2047", "2048"}
    assert sc == {"wave", "block", "rs_tile", "canon_tile", "slots_wrap", "hist_stride", "k_drop", "max_stride"}
    assert rk == set(rd.READ_KINDS)
    assert set(rd.LAZY_SIZES) <= set(rd.SIZES) and set(CPU_SIZES) <= set(rd.SIZES)
    # every refusal path, met on the oracle
    res = oracle_runs(65)[("ordinary", "all_neg_inf")]
    for name in ("median(a)", "histogram(a)", "sample(1,replace=True)+gather", "sample(65,replace=False)+gather"):
        assert res[name][0] == ("err", abi.WSMC_ESTATE), name
    assert res["sample(N+1,replace=False)"][0] == ("err", abi.WSMC_EARG)
    assert res["sample(0)"][0] == ("err", abi.WSMC_EARG)
    assert res["sample(-3)"][0] == ("err", abi.WSMC_EARG)
    # the two values that answer before the weights are looked at
    assert oracle_runs(65)[("all_equal", "all_neg_inf")]["histogram(a)"][0][0] == "ok"
    assert math.isnan(oracle_runs(65)[("one_nan@0", "all_neg_inf")]["median(a)"][0][1])
    # median_tie: 2 S_k == Q + q1 exactly at some k
    for n in (1, 65, 2049):
        q = sorted(x for x in q_variants("median_tie", n)[0] if x)
        assert any(2 * sum(q[:k]) == sum(q) + q[0] for k in range(1, len(q) + 1)), n
    # q_boundary reaches q = 0, 1 and 2; expw_cut straddles -80; ref_straddle_up moves the reference point
    q = q_variants("q_boundary", 2049)[0]
    assert {0, 1, 2} <= set(q), sorted(set(q))[:5]
    w = rd.weights("expw_cut", 2049)
    assert (w < -80.0).any() and (w == -80.0).any() and ((w > -80.0) & (w < -79.0)).any()
    assert ref_point(list(rd.weights("ref_straddle", 65)))[1] == 3.0
    assert ref_point(list(rd.weights("ref_straddle_up", 65)))[1] == 4.0


def test_the_lazy_stale_state_runs_on_the_oracle():
    """the oracle is eager: the state is the Weight's and the Resample's effect (flat weights, the
    ancestors' values); the reads leave it unchanged"""
    o = Oracle(65, seed=1)
    rd.prepare(o)
    rd.load(o, rd.columns("ordinary", 65), rd.weights("gaussian", 65), "lazy_stale")
    st = o.get_state()
    assert st["resampled"] == 1 and st["n_resamples"] == 1
    before = rd.snapshot(o)
    res = rd.run_reads(o, 65)
    after = rd.snapshot(o)
    import progfuzz as pf
    assert pf.same_value(list(before), list(after))
    assert dict((r.name, oc) for r, oc, _ in res)["ess"] == ("ok", 1.0)
    o.close()


def test_the_gpu_cells_cover_the_corpus():
    """the parametrisation of tests/test_gpu_read_edges.py: every size, every weight kind fresh, the
    lazy sizes, the three splits in both modes, and only value entries the corpus has"""
    import test_gpu_read_edges as tg
    assert {n for n, _, _ in tg.CELLS} | {n for n, _, _ in tg.BIG_CELLS} == set(rd.SIZES)
    assert {w for _, w, s in tg.CELLS if s == "fresh"} == set(rd.WEIGHT_KINDS)
    assert {(n, w) for n, w, s in tg.CELLS if s == "lazy_stale"} == {(n, w) for n in rd.LAZY_SIZES for w in rd.WEIGHT_KINDS}
    assert all(v.partition("@")[0] in rd.VALUE_KINDS for v in tg.SHARD_VALUES)
    assert {(n, k, m) for n, k, m, _ in tg.SHARD_CELLS} == {(n, k, m) for n, k in tg.SPLITS for m in ("island", "exact")}
    assert tg.SPLITS == [(2049, 2), (4099, 3), (4, 3)]

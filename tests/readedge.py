"""Directed inputs for the calls that read the state: the corpus, the read list and the comparison.

TEST INFRASTRUCTURE, the companion of tests/mathedge.py for the reductions a user sees through
`describe(state)`, `@E`, `sample(state, n)` and the diversity gate: wsmc_col_minmax,
wsmc_weighted_median, wsmc_histogram, wsmc_weighted_moments, wsmc_ess, wsmc_log_evidence,
wsmc_marginal_diversity, wsmc_sample_particles and wsmc_col_gather_rows. Nothing here is sampled
for coverage: each axis is a list of named entries, and the one RNG (`default_rng([SEED, k])`)
draws only the ordinary filler values.

    VALUES    what the scalar column `a` holds (component 1 of the dim-3 column `v3` holds the same
              values, so `comp` and the `comp * N` offset are read too; `b` is an ordinary column).
              A kind with one special value stands once per placement: `one_nan@0`, `one_nan@last`,
              `one_nan@1023`, ... (index 0, N - 1, the last index of a tile and the first of the next)
    WEIGHTS   the log-weights
    SIZES     the smallest N at which each structure changes; the sizes from 16385 on take the
              reduced cross LARGE_WEIGHTS x LARGE_VALUES
    STATES    `fresh` (the inputs uploaded) and `lazy_stale` (a constant Weight and an unwaited
              Resample on the lazy store before the reads: the columns are behind the log and the
              weight reset is pending), the latter at LAZY_SIZES only
    READS     the fixed list `reads(n)` every (values, weights) pair runs

`run_cell` issues the list on anything with the wsmc.Context / oracle.Oracle interface and returns
each read's outcome with the op counter after it; `compare` reports the first read at which two
runs differ: floats by bit pattern (a NaN equals any NaN, -0.0 differs from 0.0), integers and
arrays exactly, an error only against the same status. tests/test_read_edges.py holds the oracle to
an independent restatement; tests/test_gpu_read_edges.py holds the device to the oracle.

    python tests/readedge.py --values neg_zero --weights one_live --n 2049 --state fresh --backend oracle
    python tests/readedge.py --values one_nan@last --weights gaussian --n 4099 --backend hip --shards 3 --mode exact

print the reads' outcomes (oracle), or the first differing read with both bit patterns (hip).
"""
from __future__ import annotations

import argparse
import math
import sys
from dataclasses import dataclass

import numpy as np

import progfuzz as pf   # (puts the package and the oracle on sys.path)
from progfuzz import Opnd

from wsmc import abi  # noqa: E402

SEED = 4409                      # the ordinary values: default_rng([SEED, k])
INF, NAN = math.inf, math.nan
LN2 = 0.6931471805599453
UP1 = float(np.nextafter(1.0, 2.0))

SIZES = (1, 2, 63, 64, 65, 255, 256, 257,     # wave and block
         1023, 1024, 1025,                    # resample tile
         2047, 2048, 2049, 4097,              # canonical tile of 2048
         16385,                               # the 64 max slots wrap
         524289,                              # k_hist starts to stride
         1048577,                             # K drops from 43 to 42
         2097153)                             # k_rs_max starts to stride
LARGE = 16385                                 # from here on: the reduced cross
LAZY_SIZES = (65, 1025, 2049)
STATES = ("fresh", "lazy_stale")
TILE_EDGES = (1023, 1024, 2047, 2048)


def size_class(n) -> str:
    for name, hi in (("wave", 65), ("block", 257), ("rs_tile", 1025), ("canon_tile", 4097), ("slots_wrap", 16385),
                     ("hist_stride", 524289), ("k_drop", 1048577)):
        if n <= hi:
            return name
    return "max_stride"


def qbits(n) -> int:
    """K = min(63 - ceil(log2 n), 43) (include/wsmc_math.h wsmc_qbits)"""
    return min(63 if n <= 1 else 63 - (n - 1).bit_length(), 43)


def _rng(k):
    return np.random.default_rng([SEED, int(k)])


def ordinary(n, k):
    return _rng(k).normal(0.0, 2.0, n)


# ---- value kinds ----------------------------------------------------------------------------------------
# name -> (f(n, at), placed): `placed` kinds hold one special value at index `at`
def _v_all_equal_but_one(n, at):
    a = np.full(n, 2.5)
    a[at] = -1.25
    return a


def _v_two_values(n, at):
    a = np.where(_rng(11).random(n) < 0.4, -1.5, 3.0)
    a[0], a[-1] = -1.5, 3.0
    return a


def _v_neg_zero(n, at):
    a = np.where(_rng(12).random(n) < 0.5, 0.0, -0.0)
    a[0], a[-1] = 0.0, -0.0
    return a


def _v_zero_among(n, at):
    a = ordinary(n, 13)
    a[0::5] = 0.0
    a[1::7] = -0.0
    return a


def _v_point(special, k):
    def f(n, at):
        a = ordinary(n, k)
        a[at] = special
        return a
    return f


def _v_both_inf(n, at):
    a = ordinary(n, 17)
    a[at] = INF
    if n > 1:
        a[at + 1 if at + 1 < n else at - 1] = -INF
    return a


def _v_adjacent(n, at):
    a = np.full(n, 1.0)
    a[1::2] = UP1
    return a


ON_EDGES = [x for k in range(9) for x in (float(k), float(np.nextafter(float(k), -INF)), float(np.nextafter(float(k), INF)))]


def _v_on_edges(n, at):
    """lo = 0, hi = 8: the values exactly at lo + k (hi - lo) / 8 and their neighbours inside [0, 8]"""
    pts = np.asarray([x for x in ON_EDGES if 0.0 <= x <= 8.0])
    a = pts[_rng(18).integers(0, len(pts), n)]
    a[:min(n, len(pts))] = pts[_rng(19).permutation(len(pts))][:min(n, len(pts))]
    a[0], a[-1] = 0.0, 8.0
    return a


def _levels(n, k, pts):
    """`pts` drawn at random, the first at index 0 and the last at N - 1"""
    a = np.asarray(pts)[_rng(k).integers(0, len(pts), n)]
    a[0], a[-1] = pts[0], pts[-1]
    return a


def _v_ties_by_weight(n, at):
    return np.round(ordinary(n, 22))


VALUE_KINDS = {
    "ordinary": (lambda n, at: ordinary(n, 10), False),
    "all_equal": (lambda n, at: np.full(n, 2.5), False),
    "all_equal_but_one": (_v_all_equal_but_one, True),
    "two_values": (_v_two_values, False),
    "neg_zero": (_v_neg_zero, False),
    "zero_among": (_v_zero_among, False),
    "one_nan": (_v_point(NAN, 14), True),
    "pos_inf": (_v_point(INF, 15), True),
    "neg_inf": (_v_point(-INF, 16), True),
    "both_inf": (_v_both_inf, True),
    "adjacent": (_v_adjacent, False),
    "on_edges": (_v_on_edges, False),
    "subnormal": (lambda n, at: 5e-324 * _rng(20).integers(-50, 51, n), False),
    "huge": (lambda n, at: 1.4e308 * _rng(21).uniform(-1.0, 1.0, n), False),
    # finite extremes whose hi - lo overflows, and whose k (hi - lo) does while hi - lo does not
    "range_overflow": (lambda n, at: _levels(n, 25, (-1.5e308, -7.5e307, -1e300, 0.0, 3.0, 7.5e307, 1.5e308)), False),
    "range_over_seventh": (lambda n, at: _levels(n, 26, (0.0, 1e307, 2.4e307, 2.6e307, 5e307, 9.9e307, 1e308)), False),
    "offset": (lambda n, at: 1e15 + _rng(23).integers(0, 65, n).astype(float), False),
    "sorted": (lambda n, at: np.sort(ordinary(n, 24)), False),
    "reversed": (lambda n, at: np.sort(ordinary(n, 24))[::-1].copy(), False),
    "ties_by_weight": (_v_ties_by_weight, False),
}
LARGE_VALUES = ("ordinary", "neg_zero", "one_nan@last", "on_edges", "ties_by_weight")


def placements(n):
    """{label: index} of a special value: 0, N - 1, and both sides of the tile edges N reaches"""
    out = {"0": 0}
    for i in TILE_EDGES:
        if i < n - 1:
            out[str(i)] = i
    if n > 1:
        out["last"] = n - 1
    return out


REFUSED_VALUES = ("ordinary", "all_equal", "neg_zero", "one_nan@0")


def value_entries(n, wname=None):
    """the names of the value entries at size n, placed kinds once per placement. Two reduced
    crosses: LARGE_VALUES from N = 16385 on, and REFUSED_VALUES under a weight kind whose weights do
    not normalise (median, histogram and sample refuse there whatever the values are; `all_equal`
    and `one_nan` are the two values that answer before the weights are looked at)"""
    if n >= LARGE:
        return list(LARGE_VALUES)
    if wname is not None and wname.partition("@")[0] in NO_ANSWER:
        return list(REFUSED_VALUES)
    out = []
    for kind, (_, placed) in VALUE_KINDS.items():
        out += [f"{kind}@{p}" for p in placements(n)] if placed else [kind]
    return out


def _at(where, n):
    return n - 1 if where == "last" else min(int(where), n - 1)


def values(name, n):
    """the scalar column `a` of a value entry"""
    kind, _, where = name.partition("@")
    f, placed = VALUE_KINDS[kind]
    a = np.ascontiguousarray(f(n, _at(where or "0", n) if placed else 0), dtype=np.float64)
    assert a.shape == (n,)
    return a


def columns(name, n):
    """{column: values}: a, v3 (component 1 is a) and the ordinary b"""
    a = values(name, n)
    return {"a": a, "v3": np.stack([ordinary(n, 30), a, ordinary(n, 31)]), "b": ordinary(n, 32)}


# ---- weight kinds ---------------------------------------------------------------------------------------
def _gauss(n, k=40):
    return -0.5 * _rng(k).standard_normal(n) ** 2


def _w_one_live(n, at):
    w = np.full(n, -INF)
    w[at] = 0.0
    return w


def _w_half_dead(n, at):
    w = _gauss(n, 41)
    w[1::2] = -INF
    return w


def _w_point(special, k):
    def f(n, at):
        w = _gauss(n, k)
        w[at] = special
        return w
    return f


def _bulk(n, k):
    """weights in [-4, 0) with the max 0.0 exactly at index 0 (so the reference point is 0)"""
    w = np.maximum(_gauss(n, k), -4.0) - 2.0 ** -20
    w[0] = 0.0
    return w


def _sprinkle(w, pts, k):
    """`pts` at fixed pseudo-random places other than index 0, as many as fit beside a bulk of 7"""
    n = len(w)
    m = min(len(pts), max(0, n - 7))
    if m:
        w[1 + _rng(k).permutation(n - 1)[:m]] = pts[:m]
    return w


def _nb(v, k=2):
    out, lo, hi = [float(v)], float(v), float(v)
    for _ in range(k):
        lo, hi = float(np.nextafter(lo, -INF)), float(np.nextafter(hi, INF))
        out += [lo, hi]
    return out


def _w_q_boundary(n, at):
    """lw - ceil(M) at -K ln 2 (q = 1 or 0 by the rounding), -(K - 1) ln 2 (q = 2 or 1) and their
    neighbours, among a bulk that carries the sums"""
    K = qbits(n)
    return _sprinkle(_bulk(n, 43), _nb(-K * LN2) + _nb(-(K - 1) * LN2, 1) + [-(K + 1) * LN2], 44)


def _w_expw_cut(n, at):
    return _sprinkle(_bulk(n, 45), _nb(-80.0) + [-79.5, -80.5, -100.0, -745.0], 46)


def _w_ref_straddle(up):
    def f(n, at):
        w = _bulk(n, 47) + 3.0          # the max is 3.0 exactly: R = ceil(M) = 3
        if up:
            w[0] = float(np.nextafter(3.0, INF))   # one ulp above: R = 4
        return w
    return f


def _w_median_tie(n, at):
    """weights 0 or -inf with an odd number L of live particles: every q is 2^K, so 2 S_k == Q + q1
    exactly at k = (L + 1) / 2 and the walk's strict `>` decides"""
    w = np.zeros(n)
    w[1::3] = -INF
    if int(np.isfinite(w).sum()) % 2 == 0:
        w[np.flatnonzero(np.isfinite(w))[-1]] = -INF
    return w


# name -> (f(n, at), placed)
WEIGHT_KINDS = {
    "flat": (lambda n, at: np.zeros(n), False),
    "gaussian": (lambda n, at: _gauss(n), False),
    "one_live": (_w_one_live, True),
    "half_dead": (_w_half_dead, False),
    "all_neg_inf": (lambda n, at: np.full(n, -INF), False),
    "one_nan": (_w_point(NAN, 42), True),
    "one_pos_inf": (_w_point(INF, 42), True),
    "q_boundary": (_w_q_boundary, False),
    "expw_cut": (_w_expw_cut, False),
    "ref_straddle": (_w_ref_straddle(False), False),
    "ref_straddle_up": (_w_ref_straddle(True), False),
    "shifted_1e308": (lambda n, at: np.full(n, 1e308), False),
    "shifted_m1e300": (lambda n, at: np.full(n, -1e300), False),
    "median_tie": (_w_median_tie, False),
}
WEIGHT_NAMES = list(WEIGHT_KINDS)
LARGE_WEIGHTS = ("gaussian", "half_dead", "q_boundary")
NO_ANSWER = ("all_neg_inf", "one_nan", "one_pos_inf")   # Q == 0: median, histogram and sample refuse


def weight_entries(n):
    return list(LARGE_WEIGHTS) if n >= LARGE else list(WEIGHT_NAMES)


def weights(name, n):
    """the log-weights of a weight entry; a placed kind without a placement sits at n // 3"""
    kind, _, where = name.partition("@")
    f, placed = WEIGHT_KINDS[kind]
    w = np.ascontiguousarray(f(n, (_at(where, n) if where else n // 3) if placed else 0), dtype=np.float64)
    assert w.shape == (n,)
    return w


def live_on_rank(n, k, rank):
    """log-weights whose live particles (Gaussian log-weights) all sit on one rank of k"""
    w = np.full(n, -INF)
    lo, hi = (n * rank) // k, (n * (rank + 1)) // k
    w[lo:hi] = _gauss(hi - lo, 48)
    return w


# ---- the domain of the moments' reference ---------------------------------------------------------------
def moments_domain(vname, wname, n):
    """None where tests/test_read_edges.py holds the moments to exact rational sums, else why not
    (such a pair is pinned by "NaN / inf exactly as the oracle says" on the device only)"""
    vk, wk = vname.partition("@")[0], wname.partition("@")[0]
    if vk in ("one_nan", "pos_inf", "neg_inf", "both_inf"):
        return "a value is not finite"
    if vk in ("huge", "range_overflow", "range_over_seventh"):
        return "the sums of e z leave the double range"
    if wk in NO_ANSWER:
        return {"all_neg_inf": "no weight is finite: 0 / 0", "one_nan": "a NaN weight",
                "one_pos_inf": "a +inf weight: inf - inf"}[wk]
    return None


# ---- the reads --------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Read:
    name: str
    kind: str
    args: tuple = ()
    exprs: tuple = ()      # moments: progfuzz Opnds (progfuzz._moments_close reads them)
    cov: bool = False


_A = Opnd(0.0, (("a", 0, 1.0),))
MOMENT_READS = (
    Read("moments[a]", "moments", exprs=(_A,), cov=True),
    Read("moments[a,2v3[1]+1,v3[0],a]+cov", "moments",
         exprs=(_A, Opnd(1.0, (("v3", 1, 2.0),)), Opnd(0.0, (("v3", 0, 1.0),)), _A), cov=True),
    Read("moments[a,v3[2]]", "moments", exprs=(_A, Opnd(0.0, (("v3", 2, 1.0),))), cov=False),
)


def sample_sizes(n):
    return sorted({1, min(n, 7), n})


def reads(n):
    """the fixed list every (values, weights) pair runs, in order"""
    out = [Read("minmax(a)", "minmax", ("a", 0)), Read("minmax(v3[1])", "minmax", ("v3", 1)),
           Read("median(a)", "median", ("a", 0)), Read("median(v3[1])", "median", ("v3", 1)),
           Read("histogram(a)", "histogram", ("a", 0)), Read("histogram(v3[1])", "histogram", ("v3", 1))]
    out += list(MOMENT_READS)
    out += [Read("ess", "ess"), Read("log_evidence", "log_evidence"),
            Read("diversity[a]", "diversity", (("a",),)), Read("diversity[a,b]", "diversity", (("a", "b"),))]
    for m in sample_sizes(n):
        for replace in (True, False):
            out.append(Read(f"sample({m},replace={replace})+gather", "sample", (m, replace)))
    # the argument refusals (decided on the host before the op counter is taken)
    out += [Read("sample(N+1,replace=False)", "sample", (n + 1, False)), Read("sample(0)", "sample", (0, True)),
            Read("sample(-3)", "sample", (-3, False))]
    return out


READ_KINDS = ("minmax", "median", "histogram", "moments", "ess", "log_evidence", "diversity", "sample")


def _do(ctx, r: Read):
    R = ctx.col_find
    if r.kind == "minmax":
        return ctx.col_minmax(R(r.args[0]), r.args[1])
    if r.kind == "median":
        return ctx.weighted_median(R(r.args[0]), r.args[1])
    if r.kind == "histogram":
        return ctx.histogram(R(r.args[0]), r.args[1])
    if r.kind == "moments":
        return ctx.weighted_moments([pf.mk_opnd(ctx, o) for o in r.exprs], want_cov=r.cov)
    if r.kind == "ess":
        return ctx.ess()
    if r.kind == "log_evidence":
        return ctx.log_evidence()
    if r.kind == "diversity":
        return ctx.marginal_diversity([R(c) for c in r.args[0]])
    if r.kind == "sample":
        idx = ctx.sample_particles(r.args[0], r.args[1])
        return idx, ctx.col_gather_rows(R("a"), idx), ctx.col_gather_rows(R("v3"), idx)
    raise ValueError(r.kind)


def outcome(ctx, r: Read):
    """("ok", value) or ("err", status), progfuzz's normalisation"""
    try:
        return ("ok", _do(ctx, r))
    except (np.linalg.LinAlgError, abi.WSMCError, RuntimeError, ValueError) as e:
        return ("err", pf._code(e))


# ---- a cell on a backend ----------------------------------------------------------------------------------
def prepare(ctx):
    """the three columns of a context (created once; every cell uploads into them)"""
    for name, dim in (("a", 1), ("v3", 3), ("b", 1)):
        if ctx.col_find(name) < 0:
            ctx.col_create(name, dim)


def load(ctx, cols, lw, state="fresh"):
    """a cell's inputs, brought to `state`"""
    for name, v in cols.items():
        ctx.col_upload(ctx.col_find(name), v)
    ctx.weights_upload(lw)
    if state == "lazy_stale":
        if hasattr(ctx, "store_set_lazy"):
            ctx.store_set_lazy(True)
        d = pf.mk_dist(ctx, pf.DistSpec(abi.FAM_NORMAL, 1, (Opnd(0.0, ()),), Opnd(1.0, ())))
        ctx.weight(d, [pf.mk_opnd(ctx, Opnd(0.3, ()))])
        ctx.resample(2.0, abi.RESAMPLE_STRATIFIED, wait=False)


def run_reads(ctx, n):
    """[(read, outcome, the op counter after it)]"""
    out = []
    for r in reads(n):
        oc = outcome(ctx, r)
        out.append((r, oc, ctx.get_state()["op_counter"]))
    return out


def snapshot(ctx):
    st = {k: v for k, v in ctx.get_state().items() if k != "op_counter"}
    return st, ctx.weights_download(), {c: ctx.col_download(ctx.col_find(c)) for c in ctx.col_names()}


def run_cell(ctx, vname, wname, n, state="fresh", lw=None):
    """one (values, weights) pair on a prepared context: the reads' outcomes"""
    load(ctx, columns(vname, n), weights(wname, n) if lw is None else lw, state)
    return run_reads(ctx, n)


def _fmt(v):
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_fmt(x) for x in v) + ")"
    if v is None:
        return "None"
    a = np.asarray(v)
    if a.dtype.kind == "f":
        f = a.astype(np.float64).ravel()
        s = ", ".join(f"{x!r} (0x{b:016x})" for x, b in zip(f[:6].tolist(), f[:6].view(np.uint64).tolist()))
        return f"[{s}{', ...' if f.size > 6 else ''}]"
    f = a.ravel()
    return f"{f[:12].tolist()}{'...' if f.size > 12 else ''}"


def _first_diff(a, b):
    """the first differing leaf of two ok values, both formatted"""
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b):
        for x, y in zip(a, b):
            if not pf.same_value(x, y):
                return _first_diff(x, y)
    if a is None or b is None:
        return f"{_fmt(a)} != {_fmt(b)}"
    x, y = np.asarray(a), np.asarray(b)
    if x.shape == y.shape and x.size > 1:
        fx, fy = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
        bad = np.flatnonzero(~((fx.view(np.uint64) == fy.view(np.uint64)) | (np.isnan(fx) & np.isnan(fy))))
        if len(bad):
            i = int(bad[0])
            return f"{len(bad)} of {x.size} differ, first at {i}: {_fmt(x.ravel()[i])} != {_fmt(y.ravel()[i])}"
    return f"{_fmt(a)} != {_fmt(b)}"


def moments_close(o, r: Read, got, want) -> bool:
    """sharded moments (the shards' sums are combined in rank order, the oracle sums once): the same
    bits, or progfuzz._moments_close's any-order bound"""
    return pf.same_value(got, want) or pf._moments_close(o, r, got, want)


def compare(got, want, o=None, sharded=False):
    """None, or the first read at which `got` differs from `want` (the oracle's run): the outcome,
    then the op counter after it. sharded: weighted_moments is held to moments_close on `o`."""
    if len(got) != len(want):
        return f"{len(got)} reads against {len(want)}"
    for (r, go, gop), (_, wo, wop) in zip(got, want):
        if go[0] != wo[0]:
            return f"{r.name}: {go[0]} {_fmt(go[1]) if go[0] == 'ok' else go[1]} != the oracle's {wo[0]} " \
                   f"{_fmt(wo[1]) if wo[0] == 'ok' else wo[1]}"
        if go[0] == "err":
            if go[1] != wo[1]:
                return f"{r.name}: status {go[1]} != the oracle's {wo[1]}"
        else:
            same = moments_close(o, r, go[1], wo[1]) if (sharded and r.kind == "moments") else pf.same_value(go[1], wo[1])
            if not same:
                return f"{r.name}: {_first_diff(go[1], wo[1])}"
        if gop != wop:
            return f"{r.name}: op counter {gop} after it != the oracle's {wop}"
    return None


def differential(g, o, vname, wname, n, state="fresh", sharded=False, lw=None):
    """one cell on `g` and on the oracle `o` (both prepared): None, or what differs first. The
    oracle's state, weights and columns must be what they were before the reads (the op counter
    aside), and `g` must hold the same afterwards (progfuzz.compare)."""
    want_lw = weights(wname, n) if lw is None else lw
    cols = columns(vname, n)
    load(o, cols, want_lw, state)
    load(g, cols, want_lw, state)
    before = snapshot(o)
    want = run_reads(o, n)
    got = run_reads(g, n)
    d = compare(got, want, o, sharded)
    if d:
        return d
    after = snapshot(o)
    if not pf.same_value(list(before), list(after)):
        return "the reads changed the oracle's state, weights or columns"
    if hasattr(g, "sync"):
        g.sync()
    d = pf.compare(g, o)
    return f"after the reads: {d}" if d else None


def replay(vname, wname, n, state="fresh", shards=1, mode="island") -> str:
    return (f"python tests/readedge.py --values {vname} --weights {wname} --n {n} --state {state} --backend hip"
            + (f" --shards {shards} --mode {mode}" if shards > 1 else ""))


# ---- command line -----------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--values", required=True, help="a value entry, e.g. neg_zero or one_nan@1023")
    ap.add_argument("--weights", required=True, help="a weight entry, e.g. one_live or one_live@0")
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--state", choices=STATES, default="fresh")
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    ap.add_argument("--shards", type=int, default=1)
    ap.add_argument("--mode", choices=("island", "exact"), default="island")
    a = ap.parse_args(argv)
    from oracle import Oracle
    exact = a.mode == "exact"
    o = Oracle(a.n, seed=1, shards=a.shards, exact=exact) if a.shards > 1 else Oracle(a.n, seed=1)
    prepare(o)
    if a.backend == "oracle":
        for r, oc, op in run_cell(o, a.values, a.weights, a.n, a.state):
            print(f"{r.name:40s} {oc[0]} {_fmt(oc[1]) if oc[0] == 'ok' else oc[1]}  op={op}")
        return 0
    import wsmc
    if a.shards > 1:
        g = wsmc.Context.multi(a.n, a.shards, seed=1, devices=[0] * a.shards, transport=abi.TRANSPORT_HOST)
        if exact:
            g.comm_set_shard_mode(abi.SHARD_EXACT)
    else:
        g = wsmc.Context(a.n, seed=1)
    prepare(g)
    d = differential(g, o, a.values, a.weights, a.n, a.state, sharded=a.shards > 1)
    g.close()
    print("MISMATCH " + d if d else f"{a.values} x {a.weights} at N = {a.n} ({a.state}): the device and the oracle agree")
    return 1 if d else 0


if __name__ == "__main__":
    sys.exit(main())

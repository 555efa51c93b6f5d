"""Seeded random statement programs over the context protocol: generator, executor, comparer.

TEST INFRASTRUCTURE. A program is a list of `Stmt` (plain data, built from
``numpy.random.default_rng(seed)`` and nothing else: no context, no device). `run` issues one on
anything with the `wsmc.Context` / `oracle.Oracle` interface; `differential` issues the same list
on two of them in lockstep, the oracle first, and reports the first statement at which they
differ. The oracle is eager (no statement batches, no lazy store, no deferred state), so its
answer does not depend on how the device is driven: the `MODES` below change the device's waits
and reads only.

    python tests/progfuzz.py --seed 3 --profile mixed --mode chatty --n 1001 --backend oracle

prints the program and runs it (on `--backend hip` against the oracle, comparing as the mode says).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import pathlib
import re
import sys
from dataclasses import dataclass, field

import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]
for _p in (REPO / "weightedsampling.jl_amd", REPO / "oracle"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

from wsmc import abi, dsl  # noqa: E402  (pure Python: the library loads at the first call)

# ---- the corpus: the seed lists the GPU file runs and the CPU file checks ----------------------
MIXED_SEEDS = list(range(18))
MOVES_SEEDS = list(range(12))
CAPS_NAMES = ["kEwOps", "kEwSlots", "kEwRows", "kEwPre", "ntab4", "lagged_write", "anc_row", "seventh_lagged"]
CAPS_SEEDS = list(range(len(CAPS_NAMES)))          # caps seed k -> program CAPS_NAMES[k % 8]
EDGE_NAMES = ["degenerate"]
EDGE_SEEDS = list(range(len(EDGE_NAMES)))
PROFILES = ("mixed", "caps", "moves", "edge")
SIZES = (1, 65, 1001, 5002)
MAX_STATEMENTS = 32                                 # reads not counted

FAMILIES = {
    abi.FAM_NORMAL: "Normal", abi.FAM_HALFNORMAL: "HalfNormal", abi.FAM_UNIFORM: "Uniform",
    abi.FAM_MVNORMAL_ISO: "MvNormalIso", abi.FAM_MVNORMAL: "MvNormal", abi.FAM_BERNOULLI: "Bernoulli",
    abi.FAM_BERNOULLI_LOGIT: "BernoulliLogit", abi.FAM_EXPONENTIAL: "Exponential", abi.FAM_LOGNORMAL: "LogNormal",
    abi.FAM_LAPLACE: "Laplace", abi.FAM_CAUCHY: "Cauchy", abi.FAM_LOGISTIC: "Logistic", abi.FAM_GUMBEL: "Gumbel",
    abi.FAM_RAYLEIGH: "Rayleigh", abi.FAM_GEOMETRIC: "Geometric", abi.FAM_GAMMA: "Gamma",
    abi.FAM_INVERSEGAMMA: "InverseGamma", abi.FAM_CHISQ: "Chisq", abi.FAM_BETA: "Beta", abi.FAM_TDIST: "TDist",
    abi.FAM_POISSON: "Poisson", abi.FAM_BINOMIAL: "Binomial", abi.FAM_NEGBINOMIAL: "NegativeBinomial",
}
VECTOR_FAMILIES = (abi.FAM_MVNORMAL_ISO, abi.FAM_MVNORMAL)
SCHEMES = (abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL)
XOPS1 = (abi.X_NEG, abi.X_ABS, abi.X_SQRT, abi.X_EXP, abi.X_LOG, abi.X_LOG1P, abi.X_SIN, abi.X_COS, abi.X_NOT)
XOPS2 = (abi.X_ADD, abi.X_SUB, abi.X_MUL, abi.X_DIV, abi.X_MIN, abi.X_MAX, abi.X_POW, abi.X_LT, abi.X_LE, abi.X_GT,
         abi.X_GE, abi.X_EQ, abi.X_NE, abi.X_AND, abi.X_OR)
XOPS_ALL = (abi.X_CONST, abi.X_COL, abi.X_POWI, abi.X_IFELSE) + XOPS1 + XOPS2
XNAMES = {v: k[2:].lower() for k, v in vars(abi).items() if k.startswith("X_") and k not in ("X_CONST", "X_COL")
          and isinstance(v, int) and k not in ("XPROG_MAX", "XSTACK_MAX")}
READ_KINDS = ("download", "weights", "log_evidence", "ess", "state", "moments", "minmax", "median", "histogram",
              "score", "score_all", "diversity", "ancestors")
OPERAND_FORMS = ("const", "col", "col2", "comp")

# what a mode changes on the device; the oracle's answer is the same for all
MODES = {
    "chatty": dict(waits="all", reads=True, step_compare=True),     # locates a fault
    "quiet": dict(waits="none", reads=False, step_compare=False),   # batches grow to their caps
    "reads": dict(waits="prog", reads=True, step_compare=False),    # the program's own reads and waits
}
_ORACLE_MODE = dict(waits="all", reads=True, step_compare=False)


# ---- programs are data ------------------------------------------------------------------------
@dataclass(frozen=True)
class Opnd:
    """c0 + sum coef * column[comp] over at most two terms (wsmc_operand)"""
    c0: float = 0.0
    terms: tuple = ()   # ((name, comp, coef), ...)

    @property
    def form(self) -> str:
        if not self.terms:
            return "const"
        if any(c > 0 or v for (_, c, _), v in zip(self.terms, self._vec)):
            return "comp"
        return "col2" if len(self.terms) == 2 else "col"

    _vec: tuple = field(default=(False, False), compare=False, repr=False)

    def __repr__(self):
        s = []
        if self.c0 != 0.0 or not self.terms:
            s.append(repr(self.c0))
        for (n, c, k), v in zip(self.terms, self._vec):
            x = f"{n}[{c}]" if (c or v) else n
            s.append(x if k == 1.0 else f"{k!r}*{x}")
        return " + ".join(s)

    def cols(self):
        return [n for n, _, _ in self.terms]


@dataclass(frozen=True)
class DistSpec:
    fam: int
    dim: int
    mu: tuple           # Opnd per component (scalar families: the first parameter)
    scale: Opnd
    params: tuple = (0.0, 0.0)
    cov: tuple = ()     # FAM_MVNORMAL: row-major covariance

    def __repr__(self):
        a = ", ".join(repr(m) for m in self.mu)
        if self.fam == abi.FAM_UNIFORM:
            return f"Uniform({self.params[0]!r}, {self.params[1]!r})"
        if self.fam == abi.FAM_MVNORMAL:
            return f"MvNormal([{a}], cov={list(self.cov)})"
        return f"{FAMILIES[self.fam]}({'[' + a + ']' if self.dim > 1 else a}; {self.scale!r})"

    def cols(self):
        return [n for o in self.mu + (self.scale,) for n in o.cols()]


class Stmt:
    """one statement (or read) of a program: `op` and its arguments `a` (plain data)"""
    __slots__ = ("op", "a")

    def __init__(self, op, **a):
        self.op, self.a = op, a

    def __eq__(self, o):
        return isinstance(o, Stmt) and self.op == o.op and repr(self) == repr(o)

    def __hash__(self):
        return hash(repr(self))

    def __getattr__(self, k):
        try:
            return self.a[k]
        except KeyError:
            raise AttributeError(k)

    def __repr__(self):
        a, op = self.a, self.op
        new = lambda: f"{a['out']}" + (f"[{a['dim']}]" if a.get("dim", 1) > 1 else "")
        if op == "sample":
            return f"{new()} ~ {a['dist']!r}"
        if op == "importance":
            return f"{new()} ~ importance({a['prop']!r} -> {a['targ']!r})"
        if op in ("observe", "weight"):
            x = ", ".join(repr(o) for o in a["x"])
            return f"{x} {'=>' if op == 'observe' else '~w'} {a['dist']!r}"
        if op == "assign":
            return f"{new()} .= " + ", ".join(repr(o) for o in a["exprs"])
        if op == "assign_expr":
            return f"{new()} .= " + ", ".join(tree_repr(t) for t in a["trees"])
        if op == "move_block":
            return f"move_block(gated={a['gated']}, wait={a['wait']}, [" + "; ".join(
                f"{'autoRW' if m[0] else 'RW'} {list(m[1])} step={m[2]!r} lo={m[3]} hi={m[4]}" for m in a["moves"]) + "])"
        return f"{op}(" + ", ".join(f"{k}={v!r}" for k, v in a.items()) + ")"


def tree_repr(t) -> str:
    if t[0] == "c":
        return repr(t[1])
    if t[0] == "col":
        return f"{t[1]}[{t[2]}]" if t[2] else t[1]
    if t[0] == abi.X_POWI:
        return f"({tree_repr(t[2])})^{t[1]}"
    return f"{XNAMES[t[0]]}(" + ", ".join(tree_repr(x) for x in t[1:]) + ")"


def tree_ops(t, out=None):
    """the WSMC_X_* opcodes of a tree"""
    out = set() if out is None else out
    if t[0] == "c":
        out.add(abi.X_CONST)
    elif t[0] == "col":
        out.add(abi.X_COL)
    else:
        out.add(t[0])
        for x in (t[2:] if t[0] == abi.X_POWI else t[1:]):
            tree_ops(x, out)
    return out


def tree_cols(t, out=None):
    out = [] if out is None else out
    if t[0] == "col":
        out.append(t[1])
    elif t[0] != "c":
        for x in (t[2:] if t[0] == abi.X_POWI else t[1:]):
            tree_cols(x, out)
    return out


def to_fx(t) -> dsl.Fx:
    if t[0] == "c":
        return dsl.Fx(abi.X_CONST, c=t[1])
    if t[0] == "col":
        return dsl.Fx(abi.X_COL, col=t[1], comp=t[2])
    if t[0] == abi.X_POWI:
        return dsl.Fx(abi.X_POWI, (to_fx(t[2]),), c=float(t[1]))
    return dsl.Fx(t[0], tuple(to_fx(x) for x in t[1:]))


def _tree_size(t) -> int:
    if t[0] in ("c", "col"):
        return 1
    return 1 + sum(_tree_size(x) for x in (t[2:] if t[0] == abi.X_POWI else t[1:]))


# ---- the generator ----------------------------------------------------------------------------
# column kinds: what a column's values are known to be, so that parameters stay inside each
# family's support. `wild` (a general expression's raw value: may be NaN or infinite) is read by
# Assigns and downloads only; `heavy` marks heavy-tailed values, never used as a parameter.
_POSLIKE = ("pos", "prob")
_COUNTLIKE = ("count", "bit")
# family -> (first parameter, second parameter, output kind, continuous, heavy)
_FAM = {
    abi.FAM_NORMAL: ("real", "pos", "real", True, False),
    abi.FAM_HALFNORMAL: (None, "pos", "pos", True, False),
    abi.FAM_UNIFORM: (None, None, "real", True, False),
    abi.FAM_BERNOULLI: ("prob", None, "bit", False, False),
    abi.FAM_BERNOULLI_LOGIT: ("real", None, "bit", False, False),
    abi.FAM_EXPONENTIAL: (None, "pos", "pos", True, False),
    abi.FAM_LOGNORMAL: ("small", "small_pos", "pos", True, True),
    abi.FAM_LAPLACE: ("real", "pos", "real", True, False),
    abi.FAM_CAUCHY: ("real", "pos", "real", True, True),
    abi.FAM_LOGISTIC: ("real", "pos", "real", True, False),
    abi.FAM_GUMBEL: ("real", "pos", "real", True, False),
    abi.FAM_RAYLEIGH: (None, "pos", "pos", True, False),
    abi.FAM_GEOMETRIC: ("prob", None, "count", False, False),
    abi.FAM_GAMMA: ("shape", "pos", "pos", True, False),
    abi.FAM_INVERSEGAMMA: ("shape", "pos", "pos", True, True),
    abi.FAM_CHISQ: ("shape", None, "pos", True, False),
    abi.FAM_BETA: ("shape", "shape", "prob", True, False),
    abi.FAM_TDIST: ("shape", None, "real", True, True),
    abi.FAM_POISSON: ("shape", None, "count", False, False),
    abi.FAM_BINOMIAL: ("nint", "prob", "count", False, False),
    abi.FAM_NEGBINOMIAL: ("shape", "prob", "count", False, False),
}
_IMPORTANCE = {   # proposal / target families of one kind
    "real": (abi.FAM_NORMAL, abi.FAM_LAPLACE, abi.FAM_LOGISTIC, abi.FAM_GUMBEL, abi.FAM_CAUCHY, abi.FAM_TDIST),
    "pos": (abi.FAM_EXPONENTIAL, abi.FAM_GAMMA, abi.FAM_HALFNORMAL, abi.FAM_RAYLEIGH, abi.FAM_CHISQ),
    "prob": (abi.FAM_BETA, abi.FAM_UNIFORM),
    "count": (abi.FAM_POISSON, abi.FAM_GEOMETRIC, abi.FAM_NEGBINOMIAL),
}
_COEFS = (1.0, -1.0, 0.5, -0.5, 0.25, 2.0, 0.7, -1.3)
_COVS = {2: (1.0, 0.3, 0.3, 2.0), 3: (1.5, 0.2, -0.1, 0.2, 1.0, 0.4, -0.1, 0.4, 2.0)}


def _r(rng, lo, hi, nd=3):
    return round(float(rng.uniform(lo, hi)), nd)


class _Gen:
    def __init__(self, seed, salt, prefix=""):
        self.prefix = prefix
        self.rng = np.random.default_rng([int(seed), salt])
        self.seed = int(seed)
        self.prog = []
        self.cols = {}      # name -> dict(kind, dim, heavy, cont)
        self.nstat = 0
        self.depth = 0
        self.nfam = 0
        self.weights_changed = False

    # ---- bookkeeping
    def emit(self, op, **a):
        self.prog.append(Stmt(op, **a))
        if op != "read":
            self.nstat += 1
        if op in ("sample", "importance", "observe", "weight", "assign", "assign_expr"):
            self.depth += 1
        if op in ("observe", "weight", "importance", "weights_upload"):
            self.weights_changed = True

    def room(self, k=1):
        return self.nstat + k <= MAX_STATEMENTS

    def new(self, prefix="x"):
        return f"{self.prefix}{prefix}{len(self.cols)}"

    def setcol(self, name, kind, dim=1, heavy=False, cont=False):
        self.cols[name] = dict(kind=kind, dim=dim, heavy=heavy, cont=cont)

    def pick(self, kinds, heavy_ok=False, dim=1):
        c = [n for n, v in self.cols.items() if v["kind"] in kinds and (heavy_ok or not v["heavy"]) and
             (v["dim"] == dim if dim else True)]
        return c[int(self.rng.integers(len(c)))] if c else None

    def vecs(self, dim=None):
        return [n for n, v in self.cols.items() if v["dim"] > 1 and v["kind"] == "vec" and (dim is None or v["dim"] == dim)]

    # ---- operands by the kind of value they must have
    def term(self, name, coef, comp=0):
        return (name, comp, coef)

    def mk(self, c0, terms):
        return Opnd(float(c0), tuple(terms), tuple(self.cols[n]["dim"] > 1 for n, _, _ in terms) + (False,) * (2 - len(terms)))

    def opnd(self, want, form=None):
        rng = self.rng
        form = form or OPERAND_FORMS[int(rng.choice(4, p=[0.4, 0.3, 0.15, 0.15]))]
        scal = ("real", "pos", "prob", "count", "bit")
        if want == "real":
            c0 = _r(rng, -2, 2)
            if form == "comp" and self.vecs():
                v = self.vecs()[int(rng.integers(len(self.vecs())))]
                t = [self.term(v, float(rng.choice(_COEFS)), int(rng.integers(self.cols[v]["dim"])))]
                a = self.pick(scal)
                if a and rng.random() < 0.4:
                    t.append(self.term(a, float(rng.choice(_COEFS))))
                return self.mk(c0, t)
            a, b = self.pick(scal), self.pick(scal)
            if form == "col2" and a and b:
                return self.mk(c0 if rng.random() < 0.5 else 0.0,
                               [self.term(a, float(rng.choice(_COEFS))), self.term(b, float(rng.choice(_COEFS)))])
            if form != "const" and a:
                return self.mk(c0 if rng.random() < 0.5 else 0.0, [self.term(a, float(rng.choice(_COEFS)))])
            return self.mk(c0, [])
        if want in ("small", "small_pos"):   # LogNormal's parameters: exp(mu + sigma z) must stay finite
            a = self.pick(("prob", "bit"))
            c0 = _r(rng, -1, 1) if want == "small" else _r(rng, 0.2, 0.9)
            return self.mk(c0, [self.term(a, 0.5)] if (a and form != "const") else [])
        if want in ("pos", "shape"):
            c0 = _r(rng, 0.5, 3.0) if want == "shape" else _r(rng, 0.3, 2.5)
            kinds = _POSLIKE + _COUNTLIKE
            a, b = self.pick(kinds), self.pick(kinds)
            if form in ("col2", "comp") and a and b:
                return self.mk(c0, [self.term(a, float(rng.choice((0.25, 0.5, 1.0)))), self.term(b, 0.5)])
            if form != "const" and a:
                return self.mk(c0 if rng.random() < 0.7 else 0.125, [self.term(a, float(rng.choice((0.25, 0.5, 1.0, 2.0))))])
            return self.mk(c0, [])
        if want == "prob":
            a, b = self.pick(("prob", "bit")), self.pick(("prob", "bit"))
            if form in ("col2", "comp") and a and b:
                return self.mk(_r(rng, 0.02, 0.1), [self.term(a, 0.5), self.term(b, 0.25)])
            if form != "const" and a:
                return self.mk(_r(rng, 0.02, 0.1), [self.term(a, float(rng.choice((0.5, 0.75, 0.85))))])
            return self.mk(_r(rng, 0.05, 0.95), [])
        if want == "nint":
            a, b = self.pick(_COUNTLIKE), self.pick(_COUNTLIKE)
            if form in ("col2", "comp") and a and b:
                return self.mk(float(rng.integers(1, 6)), [self.term(a, 1.0), self.term(b, 1.0)])
            if form != "const" and a:
                return self.mk(float(rng.integers(1, 6)), [self.term(a, 1.0)])
            return self.mk(float(rng.integers(1, 41)), [])
        raise ValueError(want)

    def dist(self, fam, dim=1):
        rng = self.rng
        zero = self.mk(0.0, [])
        if fam == abi.FAM_UNIFORM:
            a, b = ((0.0, 1.0) if rng.random() < 0.5 else (_r(rng, -3, 0), _r(rng, 0.5, 4)))
            return DistSpec(fam, 1, (zero,), self.mk(1.0, []), (a, b))
        if fam == abi.FAM_MVNORMAL_ISO:
            return DistSpec(fam, dim, tuple(self.opnd("real") for _ in range(dim)),
                            self.opnd("pos", "const" if rng.random() < 0.6 else None))
        if fam == abi.FAM_MVNORMAL:
            return DistSpec(fam, dim, tuple(self.opnd("real") for _ in range(dim)), zero, cov=_COVS[dim])
        p1, p2 = _FAM[fam][:2]
        return DistSpec(fam, 1, (self.opnd(p1) if p1 else zero,), self.opnd(p2) if p2 else self.mk(1.0, []))

    def out_kind(self, d):
        if d.fam in VECTOR_FAMILIES:
            return "vec", False, False
        k, cont, heavy = _FAM[d.fam][2:]
        if d.fam == abi.FAM_UNIFORM and d.params == (0.0, 1.0):
            k = "prob"
        return k, cont, heavy

    def next_family(self):
        """families in a seed-shifted round robin, so a handful of seeds meets every one"""
        fams = sorted(FAMILIES)
        f = fams[(self.seed * 5 + self.nfam) % len(fams)]
        self.nfam += 1
        return f

    # ---- statements
    def sample(self, fam=None, out=None):
        rng = self.rng
        fam = self.next_family() if fam is None else fam
        dim = 1
        if fam == abi.FAM_MVNORMAL_ISO:
            dim = int(rng.integers(2, 5))
        elif fam == abi.FAM_MVNORMAL:
            dim = int(rng.integers(2, 4))
        d = self.dist(fam, dim)
        kind, cont, heavy = self.out_kind(d)
        if out is None:
            same = [n for n, v in self.cols.items() if v["kind"] == kind and v["dim"] == dim]
            out = same[int(rng.integers(len(same)))] if (same and rng.random() < 0.3) else self.new("v" if dim > 1 else "x")
        self.emit("sample", out=out, dim=dim, dist=d)
        self.setcol(out, kind, dim, heavy, cont)
        return out

    def value(self, fam, d):
        """an Observe's value inside the family's support: a constant or a column operand"""
        rng = self.rng
        col = rng.random() < 0.5
        if fam in VECTOR_FAMILIES:
            v = self.vecs(d.dim)
            if col and v:
                n = v[int(rng.integers(len(v)))]
                return tuple(self.mk(0.0, [self.term(n, 1.0, k)]) for k in range(d.dim))
            return tuple(self.mk(_r(rng, -2, 2), []) for _ in range(d.dim))
        kind = self.out_kind(d)[0]
        if fam == abi.FAM_UNIFORM:
            a, b = d.params
            n = self.pick(("prob",), True)
            if col and n and a <= 0.0 and b >= 1.0:
                return (self.mk(0.0, [self.term(n, 1.0)]),)
            return (self.mk(round(a + (b - a) * float(rng.uniform(0.1, 0.9)), 3), []),)
        if kind == "real":
            return (self.opnd("real") if col else self.mk(_r(rng, -3, 3), []),)
        if kind == "pos":
            n = self.pick(_POSLIKE, True)
            if col and n:
                return (self.mk(0.0 if rng.random() < 0.5 else 0.25, [self.term(n, float(rng.choice((1.0, 0.5, 2.0))))]),)
            return (self.mk(_r(rng, 0.1, 4), []),)
        if kind == "prob":
            n = self.pick(("prob",), True)
            if col and n:
                return (self.mk(0.0, [self.term(n, 1.0)]),)
            return (self.mk(_r(rng, 0.05, 0.95), []),)
        if kind == "bit" or fam == abi.FAM_BINOMIAL:
            n = self.pick(("bit",), True)
            if col and n:
                return (self.mk(0.0, [self.term(n, 1.0)]),)
            return (self.mk(float(rng.integers(0, 2)), []),)
        n = self.pick(_COUNTLIKE, True)   # count
        if col and n:
            return (self.mk(float(rng.integers(0, 3)), [self.term(n, 1.0)]),)
        return (self.mk(float(rng.integers(0, 8)), []),)

    def observe(self, fam=None, op=None):
        fam = self.next_family() if fam is None else fam
        dim = 1 if fam not in VECTOR_FAMILIES else int(self.rng.integers(2, 4 if fam == abi.FAM_MVNORMAL else 5))
        d = self.dist(fam, dim)
        op = op or ("observe" if self.rng.random() < 0.7 else "weight")
        self.emit(op, dist=d, x=self.value(fam, d))

    def importance(self):
        kind = ("real", "pos", "prob", "count")[int(self.rng.integers(4))]
        fams = _IMPORTANCE[kind]
        fp, ft = (int(f) for f in self.rng.choice(fams, 2))
        if kind == "prob":   # both on (0, 1)
            mk01 = lambda f: (DistSpec(f, 1, (self.mk(0.0, []),), self.mk(1.0, []), (0.0, 1.0)) if f == abi.FAM_UNIFORM
                              else self.dist(f))
            dp, dt = mk01(fp), mk01(ft)
        else:
            dp, dt = self.dist(fp), self.dist(ft)
        out = self.new("x")
        self.emit("importance", out=out, dim=1, prop=dp, targ=dt)
        heavy = _FAM[fp][4] or _FAM[ft][4]
        self.setcol(out, "count" if kind == "count" else kind, 1, heavy, False)

    def assign(self, out=None, keep=False):
        """operand-form Assign. keep: out .= k out + c with its kind preserved (a Move target stays one)"""
        rng = self.rng
        if keep:
            v = self.cols[out]
            k, c = ((0.5, 0.1) if v["kind"] != "real" else (float(rng.choice((0.5, 2.0, -1.0))), _r(rng, -1, 1)))
            self.emit("assign", out=out, dim=1, exprs=(self.mk(c, [self.term(out, k)]),))
            return
        vs = self.vecs()
        if vs and rng.random() < 0.35:   # a vector column, reading its own components (rotated) or another's
            out = vs[int(rng.integers(len(vs)))] if rng.random() < 0.6 else self.new("v")
            dim = self.cols[out]["dim"] if out in self.cols else int(rng.integers(2, 5))
            src = [n for n in vs if self.cols[n]["dim"] >= dim] or None
            ex = []
            for k in range(dim):
                if src:
                    s = src[int(rng.integers(len(src)))]
                    ex.append(self.mk(0.0 if rng.random() < 0.5 else _r(rng, -1, 1),
                                      [self.term(s, float(rng.choice(_COEFS)), (k + 1) % self.cols[s]["dim"])]))
                else:
                    ex.append(self.opnd("real"))
            self.emit("assign", out=out, dim=dim, exprs=tuple(ex))
            self.setcol(out, "vec", dim)
            return
        want = "pos" if rng.random() < 0.4 else "real"
        e = self.anyopnd() if rng.random() < 0.3 else self.opnd(want)
        kinds = {self.cols[n]["kind"] for n in e.cols()}
        heavy = any(self.cols[n]["heavy"] for n in e.cols())
        if "wild" in kinds:
            kind = "wild"
        elif e.c0 > 0 and all(k > 0 for _, _, k in e.terms) and kinds <= set(_POSLIKE + _COUNTLIKE):
            kind = "pos"
        else:
            kind = "real"
        if out is None:   # an existing column keeps its kind: the tape's terms stay inside their supports
            ex = [n for n, v in self.cols.items() if v["dim"] == 1 and v["kind"] == kind]
            out = ex[int(rng.integers(len(ex)))] if (ex and rng.random() < 0.35) else self.new("a")
        self.emit("assign", out=out, dim=1, exprs=(e,))
        self.setcol(out, kind, 1, heavy, False)

    def anyopnd(self):
        """an operand over any scalar columns, heavy and wild included (Assign only)"""
        rng = self.rng
        c = [n for n, v in self.cols.items() if v["dim"] == 1]
        if not c:
            return self.mk(_r(rng, -2, 2), [])
        t = [self.term(c[int(rng.integers(len(c)))], float(rng.choice(_COEFS)))]
        if rng.random() < 0.5:
            t.append(self.term(c[int(rng.integers(len(c)))], float(rng.choice(_COEFS))))
        return self.mk(_r(rng, -2, 2) if rng.random() < 0.5 else 0.0, t)

    def tree(self, depth, must=None):
        rng = self.rng
        if depth == 0 or (must is None and rng.random() < 0.15):
            if rng.random() < 0.3:
                return ("c", float(rng.choice((0.0, -0.0, 1.0, 0.5, -1.5, 2.0, 3.0, 1e-3, 40.0))))
            names = list(self.cols)
            n = names[int(rng.integers(len(names)))]
            return ("col", n, int(rng.integers(self.cols[n]["dim"])))
        op = must if must is not None else int(rng.choice(XOPS_ALL[2:]))
        if op == abi.X_POWI:
            return (op, int(rng.choice((-3, -2, -1, 0, 1, 2, 3, 4, 5, 7))), self.tree(depth - 1))
        if op == abi.X_IFELSE:
            return (op, self.tree(depth - 1), self.tree(depth - 1), self.tree(depth - 1))
        if op in XOPS1:
            return (op, self.tree(depth - 1))
        return (op, self.tree(depth - 1), self.tree(depth - 1))

    def guarded(self, t, kind):
        """t where it lies inside the kind's range, else a constant (NaN compares false): a value a
        distribution may read"""
        lo, hi, other = {"real": (-1e6, 1e6, 0.25), "pos": (1e-3, 1e3, 1.0), "prob": (0.01, 0.99, 0.5)}[kind]
        return (abi.X_IFELSE, (abi.X_AND, (abi.X_GT, t, ("c", lo)), (abi.X_LT, t, ("c", hi))), t, ("c", other))

    def assign_expr(self, must=None):
        rng = self.rng
        vs = self.vecs()
        dim = 1
        out = None
        if vs and rng.random() < 0.25:   # a vector output, possibly one the expression reads
            out = vs[int(rng.integers(len(vs)))]
            dim = self.cols[out]["dim"]
        kind = ("wild", "real", "pos", "prob")[int(rng.choice(4, p=[0.3, 0.3, 0.25, 0.15]))] if dim == 1 else "vec"
        trees = []
        for k in range(dim):
            for attempt in range(20):
                t = self.tree(2 if (dim > 1 or kind != "wild") else 3, must if k == 0 else None)
                if dim > 1 and k == 0 and rng.random() < 0.7:   # reads its own components
                    t = (abi.X_ADD, t, ("col", out, (k + 1) % dim))
                g = t if kind == "wild" else self.guarded(t, "real" if kind == "vec" else kind)
                if _tree_size(g) <= abi.XPROG_MAX // (2 * dim) and to_fx(g)._need() <= abi.XSTACK_MAX:
                    break
            else:
                g = ("c", 1.0)
            trees.append(g)
        if out is None:
            # an existing column keeps its kind: the tape's terms stay inside their supports
            same = [n for n, v in self.cols.items() if v["dim"] == 1 and v["kind"] == kind]
            reads = [n for t in trees for n in tree_cols(t) if n in same]
            r = rng.random()
            if reads and r < 0.35:     # a column the expression itself reads
                out = reads[int(rng.integers(len(reads)))]
            elif same and r < 0.55:    # another existing column
                out = same[int(rng.integers(len(same)))]
            else:
                out = self.new("e")
        self.emit("assign_expr", out=out, dim=dim, trees=tuple(trees))
        self.setcol(out, kind, dim, False, False)

    def resample(self, ess=None, scheme=None):
        rng = self.rng
        self.emit("resample", ess=float(rng.choice((1.0, 0.5, 0.3), p=[0.4, 0.35, 0.25])) if ess is None else ess,
                  scheme=int(rng.choice(SCHEMES, p=[0.5, 0.25, 0.25])) if scheme is None else scheme,
                  wait=bool(rng.random() < 0.5))
        self.weights_changed = False

    def targets(self, dmax=4):
        c = [n for n, v in self.cols.items() if v["cont"] and v["dim"] == 1]
        if not c:
            return None
        d = int(min(len(c), self.rng.integers(1, dmax + 1)))
        return tuple(str(x) for x in self.rng.choice(c, d, replace=False))

    def bounds(self, t):
        lo = tuple(0.0 if self.cols[n]["kind"] in _POSLIKE else -math.inf for n in t)
        hi = tuple(1.0 if self.cols[n]["kind"] == "prob" else math.inf for n in t)
        if all(x == -math.inf for x in lo):
            return None, None
        return lo, hi

    def movespec(self, d=None):
        t = self.targets()
        if t is None:
            return None
        if d is not None:
            t = t[:d]
        auto = bool(self.rng.random() < 0.65)
        lo, hi = self.bounds(t)
        return (1 if auto else 0, t, 1e-3 if auto else _r(self.rng, 0.1, 0.6, 2), lo, hi)

    def move(self, form=None):
        rng = self.rng
        form = form or ("move", "move_gated", "move_block")[int(rng.integers(3))]
        if form == "move_block":
            # disjoint or overlapping targets, autoRW and RW: one fused kernel or one by one
            ms = [m for m in (self.movespec(int(rng.integers(1, 3))) for _ in range(int(rng.integers(1, 4)))) if m]
            if ms:
                self.emit("move_block", moves=tuple(ms), gated=bool(rng.random() < 0.5), wait=bool(rng.random() < 0.5))
            return bool(ms)
        m = self.movespec()
        if m is None:
            return False
        div = 0.6 if rng.random() < 0.12 else math.nan   # the host-decided diversity gate, now and then
        if form == "move":
            self.emit("move", proposal=m[0], targets=m[1], step=m[2], lo=m[3], hi=m[4], diversity=div,
                      wait=bool(rng.random() < 0.5))
        else:
            self.emit("move_gated", proposal=m[0], targets=m[1], step=m[2], lo=m[3], hi=m[4], diversity=div)
        return True

    def upload(self, out=None):
        rng = self.rng
        c = [n for n, v in self.cols.items() if v["kind"] in ("real", "pos", "prob", "count", "bit", "vec")]
        out = out or c[int(rng.integers(len(c)))]
        v = self.cols[out]
        self.emit("col_upload", out=out, kind=v["kind"], dim=v["dim"], vseed=int(rng.integers(1 << 30)))
        v["heavy"] = False

    def read(self, kind=None):
        rng = self.rng
        kind = kind or READ_KINDS[int(rng.integers(len(READ_KINDS)))]
        tame = [n for n, v in self.cols.items() if v["kind"] != "wild"]
        a = {}
        if kind == "download":
            names = list(self.cols)
            a["col"] = names[int(rng.integers(len(names)))]
        elif kind in ("minmax", "median", "histogram"):
            n = tame[int(rng.integers(len(tame)))]
            a["col"], a["comp"] = n, int(rng.integers(self.cols[n]["dim"]))
        elif kind == "moments":
            sc = [n for n in tame if self.cols[n]["dim"] == 1]
            k = int(rng.integers(1, 4))
            ex = [self.mk(0.0, [self.term(sc[int(rng.integers(len(sc)))], 1.0)]) for _ in range(k)]
            if rng.random() < 0.5:
                ex[0] = self.opnd("real")
            a["exprs"], a["cov"] = tuple(ex), bool(rng.random() < 0.7)
        elif kind == "score":
            a["depth"] = int(rng.integers(0, self.depth + 1))
        elif kind == "diversity":
            sc = [n for n in tame if self.cols[n]["dim"] == 1]
            a["targets"] = tuple(str(x) for x in rng.choice(sc, int(min(len(sc), rng.integers(1, 4))), replace=False))
        self.emit("read", kind=kind, **a)

    def prologue(self):
        """one column of each kind, so every parameter form has something to read"""
        self.sample(abi.FAM_NORMAL)
        self.sample(abi.FAM_GAMMA)
        self.sample(abi.FAM_BETA)
        self.sample(abi.FAM_POISSON if self.seed % 2 else abi.FAM_BERNOULLI)


def _gen_mixed(seed, prefix=""):
    g = _Gen(seed, 1, prefix)
    rng = g.rng
    g.prologue()
    while g.room():
        r = rng.random()
        if r < 0.26:
            g.sample()
        elif r < 0.47:
            g.observe()
        elif r < 0.56:
            g.assign()
        elif r < 0.64:
            n_x = sum(1 for s in g.prog if s.op == "assign_expr")
            ops = [o for o in XOPS_ALL[2:]]
            g.assign_expr(ops[(seed * 3 + n_x) % len(ops)])   # every opcode within a few seeds
        elif r < 0.76:
            if g.weights_changed or rng.random() < 0.2:
                g.resample()
                if rng.random() < 0.5 and g.room():
                    g.move()
        elif r < 0.81:
            g.move()
        elif r < 0.84:
            g.importance()
        elif r < 0.87:
            c = [n for n, v in g.cols.items()]
            g.emit("sample_particles", n=int(rng.choice((1, 7, 100))), replace=bool(rng.random() < 0.5),
                   col=c[int(rng.integers(len(c)))])
        elif r < 0.90:
            g.upload()
        elif r < 0.92:
            g.emit("weights_upload", vseed=int(rng.integers(1 << 30)))
        elif r < 0.945:
            g.emit("store_resample", vseed=int(rng.integers(1 << 30)))
        elif r < 0.965 and g.depth > 2:
            d = int(rng.integers(1, g.depth + 1))   # a loop body re-entered at an earlier depth
            g.emit("set_depth", depth=d)
            g.depth = d
        if rng.random() < 0.3:
            g.read()
    g.read("state")
    return g.prog


def _gen_moves(seed, prefix=""):
    """Resample, then 1 to 6 Moves (gated and not), the carried scores invalidated in between by
    each of test_move_carried_scores' variants in a random order"""
    g = _Gen(seed, 2, prefix)
    rng = g.rng
    fams = (abi.FAM_NORMAL, abi.FAM_GAMMA, abi.FAM_BETA, abi.FAM_LAPLACE, abi.FAM_EXPONENTIAL, abi.FAM_LOGISTIC)
    for k in range(int(rng.integers(2, 5))):
        g.sample(fams[(seed + k) % len(fams)] if k else abi.FAM_NORMAL, out=g.new("x"))
    for _ in range(2):
        g.observe(abi.FAM_NORMAL, "observe")
    g.resample(1.0, int(SCHEMES[seed % 3]))
    inval = list(rng.permutation(["assign", "upload", "store_resample", "resample", "sample", "set_depth", "none"]))
    nmoves = int(rng.integers(1, 7))
    for m in range(nmoves):
        if not g.room(4):
            break
        g.move(("move", "move_gated", "move_block")[int(rng.integers(3))])
        if rng.random() < 0.4:
            g.read()
        what = inval[m % len(inval)]
        t = g.targets(1)[0]
        if what == "assign":
            g.assign(t, keep=True)
        elif what == "upload":
            g.upload(t)
        elif what == "store_resample":
            g.emit("store_resample", vseed=int(rng.integers(1 << 30)))
        elif what == "resample":
            g.observe(abi.FAM_NORMAL, "observe")
            g.resample(float(rng.choice((1.0, 0.5))))
        elif what == "sample":   # a Sample into a scored column: earlier terms read the new values
            k = g.cols[t]["kind"]
            g.sample({"real": abi.FAM_NORMAL, "pos": abi.FAM_EXPONENTIAL, "prob": abi.FAM_BETA}[k], out=t)
        elif what == "set_depth" and g.depth > 3:
            g.emit("set_depth", depth=g.depth - 1)
            g.depth -= 1
    if g.room(2):
        g.observe(abi.FAM_NORMAL, "observe")
        g.move("move")
    g.read("state")
    return g.prog


# ---- the directed `caps` programs: long stretches with no read and no waited call ---------------
def _flush(g):
    """launches the open batch: a general-expression Assign always does (wsmc_assign_expr)"""
    g.emit("assign_expr", out="flush", dim=1, trees=((abi.X_ADD, ("col", "x0", 0), ("c", _r(g.rng, 0, 1))),))
    g.setcol("flush", "real")


def _const(g, lo=-1.0, hi=1.0):
    return g.mk(_r(g.rng, lo, hi), [])


def _normal(g, mu, sd=None):
    return DistSpec(abi.FAM_NORMAL, 1, (mu,), sd or _const(g, 0.5, 2.0))


def _col(g, n, k=1.0, comp=0):
    return g.mk(0.0, [g.term(n, k, comp)])


def _gen_caps(seed):
    name = CAPS_NAMES[seed % len(CAPS_NAMES)]
    g = _Gen(seed, 3)
    rng = g.rng
    g.sample(abi.FAM_NORMAL, out="x0")

    def samples(k, prefix):
        for j in range(k):
            n = f"{prefix}{j}"
            g.emit("sample", out=n, dim=1, dist=_normal(g, _const(g)))
            g.setcol(n, "real", cont=True)

    def tail():
        g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
        g.resample(0.5, abi.RESAMPLE_STRATIFIED)
        if g.room():   # (kEwSlots' 17 uploads leave no statement for it)
            g.emit("move_gated", proposal=1, targets=("x0",), step=1e-3, lo=None, hi=None, diversity=math.nan)

    if name == "kEwOps":          # 5, 6 and 7 consecutive batchable statements (after x0's Sample: a flush first)
        for k in (5, 6, 7):
            _flush(g)
            for j in range(k):
                if j % 2:
                    g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
                else:
                    n = f"s{k}_{j}"
                    g.emit("sample", out=n, dim=1, dist=_normal(g, _col(g, "x0", 0.5)))
                    g.setcol(n, "real")
    elif name == "kEwSlots":      # terms reading 15, 16 and 17 distinct columns
        for j in range(17):
            g.emit("col_upload", out=f"c{j}", kind="pos", dim=1, vseed=int(rng.integers(1 << 30)))
            g.setcol(f"c{j}", "pos")
        for k in (15, 16, 17):
            _flush(g)
            cols = [f"c{j}" for j in range(k)]
            while cols:
                a = cols[:6]
                cols = cols[6:]
                a = a + [a[-1]] * (6 - len(a))
                g.emit("observe", dist=DistSpec(abi.FAM_NORMAL, 1, (g.mk(0.0, [g.term(a[0], 1.0), g.term(a[1], 0.5)]),),
                                                 g.mk(0.5, [g.term(a[2], 1.0), g.term(a[3], 0.5)])),
                       x=(g.mk(0.0, [g.term(a[4], 1.0), g.term(a[5], -1.0)]),))
    elif name in ("kEwRows", "kEwPre"):
        for n, d in (("va", 4), ("vb", 4), ("v3", 3), ("v2", 2)):
            g.emit("sample", out=n, dim=d, dist=DistSpec(abi.FAM_MVNORMAL_ISO, d, tuple(_const(g) for _ in range(d)),
                                                         _const(g, 0.5, 1.5)))
            g.setcol(n, "vec", d)
        mvn = lambda third: DistSpec(abi.FAM_MVNORMAL_ISO, 2, (g.mk(0.0, [g.term("va", 1.0, 3), g.term("vb", 1.0, 3)]),
                                                                _col(g, third, 1.0, 0)), _const(g, 0.5, 1.5))
        if name == "kEwRows":     # 10 preloaded components, then 1, 2 and 3 outputs: 11, 12 and 13 rows
            for k in (1, 2, 3):
                _flush(g)
                g.emit("observe", dist=mvn("v2"), x=(_const(g), _const(g)))
                samples(k, f"r{k}_")
                # reads the last output: from its row, or (the 13th) unstaged -> the batch launches first
                g.emit("observe", dist=_normal(g, _col(g, f"r{k}_{k - 1}")), x=(_const(g),))
        else:                     # 9, 10 and 11 preloaded components: two weight terms, then two Assigns
            for third in ("x0", "v2", "v3"):
                _flush(g)
                g.emit("observe", dist=_normal(g, g.mk(0.0, [g.term("va", 1.0, 3), g.term("vb", 1.0, 3)])), x=(_const(g),))
                g.emit("observe", dist=_normal(g, _col(g, third, 1.0, 0)), x=(_const(g),))   # the 11th: launches first
                _flush(g)
                g.emit("assign", out="t", dim=1, exprs=(g.mk(0.0, [g.term("va", 1.0, 1), g.term("vb", 1.0, 2)]),))
                g.setcol("t", "real")
                g.emit("assign", out="t2", dim=1, exprs=(g.mk(0.0, [g.term(third, 1.0, 0), g.term("t", 1.0)]),))
                g.setcol("t2", "real")           # the 11th: read from memory, the batch stays
    elif name == "ntab4":         # a fifth in-place rewrite of a column read through the ancestors
        samples(5, "p")
        g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
        g.resample(1.0, abi.RESAMPLE_STRATIFIED)
        for j in range(5):
            g.emit("assign", out=f"p{j}", dim=1, exprs=(g.mk(_r(rng, -1, 1), [g.term(f"p{j}", 0.5)]),))
    elif name == "lagged_write":  # an in-place write of a column the open batch reads through the ancestors
        samples(2, "p")
        g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
        g.resample(1.0, abi.RESAMPLE_SYSTEMATIC)
        g.emit("assign", out="t", dim=1, exprs=(g.mk(1.0, [g.term("p0", 1.0)]),))
        g.setcol("t", "real")
        g.emit("assign", out="p0", dim=1, exprs=(_const(g),))                       # wsmc_assign's condition
        g.emit("assign", out="t2", dim=1, exprs=(g.mk(1.0, [g.term("p1", 1.0)]),))
        g.setcol("t2", "real")
        g.emit("sample", out="p1", dim=1, dist=_normal(g, _const(g)))               # wsmc_sample's
    elif name == "anc_row":       # a lagged read by a batch that already holds an ancestor row
        samples(2, "p")
        g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
        g.resample(1.0, abi.RESAMPLE_STRATIFIED)
        g.emit("assign", out="t", dim=1, exprs=(g.mk(1.0, [g.term("p0", 1.0)]),))
        g.setcol("t", "real")
        g.resample(1.0, abi.RESAMPLE_STRATIFIED)   # the weights did not change: a no-op, the batch stays open
        g.emit("assign", out="t2", dim=1, exprs=(g.mk(1.0, [g.term("p1", 1.0)]),))
        g.setcol("t2", "real")
        g.emit("observe", dist=_normal(g, _col(g, "t2")), x=(_const(g),))
        g.resample(1.0, abi.RESAMPLE_STRATIFIED)   # the next epoch: t (one behind) and p1 (two behind: traced first)
        g.emit("assign", out="t3", dim=1, exprs=(g.mk(0.0, [g.term("t", 1.0), g.term("p1", 1.0)]),))
        g.setcol("t3", "real")
    elif name == "seventh_lagged":
        # a column read one Resample behind in a batch that also overwrites it, stored in the seventh
        # statement after six that filled the rows; an asynchronous gated Move reads it first
        g.emit("sample", out="va", dim=4, dist=DistSpec(abi.FAM_MVNORMAL_ISO, 4, tuple(_const(g) for _ in range(4)),
                                                        _const(g, 0.5, 1.5)))
        g.setcol("va", "vec", 4)
        samples(1, "p")
        g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
        g.resample(1.0, abi.RESAMPLE_STRATIFIED)
        for j in range(6):   # va, x0 and p0 through the ancestors (6 rows) and six outputs: 12 rows
            g.emit("assign", out=f"t{j}", dim=1,
                   exprs=(g.mk(_r(rng, -1, 1), [g.term("va", 1.0, j % 4), g.term("x0" if j % 2 else "p0", 0.5)]),))
            g.setcol(f"t{j}", "real")
        g.emit("assign", out="x0", dim=1, exprs=(g.mk(0.0, [g.term("x0", 0.5), g.term("t5", 0.25)]),))
    tail()
    g.read("state")
    return g.prog


def _gen_edge(seed):
    """directed degenerate programs (kept out of `mixed`): every weight -inf, a NaN weight"""
    g = _Gen(seed, 4)
    g.prologue()
    g.emit("weights_upload", vseed=-1)   # all -inf
    g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
    g.emit("sample_particles", n=5, replace=True, col="x0")   # fails on both sides
    g.resample(1.0, abi.RESAMPLE_STRATIFIED)
    g.read("log_evidence")
    g.read("ess")
    g.sample(abi.FAM_NORMAL)
    g.emit("weights_upload", vseed=-2)   # one NaN
    g.emit("observe", dist=_normal(g, _col(g, "x0")), x=(_const(g),))
    g.resample(0.5, abi.RESAMPLE_SYSTEMATIC)
    g.read("state")
    return g.prog


def gen(seed: int, profile: str, prefix: str = "") -> list:
    """the program of (seed, profile); prefix: its column names' (`mixed` and `moves`: a second
    program on a context that already ran one)"""
    if prefix:
        return {"mixed": _gen_mixed, "moves": _gen_moves}[profile](int(seed), prefix)
    return {"mixed": _gen_mixed, "moves": _gen_moves, "caps": _gen_caps, "edge": _gen_edge}[profile](int(seed))


def for_shards(prog, exact: bool) -> list:
    """the program a multi-device handle can run: resample!(store, idx) needs one shard and exact
    shards refuse multinomial draws (include/wsmc.h). A Move under exact sharding is the
    exact-sharded oracle's (per-shard moment order), which `differential` is given."""
    out = []
    for s in prog:
        if s.op == "store_resample":
            continue
        if exact and s.op == "resample" and s.scheme == abi.RESAMPLE_MULTINOMIAL:
            s = Stmt("resample", **{**s.a, "scheme": abi.RESAMPLE_STRATIFIED})
        out.append(s)
    return out


def caps_name(seed: int) -> str:
    return CAPS_NAMES[seed % len(CAPS_NAMES)]


# ---- the executor -----------------------------------------------------------------------------
def mk_opnd(ctx, o: Opnd) -> abi.Operand:
    r = abi.Operand.const(o.c0)
    for k, (name, comp, coef) in enumerate(o.terms):
        c = ctx.col_find(name)
        if c < 0:
            raise KeyError(name)
        r.col[k], r.comp[k], r.coef[k] = c, int(comp), float(coef)
    return r


def mk_dist(ctx, s: DistSpec) -> abi.Dist:
    d = abi.Dist()
    d.family, d.dim, d.mean_fn = s.fam, s.dim, abi.MEAN_AFFINE
    for k in range(4):
        d.mu[k] = mk_opnd(ctx, s.mu[k]) if k < len(s.mu) else abi.Operand.const(0.0)
    d.scale = mk_opnd(ctx, s.scale)
    d.param[0], d.param[1] = s.params
    if s.fam == abi.FAM_MVNORMAL:
        S = (C.c_double * len(s.cov))(*s.cov)
        abi.check(abi.load_library().wsmc_dist_mvnormal_cov(C.byref(d), S))
    return d


def upload_values(kind, dim, n, vseed):
    r = np.random.default_rng(vseed)
    if kind in ("pos",):
        v = r.gamma(2.0, 0.7, dim * n) + 0.05
    elif kind == "prob":
        v = r.uniform(0.02, 0.98, dim * n)
    elif kind == "count":
        v = r.poisson(3.0, dim * n).astype(float)
    elif kind == "bit":
        v = r.integers(0, 2, dim * n).astype(float)
    else:
        v = r.normal(0.0, 1.5, dim * n)
    return v.reshape(dim, n) if dim > 1 else v


def weight_values(n, vseed):
    if vseed == -1:
        return np.full(n, -np.inf)
    if vseed == -2:
        w = np.linspace(-1.0, 0.0, n)
        w[n // 2] = np.nan
        return w
    r = np.random.default_rng(vseed)
    w = r.normal(0.0, 2.0, n)
    w[r.random(n) < 0.05] = -np.inf
    if not np.isfinite(w).any():
        w[0] = 0.0
    return w


def _out(ctx, s):
    c = ctx.col_find(s.out)
    return c if c >= 0 else ctx.col_create(s.out, s.a.get("dim", 1))


def _ids(ctx, names):
    return [ctx.col_find(n) for n in names]


def _code(e) -> int:
    """an error's wsmc_status, whichever side raised it"""
    if isinstance(e, np.linalg.LinAlgError):
        return abi.WSMC_ENOTPD
    if isinstance(e, abi.WSMCError):
        return int(e.code)
    if isinstance(e, RuntimeError):
        m = re.search(r"\((\d+)\)", str(e))
        return int(m.group(1)) if m else -1
    if isinstance(e, ValueError):
        return abi.WSMC_EARG
    raise e


def _wait(s, mode, expect):
    if expect is not None and expect[0] == "err":
        return True   # the error surfaces at this statement
    return {"all": True, "none": False, "prog": bool(s.a.get("wait", True))}[mode["waits"]]


def _issue(ctx, s, mode, expect):
    op = s.op
    R = ctx.col_find
    if op == "sample":
        return ctx.sample(_out(ctx, s), mk_dist(ctx, s.dist))
    if op == "importance":
        return ctx.sample_importance(_out(ctx, s), mk_dist(ctx, s.prop), mk_dist(ctx, s.targ))
    if op in ("observe", "weight"):
        return getattr(ctx, op)(mk_dist(ctx, s.dist), [mk_opnd(ctx, o) for o in s.x])
    if op == "assign":
        c = _out(ctx, s)
        return ctx.assign(c, [mk_opnd(ctx, o) for o in s.exprs])
    if op == "assign_expr":
        c = _out(ctx, s)
        prog, lens = dsl.xprogram([to_fx(t) for t in s.trees], R)
        return ctx.assign_expr(c, prog, lens)
    if op == "resample":
        return ctx.resample(s.ess, s.scheme, wait=_wait(s, mode, expect))
    if op == "move":
        return ctx.move(s.proposal, _ids(ctx, s.targets), s.step, s.lo, s.hi, -1, s.diversity,
                        wait=_wait(s, mode, expect))
    if op == "move_gated":
        ctx.move_gated(s.proposal, _ids(ctx, s.targets), s.step, s.lo, s.hi, -1, s.diversity)
        if expect is not None and expect[0] == "err" and hasattr(ctx, "sync"):
            ctx.sync()   # asynchronous on the device: the failure is reported by the next synchronizing call
        return None
    if op == "move_block":
        ms = [(m[0], _ids(ctx, m[1]), m[2], m[3], m[4]) for m in s.moves]
        return ctx.move_block(ms, gated=s.gated, wait=_wait(s, mode, expect))
    if op == "sample_particles":
        idx = ctx.sample_particles(s.n, s.replace)
        return idx, ctx.col_gather_rows(R(s.col), idx)
    if op == "col_upload":
        return ctx.col_upload(_out(ctx, s), upload_values(s.kind, s.dim, ctx.n, s.vseed))
    if op == "weights_upload":
        return ctx.weights_upload(weight_values(ctx.n, s.vseed))
    if op == "store_resample":
        return ctx.store_resample(np.random.default_rng(s.vseed).integers(0, ctx.n, ctx.n).astype(np.int32))
    if op == "set_depth":
        return ctx.set_depth(s.depth)
    if op == "read":
        return _read(ctx, s)
    raise ValueError(op)


def _read(ctx, s):
    k = s.kind
    R = ctx.col_find
    if k == "download":
        return ctx.col_download(R(s.col))
    if k == "weights":
        return ctx.weights_download()
    if k == "log_evidence":
        return ctx.log_evidence()
    if k == "ess":
        return ctx.ess()
    if k == "state":
        return ctx.get_state()
    if k == "moments":
        return ctx.weighted_moments([mk_opnd(ctx, o) for o in s.exprs], want_cov=s.cov)
    if k == "minmax":
        return ctx.col_minmax(R(s.col), s.comp)
    if k == "median":
        return ctx.weighted_median(R(s.col), s.comp)
    if k == "histogram":
        return ctx.histogram(R(s.col), s.comp)
    if k == "score":
        return ctx.score(min(s.depth, ctx.get_state()["depth"]))
    if k == "score_all":   # every depth from 0 to the current one
        return [ctx.score(d) for d in range(ctx.get_state()["depth"] + 1)]
    if k == "diversity":
        return ctx.marginal_diversity(_ids(ctx, s.targets))
    if k == "ancestors":
        return ctx.last_ancestors() if ctx.get_state()["n_resamples"] > 0 else None
    raise ValueError(k)


def step(ctx, s, mode, expect=None):
    """issue one statement: ("ok", value) or ("err", status)"""
    try:
        return ("ok", _issue(ctx, s, mode, expect))
    except (np.linalg.LinAlgError, abi.WSMCError, RuntimeError, ValueError) as e:
        return ("err", _code(e))


def run(ctx, prog, mode="chatty", on_step=None):
    """issue `prog` on one context; returns each statement's outcome (None: a read the mode skips)"""
    mode = MODES[mode] if isinstance(mode, str) else mode
    out = []
    for i, s in enumerate(prog):
        if s.op == "read" and not mode["reads"]:
            out.append(None)
            continue
        out.append(step(ctx, s, mode))
        if on_step:
            on_step(i, s, out[-1])
    return out


# ---- the comparer -----------------------------------------------------------------------------
def same_value(a, b) -> bool:
    """tests/test_gpu_expr.py same_bits' rule on anything a statement returns: bit for bit, a NaN
    matches any NaN"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = a.astype(np.float64), b.astype(np.float64)
        return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def _where(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    bad = np.flatnonzero(~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return f"{len(bad)} of {len(a)} differ, first at {bad[:4].tolist()}: {a[bad[:3]].tolist()} != {b[bad[:3]].tolist()}"


def compare(g, o):
    """None, or what differs first: every column, the weights, every get_state field, the log
    evidence, and the last ancestors once a Resample has resampled"""
    ng, no = g.col_names(), o.col_names()
    if ng != no:
        return f"column names {ng} != {no}"
    for name in ng:
        a, b = g.col_download(g.col_find(name)), o.col_download(o.col_find(name))
        if not same_value(a, b):
            return f"column {name}: " + _where(a, b)
    a, b = g.weights_download(), o.weights_download()
    if not same_value(a, b):
        return "weights: " + _where(a, b)
    sg, so = g.get_state(), o.get_state()
    for k in so:
        if not same_value(sg[k], so[k]):
            return f"state.{k}: {sg[k]!r} != {so[k]!r}"
    a, b = g.log_evidence(), o.log_evidence()
    if not same_value(a, b):
        return f"log_evidence: {a!r} != {b!r}"
    if so["n_resamples"] > 0 and not same_value(g.last_ancestors(), o.last_ancestors()):
        return "last_ancestors differ"
    return None


class Mismatch(AssertionError):
    def __init__(self, index, msg):
        super().__init__(msg)
        self.index = index


def _unwaited(s, m, oo) -> bool:
    """g was told not to wait at this statement, so it returns None where the oracle returns a value"""
    return s.op in ("resample", "move", "move_block") and not _wait(s, m, oo)


def _moments_close(o, s, a, b) -> bool:
    """wsmc_weighted_moments on shards against the oracle's single canonical sum: the two differ by
    the order of N-term sums only. A sum of N terms in any order is within (N - 1) eps sum|v_i| of
    the exact one, so with z = max|expr| the means (two sums and a quotient, both sides) agree
    within 8 N eps z, and the centred second moments (terms <= (2 z)^2, plus 4 z times the means'
    difference) within 64 N eps z^2. z is taken over the expressions whose values are all finite (a
    finite component involves no other); a component that is not finite on either side must be the
    same NaN or the same infinity on both."""
    n, eps = o.n, np.finfo(float).eps
    zm = 0.0
    for e in s.exprs:
        v = np.full(n, e.c0)
        for name, comp, coef in e.terms:
            c = o.col_download(o.col_find(name))
            v = v + coef * (c[comp] if c.ndim > 1 else c)
        if np.isfinite(v).all():
            zm = max(zm, float(np.max(np.abs(v))))

    def close(x, y, tol):
        x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
        if x.shape != y.shape:
            return False
        fin = np.isfinite(x) & np.isfinite(y)
        rest = (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))
        with np.errstate(invalid="ignore"):
            return bool(np.all(np.where(fin, np.abs(x - y) <= tol, rest)))

    (ma, ca), (mb, cb) = a, b
    ok = close(ma, mb, 8 * n * eps * zm)
    if ca is not None or cb is not None:
        ok = ok and ca is not None and cb is not None and close(ca, cb, 64 * n * eps * zm * zm)
    return ok


def differential(g, o, prog, mode, info="", hook=None, sharded=False, every_statement=False):
    """`prog` on `o` (the oracle) and `g` in lockstep, the oracle first at every statement: the same
    error status at the same statement, the same returned values (None from `g` only where it was
    told not to wait), the same state after every statement (`chatty`, or every_statement) and at
    the end. hook(i, g) runs after g's statement i. sharded: `g` is a multi-device handle, whose
    weighted_moments sums per shard in rank order (csrc/wsmc_api.hip wsmc_weighted_moments, the
    sharded autoRW's moment protocol of DESIGN.md §5) where the oracle sums once: that read is held
    to _moments_close's bound, everything else stays bit for bit.
    Raises Mismatch at the first difference; returns the oracle's outcomes."""
    m = MODES[mode]
    outcomes = []

    def fail(i, what):
        at = f"statement {i}: {prog[i]!r}" if i < len(prog) else "the final state (the replay command locates it)"
        raise Mismatch(i, f"{info}: {what}\n  at {at}")

    for i, s in enumerate(prog):
        if s.op == "read" and not m["reads"]:
            outcomes.append(None)
            continue
        oo = step(o, s, _ORACLE_MODE)
        go = step(g, s, m, expect=oo)
        outcomes.append(oo)
        if hook:
            hook(i, g)
        if oo[0] != go[0] or (oo[0] == "err" and oo[1] != go[1]):
            fail(i, f"outcome {go} != the oracle's {oo}")
        if oo[0] == "ok" and not (go[1] is None and _unwaited(s, m, oo)):
            if sharded and s.op == "read" and s.kind == "moments":
                same = _moments_close(o, s, go[1], oo[1])
            else:
                same = same_value(go[1], oo[1])
            if not same:
                fail(i, f"returned {go[1]!r} != the oracle's {oo[1]!r}")
        if m["step_compare"] or every_statement:
            d = compare(g, o)
            if d:
                fail(i, d)
    if hasattr(g, "sync"):
        g.sync()
    if hasattr(g, "store_materialize"):
        g.store_materialize()
    d = compare(g, o)
    if d:
        fail(len(prog), d)
    return outcomes


def replay(seed, profile, mode, n, lazy=True) -> str:
    return (f"python tests/progfuzz.py --seed {seed} --profile {profile} --mode {mode} --n {n} --backend hip"
            + ("" if lazy else " --eager"))


def info(seed, profile, mode, n, lazy=True) -> str:
    return f"seed={seed} profile={profile} mode={mode} N={n} lazy={lazy} [{replay(seed, profile, mode, n, lazy)}]"


def ctx_seed(seed, profile) -> int:
    return 1000 * (PROFILES.index(profile) + 1) + int(seed)


# ---- the statement batch, restated from the program text ----------------------------------------
K_OPS, K_SLOTS, K_ROWS, K_PRE = 6, 16, 12, 10   # csrc/wsmc_ew.h:68-71


def batch_model(prog):
    """The batches a `quiet`, lazy, single context forms from `prog`, by the rules of
    csrc/wsmc_api.hip (nothing is waited for, so every rule is a function of the program text):
      ew_preload :228-240, ew_out_rows :243-254, ew_remap :257-279 (rows and slots);
      wsmc_assign :2140-2226 (lagged operands, the four launch conditions :2173-2176, the table moves);
      wsmc_sample :2336-2353 and weigh :2457-2479 (full, lagged output, staging failure);
      wsmc_resample :2558-2562, :2592 and store_resample_row :631-632 (a Resample of unchanged weights
      is a no-op that leaves the batch open; any other launches it and starts an epoch);
      everything else launches the batch first (CHECK_CTX), except col_create / set_depth.
    (Line numbers as of this file's last change; the function names are what to look for.)
    tests/test_gpu_random_programs.py holds the model to the library: the number of batches it
    predicts for each `caps` program is the number the library launches (abi.jit_stats()).
    Returns (batches, events): a batch is a dict(nops, nslots, nrows, npre, ntab, anc, why) recorded when
    it launches; events are (name, statement index)."""
    cols = {}       # name -> [dim, epoch]
    epoch = 0
    wchanged = False
    B = dict(nops=0, slots=set(), nrows=0, npre=0, ntab=0, anc=None, rows=set(), unstaged=set(), lag=set())
    batches, events = [], []

    def flush(why, i):
        if B["nops"]:
            batches.append(dict(nops=B["nops"], nslots=len(B["slots"]), nrows=B["nrows"], npre=B["npre"], ntab=B["ntab"],
                                anc=B["anc"], why=why, at=i))
        B.update(nops=0, slots=set(), nrows=0, npre=0, ntab=0, anc=None, rows=set(), unstaged=set(), lag=set())

    def ensure(name, dim):
        if name not in cols:
            cols[name] = [dim, epoch]

    def preload(name, lag, i):
        dim = cols[name][0]
        if B["nrows"] + dim > K_ROWS:
            events.append(("rows_full", i))
            return False
        if B["npre"] + dim > K_PRE:
            events.append(("pre_full", i))
            return False
        B["nrows"] += dim
        B["npre"] += dim
        B["rows"].add((name, lag))
        return True

    def out_rows(name, i):
        if (name, 0) in B["rows"]:
            return
        dim = cols[name][0]
        if B["nrows"] + dim > K_ROWS:
            B["unstaged"].add(name)
            events.append(("unstaged_output", i))
            return
        B["nrows"] += dim
        B["rows"].add((name, 0))

    def stage(reads, i):
        keep = (set(B["slots"]), B["nrows"], B["npre"], set(B["rows"]))
        for n in reads:
            ok = n not in B["unstaged"]
            if not ok:
                events.append(("reads_unstaged", i))
            if ok and n not in B["slots"]:
                if len(B["slots"]) == K_SLOTS:
                    events.append(("slots_full", i))
                    ok = False
                elif (n, 0) not in B["rows"]:
                    ok = preload(n, 0, i)
                if ok:
                    B["slots"].add(n)
            if not ok:
                B["slots"], B["nrows"], B["npre"], B["rows"] = keep
                return False
        return True

    for i, s in enumerate(prog):
        op = s.op
        if op == "read":
            continue
        if op in ("sample", "observe", "weight"):
            reads = s.dist.cols() + ([n for o in s.x for n in o.cols()] if op != "sample" else [])
            for n in reads:
                cols[n][1] = epoch      # need_cols: stale reads are traced up to date first
            if op == "sample":
                ensure(s.out, s.dim)
                if B["nops"] and (B["nops"] == K_OPS or s.out in B["lag"]):
                    flush("full" if B["nops"] == K_OPS else "lagged_write", i)
            elif B["nops"] == K_OPS:
                flush("full", i)
            if not stage(reads, i):
                flush("stage", i)
                if not stage(reads, i):   # no batch takes it: the statement's own kernel
                    events.append(("unbatched", i))
                    if op == "sample":
                        cols[s.out][1] = epoch
                    else:
                        wchanged = True
                    continue
            if op == "sample":
                out_rows(s.out, i)
                cols[s.out][1] = epoch
            else:
                wchanged = True
            B["nops"] += 1
        elif op == "assign":
            ensure(s.out, s.dim)
            reads = [n for o in s.exprs for n in o.cols()]
            for n in reads:
                if cols[n][1] < epoch - 1:
                    cols[n][1] = epoch   # further behind: brought up to date first
            lagged = [n for n in reads if cols[n][1] < epoch]
            behind = s.out in lagged
            row = epoch - 1 if lagged else None
            if B["nops"]:
                why = ("full" if B["nops"] == K_OPS else
                       "anc_row" if (lagged and B["anc"] is not None and B["anc"] != row) else
                       "ntab" if (behind and B["ntab"] == 4) else
                       "lagged_write" if (not behind and s.out in B["lag"]) else None)
                if lagged and B["anc"] is not None and B["anc"] == row:
                    events.append(("second_lagged_read_same_row", i))
                if why:
                    flush(why, i)
            for n in reads:
                lag = 1 if n in lagged else 0
                if lag:
                    B["lag"].add(n)
                if (n, lag) not in B["rows"] and n not in B["unstaged"]:
                    if not preload(n, lag, i):
                        events.append(("unstaged_read", i))
            if behind:
                B["rows"].discard((s.out, 0))   # a fresh buffer: another pointer
                B["ntab"] += 1
            out_rows(s.out, i)
            if lagged:
                B["anc"] = row
            cols[s.out][1] = epoch
            B["nops"] += 1
        elif op == "resample":
            if not wchanged:
                continue
            flush("resample", i)
            epoch += 1
            wchanged = False
        elif op == "set_depth":
            continue
        else:
            flush(op, i)
            if op in ("assign_expr", "importance", "col_upload"):
                ensure(s.out, s.a.get("dim", 1))
                cols[s.out][1] = epoch
            if op == "store_resample":
                epoch += 1
            if op in ("importance", "weights_upload"):
                wchanged = True
    flush("end", len(prog))
    return batches, events


# ---- what a corpus covers (tests/test_random_programs.py asserts on it) --------------------------
def static_coverage(prog, cov=None):
    cov = cov if cov is not None else dict(sample=set(), weigh=set(), xops=set(), forms=set(), schemes=set(),
                                           moves=set(), reads=set(), dims=set())

    def dist(d):
        for o in d.mu[:d.dim] + (d.scale,):
            cov["forms"].add(o.form)

    for s in prog:
        if s.op == "sample":
            cov["sample"].add(s.dist.fam)
            cov["dims"].add((s.dist.fam, s.dim))
            dist(s.dist)
        elif s.op in ("observe", "weight"):
            cov["weigh"].add(s.dist.fam)
            dist(s.dist)
            for o in s.x:
                cov["forms"].add(o.form)
        elif s.op == "importance":
            dist(s.prop)
            dist(s.targ)
        elif s.op == "assign":
            for o in s.exprs:
                cov["forms"].add(o.form)
        elif s.op == "assign_expr":
            for t in s.trees:
                cov["xops"] |= tree_ops(t)
        elif s.op == "resample":
            cov["schemes"].add(s.scheme)
        elif s.op in ("move", "move_gated"):
            cov["moves"] |= {s.op, "bounded" if s.lo is not None else "unbounded", f"d{len(s.targets)}",
                             "autoRW" if s.proposal else "RW"}
        elif s.op == "move_block":
            cov["moves"].add("move_block")
            for m in s.moves:
                cov["moves"] |= {"bounded" if m[3] is not None else "unbounded", f"d{len(m[1])}",
                                 "autoRW" if m[0] else "RW"}
        elif s.op == "read":
            cov["reads"].add(s.kind)
    return cov


# ---- command line -----------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile", choices=PROFILES, default="mixed")
    ap.add_argument("--mode", choices=sorted(MODES), default="chatty")
    ap.add_argument("--n", type=int, default=1001)
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    ap.add_argument("--eager", action="store_true", help="store_set_lazy(False)")
    a = ap.parse_args(argv)
    from oracle import Oracle
    prog = gen(a.seed, a.profile)
    for i, s in enumerate(prog):
        print(f"{i:3d}  {s!r}")
    cs = ctx_seed(a.seed, a.profile)
    if a.backend == "oracle":
        o = Oracle(a.n, seed=cs)
        for i, r in enumerate(run(o, prog, a.mode)):
            if r is not None and (r[0] == "err" or (r[1] is not None and np.size(r[1]) <= 8)):
                print(f"{i:3d}  -> {r}")
        print("state", o.get_state(), "log_evidence", o.log_evidence())
        return 0
    import wsmc
    rc = 0
    # as the test drives it (the mode's own waits, reads and comparisons), then once more on fresh
    # contexts comparing the whole state after every statement, which locates a difference
    for every, what in ((False, f"as `{a.mode}` compares"), (True, "compared after every statement")):
        g, o = wsmc.Context(a.n, seed=cs), Oracle(a.n, seed=cs)
        g.store_set_lazy(not a.eager)
        try:
            differential(g, o, prog, a.mode, info(a.seed, a.profile, a.mode, a.n, not a.eager), every_statement=every)
            print(f"same as the oracle ({what}); state", g.get_state(), "log_evidence", g.log_evidence())
        except Mismatch as e:
            print(f"MISMATCH ({what})", e)
            rc = 1
        g.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())

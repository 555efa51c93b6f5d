"""Seeded random scalar state-space specs for wsmc_ssm_run: generator, runner, comparer, replay.

TEST INFRASTRUCTURE, the companion of tests/progfuzz.py for the fused run. A case is a
`wsmc_ssm_spec` filled by hand (plain data, built from ``numpy.random.default_rng([seed, salt])``
and nothing else: no context, no device), its data table and a printable line per statement.
`differential` runs one on a fresh `wsmc.Context` through `ssm_run` and on a fresh `oracle.Oracle`
through `SSM.statements` (the statements issued one by one: by include/wsmc.h the definition of
the run's result) and compares everything bit for bit; a difference is located by rerunning
shorter horizons.

    python tests/ssmfuzz.py --seed 3 --profile mixed --n 1001 --ess 0.5 --scheme stratified --segment 5 --backend oracle

prints the spec and runs it (`--backend hip`: against the oracle, comparing; `--name` picks a
directed case).

The generator keeps a loop invariant, so that T steps cannot drift out of a family's support or
overflow. Each column has one kind for the whole spec (real, pos, prob, count, bit or wild, and
the flag `heavy` on a real / pos column a heavy-tailed family writes) and is rewritten only by
statements whose output is of that kind. A wild column (a program's raw value: NaN and
infinities included) and a heavy one are read by Assigns, programs and observed values only; a
heavy value reaches a parameter only through a program that clamps it (min / max) into another
column. A real column's coefficients on real columns sum to at most 0.95 in magnitude. A
positive parameter reads an unbounded column (pos, count) with a coefficient of at most 0.25,
and then the family's other parameter reads bounded columns only, so that the mean of what is
drawn is a contraction of what was read (0.25 times the other parameter, which stays below 3.5).
An OBSERVE's dist writes nothing and takes stronger coefficients; the last OBSERVE of a step reads
the column the SAMPLE before it drew, so the weights differ between particles at every step. A count column is rewritten by an
Assign only additively (one count column with coefficient 1, plus bits).
"""
from __future__ import annotations

import argparse
import math
import sys
from dataclasses import dataclass

import numpy as np

import progfuzz as pf   # (puts the package and the oracle on sys.path)
from progfuzz import _FAM, FAMILIES, _where, same_value, to_fx, tree_ops, tree_repr

from wsmc import abi, dsl  # noqa: E402
from wsmc.ssm import SSM  # noqa: E402

T = 24                      # with set_ssm_segment(5): five launches, the last of 4 steps
SEED = 42                   # the contexts' seed, in the GPU file and the CPU file alike
MIXED_SEEDS = list(range(24))
THRESHOLDS = ["thresholds_poisson", "thresholds_gamma", "thresholds_binomial", "thresholds_negbin"]
DIRECTED = (["prog96", "prog97", "full", "init_observe", "observe_first", "nodata", "wide_data", "no_init"]
            + THRESHOLDS + ["all_xops", "partial_support", "pre_state"])
PROFILES = ("mixed", "directed")
SCALAR_FAMILIES = sorted(_FAM)
FORMS = ("const", "col", "col2", "data", "data_col", "col_data")   # data_col: data in slot 0; col_data: in slot 1
POSITIONS = ("mean", "scale", "value", "assign")
SCHEMES = {"stratified": abi.RESAMPLE_STRATIFIED, "systematic": abi.RESAMPLE_SYSTEMATIC,
           "multinomial": abi.RESAMPLE_MULTINOMIAL}
PROG_MAX = abi.XPROG_MAX    # program instructions over the whole spec the persistent kernel takes
STATE = ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples", "last_ess_perc")
DATA = dsl.DATA
_SALT = 7


# ---- specs are data ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Opnd:
    """wsmc_operand with its two slots as they are stored: None, ("col", index, coef) or
    ("data", j)"""
    c0: float = 0.0
    slots: tuple = (None, None)

    @property
    def form(self) -> str:
        a, b = self.slots
        kinds = tuple(None if s is None else s[0] for s in (a, b))
        return {(None, None): "const", ("col", None): "col", (None, "col"): "col", ("col", "col"): "col2",
                ("data", None): "data", (None, "data"): "data", ("data", "col"): "data_col",
                ("col", "data"): "col_data"}[kinds]

    def fill(self, o: abi.Operand) -> None:
        o.c0 = float(self.c0)
        for k, s in enumerate(self.slots):
            if s is None:
                o.col[k], o.comp[k], o.coef[k] = -1, 0, 0.0
            elif s[0] == "col":
                o.col[k], o.comp[k], o.coef[k] = int(s[1]), 0, float(s[2])
            else:
                o.col[k], o.comp[k], o.coef[k] = abi.OPERAND_DATA, int(s[1]), 1.0

    def __repr__(self):
        out = []
        if self.c0 != 0.0 or self.slots == (None, None):
            out.append(repr(self.c0))
        for k, s in enumerate(self.slots):
            if s is None:
                if self.slots[1 - k] is not None and k == 0:
                    out.append("_")   # an empty slot 0 before a used slot 1
                continue
            out.append(f"Data[{s[1]}]" if s[0] == "data" else (f"c{s[1]}" if s[2] == 1.0 else f"{s[2]!r}*c{s[1]}"))
        return " + ".join(out)


def K(c0=0.0, a=None, b=None) -> Opnd:
    return Opnd(float(c0), (a, b))


def col(i, coef=1.0):
    return ("col", int(i), float(coef))


def dat(j):
    return ("data", int(j))


@dataclass(frozen=True)
class DistD:
    fam: int
    mu: Opnd = Opnd(0.0)
    scale: Opnd = Opnd(1.0)
    params: tuple = (0.0, 0.0)

    def fill(self, d: abi.Dist) -> None:
        d.family, d.mean_fn, d.dim, d.reserved = self.fam, abi.MEAN_AFFINE, 1, 0
        for k in range(4):
            Opnd(0.0).fill(d.mu[k])
        self.mu.fill(d.mu[0])
        self.scale.fill(d.scale)
        d.param[0], d.param[1] = (float(p) for p in self.params)

    def __repr__(self):
        if self.fam == abi.FAM_UNIFORM:
            return f"Uniform({self.params[0]!r}, {self.params[1]!r})"
        return f"{FAMILIES[self.fam]}({self.mu!r}; {self.scale!r})"


# a statement: ("sample", col, DistD) | ("assign", col, Opnd) | ("expr", col, tree) | ("observe", Opnd, DistD);
# a tree is progfuzz's, its column leaves ("col", "c<k>", 0) or ("col", DATA, j)
def S(c, d):
    return ("sample", int(c), d)


def A(c, o):
    return ("assign", int(c), o)


def X(c, tree):
    return ("expr", int(c), tree)


def O(value, d):
    return ("observe", value, d)


def cl(i):
    return ("col", f"c{i}", 0)


def dl(j):
    return ("col", DATA, int(j))


def cst(v):
    return ("c", float(v))


def _resolve(name):
    return abi.OPERAND_DATA if name == DATA else int(name[1:])


def stmt_repr(st) -> str:
    if st[0] == "sample":
        return f"c{st[1]} ~ {st[2]!r}"
    if st[0] == "assign":
        return f"c{st[1]} .= {st[2]!r}"
    if st[0] == "expr":
        return f"c{st[1]} .= " + tree_repr(st[2]).replace(DATA, "Data")
    return f"{st[1]!r} => {st[2]!r}"


def _fill_stmt(out: abi.SsmStmt, st) -> None:
    """wsmc.ssm.SSM._lower's fields, from a descriptor"""
    out.col = -1
    Opnd(0.0).fill(out.value)
    if st[0] == "sample":
        out.kind, out.col = abi.SSM_SAMPLE, st[1]
        st[2].fill(out.dist)
    elif st[0] == "observe":
        out.kind = abi.SSM_OBSERVE
        st[1].fill(out.value)
        st[2].fill(out.dist)
    elif st[0] == "assign":
        out.kind, out.col = abi.SSM_ASSIGN, st[1]
        st[2].fill(out.value)
    else:
        out.kind, out.col = abi.SSM_ASSIGN_EXPR, st[1]
        prog, lens = dsl.xprogram([to_fx(st[2])], _resolve)
        if lens[0] > abi.SSM_XPROG_MAX:
            raise ValueError(f"a program of {lens[0]} instructions")
        out.prog_len = lens[0]
        for k in range(lens[0]):
            out.prog[k] = prog[k]


def prog_len(tree) -> int:
    return dsl.xprogram([to_fx(tree)], _resolve)[1][0]


class Case:
    """one spec with its data: .ssm (a wsmc.SSM over the raw struct), .data (T x data_dim, None
    without data), .T, .lines (the printable statements), .init / .step (the descriptors)"""

    def __init__(self, name, n_cols, init, step, data_dim=0, data=None, T=T, kinds=None, data_kinds=None):
        self.name, self.n_cols, self.init, self.step = name, int(n_cols), list(init), list(step)
        self.data_dim, self.T, self.kinds, self.data_kinds = int(data_dim), int(T), kinds, data_kinds
        self.data = None if data_dim == 0 else np.ascontiguousarray(np.asarray(data, dtype=np.float64).reshape(T, data_dim))
        sp = abi.SsmSpec()
        sp.n_cols, sp.data_dim, sp.n_init, sp.n_step = self.n_cols, self.data_dim, len(self.init), len(self.step)
        for k in range(self.n_cols):
            sp.col_names[k].value = f"c{k}".encode()
        for k, st in enumerate(self.init):
            _fill_stmt(sp.init[k], st)
        for k, st in enumerate(self.step):
            _fill_stmt(sp.step[k], st)
        self.spec = sp
        self.ssm = SSM.from_spec(sp)
        self.lines = ([f"cols {n_cols}" + (f" {kinds}" if kinds else "") + f"  data_dim {data_dim}"
                       + (f" {data_kinds}" if data_kinds else "") + f"  T {T}"]
                      + [f"init[{k}]  {stmt_repr(s)}" for k, s in enumerate(self.init)]
                      + [f"step[{k}]  {stmt_repr(s)}" for k, s in enumerate(self.step)])

    def text(self) -> str:
        return "\n".join(self.lines)

    def statements(self):
        return [("init", k, s) for k, s in enumerate(self.init)] + [("step", k, s) for k, s in enumerate(self.step)]

    @property
    def n_prog(self) -> int:
        sp = self.spec
        return (sum(sp.init[q].prog_len for q in range(sp.n_init) if sp.init[q].kind == abi.SSM_ASSIGN_EXPR) +
                sum(sp.step[q].prog_len for q in range(sp.n_step) if sp.step[q].kind == abi.SSM_ASSIGN_EXPR))

    def feat(self) -> int:
        """the kernel variant, by include/wsmc_terms.h wsmc_dist_feat's rule: 2 with a log-Gamma
        family, else 1 with a family of Bernoulli .. Geometric, else 0"""
        fams = [s[2].fam for _, _, s in self.statements() if s[0] in ("sample", "observe")]
        if any(f >= abi.FAM_GAMMA for f in fams):
            return 2
        return 1 if any(abi.FAM_BERNOULLI <= f <= abi.FAM_GEOMETRIC for f in fams) else 0

    def route(self, n, scheme, cap) -> str:
        """the route a run on a fresh context takes (include/wsmc.h wsmc_ssm_run)"""
        ok = n <= cap[self.n_cols] and scheme != abi.RESAMPLE_MULTINOMIAL and self.n_prog <= PROG_MAX
        return "persistent" if ok else "statements"


# ---- the generator ----------------------------------------------------------------------------
_DATA_KINDS = ("real", "pos", "prob", "count", "bit")
_CMP = (abi.X_LT, abi.X_LE, abi.X_GT, abi.X_GE, abi.X_EQ, abi.X_NE, abi.X_AND, abi.X_OR)
_UNBOUNDED = ("pos", "count")
# what a kind of value needs. alone: the constant of the `const` form; c0: the constant beside
# columns; pool: column kind -> coefficients; data: the data kinds it may take (then c0 = 0);
# heavy: heavy columns may be read (observed values and Assigns into heavy / wild columns)
_R1 = (0.9, -0.5, 0.7, 0.95, -0.95)     # a real column's coefficient on one real column ...
_R2 = (0.45, -0.45, 0.3, -0.25)         # ... and on each of two (the sum stays within 0.95)


def _r(rng, lo, hi, nd=3):
    return round(float(rng.uniform(lo, hi)), nd)


def _ri(rng, lo, hi):
    return float(rng.integers(lo, hi + 1))


_WANT = {
    # parameters
    "real": dict(alone=lambda r: _r(r, -2, 2), c0=lambda r: _r(r, -2, 2) if r.random() < 0.5 else 0.0,
                 pool={"real": _R1, "pos": (0.25, -0.25), "count": (0.25, -0.25), "prob": (1.0, -1.0, 0.5), "bit": (1.0, -1.0, 0.5)},
                 data=_DATA_KINDS),
    "pos": dict(alone=lambda r: _r(r, 0.3, 2.5), c0=lambda r: _r(r, 0.3, 2.5),
                pool={"prob": (0.25, 0.5), "bit": (0.25, 0.5), "pos": (0.25,), "count": (0.25,)}, data=("pos", "prob")),
    "shape": dict(alone=lambda r: _r(r, 0.5, 3.0), c0=lambda r: _r(r, 0.5, 2.5),
                  pool={"prob": (0.25, 0.5), "bit": (0.25, 0.5), "pos": (0.25,), "count": (0.25,)}, data=("pos", "prob")),
    "prob": dict(alone=lambda r: _r(r, 0.05, 0.95), c0=lambda r: _r(r, 0.02, 0.1),
                 pool={"prob": (0.5, 0.75, 0.85), "bit": (0.5, 0.75)}, pair=(0.5, 0.25), data=("prob",), dcoef=(0.5,)),
    "nint": dict(alone=lambda r: _ri(r, 1, 40), c0=lambda r: _ri(r, 1, 5), pool={"count": (1.0,), "bit": (1.0,)},
                 second=("bit",), data=()),
    "small": dict(alone=lambda r: _r(r, -1, 1), c0=lambda r: _r(r, -1, 1), pool={"prob": (0.5,), "bit": (0.5,)}, data=("prob",)),
    "small_pos": dict(alone=lambda r: _r(r, 0.2, 0.9), c0=lambda r: _r(r, 0.2, 0.9), pool={"prob": (0.5,), "bit": (0.5,)}, data=()),
    # observed values (inside the family's support for every particle) and Assigns into heavy columns
    "vreal": dict(alone=lambda r: _r(r, -3, 3), c0=lambda r: _r(r, -2, 2) if r.random() < 0.5 else 0.0,
                  pool={k: (1.0, -1.0, 0.5, 2.0, 0.7, -1.3) for k in ("real", "pos", "prob", "count", "bit")},
                  data=_DATA_KINDS, heavy=True),
    "vpos": dict(alone=lambda r: _r(r, 0.1, 4), c0=lambda r: 0.25,
                 pool={"pos": (1.0, 0.5, 2.0), "prob": (1.0, 0.5, 2.0), "count": (1.0, 0.5), "bit": (1.0, 0.5)},
                 data=("pos", "prob"), heavy=True),
    "vprob": dict(alone=lambda r: _r(r, 0.05, 0.95), c0=lambda r: 0.05, pool={"prob": (0.5,), "bit": (0.25,)}, pair=(0.5, 0.25),
                  data=("prob",), dcoef=(0.5,)),
    "vcount": dict(alone=lambda r: _ri(r, 0, 7), c0=lambda r: _ri(r, 0, 2), pool={"count": (1.0,), "bit": (1.0,)},
                   data=("count", "bit")),
    "vbit": dict(alone=lambda r: _ri(r, 0, 1), c0=lambda r: 0.0, pool={"bit": (1.0,)}, data=("bit",),
                 forms=("const", "col", "data")),
    # Assigns by the kind of the column they write
    "apos": dict(alone=lambda r: _r(r, 0.3, 2.5), c0=lambda r: _r(r, 0.3, 2.5),
                 pool={"prob": (0.25, 0.5, 1.0), "bit": (0.25, 0.5, 1.0), "pos": (0.25,), "count": (0.25,)}, data=("pos", "prob")),
    "acount": dict(alone=lambda r: _ri(r, 0, 5), c0=lambda r: _ri(r, 0, 2), pool={"count": (1.0,), "bit": (1.0,)},
                   second=("bit",), data=("count", "bit")),
    "any": dict(alone=lambda r: _r(r, -2, 2), c0=lambda r: _r(r, -2, 2) if r.random() < 0.5 else 0.0,
                pool={k: pf._COEFS for k in ("real", "pos", "prob", "count", "bit", "wild")}, data=_DATA_KINDS, heavy=True),
}
# an OBSERVE's dist writes nothing, so its parameters need no contraction: stronger coefficients, so
# that the weights tell the particles apart
_OBS_POOL = {
    "real": {"real": (1.0, -1.0, 0.5, 2.0), "pos": (1.0, -0.5), "count": (1.0, -0.5), "prob": (2.0, -1.0), "bit": (2.0, -1.0)},
    "pos": {"prob": (1.0, 2.0), "bit": (1.0, 2.0), "pos": (0.5, 1.0), "count": (0.5, 1.0)},
    "shape": {"prob": (1.0, 2.0), "bit": (1.0, 2.0), "pos": (0.5, 1.0), "count": (0.5, 1.0)},
}
_ASSIGN_WANT = {"real": "real", "pos": "apos", "prob": "prob", "count": "acount", "bit": "vbit", "wild": "any"}
_VALUE_WANT = {"real": "vreal", "pos": "vpos", "prob": "vprob", "count": "vcount", "bit": "vbit"}


class _SsmGen:
    def __init__(self, seed):
        self.seed = int(seed)
        self.rng = np.random.default_rng([self.seed, _SALT])
        self.tg = pf._Gen(self.seed, _SALT + 1)   # progfuzz's expression-tree generator (its own stream)
        self.cols = []          # dict(kind, heavy)
        self.data_kinds = []
        self.in_step = False
        self.observing = False
        self.nform = {p: 0 for p in POSITIONS}
        self.n_prog = 0
        self.n_x = 0
        self.ps = (self.seed * 5) % len(SCALAR_FAMILIES)        # the SAMPLE round robin
        po = (self.seed * 8 + 3) % len(SCALAR_FAMILIES)         # the OBSERVE round robin
        self.obs_queue = (SCALAR_FAMILIES[po:] + SCALAR_FAMILIES[:po]) * 2

    # ---- columns by kind
    def pick_pool(self, w, bounded_only=False, second=False):
        """[(column, coefficients)] a value of kind `w` may read"""
        spec = _WANT[w]
        if self.observing and w in _OBS_POOL:
            spec = dict(spec, pool=_OBS_POOL[w])
        out = []
        for i, c in enumerate(self.cols):
            k = c["kind"]
            if k not in spec["pool"] or (c["heavy"] and not spec.get("heavy")):
                continue
            if bounded_only and k in _UNBOUNDED:
                continue
            if second and "second" in spec and k not in spec["second"]:
                continue
            out.append((i, spec["pool"][k]))
        return out

    def operand(self, position, w, bounded_only=False, forms=None):
        """an operand of kind `w`: the first form that can be built, the forms taken in a rotation
        per position so that every form meets every position"""
        n = self.nform[position]
        self.nform[position] += 1
        order = [FORMS[(self.seed + n + k) % len(FORMS)] for k in range(len(FORMS))]
        for f in order:
            if forms is not None and f not in forms:
                continue
            o = self.build(w, f, bounded_only)
            if o is not None:
                return o
        raise AssertionError((w, position))

    def build(self, w, form, bounded_only=False):
        rng, spec = self.rng, _WANT[w]
        if form not in spec.get("forms", FORMS):
            return None
        if form == "const":
            return K(spec["alone"](rng))
        pool = self.pick_pool(w, bounded_only)
        dpool = [j for j, k in enumerate(self.data_kinds) if k in spec["data"]] if self.in_step else []
        pick = lambda p: p[int(rng.integers(len(p)))]
        unb = lambda i: self.cols[i]["kind"] in _UNBOUNDED

        def term(entry, scale=1.0):
            i, coefs = entry
            return col(i, float(coefs[int(rng.integers(len(coefs)))]) * scale)

        if form == "col":
            if not pool:
                return None
            return K(spec["c0"](rng), term(pick(pool)))
        if form == "col2":
            second = self.pick_pool(w, bounded_only, second=True)
            if not pool or not second:
                return None
            a, b = pick(pool), pick(second)
            if "pair" in spec:
                return K(spec["c0"](rng), col(a[0], spec["pair"][0]), col(b[0], spec["pair"][1]))
            if w == "real" and not self.observing:   # the coefficients on real columns sum to at most 0.95
                ta = col(a[0], float(rng.choice(_R2))) if self.cols[a[0]]["kind"] == "real" else term(a)
                tb = col(b[0], float(rng.choice(_R2))) if self.cols[b[0]]["kind"] == "real" else term(b)
                return K(spec["c0"](rng), ta, tb)
            half = 0.5 if (not self.observing and unb(a[0]) and unb(b[0]) and w in ("pos", "shape", "apos")) else 1.0
            return K(spec["c0"](rng), term(a, half), term(b, half))
        if not dpool:
            return None
        j = pick(dpool)
        if form == "data":
            return K(0.0, dat(j)) if rng.random() < 0.7 else K(0.0, None, dat(j))
        if not pool:
            return None
        e = pick(pool)
        t = col(e[0], float(rng.choice(spec["dcoef"]))) if "dcoef" in spec else term(e)
        return K(0.0, dat(j), t) if form == "data_col" else K(0.0, t, dat(j))

    def reads_unbounded(self, o: Opnd) -> bool:
        return any(s is not None and s[0] == "col" and self.cols[s[1]]["kind"] in _UNBOUNDED for s in o.slots)

    def dist(self, fam):
        rng = self.rng
        if fam == abi.FAM_UNIFORM:
            a, b = self.uniform_params
            return DistD(fam, K(0.0), K(1.0), (a, b))
        p1, p2 = _FAM[fam][:2]
        mu = self.operand("mean", p1) if p1 else K(0.0)
        # the mean of a draw is a contraction of what its parameters read: at most one of them
        # reads an unbounded column; NegativeBinomial's mean r (1 - p) / p takes a constant p
        tight = p1 in ("shape", "nint") and self.reads_unbounded(mu) and not self.observing
        if p2 and fam == abi.FAM_NEGBINOMIAL and tight:
            sc = K(_r(rng, 0.4, 0.9))
        else:
            sc = self.operand("scale", p2, bounded_only=tight) if p2 else K(1.0)
        return DistD(fam, mu, sc)

    def out_kind(self, fam):
        k, _, heavy = _FAM[fam][2:]
        if fam == abi.FAM_UNIFORM and self.uniform_params == (0.0, 1.0):
            k = "prob"
        return k, heavy

    def col_for(self, kind, heavy, n_cols, create=True):
        for i, c in enumerate(self.cols):
            if (c["kind"], c["heavy"]) == (kind, heavy):
                return i
        if create and len(self.cols) < n_cols:
            self.cols.append(dict(kind=kind, heavy=heavy))
            return len(self.cols) - 1
        return None

    # ---- statements
    def sample(self, fam, c):
        return S(c, self.dist(fam))

    def observe(self, fam, informative):
        """value => dist; informative: a set of columns of which the density reads one (those the
        step draws, so that the weights differ between particles at every step), or None"""
        if informative and fam == abi.FAM_UNIFORM:
            return None                     # (a constant density)
        for _ in range(12):
            self.observing = True
            d = self.dist(fam)
            self.observing = False
            if fam == abi.FAM_UNIFORM:
                a, b = d.params
                if (a, b) == (0.0, 1.0):
                    v = self.operand("value", "vprob")
                else:
                    v = K(round(a + (b - a) * float(self.rng.uniform(0.1, 0.9)), 3))
            elif fam == abi.FAM_BINOMIAL:
                v = self.operand("value", "vbit")
            else:
                v = self.operand("value", _VALUE_WANT[_FAM[fam][2]])
            reads = any(s is not None and s[0] == "col" and s[1] in (informative or ()) for o in (d.mu, d.scale, v)
                        for s in o.slots)
            if reads or not informative:
                return O(v, d)
        return None

    def next_observe(self, informative):
        """the next family of the round robin (one that can read an `informative` column)"""
        for k, f in enumerate(self.obs_queue):
            st = self.observe(f, informative)
            if st is not None:
                del self.obs_queue[k]
                return st
        raise AssertionError("no family can observe the column")

    def assign(self, c):
        k = self.cols[c]
        w = _ASSIGN_WANT[k["kind"]]
        if k["heavy"]:
            w = "vreal" if k["kind"] == "real" else "vpos"
        return A(c, self.operand("assign", w))

    def tree_cols(self):
        cols = {f"c{i}": dict(kind=c["kind"], dim=1, heavy=c["heavy"], cont=False) for i, c in enumerate(self.cols)}
        if self.in_step and self.data_kinds:
            cols[DATA] = dict(kind="real", dim=len(self.data_kinds), heavy=False, cont=False)
        return cols

    def expr(self, c, budget):
        """c .= a program of at most `budget` instructions whose value is of the column's kind; None
        when none fits"""
        rng, tg = self.rng, self.tg
        tg.cols = self.tree_cols()
        k = self.cols[c]
        kind = k["kind"]
        ops = list(pf.XOPS_ALL[2:])
        must = ops[(self.seed * 3 + self.n_x) % len(ops)]
        heavy_src = [i for i, x in enumerate(self.cols) if x["heavy"] and x["kind"] == kind]
        for attempt in range(30):
            depth = 2 if attempt < 15 else 1
            if kind == "wild":
                t = tg.tree(3 if attempt < 10 else depth, must)
            elif kind in ("real", "pos") and not k["heavy"] and heavy_src and attempt < 4:
                # the clamp that lets a heavy-tailed value reach a parameter
                lo, hi = (-50.0, 50.0) if kind == "real" else (0.01, 50.0)
                t = (abi.X_MIN, (abi.X_MAX, cl(heavy_src[int(rng.integers(len(heavy_src)))]), cst(lo)), cst(hi))
            elif kind in ("real", "pos", "prob"):
                t = tg.guarded(tg.tree(depth, must), kind)
            elif kind == "bit":
                op = int(rng.choice(_CMP + (abi.X_NOT,)))
                t = (op, tg.tree(depth)) if op == abi.X_NOT else (op, tg.tree(depth), tg.tree(depth))
            else:   # count: a sum of two truth values
                t = (abi.X_ADD, (int(rng.choice(_CMP)), tg.tree(1), tg.tree(1)), (int(rng.choice(_CMP)), tg.tree(1), tg.tree(1)))
            if to_fx(t)._need() <= abi.XSTACK_MAX and prog_len(t) <= min(budget, abi.SSM_XPROG_MAX):
                self.n_x += 1
                return X(c, t)
        return None


def _data_values(rng, kind, n):
    if kind == "real":
        return np.round(rng.normal(0.0, 1.5, n), 3)
    if kind == "pos":
        return np.round(rng.uniform(0.2, 3.0, n), 3)
    if kind == "prob":
        return np.round(rng.uniform(0.05, 0.45, n), 3)
    if kind == "count":
        return rng.integers(0, 7, n).astype(float)
    return rng.integers(0, 2, n).astype(float)


def gen_mixed(seed) -> Case:
    g = _SsmGen(seed)
    rng = g.rng
    n_cols = 1 + seed % 4
    data_dim = seed % 5
    n_init = (0, 4, 1, 2, 3, 2)[seed % 6]
    n_obs = 1 + seed % 3
    n_step = max(2 + (seed * 5 + 3) % 7, n_obs + 1)
    g.data_kinds = [_DATA_KINDS[(seed + 2 * j) % 5] for j in range(data_dim)]
    a, b = (0.0, 1.0) if rng.random() < 0.5 else (_r(rng, -3, 0), _r(rng, 0.5, 4))
    g.uniform_params = (a, b)

    # the skeleton: where the OBSERVEs stand (forced by the seed where coverage needs it), then the
    # kinds of the other statements
    pos = set()
    free = list(range(n_step))
    if seed % 4 == 1:
        pos.add(0)
    if seed % 3 == 0:                       # the step ends with a non-OBSERVE
        free = free[:-1]
    while len(pos) < n_obs:
        pos.add(int(rng.choice([q for q in free if q not in pos])))
    step_kinds = ["observe" if q in pos else ("sample", "assign", "expr")[int(rng.choice(3, p=[0.45, 0.25, 0.3]))]
                  for q in range(n_step)]
    # the statement before the last OBSERVE (cyclically, other OBSERVEs passed over) is a SAMPLE, and
    # that OBSERVE reads its column: the particles move and the weights differ at every step
    live_q = max(pos)
    while live_q in pos:
        live_q = (live_q - 1) % n_step
    step_kinds[live_q] = "sample"
    init_kinds = [("sample", "assign", "expr")[int(rng.choice(3, p=[0.7, 0.15, 0.15]))] for _ in range(n_init)]
    if init_kinds:
        init_kinds[0] = "sample"
    if seed % 4 == 2 and n_init >= 2:       # an OBSERVE in `init`
        init_kinds[-1] = "observe"

    # families in the round robin, each SAMPLE's taken as the next whose output kind has (or can
    # still get) a column; what is left of the columns takes the kinds no family writes
    fams = {}
    for where, kinds in (("init", init_kinds), ("step", step_kinds)):
        for q, kd in enumerate(kinds):
            if kd != "sample":
                continue
            for k in range(len(SCALAR_FAMILIES)):
                f = SCALAR_FAMILIES[(g.ps + k) % len(SCALAR_FAMILIES)]
                c = g.col_for(*g.out_kind(f), n_cols)
                if c is not None:
                    fams[where, q] = (f, c)
                    g.ps = (g.ps + k + 1) % len(SCALAR_FAMILIES)
                    break
    spare = ("wild", "real", "pos", "bit", "prob", "count")
    while len(g.cols) < n_cols:
        g.cols.append(dict(kind=spare[(seed + len(g.cols)) % len(spare)], heavy=False))

    fresh = {fams["step", live_q][1]}

    def build(where, kinds):
        out = []
        last_obs = max([q for q, kd in enumerate(kinds) if kd == "observe"], default=-1)
        for q, kd in enumerate(kinds):
            if kd == "sample":
                out.append(g.sample(*fams[where, q]))
                continue
            if kd == "observe":
                out.append(g.next_observe(fresh if (q == last_obs and where == "step") else None))
                continue
            c = int(rng.integers(n_cols))
            st = g.expr(c, PROG_MAX - g.n_prog) if kd == "expr" else None
            if st is None:
                st = g.assign(c)
            else:
                g.n_prog += prog_len(st[2])
            out.append(st)
        return out

    init = build("init", init_kinds)
    g.in_step = True
    step = build("step", step_kinds)
    data = np.column_stack([_data_values(rng, k, T) for k in g.data_kinds]) if data_dim else None
    kinds = [c["kind"] + ("*" if c["heavy"] else "") for c in g.cols]
    return Case(f"mixed-{seed}", n_cols, init, step, data_dim, data, T, kinds, list(g.data_kinds))


# ---- the directed cases -----------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng([DIRECTED.index(name), _SALT + 2])


def _normal(mu, sc):
    return DistD(abi.FAM_NORMAL, mu if isinstance(mu, Opnd) else K(mu), sc if isinstance(sc, Opnd) else K(sc))


def _chain(leaves, ops, last):
    """a left-nested chain over the leaves (stack depth 2) closed by the unary `last`: 2 n instructions"""
    t = leaves[0]
    for k, x in enumerate(leaves[1:]):
        t = (ops[k % len(ops)], t, x)
    return (last, t)


def _deep(leaves):
    """a right-nested chain of differences: the last leaf is pushed on len(leaves) - 1 others"""
    t = leaves[-1]
    for x in reversed(leaves[:-1]):
        t = (abi.X_SUB, x, t)
    return t


_CHAIN_OPS = (abi.X_ADD, abi.X_MUL, abi.X_SUB, abi.X_MIN, abi.X_MAX)


def _prog32(cols, shift=0):
    """32 instructions: 16 leaves over the columns (and constants), 15 operators, a sine"""
    leaves = [cl(cols[(k + shift) % len(cols)]) if k % 3 != 2 else cst((0.5, -1.25, 2.0, 0.75, 3.0)[(k + shift) % 5])
              for k in range(16)]
    t = _chain(leaves, _CHAIN_OPS[shift % 5:] + _CHAIN_OPS[:shift % 5], abi.X_SIN)
    assert prog_len(t) == 32
    return t


def _gen_prog(name):
    """three programs of 32 instructions (96: the persistent kernel's argument holds them); prog97
    has one more instruction, which the kernel's argument does not hold: the statement route"""
    rng = _rng(name)
    data = np.round(rng.normal(0.0, 1.0, T), 3)
    step = [S(0, _normal(K(0.0, col(0, 0.9)), 0.5))]
    if name == "prog97":
        step.append(X(3, cl(0)))
    step += [X(1, _prog32([0, 1, 2, 3], 0)), X(2, _prog32([1, 0, 3], 1)), X(3, _prog32([2, 3, 0], 2)),
             O(K(0.0, dat(0)), _normal(K(0.0, col(0)), 1.0))]
    return Case(name, 4, [S(0, _normal(0.0, 1.0))], step, 1, data, T, ["real", "wild", "wild", "wild"])


def _gen_full(name):
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.normal(0, 0.3, T), 3),
                            np.round(rng.uniform(0.5, 2, T), 3), rng.integers(0, 3, T).astype(float)])
    x, s, k, e = 0, 1, 2, 3
    p32 = _chain([cl(x), cl(s), cl(k), cl(e), dl(2), cst(0.5), cl(x), dl(0), cl(s), cst(-1.5), cl(k), dl(3), cl(e),
                  cst(2.0), dl(1), cl(x)], _CHAIN_OPS, abi.X_COS)
    deep = _deep([cl(x), cl(s), dl(2), cl(k), cst(1.5), cl(e), dl(1), cl(x)])
    assert prog_len(p32) == 32 and to_fx(deep)._need() == 8
    init = [S(x, _normal(0.0, 1.0)), S(s, DistD(abi.FAM_GAMMA, K(2.0), K(0.5))), S(k, DistD(abi.FAM_POISSON, K(3.0))),
            A(e, K(0.0, col(x, 0.5), col(s, 1.0)))]
    step = [S(x, _normal(K(0.0, dat(1), col(x, 0.9)), K(0.2, col(s, 0.25)))),
            O(K(0.0, dat(0)), _normal(K(0.0, col(x)), 0.7)),
            S(s, DistD(abi.FAM_GAMMA, K(2.0, col(k, 0.25)), K(0.5))),
            X(e, p32),
            S(k, DistD(abi.FAM_POISSON, K(0.5, col(s, 0.25)))),
            O(K(0.0, col(k), dat(3)), DistD(abi.FAM_POISSON, K(1.0, col(s, 1.0)))),
            X(e, deep),
            A(s, K(0.5, col(s, 0.5)))]
    return Case(name, 4, init, step, 4, data, T, ["real", "pos", "count", "wild"])


def _gen_init_observe(name):
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    init = [S(0, _normal(0.0, 1.0)), O(K(0.5), _normal(K(0.0, col(0)), 0.3)), S(1, _normal(K(0.0, col(0)), 1.0)),
            O(K(0.0, col(0)), _normal(K(0.0, col(1)), 0.5))]
    step = [S(0, _normal(K(0.0, col(0, 0.9)), 0.5)), O(K(0.0, dat(0)), _normal(K(0.0, col(0)), 1.0))]
    return Case(name, 2, init, step, 1, data, T, ["real", "real"])


def _gen_observe_first(name):
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.normal(0, 0.5, T), 3)])
    x, z, m = 0, 1, 2
    step = [O(K(0.0, dat(0)), _normal(K(0.0, col(x)), 1.0)),
            S(x, _normal(K(0.0, col(x, 0.9)), 0.5)),
            O(K(0.0, dat(1)), _normal(K(0.0, col(x, 0.5)), 0.8)),
            X(z, (abi.X_DIV, (abi.X_POWI, 2, cl(x)), cst(20.0))),
            O(K(0.0, dat(0)), _normal(K(0.0, col(z)), 1.5)),
            S(x, _normal(K(0.0, col(x, 0.95)), 0.3)),
            A(m, K(1.0, col(x, 2.0)))]
    return Case(name, 3, [S(x, _normal(0.0, 1.0))], step, 2, data, T, ["real", "real", "real"])


def _gen_nodata(name):
    step = [S(0, _normal(K(0.0, col(0, 0.9)), 0.5)), A(1, K(0.0, col(0, 0.5))),
            O(K(0.3), _normal(K(0.0, col(0)), 1.0)), O(K(0.0, col(1)), _normal(0.0, 0.6))]
    return Case(name, 2, [S(0, _normal(0.0, 1.0))], step, 0, None, T, ["real", "real"])


def _gen_wide_data(name):
    rng = _rng(name)
    data = np.column_stack([np.full(T, 1e300), np.round(rng.normal(0, 1, T), 3), np.full(T, math.nan),
                            np.round(rng.uniform(0.3, 1.2, T), 3)])   # columns 0 and 2 are never read
    step = [S(0, _normal(K(0.0, col(0, 0.9)), K(0.0, dat(3)))), X(1, (abi.X_ADD, cl(0), dl(1))),
            O(K(0.5), _normal(K(0.0, col(1)), 1.0))]
    return Case(name, 2, [S(0, _normal(0.0, 1.0))], step, 4, data, T, ["real", "real"])


def _gen_no_init(name):
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    step = [S(0, _normal(K(0.1, col(0, 0.9)), 0.5)), A(1, K(1.0, col(1))), O(K(0.0, dat(0)), _normal(K(0.0, col(0)), 1.0))]
    return Case(name, 2, [], step, 1, data, T, ["real", "count"])


# thresholds: the parameter values two bits choose between, by family. The samplers change
# branch between them (include/wsmc_terms.h): Poisson at a rate of 10 (inversion / PTRS), Gamma at
# a shape of 1 (the boost below it), Binomial at n min(p, 1 - p) = 10 (inversion / BTRS) and at
# p = 1/2 (the mirrored draw), NegativeBinomial through its Gamma and Poisson.
THRESHOLD_VALUES = {
    "thresholds_poisson": (0.5, 9.99, 10.0, 300.0),
    "thresholds_gamma": (0.2, 1.0, 50.0, 1.0),
    "thresholds_binomial": (0.2, 0.3, 0.8, 0.7),      # n = 40: n min(p, 1 - p) = 8, 12, 8, 12
    "thresholds_negbin": (0.4, 40.0, 0.4, 40.0),
}


def _gen_thresholds(name):
    rng = _rng(name)
    a, b, c, d = THRESHOLD_VALUES[name]
    b1, b2, p, v = 0, 1, 2, 3
    sel = (abi.X_IFELSE, cl(b1), (abi.X_IFELSE, cl(b2), cst(a), cst(b)), (abi.X_IFELSE, cl(b2), cst(c), cst(d)))
    if name == "thresholds_poisson":
        dist, data = DistD(abi.FAM_POISSON, K(0.0, col(p))), rng.integers(0, 13, T).astype(float)
    elif name == "thresholds_gamma":
        dist, data = DistD(abi.FAM_GAMMA, K(0.0, col(p)), K(1.0)), np.round(rng.uniform(0.2, 3.0, T), 3)
    elif name == "thresholds_binomial":
        dist, data = DistD(abi.FAM_BINOMIAL, K(40.0), K(0.0, col(p))), rng.integers(5, 30, T).astype(float)
    else:
        dist, data = DistD(abi.FAM_NEGBINOMIAL, K(0.0, col(p)), K(0.5)), rng.integers(0, 13, T).astype(float)
    half = DistD(abi.FAM_BERNOULLI, K(0.5))
    step = [S(b1, half), S(b2, half), X(p, sel), S(v, dist), O(K(0.0, dat(0)), dist), O(K(0.0, col(v)), dist)]
    return Case(name, 4, [], step, 1, data, T, ["bit", "bit", "pos", "count" if name != "thresholds_gamma" else "pos"])


def _gen_all_xops(name):
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    x = cl(0)
    X_ = abi
    p1 = (X_.X_IFELSE, (X_.X_AND, (X_.X_GE, x, cst(-0.5)), (X_.X_NOT, (X_.X_GT, x, cst(1.0)))), (X_.X_SQRT, x),
          (X_.X_LOG, (X_.X_MAX, x, cst(0.0))))   # NaN on [-0.5, 0), -inf below it
    p2 = (X_.X_NEG, (X_.X_SUB, (X_.X_DIV, (X_.X_EXP, (X_.X_MUL, x, cst(400.0))), (X_.X_ABS, x)),
                     (X_.X_DIV, cst(1.0), (X_.X_MIN, x, cst(0.0)))))
    p3 = (X_.X_ADD, (X_.X_ADD, (X_.X_POWI, 3, (X_.X_SIN, x)), (X_.X_POW, (X_.X_MAX, x, cst(0.5)), (X_.X_COS, x))),
          (X_.X_MUL, (X_.X_LOG1P, x),
           (X_.X_OR, (X_.X_LE, x, cst(0.0)), (X_.X_OR, (X_.X_EQ, x, cst(0.0)), (X_.X_NE, (X_.X_LT, x, cst(1.0)), cst(0.0))))))
    step = [S(0, _normal(K(0.0, col(0, 0.9)), 1.0)), O(K(0.0, dat(0)), _normal(K(0.0, col(0)), 1.0)),
            X(1, p1), X(2, p2), X(3, p3)]
    return Case(name, 4, [S(0, _normal(0.0, 1.0))], step, 1, data, T, ["real", "wild", "wild", "wild"])


PARTIAL_ALL_AT = 20    # partial_support: the step whose OBSERVE is -inf for every particle


def _gen_partial_support(name):
    data = np.round(_rng(name).uniform(0.0, 1.5, T), 3)
    data[PARTIAL_ALL_AT] = -100.0
    step = [S(0, _normal(K(0.0, col(0, 0.9)), 1.0)), O(K(0.0, col(0), dat(0)), DistD(abi.FAM_EXPONENTIAL, K(0.0), K(1.0)))]
    return Case(name, 1, [S(0, _normal(0.0, 1.0))], step, 1, data, T, ["real"])


def _gen_pre_state(name):
    """the spec run_pre_state runs: no `init`, its two columns made by statements before the run"""
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    step = [S(0, _normal(K(0.0, col(0, 0.9), col(1, 0.25)), 0.5)), A(1, K(0.0, col(1, 0.5), col(0, 0.25))),
            O(K(0.0, dat(0)), _normal(K(0.0, col(0)), 1.0))]
    return Case(name, 2, [], step, 1, data, T, ["real", "real"])


_DIRECTED_GEN = {"prog96": _gen_prog, "prog97": _gen_prog, "full": _gen_full, "init_observe": _gen_init_observe,
                 "observe_first": _gen_observe_first, "nodata": _gen_nodata, "wide_data": _gen_wide_data,
                 "no_init": _gen_no_init, "all_xops": _gen_all_xops, "partial_support": _gen_partial_support,
                 "pre_state": _gen_pre_state, **{n: _gen_thresholds for n in THRESHOLDS}}


def gen(seed, profile="mixed") -> Case:
    """mixed: seed in MIXED_SEEDS; directed: seed an index into DIRECTED, or the name itself"""
    if profile == "mixed":
        return gen_mixed(int(seed))
    name = seed if isinstance(seed, str) else DIRECTED[int(seed)]
    return _DIRECTED_GEN[name](name)


def corpus():
    return [gen(s, "mixed") for s in MIXED_SEEDS] + [gen(n, "directed") for n in DIRECTED]


# ---- the comparer -----------------------------------------------------------------------------
def compare(g, o, ev=None, trace=None, ess=None):
    """None, or what differs first between two backends after the same run: the column names, every
    column, the weights, every state field, the last ancestors, both evidences (ev: what g's run
    returned), the ESS traces, score(-1) and the fold over the whole tape. Finite values by their
    bits (-0.0 differs from 0.0), NaNs equal by position."""
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
    for k in STATE:
        if not same_value(sg[k], so[k]):
            return f"state.{k}: {sg[k]!r} != {so[k]!r}"
    a, b = g.last_ancestors(), o.last_ancestors()
    if not same_value(a, b):
        return "last_ancestors: " + _where(a, b)
    for what, a in (("the run's log evidence", ev), ("log_evidence()", g.log_evidence())):
        if a is not None and not same_value(a, o.log_evidence()):
            return f"{what}: {a!r} != {o.log_evidence()!r}"
    if trace is not None or ess is not None:
        if trace is None or ess is None or len(trace) != len(ess):
            return f"ESS trace: {None if trace is None else len(trace)} steps != {None if ess is None else len(ess)}"
        if not same_value(trace, ess):
            return "ESS trace (by step): " + _where(trace, ess)
    for d, what in ((-1, "score(-1)"), (so["depth"], "score(depth)")):
        a, b = g.score(d), o.score(d)
        if not same_value(a, b):
            return f"{what}: " + _where(a, b)
    return None


class Mismatch(AssertionError):
    pass


def replay(case, n, ess, scheme, segment, backend="hip") -> str:
    which = f"--seed {case.name[6:]} --profile mixed" if case.name.startswith("mixed-") else f"--name {case.name} --profile directed"
    names = {v: k for k, v in SCHEMES.items()}
    return (f"python tests/ssmfuzz.py {which} --n {n} --ess {ess} --scheme {names[scheme]} "
            f"--segment {0 if segment is None else segment} --backend {backend}")


def oracle_context(n, seed=SEED, base=None):
    """an Oracle behind Context.ssm_run's interface (the statements, which define the run): the CPU
    tests and `--backend oracle` drive `differential` and `run_pre_state` with it, no device"""
    from oracle import Oracle

    class OracleRun(base or Oracle):
        runs = 0

        def ssm_run(self, spec, data, ess_perc_min=1.0, scheme=abi.RESAMPLE_STRATIFIED, ess_trace=False, T=None):
            _, trace = spec.statements(self, data, ess_perc_min, scheme, T=T)
            self.runs += 1
            return (self.log_evidence(), trace) if ess_trace else self.log_evidence()

        def ssm_stats(self):
            return {"persistent_runs": self.runs, "statement_runs": 0}

        def set_ssm_segment(self, steps):
            pass

    return OracleRun(n, seed=seed)


def _fresh(n, segment, route, context):
    import wsmc
    from oracle import Oracle
    g = context(n) if context else wsmc.Context(n, seed=SEED)
    o = Oracle(n, seed=SEED)
    if segment is not None:
        g.set_ssm_segment(segment)
    if route == "statements":   # a column that is not the spec's: the run issues the statements itself
        for c in (g, o):
            c.assign(c.col_create("other", 1), [abi.Operand.const(0.3)])
    return g, o


def _run_pair(case, g, o, ess, scheme, horizon=None):
    """the fused run on g, the statements on o; what differs (None: nothing)"""
    h = case.T if horizon is None else horizon
    data = None if case.data is None else case.data[:h]
    ev, trace = g.ssm_run(case.ssm, data, ess_perc_min=ess, scheme=scheme, ess_trace=True, T=h)
    flags, etr = case.ssm.statements(o, data, ess_perc_min=ess, scheme=scheme, T=h)
    return compare(g, o, ev, trace, etr), flags


def locate(case, n, ess, scheme, segment, route, context=None):
    """the first differing step of a run that differs at the full horizon: fresh contexts at horizons
    1, 2, 4, ..., then a bisection. (step, what differs at the horizon that first shows it)"""
    def differs(h):
        g, o = _fresh(n, segment, route, context)
        try:
            return _run_pair(case, g, o, ess, scheme, h)[0]
        finally:
            g.close()
            o.close()

    lo, hi, why = 0, None, None      # horizons <= lo agree, horizon hi differs
    h = 1
    while hi is None and h < case.T:
        d = differs(h)
        if d:
            hi, why = h, d
        else:
            lo, h = h, h * 2
    if hi is None:
        hi, why = case.T, differs(case.T)
        if why is None:
            return None, "the rerun at the full horizon agrees (the difference does not reproduce)"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        d = differs(mid)
        if d:
            hi, why = mid, d
        else:
            lo = mid
    return hi - 1, why


def differential(case, n, ess=0.5, scheme=abi.RESAMPLE_STRATIFIED, segment=None, route="persistent", context=None):
    """`case` through ssm_run(..., ess_trace=True) on a fresh context and through SSM.statements on a
    fresh oracle of one seed; everything compared, and the route asserted from ssm_stats(). segment:
    steps per launch (None: the library's default). route="statements": a foreign column on both
    sides first. A difference (every call having returned WSMC_OK) is located and raised as
    Mismatch; an error of a call is raised as it is. Returns (the oracle's flags, the context's
    state)."""
    g, o = _fresh(n, segment, route, context)
    try:
        d, flags = _run_pair(case, g, o, ess, scheme)
        st = g.ssm_stats()
        took = (st["persistent_runs"], st["statement_runs"])
        state = g.get_state()
    finally:
        g.close()
        o.close()
    want = (1, 0) if route == "persistent" else (0, 1)
    assert took == want, f"{case.name} N={n}: (persistent, statement) runs {took}, expected {want} ({route})"
    if d:
        step, why = locate(case, n, ess, scheme, segment, route, context)
        raise Mismatch(f"{case.name} N={n} ess={ess} scheme={scheme} segment={segment} route={route}: {d}\n"
                       f"  first differing step: {step}: {why}\n  [{replay(case, n, ess, scheme, segment)}]\n{case.text()}")
    return flags, state


# ---- pre_state: a run entered from, and followed by, the statement operators ---------------------
def run_pre_state(n, ess, scheme=abi.RESAMPLE_STRATIFIED, context=None, check=True):
    """1. the spec's two columns through statements: Sample, Sample, Observe, resample(1.0), which
    resamples and (on a lazy store) leaves unmaterialised genealogy; 2. ssm_run without `init`
    (persistent: weights_changed is clear); 3. an autoRW Move on a spec column, whose fold reads
    the tape the run booked; 4. Observe, Resample, score(depth); 5. ssm_run again. Compared with
    the oracle after 2, 4 and 5. Returns the oracle's outcomes."""
    import wsmc
    from oracle import Oracle
    case = gen("pre_state", "directed")
    g = context(n) if context else wsmc.Context(n, seed=SEED)
    o = Oracle(n, seed=SEED)
    out = {}

    def same(what, a, b):
        if check and not same_value(a, b):
            raise Mismatch(f"pre_state N={n} ess={ess}: {what}: {a!r} != the oracle's {b!r}\n{case.text()}")

    def both(what, ev=None, trace=None, etr=None):
        d = compare(g, o, ev, trace, etr) if check else None
        if d:
            raise Mismatch(f"pre_state N={n} ess={ess}: after {what}: {d}\n{case.text()}")

    try:
        if hasattr(g, "store_set_lazy"):
            g.store_set_lazy(True)
        res = []
        for c in (g, o):
            ids = [c.col_create("c0", 1), c.col_create("c1", 1)]
            d0, d1 = abi.Dist(), abi.Dist()
            _normal(0.0, 1.0).fill(d0)
            _normal(K(0.0, col(ids[0], 0.5)), 1.0).fill(d1)
            c.sample(ids[0], d0)
            c.sample(ids[1], d1)
            ob = abi.Dist()
            _normal(K(0.0, col(ids[0])), 0.5).fill(ob)
            c.observe(ob, [abi.Operand.const(0.3)])
            res.append(c.resample(1.0, scheme))
        same("the first Resample", res[0], res[1])
        out["first_resample"] = res[1]
        if hasattr(g, "store_info"):   # the run is entered with genealogy it must materialise
            assert g.store_info()["stale_columns"] > 0, g.store_info()
        for k, data in enumerate((case.data, case.data[::-1].copy()[:10])):
            if k == 1:
                acc = [c.move(abi.PROPOSAL_AUTORW, [c.col_find("c0")], 1e-3) for c in (g, o)]
                same("the Move's accepted count", acc[0], acc[1])
                out["accepted"] = acc[1]
                res = []
                for c in (g, o):
                    ob = abi.Dist()
                    _normal(K(0.0, col(c.col_find("c1"))), 0.8).fill(ob)
                    c.observe(ob, [abi.Operand.const(-0.2)])
                    res.append(c.resample(ess, scheme))
                same("the Resample after the Move", res[0], res[1])
                same("score(depth)", g.score(g.get_state()["depth"]), o.score(o.get_state()["depth"]))
                both("the Move, Observe and Resample")
            ev, trace = g.ssm_run(case.ssm, data, ess_perc_min=ess, scheme=scheme, ess_trace=True)
            flags, etr = case.ssm.statements(o, data, ess_perc_min=ess, scheme=scheme)
            both(f"run {k + 1}", ev, trace, etr)
            out[f"flags{k + 1}"] = flags
            if hasattr(g, "ssm_stats"):
                st = g.ssm_stats()
                assert (st["persistent_runs"], st["statement_runs"]) == (k + 1, 0), st
        out["state"] = o.get_state()
    finally:
        g.close()
        o.close()
    return out


# ---- command line -----------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--name", choices=DIRECTED, default=None, help="a directed case (with --profile directed)")
    ap.add_argument("--profile", choices=PROFILES, default="mixed")
    ap.add_argument("--n", type=int, default=1001)
    ap.add_argument("--ess", type=float, default=0.5)
    ap.add_argument("--scheme", choices=sorted(SCHEMES), default="stratified")
    ap.add_argument("--segment", type=int, default=0, help="steps per launch (0: the library's default)")
    ap.add_argument("--route", choices=("persistent", "statements"), default=None)
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    a = ap.parse_args(argv)
    from oracle import Oracle
    case = gen(a.name if (a.profile == "directed" and a.name) else a.seed, a.profile)
    print(case.text())
    scheme = SCHEMES[a.scheme]
    if case.name == "pre_state":
        if a.backend == "oracle":
            print(run_pre_state(a.n, a.ess, scheme, context=oracle_context, check=False))
            return 0
        try:
            print("same as the oracle;", run_pre_state(a.n, a.ess, scheme))
            return 0
        except Mismatch as e:
            print("MISMATCH", e)
            return 1
    if a.backend == "oracle":
        o = Oracle(a.n, seed=SEED)
        flags, ess = case.ssm.statements(o, case.data, ess_perc_min=a.ess, scheme=scheme, T=case.T)
        print("resampled", "".join("x" if f else "." for f in flags))
        print("ESS%", np.array2string(np.asarray(ess), precision=4, max_line_width=160))
        print("state", o.get_state(), "log_evidence", o.log_evidence())
        return 0
    import wsmc
    g = wsmc.Context(1, seed=SEED)
    cap = g.ssm_stats()["cap"]
    g.close()
    route = a.route or case.route(a.n, scheme, cap)
    try:
        flags, state = differential(case, a.n, a.ess, scheme, a.segment or None, route)
        print(f"same as the oracle ({route} route); resampled", "".join("x" if f else "." for f in flags), "state", state)
        return 0
    except Mismatch as e:
        print("MISMATCH", e)
        return 1


if __name__ == "__main__":
    sys.exit(main())

"""Seeded random and directed scalar-SSM specs with the two weighting statements of the guided
fused runs: importance Samples (WSMC_SSM_SAMPLE_IMPORTANCE) and WEIGHTs (WSMC_SSM_WEIGHT).

TEST INFRASTRUCTURE, built on tests/ssmfuzz.py by import: its `Case`, `compare` and
`differential` run and compare a case here as they do there (the fused run on a fresh
`wsmc.Context` against `SSM.statements` on a fresh `oracle.Oracle`, everything bit for bit).

    python tests/ssmguidedfuzz.py --seed 3 --n 1001 --ess 0.5 --scheme stratified --segment 5 --backend hip
    python tests/ssmguidedfuzz.py --name after_last_observe --backend oracle

Two more statement descriptors beside ssmfuzz's:
    ("isample", col, proposal DistD, target DistD)      col ~ importance_kernel(proposal, target)
    ("weight", value Opnd, DistD)                       _ ~ dist, scored at value

The random profile keeps ssmfuzz's loop invariant by construction rather than by search. Each spec
has one state column per kind it uses, every one rewritten each step by a plain SAMPLE or an
importance Sample of a family of that kind whose parameters are constants, data or bounded reads
(ssmfuzz's operand generator, with its contraction rules). A proposal and its target are two
families of one output kind (the draw lies in the target's support: Uniform(0, 1) goes with Beta),
the proposals taken in a round robin over the 21 scalar families and each target the next family
of its proposal's kind, so that every family is met in both roles over the seeds; the four
parameter positions of an importance Sample (proposal mean and scale, target mean and scale) each
take their operand form from a rotation of their own. Heavy families draw into columns that only
values and Assigns read.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

import ssmfuzz as sf
from ssmfuzz import A, DistD, K, O, S, X, col, dat
from progfuzz import _FAM, FAMILIES

from wsmc import abi, models  # noqa: E402

T = 12                      # with set_ssm_segment(5): three launches, the last of 2 steps
SEED = sf.SEED
SEEDS = list(range(24))
DIRECTED = ["self_reading", "data_slots", "init_importance", "after_last_observe", "eight_statements", "uniform_in_normal",
            "all_neg_inf", "nan_weights", "base_families", "extended_families", "log_gamma", "four_columns", "lgssm1d_guided"]
PROFILES = ("random", "directed")
IS_POSITIONS = ("prop_mean", "prop_scale", "targ_mean", "targ_scale")
_SALT = 31


def IS(c, prop, targ):
    return ("isample", int(c), prop, targ)


def W(value, d):
    return ("weight", value, d)


def _plain(st):
    """the statement ssmfuzz.Case can fill in an importance Sample's or a WEIGHT's place"""
    if st[0] == "isample":
        return S(st[1], st[2])
    if st[0] == "weight":
        return O(st[1], st[2])
    return st


def stmt_repr(st) -> str:
    if st[0] == "isample":
        return f"c{st[1]} ~ importance_kernel({st[2]!r}, {st[3]!r})"
    if st[0] == "weight":
        return f"_ ~ {st[2]!r} at {st[1]!r}"
    return sf.stmt_repr(st)


class GuidedCase(sf.Case):
    """ssmfuzz.Case with the two new kinds: the struct is filled through their plain twins, then the
    kind and the target are set in place (SSM.from_spec uses the struct as it is)"""

    def __init__(self, name, n_cols, init, step, data_dim=0, data=None, T=T, kinds=None, data_kinds=None):
        super().__init__(name, n_cols, [_plain(s) for s in init], [_plain(s) for s in step], data_dim, data, T, kinds, data_kinds)
        self.init, self.step = list(init), list(step)
        for arr, lst in ((self.spec.init, self.init), (self.spec.step, self.step)):
            for k, st in enumerate(lst):
                if st[0] == "isample":
                    arr[k].kind = abi.SSM_SAMPLE_IMPORTANCE
                    st[3].fill(arr[k].target)
                elif st[0] == "weight":
                    arr[k].kind = abi.SSM_WEIGHT
        self.lines = (self.lines[:1] + [f"init[{k}]  {stmt_repr(s)}" for k, s in enumerate(self.init)]
                      + [f"step[{k}]  {stmt_repr(s)}" for k, s in enumerate(self.step)])

    def dists(self):
        for _, _, s in self.statements():
            if s[0] in ("sample", "observe", "weight"):
                yield s[2]
            elif s[0] == "isample":
                yield s[2]
                yield s[3]

    def feat(self) -> int:
        fams = [d.fam for d in self.dists()]
        if any(f >= abi.FAM_GAMMA for f in fams):
            return 2
        return 1 if any(abi.FAM_BERNOULLI <= f <= abi.FAM_GEOMETRIC for f in fams) else 0

    @property
    def guided(self) -> bool:
        return any(s[0] in ("isample", "weight") for _, _, s in self.statements())

    @property
    def trace_slot(self):
        """(slots a step, the last OBSERVE's slot): the Resamples of a step that can run"""
        slots = [s[0] for s in self.step if s[0] in ("observe", "weight", "isample")]
        return len(slots), max(k for k, s in enumerate(slots) if s == "observe")


# ---- the random profile -----------------------------------------------------------------------
_BY_KIND = {}
for _f in sf.SCALAR_FAMILIES:
    _BY_KIND.setdefault(_FAM[_f][2], []).append(_f)
# Uniform(0, 1) draws a probability: it stands with Beta, so that every family has a partner of its kind
_BY_KIND["real"].remove(abi.FAM_UNIFORM)
_BY_KIND["prob"].append(abi.FAM_UNIFORM)
# the kind a family's draw is of here, and the order the two round robins go through the families in
_KIND_OF = {f: k for k, fs in _BY_KIND.items() for f in fs}
_ORDER = sorted(sf.SCALAR_FAMILIES)


class _Gen(sf._SsmGen):
    def __init__(self, seed):
        super().__init__(seed)
        self.rng = np.random.default_rng([self.seed, _SALT])
        self.uniform_params = (0.0, 1.0)
        self.isform = {p: 0 for p in IS_POSITIONS}

    def is_operand(self, position, w, bounded_only=False):
        """ssmfuzz's `operand`, with a rotation of the forms per importance-Sample position"""
        n = self.isform[position]
        self.isform[position] += 1
        order = [sf.FORMS[(self.seed + n + 2 * IS_POSITIONS.index(position) + k) % len(sf.FORMS)] for k in range(len(sf.FORMS))]
        for f in order:
            o = self.build(w, f, bounded_only)
            if o is not None:
                return o
        raise AssertionError((w, position))

    def is_dist(self, fam, role):
        if fam == abi.FAM_UNIFORM:
            return DistD(fam, K(0.0), K(1.0), (0.0, 1.0))
        p1, p2 = _FAM[fam][:2]
        mu = self.is_operand(role + "_mean", p1) if p1 else K(0.0)
        tight = p1 in ("shape", "nint") and self.reads_unbounded(mu)
        if p2 and fam == abi.FAM_NEGBINOMIAL and tight:
            sc = K(sf._r(self.rng, 0.4, 0.9))
        else:
            sc = self.is_operand(role + "_scale", p2, bounded_only=tight) if p2 else K(1.0)
        return DistD(fam, mu, sc)


_N_IS = (1, 2, 0, 2, 1, 1)


def gen_random(seed) -> GuidedCase:
    seed = int(seed)
    g = _Gen(seed)
    rng = g.rng
    n_is = _N_IS[seed % 6]                         # importance Samples, over init and step
    n_w = (1, 0, 2, 1, 2, 0)[(seed // 2) % 6]      # WEIGHTs
    if n_is + n_w == 0:
        n_w = 1
    n_obs = 1 + seed % 3
    data_dim = 1 + seed % 4
    g.data_kinds = [sf._DATA_KINDS[(seed + 2 * j) % 5] for j in range(data_dim)]
    # the corpus' importance Samples are numbered through the seeds: number k proposes from family
    # k of the order (mod 21) under the next family of that kind as its target (the one after it
    # from k = 21 on), so the first 21 of them meet every family in both roles
    pairs = []
    for j in range(n_is):
        k = sum(_N_IS[s % 6] for s in range(seed)) + j
        prop = _ORDER[k % len(_ORDER)]
        mates = _BY_KIND[_KIND_OF[prop]]
        pairs.append((prop, mates[(mates.index(prop) + 1 + k // len(_ORDER)) % len(mates)]))
    # the state columns: one per kind the importance Samples draw, and a real one the OBSERVEs read
    kinds = []
    for prop, _ in pairs:
        k = (_KIND_OF[prop], _FAM[prop][4])
        if k not in kinds:
            kinds.append(k)
    if ("real", False) not in kinds and len(kinds) < 4:
        kinds.append(("real", False))
    if len(kinds) < 2 + seed % 3 and len(kinds) < 4:
        kinds.append((("pos", False), ("prob", False), ("count", False))[seed % 3])
        kinds = list(dict.fromkeys(kinds))
    g.cols = [dict(kind=k, heavy=h) for k, h in kinds]
    n_cols = len(g.cols)
    col_of = {k: i for i, k in enumerate(kinds)}
    # a plain family per column, for the SAMPLE that starts it in `init` and keeps it moving in `step`
    plain = {}
    for i, (k, h) in enumerate(kinds):
        fs = [f for f in _BY_KIND[k] if _FAM[f][4] == h and f != abi.FAM_UNIFORM] or [f for f in _BY_KIND[k] if f != abi.FAM_UNIFORM]
        plain[i] = fs[(seed + i) % len(fs)]

    # where the new statements stand: importance Sample 0 goes to `init` for seeds 1 mod 4, a WEIGHT
    # for seeds 2 mod 4, the others to `step`
    init = [g.sample(plain[i], i) for i in range(min(n_cols, 3))]   # (constants and earlier columns: init reads no data)
    step = []
    is_init = 1 if (n_is and seed % 4 == 1) else 0
    w_init = 1 if (n_w and seed % 4 == 2 and len(init) < 4) else 0

    def isample(j):
        prop, targ = pairs[j]
        c = col_of[(_KIND_OF[prop], _FAM[prop][4])]
        return IS(c, g.is_dist(prop, "prop"), g.is_dist(targ, "targ"))

    def weight():
        fam = g.obs_queue.pop(0)
        for _ in range(len(sf.SCALAR_FAMILIES)):
            st = g.observe(fam, None)
            if st is not None:
                return W(st[1], st[2])
            fam = g.obs_queue.pop(0)
        raise AssertionError("no WEIGHT")

    if is_init and len(init) < 4:
        init.append(isample(0))
    else:
        is_init = 0
    if w_init and len(init) < 4:
        init.append(weight())
    else:
        w_init = 0
    g.in_step = True
    body = [("isample", j) for j in range(is_init, n_is)] + [("weight", None)] * (n_w - w_init)
    moved = {col_of[(_KIND_OF[p], _FAM[p][4])] for p, _ in pairs[is_init:]}
    body += [("sample", i) for i in range(n_cols) if i not in moved][:max(0, 8 - n_obs - len(body))]
    order = list(rng.permutation(len(body)))
    body = [body[k] for k in order]
    # the OBSERVEs: the last one after a statement that draws, for seeds 0 mod 3 not at the step's end
    slots = sorted(int(v) for v in rng.choice(len(body) + 1, size=n_obs, replace=True))
    if seed % 3 == 0 and len(body) > 1:
        slots = [min(s, len(body) - 1) for s in slots]
    drew = set()
    out = []
    for k in range(len(body) + 1):
        for _ in range(slots.count(k)):
            out.append(("observe", frozenset(drew) or None))
        if k < len(body):
            out.append(body[k])
            if body[k][0] != "weight":
                drew.add(body[k][1] if body[k][0] == "sample" else col_of[(_KIND_OF[pairs[body[k][1]][0]], _FAM[pairs[body[k][1]][0]][4])])
    if out[0][0] == "observe" and out[0][1] is None and len(out) > 1 and seed % 4 != 1:
        out.pop(0)               # nothing drawn yet: the OBSERVE goes to the end, where it reads what the step drew
        out.append(("observe", frozenset(drew) or None))
    for kd, arg in out[:8]:
        if kd == "isample":
            step.append(isample(arg))
        elif kd == "weight":
            step.append(weight())
        elif kd == "sample":
            step.append(g.sample(plain[arg], arg))
        else:
            step.append(g.next_observe(set(arg) if arg else None))
    if not any(s[0] == "observe" for s in step):
        step[-1] = g.next_observe(None)
    data = np.column_stack([sf._data_values(rng, k, T) for k in g.data_kinds])
    return GuidedCase(f"random-{seed}", n_cols, init, step, data_dim, data, T, [k + ("*" if h else "") for k, h in kinds],
                      list(g.data_kinds))


# ---- the directed cases -----------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng([DIRECTED.index(name), _SALT + 2])


def _normal(mu, sc):
    return DistD(abi.FAM_NORMAL, mu if isinstance(mu, sf.Opnd) else K(mu), sc if isinstance(sc, sf.Opnd) else K(sc))


def _obs(c=0, sc=1.0, j=0):
    return O(K(0.0, dat(j)), _normal(K(0.0, col(c)), sc))


def _gen_self_reading(name):
    """proposal and target both read the output column: the draw uses the old value, both
    densities are taken with the new one in their parameters"""
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    step = [IS(0, _normal(K(0.1, col(0, 0.9)), K(0.6)), _normal(K(0.0, col(0, 0.5)), K(0.8, col(1, 0.25)))), _obs(0)]
    return GuidedCase(name, 2, [S(0, _normal(0.0, 1.0)), S(1, DistD(abi.FAM_BERNOULLI, K(0.5)))], step, 1, data, T, ["real", "bit"])


def _gen_data_slots(name):
    """a data slot in the proposal's mean (slot 0), in the target's mean (slot 1 behind a column), in both scales"""
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.uniform(0.4, 1.5, T), 3)])
    step = [A(1, K(0.0, col(0))),
            IS(0, _normal(K(0.0, dat(0), col(1, 0.5)), K(0.0, dat(1))), _normal(K(0.0, col(1, 0.9), dat(0)), K(0.0, None, dat(1)))),
            _obs(0, 0.7)]
    return GuidedCase(name, 2, [S(0, _normal(0.0, 1.0))], step, 2, data, T, ["real", "real"])


def _gen_init_importance(name):
    """an importance Sample in `init`: its Resample runs (ess 1.0) before the first step"""
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    init = [S(1, _normal(0.0, 1.0)), IS(0, _normal(K(0.0, col(1, 0.5)), 2.0), _normal(0.5, 0.7))]
    step = [S(0, _normal(K(0.0, col(0, 0.9)), 0.5)), _obs(0)]
    return GuidedCase(name, 2, init, step, 1, data, T, ["real", "real"])


def _gen_after_last_observe(name):
    """an importance Sample and a WEIGHT after the step's last OBSERVE: the trace slot (1) is not the
    step's last slot (3), and the trace point's columns are not the step's final ones"""
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.normal(0, 0.5, T), 3)])
    step = [W(K(0.0, col(0)), _normal(0.0, 3.0)),
            _obs(0, 1.0),
            A(1, K(0.0, col(0))),
            IS(0, _normal(K(0.0, col(1, 0.8), dat(1)), 0.7), _normal(K(0.0, col(1, 0.9)), 0.5)),
            W(K(0.0, dat(0)), DistD(abi.FAM_LAPLACE, K(0.0, col(0)), K(1.5)))]
    return GuidedCase(name, 2, [S(0, _normal(0.0, 1.0))], step, 2, data, T, ["real", "real"])


def _gen_eight_statements(name):
    """eight step statements: two importance Samples, a WEIGHT and two OBSERVEs among them"""
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.normal(0, 0.5, T), 3)])
    x, xp, v = 0, 1, 2
    step = [A(xp, K(0.0, col(x))),
            IS(x, _normal(K(0.0, col(xp, 0.5), dat(0)), 0.8), _normal(K(0.0, col(xp, 0.9)), 1.0)),
            _obs(x, 0.9),
            X(v, (abi.X_MUL, sf.cl(x), sf.cst(0.5))),
            IS(v, DistD(abi.FAM_LOGISTIC, K(0.0, col(v)), K(0.5)), DistD(abi.FAM_LAPLACE, K(0.0, col(x, 0.5)), K(0.7))),
            W(K(0.0, col(v)), _normal(K(0.0, dat(1)), 2.0)),
            _obs(v, 1.2, 1),
            A(xp, K(1.0, col(v, 2.0)))]
    return GuidedCase(name, 3, [S(x, _normal(0.0, 1.0))], step, 2, data, T, ["real", "real", "real"])


def _gen_uniform_in_normal(name):
    """a Uniform(-1, 1) target inside a Normal proposal: the draws outside get a weight of -inf"""
    data = np.round(_rng(name).normal(0.0, 0.5, T), 3)
    step = [IS(0, _normal(K(0.0, col(0, 0.5)), 1.0), DistD(abi.FAM_UNIFORM, K(0.0), K(1.0), (-1.0, 1.0))), _obs(0, 0.8)]
    return GuidedCase(name, 1, [S(0, _normal(0.0, 0.3))], step, 1, data, T, ["real"])


ALL_NEG_INF_AT = 6    # all_neg_inf: the step from which every weight is -inf


def _gen_all_neg_inf(name):
    """the WEIGHT scores data - x under Uniform(-50, 0): finite while data is 0, -inf for every
    particle once it is 100. From that step on every weight is -inf (an importance Sample adds a
    finite number to it), no Resample runs again and the ESS% stays NaN"""
    data = np.zeros(T)
    data[ALL_NEG_INF_AT:] = 100.0
    step = [IS(0, DistD(abi.FAM_HALFNORMAL, K(0.0), K(1.0)), DistD(abi.FAM_EXPONENTIAL, K(0.0), K(1.0))),
            A(1, K(0.0, col(0), None)),
            O(K(0.0, col(0, 1.0), None), DistD(abi.FAM_EXPONENTIAL, K(0.0), K(2.0))),
            W(K(0.0, dat(0), col(0, -1.0)), DistD(abi.FAM_UNIFORM, K(0.0), K(1.0), (-50.0, 0.0)))]
    return GuidedCase(name, 2, [S(0, DistD(abi.FAM_HALFNORMAL, K(0.0), K(1.0)))], step, 1, data, T, ["pos", "pos"])


def _gen_nan_weights(name):
    """a target whose scale goes negative for some particles: NaN weights from the first step"""
    data = np.round(_rng(name).normal(0.0, 1.0, T), 3)
    step = [A(1, K(0.0, col(0))),
            IS(0, _normal(K(0.0, col(1, 0.9)), 1.0), _normal(K(0.0, col(1, 0.9)), K(0.5, col(1, 1.0)))),
            _obs(0)]
    return GuidedCase(name, 2, [S(0, _normal(0.0, 1.0))], step, 1, data, T, ["real", "real"])


def _gen_base_families(name):
    """Normal, HalfNormal and Uniform alone: the plain kernel variant"""
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.uniform(0.1, 0.9, T), 3)])
    step = [IS(0, _normal(K(0.0, col(0, 0.7), dat(0)), 1.2), _normal(K(0.0, col(0, 0.9)), 0.8)),
            IS(1, DistD(abi.FAM_HALFNORMAL, K(0.0), K(0.5, col(2, 0.5))), DistD(abi.FAM_HALFNORMAL, K(0.0), K(1.0))),
            IS(2, DistD(abi.FAM_UNIFORM, K(0.0), K(1.0), (0.0, 1.0)), DistD(abi.FAM_UNIFORM, K(0.0), K(1.0), (-0.5, 1.5))),
            W(K(0.0, col(1)), DistD(abi.FAM_HALFNORMAL, K(0.0), K(0.0, dat(1)))),
            _obs(0)]
    init = [S(0, _normal(0.0, 1.0)), S(1, DistD(abi.FAM_HALFNORMAL, K(0.0), K(1.0))), S(2, DistD(abi.FAM_UNIFORM, K(0.0), K(1.0), (0.0, 1.0)))]
    return GuidedCase(name, 3, init, step, 2, data, T, ["real", "pos", "prob"])


def _gen_extended_families(name):
    """Bernoulli .. Geometric without a log-Gamma family: the extended kernel variant"""
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), rng.integers(0, 5, T).astype(float)])
    step = [IS(0, DistD(abi.FAM_LAPLACE, K(0.0, col(0, 0.8)), K(0.9)), DistD(abi.FAM_GUMBEL, K(0.0, col(0, 0.5)), K(1.0))),
            IS(1, DistD(abi.FAM_EXPONENTIAL, K(0.0), K(0.5, col(2, 0.5))), DistD(abi.FAM_RAYLEIGH, K(0.0), K(1.0))),
            IS(2, DistD(abi.FAM_BERNOULLI, K(0.4)), DistD(abi.FAM_BERNOULLI_LOGIT, K(0.0, col(0, 0.5)))),
            W(K(0.0, dat(1)), DistD(abi.FAM_GEOMETRIC, K(0.2, col(2, 0.5)))),
            O(K(0.0, dat(0)), DistD(abi.FAM_LOGISTIC, K(0.0, col(0)), K(0.8)))]
    init = [S(0, _normal(0.0, 1.0)), S(1, DistD(abi.FAM_EXPONENTIAL, K(0.0), K(1.0))), S(2, DistD(abi.FAM_BERNOULLI, K(0.5)))]
    return GuidedCase(name, 3, init, step, 2, data, T, ["real", "pos", "bit"])


def _gen_log_gamma(name):
    """a Gamma proposal under an InverseGamma target, a Poisson proposal under a NegativeBinomial
    one: the log-Gamma kernel variant (a sampler that rejects, and two log-Gammas, live at once)"""
    rng = _rng(name)
    data = np.column_stack([np.round(rng.uniform(0.3, 3.0, T), 3), rng.integers(0, 9, T).astype(float)])
    step = [IS(0, DistD(abi.FAM_GAMMA, K(2.0, col(2, 0.25)), K(0.0, col(2, 0.5), dat(0))), DistD(abi.FAM_INVERSEGAMMA, K(3.0), K(1.0, col(2, 0.5)))),
            IS(1, DistD(abi.FAM_POISSON, K(1.0, col(2, 2.0))), DistD(abi.FAM_NEGBINOMIAL, K(2.5), K(0.4))),
            S(2, DistD(abi.FAM_BETA, K(2.0), K(3.0))),
            W(K(0.0, col(2)), DistD(abi.FAM_BETA, K(1.5), K(1.5))),
            O(K(0.0, dat(0)), DistD(abi.FAM_GAMMA, K(1.0, col(0, 1.0)), K(1.0))),
            O(K(0.0, dat(1)), DistD(abi.FAM_POISSON, K(0.5, col(1, 0.5))))]
    init = [S(0, DistD(abi.FAM_GAMMA, K(2.0), K(0.5))), S(1, DistD(abi.FAM_POISSON, K(2.0))), S(2, DistD(abi.FAM_BETA, K(2.0), K(2.0)))]
    return GuidedCase(name, 3, init, step, 2, data, T, ["pos", "count", "prob"])


def _gen_four_columns(name):
    rng = _rng(name)
    data = np.column_stack([np.round(rng.normal(0, 1, T), 3), np.round(rng.normal(0, 0.5, T), 3)])
    x, xp, m, s = 0, 1, 2, 3
    init = [S(x, _normal(0.0, 1.0)), S(s, DistD(abi.FAM_GAMMA, K(4.0), K(0.25))),
            IS(m, _normal(K(0.0, col(x)), 1.0), _normal(0.0, 1.5)), W(K(0.0, col(s)), DistD(abi.FAM_EXPONENTIAL, K(0.0), K(1.0)))]
    step = [A(xp, K(0.0, col(x))),
            A(m, K(0.0, col(xp, 0.45), dat(0))),
            IS(x, _normal(K(0.0, col(m)), K(0.0, col(s, 0.5))), _normal(K(0.0, col(xp, 0.9)), K(0.0, col(s)))),
            _obs(x, 0.6),
            IS(s, DistD(abi.FAM_GAMMA, K(4.0), K(0.0, col(s, 0.25))), DistD(abi.FAM_LOGNORMAL, K(0.0), K(0.5))),
            W(K(0.0, dat(1)), _normal(K(0.0, col(x, 0.5)), K(0.0, col(s))))]
    return GuidedCase(name, 4, init, step, 2, data, T, ["real", "real", "real", "pos"])


class ModelCase:
    """models.lgssm1d_guided() itself behind GuidedCase's interface (the builder's spec, not a raw one)"""

    def __init__(self, name):
        self.name, self.ssm, self.T = name, models.lgssm1d_guided(), T
        self.spec = self.ssm.spec
        self.data = models.lgssm1d_data(T).reshape(T, 1)
        self.n_cols, self.data_dim = 3, 1
        self.init = [S(0, _normal(0.0, 1.0))]
        self.step = [A(1, K(0.0, col(0))), ("expr", 2, None), IS(0, _normal(K(0.0, col(2)), 0.0), _normal(K(0.0, col(1)), 1.0)), _obs(0)]
        self.lines = ["models.lgssm1d_guided()  T %d" % T]
        self.n_prog = sum(self.spec.step[q].prog_len for q in range(self.spec.n_step))
        self.guided, self.trace_slot = True, (2, 1)

    text = sf.Case.text
    statements = sf.Case.statements
    route = sf.Case.route
    dists = GuidedCase.dists
    feat = GuidedCase.feat


_DIRECTED_GEN = {"self_reading": _gen_self_reading, "data_slots": _gen_data_slots, "init_importance": _gen_init_importance,
                 "after_last_observe": _gen_after_last_observe, "eight_statements": _gen_eight_statements,
                 "uniform_in_normal": _gen_uniform_in_normal, "all_neg_inf": _gen_all_neg_inf, "nan_weights": _gen_nan_weights,
                 "base_families": _gen_base_families, "extended_families": _gen_extended_families, "log_gamma": _gen_log_gamma,
                 "four_columns": _gen_four_columns, "lgssm1d_guided": ModelCase}


def gen(seed, profile="random"):
    if profile == "random":
        return gen_random(int(seed))
    name = seed if isinstance(seed, str) else DIRECTED[int(seed)]
    return _DIRECTED_GEN[name](name)


def corpus():
    return [gen(s, "random") for s in SEEDS] + [gen(n, "directed") for n in DIRECTED]


def replay(case, n, ess, scheme, segment, backend="hip") -> str:
    which = f"--seed {case.name[7:]}" if case.name.startswith("random-") else f"--name {case.name}"
    names = {v: k for k, v in sf.SCHEMES.items()}
    return (f"python tests/ssmguidedfuzz.py {which} --n {n} --ess {ess} --scheme {names[scheme]} "
            f"--segment {0 if segment is None else segment} --backend {backend}")


def differential(case, n, ess=0.5, scheme=abi.RESAMPLE_STRATIFIED, segment=None, route="persistent", context=None):
    """ssmfuzz.differential, with this file's replay line in a Mismatch"""
    try:
        return sf.differential(case, n, ess, scheme, segment, route, context)
    except sf.Mismatch as e:
        raise sf.Mismatch(f"{e}\n  [{replay(case, n, ess, scheme, segment)}]") from None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--name", choices=DIRECTED, default=None, help="a directed case")
    ap.add_argument("--n", type=int, default=1001)
    ap.add_argument("--ess", type=float, default=0.5)
    ap.add_argument("--scheme", choices=sorted(sf.SCHEMES), default="stratified")
    ap.add_argument("--segment", type=int, default=0, help="steps per launch (0: the library's default)")
    ap.add_argument("--route", choices=("persistent", "statements"), default=None)
    ap.add_argument("--backend", choices=("oracle", "hip"), default="oracle")
    a = ap.parse_args(argv)
    case = gen(a.name, "directed") if a.name else gen(a.seed, "random")
    print(case.text())
    scheme = sf.SCHEMES[a.scheme]
    if a.backend == "oracle":
        from oracle import Oracle
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
    except sf.Mismatch as e:
        print("MISMATCH", e)
        return 1


if __name__ == "__main__":
    sys.exit(main())

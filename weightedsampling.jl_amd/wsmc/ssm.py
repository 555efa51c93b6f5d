"""Scalar state-space models the caller specifies (include/wsmc.h wsmc_ssm_spec, wsmc_ssm_run).

    from wsmc import SSM, Col, Normal
    from wsmc.dsl import Data, exp
    from wsmc.ssm import sample, assign, observe

    sv = (SSM(cols=["h", "s"])
          .init(sample("h", Normal(0.0, 0.5)))
          .step(sample("h", Normal(0.95 * Col("h"), 0.2)),
                assign("s", exp(Col("h") / 2)),
                observe(Data(0), Normal(0.0, Col("s")))))
    ev = ctx.ssm_run(sv, y)                    # one call (a persistent workgroup where it fits)
    sv.statements(ctx_or_oracle, y)            # the same statements, issued one by one

`sample(col, importance_kernel(proposal, target))` is the reference's `x ~ importance_kernel(...)`:
the draw comes from the proposal and the weights gain logpdf(target, x) - logpdf(proposal, x), both
read after x is stored (a transition target needs the old state copied to another column first);
`weight(value, kernel)` is `_ ~ kernel` scored at value. A proposal with lighter tails than its
target gives weights of unbounded variance: the evidence estimate then gets worse, not better.

Every `sample`, `observe` and `weight` is followed by its auto-inserted Resample (what @model inserts); an
`assign` whose right-hand side is affine in at most two columns lowers to WSMC_SSM_ASSIGN, every
other one to WSMC_SSM_ASSIGN_EXPR (a postfix program). `Data(j)` is column j of the run's data
table at the current step; only `step` may read it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import Operand
from .dsl import DATA, Expr, Fx, Kernel, xprogram


def sample(col: str, kernel):
    """col ~ kernel, or col ~ importance_kernel(proposal, target) (wsmc.importance_kernel)"""
    if hasattr(kernel, "proposal") and hasattr(kernel, "target"):
        return (abi.SSM_SAMPLE_IMPORTANCE, str(col), kernel)
    return (abi.SSM_SAMPLE, str(col), kernel)


def assign(col: str, rhs):
    """col .= rhs"""
    return (abi.SSM_ASSIGN, str(col), rhs)


def observe(value, kernel: Kernel):
    """value => kernel"""
    return (abi.SSM_OBSERVE, value, kernel)


def weight(value, kernel: Kernel):
    """_ ~ kernel, scored at value"""
    return (abi.SSM_WEIGHT, value, kernel)


def _general(rhs) -> bool:
    """the right-hand side needs a program: an Fx, or an affine form whose merged operand would
    round differently from the user's own order (Expr.fx)"""
    if isinstance(rhs, Fx) or (isinstance(rhs, Expr) and rhs.fx is not None):
        return True
    # a data reference the operand form cannot fold exactly (a scaled one, one beside a constant,
    # two of them): the same affine form as a program, where a data read is a leaf
    data = [coef for name, _, coef in rhs.terms if name == DATA] if isinstance(rhs, Expr) else []
    return bool(data) and (len(data) > 1 or data[0] != 1.0 or rhs.c0 != 0.0)


def batch_arguments(specs, data, n, seeds, T=None):
    """Context.ssm_run_batch's arguments, checked on the host alone: (the specs as a list of 1 or
    B, the tables as a list of 1 or B arrays of one shape, the seeds as B uint64). ValueError names
    the argument whose length fits neither 1 nor B = len(seeds)."""
    seeds_a = np.ascontiguousarray(np.asarray([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64))
    B = len(seeds_a)
    if B < 1:
        raise ValueError("seeds: at least one filter")
    if int(n) < 1:
        raise ValueError("n: at least one particle")
    spec_list = list(specs) if isinstance(specs, (list, tuple)) else [specs]
    if len(spec_list) not in (1, B):
        raise ValueError(f"specs: one spec or one per filter ({B}), got {len(spec_list)}")
    first = spec_list[0]
    # B tables: a 3-D array, or a list of arrays (a list of numbers or of rows is one table)
    many = isinstance(data, np.ndarray) and data.ndim == 3
    many = many or (isinstance(data, (list, tuple)) and len(data) > 0 and all(isinstance(d, np.ndarray) for d in data))
    tabs = [first.table(d, T) for d in data] if many else [first.table(data, T)]
    if len(tabs) not in (1, B):
        raise ValueError(f"data: one table or one per filter ({B}), got {len(tabs)}")
    if any(t.shape != tabs[0].shape for t in tabs):
        raise ValueError("data: the filters' tables must have one length")
    if len(tabs[0]) < 1:
        raise ValueError("data: at least one step")
    return spec_list, tabs, seeds_a


def smooth_parts(smooth) -> tuple:
    """Context.ssm_run's `smooth` argument as the parts wanted: () for a false value, all three for
    True, else the names given (ValueError for one that is none of them)"""
    if not smooth:
        return ()
    parts = ("paths", "mean", "var") if smooth is True else ((smooth,) if isinstance(smooth, str) else tuple(smooth))
    bad = [p for p in parts if p not in ("paths", "mean", "var")]
    if bad:
        raise ValueError(f"smooth: unknown part {bad[0]!r}")
    return parts


TRACE_PARTS = ("ess", "mean", "var", "log_evidence")


def trace_parts(trace) -> tuple:
    """Context.ssm_run's `trace` argument as the parts wanted: () for a false value, all four for
    True, else the names given (ValueError for one that is none of them)"""
    parts = TRACE_PARTS if trace is True else tuple(trace or ())
    bad = [p for p in parts if p not in TRACE_PARTS]
    if bad:
        raise ValueError(f"trace: unknown part {bad[0]!r}")
    return parts


def _out_buffers(out, shapes: dict):
    """a host array per part wanted, and `out` (SsmTraceOut / SsmSmoothOut) pointing at them"""
    buf = {p: np.empty(shape) for p, shape in shapes.items()}
    for p, a in buf.items():
        setattr(out, p, a.ctypes.data_as(C.POINTER(C.c_double)))
    return buf, out


def trace_buffers(parts, lead: tuple, S: int):
    """(buffers by part, SsmTraceOut) of a traced run: lead = (T,), of a traced batch: (B, T)"""
    return _out_buffers(abi.SsmTraceOut(), {p: lead + ((S,) if p in ("mean", "var") else ()) for p in parts})


def smooth_buffers(parts, lead: tuple, S: int, n: int):
    """(buffers by part, SsmSmoothOut) of a smoothed run or batch, as trace_buffers"""
    return _out_buffers(abi.SsmSmoothOut(), {p: lead + ((S, n) if p == "paths" else (S,)) for p in parts})


def _by_name(a, cols):
    return None if a is None else {c: a[..., k].copy() for k, c in enumerate(cols)}


def trace_by_name(buf: dict, cols) -> tuple:
    """trace_buffers' arrays as (ess, mean, var, log_evidence), mean and var as column name -> rows; None: not asked for"""
    return buf.get("ess"), _by_name(buf.get("mean"), cols), _by_name(buf.get("var"), cols), buf.get("log_evidence")


def smooth_by_name(buf: dict, cols) -> tuple:
    """smooth_buffers' arrays as (paths, mean, var), each column name -> rows (the paths are views); None: not asked for"""
    paths = {c: buf["paths"][..., k, :] for k, c in enumerate(cols)} if "paths" in buf else None
    return paths, _by_name(buf.get("mean"), cols), _by_name(buf.get("var"), cols)


class SsmTrace:
    """The per-step filtering trace of a scalar-SSM run (include/wsmc.h wsmc_ssm_trace). Row t is
    taken after step t's last observe, before the Resample that follows it: `ess` [T] that
    Resample's ESS%; `mean` / `var` (column name -> [T]) E[x_t | y_1:t] and the uncorrected
    variance under exp_norm of the weights (Context.weighted_moments of the column alone);
    `log_evidence` [T], cumulative (its first difference is log p(y_t | y_1:t-1))."""

    def __init__(self, ess, mean, var, log_evidence):
        self.ess, self.mean, self.var, self.log_evidence = ess, mean, var, log_evidence

    def predictive_loglik(self) -> np.ndarray:
        """log p(y_t | y_1:t-1), t = 0 .. T-1: the first difference of log_evidence"""
        return np.diff(self.log_evidence, prepend=0.0)


class SsmSmooth:
    """The smoothed output of a scalar-SSM run (include/wsmc.h wsmc_ssm_smooth): the genealogy of
    the final particles traced back through every resampling step. `paths` (column name -> [T, N]):
    paths[name][t][i] is the column's value at trace point t (after step t's last observe, before
    the Resample that follows it) of final particle i's ancestor; `mean` / `var` (name -> [T]):
    E[x_t | y_1:T] and the uncorrected variance under exp_norm of the final weights
    (Context.weighted_moments of row t); `log_weights` [N], the final ones. A part that was not
    asked for is None."""

    def __init__(self, paths, mean, var, log_weights):
        self.paths, self.mean, self.var, self.log_weights = paths, mean, var, log_weights

    def draw(self, k: int, rng=None) -> dict:
        """k posterior trajectories (name -> [k, T]), picked with replacement by exp_norm of the
        final weights on the host: the analogue of the reference's sample(state, k)"""
        if self.paths is None:
            raise ValueError("draw: the paths were not asked for")
        rng = np.random.default_rng() if rng is None else rng
        lw = np.asarray(self.log_weights, dtype=np.float64)
        w = np.exp(lw - np.max(lw))
        idx = rng.choice(len(w), size=int(k), p=w / w.sum())
        return {name: p[:, idx].T.copy() for name, p in self.paths.items()}


class SsmRecord:
    """What a filter leaves for backward simulation: `cols` [T, S, n], every column at each trace
    point (after step t's last observe, before the Resample that follows it), in the spec's order,
    and `log_weights` [T, n], the log-weights there."""

    def __init__(self, cols, log_weights):
        self.cols = np.ascontiguousarray(np.asarray(cols, dtype=np.float64))
        self.log_weights = np.ascontiguousarray(np.asarray(log_weights, dtype=np.float64))
        if self.cols.ndim != 3 or self.log_weights.shape != (self.cols.shape[0], self.cols.shape[2]):
            raise ValueError("record: cols [T, S, n] and log_weights [T, n]")


class SsmBackward:
    """M trajectories drawn by forward filtering, backward simulation (include/wsmc.h
    wsmc_ssm_backward): `idx` [T, M] int32, the filter particle trajectory m passes through at
    trace point t; `paths` (column name -> [T, M]) the record's columns there; `mean` / `var`
    (name -> [T]) E[x_t | y_1:T] and the uncorrected variance over the M equal-weight
    trajectories (Context.weighted_moments of row t on M particles with fresh weights); `record`
    the SsmRecord they were drawn from, when asked for. An auxiliary column assigned from the old
    state (kitagawa's m, the guided spec's xp and m) holds in row t+1 the filter particle's own
    value: f of its genealogical parent, not f of the drawn x_t."""

    def __init__(self, idx, paths, mean, var, record=None):
        self.idx, self.paths, self.mean, self.var, self.record = idx, paths, mean, var, record

    def draw(self, k: int) -> dict:
        """the first k trajectories (name -> [k, T]): they are already equal-weight draws"""
        k = int(k)
        if not 0 <= k <= self.idx.shape[1]:
            raise ValueError(f"draw: {k} of {self.idx.shape[1]} trajectories")
        return {name: p[:, :k].T.copy() for name, p in self.paths.items()}


def backward_buffers(T: int, S: int, n: int, M: int, lead: tuple = (), record: bool = False):
    """(arrays by part, SsmBackwardOut pointing at them) of a backward pass, as trace_buffers"""
    buf = {"idx": np.empty(lead + (T, M), dtype=np.int32), "paths": np.empty(lead + (T, S, M)),
           "mean": np.empty(lead + (T, S)), "var": np.empty(lead + (T, S))}
    if record:
        buf["particles"] = np.empty(lead + (T, S, n))
        buf["log_weights"] = np.empty(lead + (T, n))
    out = abi.SsmBackwardOut()
    for p, a in buf.items():
        setattr(out, p, a.ctypes.data_as(C.POINTER(C.c_int32 if p == "idx" else C.c_double)))
    return buf, out


def backward_by_name(buf: dict, cols) -> SsmBackward:
    """backward_buffers' arrays of one filter as an SsmBackward"""
    rec = SsmRecord(buf["particles"], buf["log_weights"]) if "particles" in buf else None
    return SsmBackward(buf["idx"], {c: buf["paths"][:, k, :] for k, c in enumerate(cols)},
                       _by_name(buf["mean"], cols), _by_name(buf["var"], cols), rec)


def _operand_reads(o) -> int:
    """the spec columns an operand reads, as a bit mask (a data slot is no column)"""
    return (1 << o.col[0] if o.col[0] >= 0 else 0) | (1 << o.col[1] if o.col[1] >= 0 else 0)


def _dist_reads(d) -> int:
    return _operand_reads(d.mu[0]) | _operand_reads(d.scale)


def _fold_operand(o, ids, patch):
    """the operand over column ids, its data slot removed: the step's value goes to c0 through
    `patch`, a list of (object, field, data column)"""
    r = Operand()
    C.memmove(C.byref(r), C.byref(o), C.sizeof(Operand))
    for k in range(2):
        if o.col[k] == abi.OPERAND_DATA:
            patch.append((r, "c0", int(o.comp[k])))
            r.col[k], r.comp[k], r.coef[k] = -1, 0, 0.0
        elif o.col[k] >= 0:
            r.col[k] = ids[o.col[k]]
    return r


def _fold_dist(d, ids, patch):
    r = abi.Dist()
    C.memmove(C.byref(r), C.byref(d), C.sizeof(abi.Dist))
    for k in range(4):
        ops = []
        r.mu[k] = _fold_operand(d.mu[k], ids, ops)
        patch += [(r.mu[k], f, j) for _, f, j in ops]   # (a view into r: the copy above is not)
    ops = []
    r.scale = _fold_operand(d.scale, ids, ops)
    patch += [(r.scale, f, j) for _, f, j in ops]
    return r


def _fold_prog(s, ids, patch):
    """(program, lengths) of an ASSIGN_EXPR over column ids, a data read turned into a constant"""
    prog = (abi.XInst * s.prog_len)()
    for k in range(s.prog_len):
        prog[k] = s.prog[k]
        if prog[k].op != abi.X_COL:
            continue
        if prog[k].col == abi.OPERAND_DATA:
            patch.append((prog[k], "c", int(prog[k].comp)))
            prog[k].op, prog[k].col, prog[k].comp = abi.X_CONST, -1, 0
        else:
            prog[k].col = ids[prog[k].col]
    return prog, [int(s.prog_len)]


STORE_COLUMNS = 4096   # the columns one context's store holds


class SSM:
    """A builder for wsmc_ssm_spec: SSM(cols=[...]).init(...).step(...)."""

    def __init__(self, cols, data_dim: int | None = None):
        self.cols = [str(c) for c in cols]
        self._init: list = []
        self._step: list = []
        self._data_dim = data_dim
        self._spec = None

    @classmethod
    def from_spec(cls, spec: abi.SsmSpec) -> "SSM":
        """A ready wsmc_ssm_spec (filled by hand: the operand forms the builder does not write,
        such as a data slot behind a column) with everything but the builder: .spec, .cols,
        .table, .check and .statements. The struct is used as it is, not copied or lowered."""
        r = cls([spec.col_names[k].value.decode() for k in range(spec.n_cols)], data_dim=spec.data_dim)
        r._spec = spec
        return r

    def init(self, *stmts) -> "SSM":
        self._init += list(stmts)
        self._spec = None
        return self

    def step(self, *stmts) -> "SSM":
        self._step += list(stmts)
        self._spec = None
        return self

    # ---- lowering ----
    def _resolve(self, name):
        if name == DATA:
            return abi.OPERAND_DATA
        try:
            return self.cols.index(name)
        except ValueError:
            raise KeyError(f"unknown column {name!r} (the spec's columns are {self.cols})") from None

    def _lower(self, st, out: abi.SsmStmt) -> None:
        kind = st[0]
        out.kind = kind
        out.col = -1
        out.value = Operand.const(0.0)
        if kind == abi.SSM_SAMPLE:
            out.col = self._resolve(st[1])
            out.dist = st[2].dist(self._resolve)
        elif kind == abi.SSM_SAMPLE_IMPORTANCE:
            out.col = self._resolve(st[1])
            out.dist = st[2].proposal.dist(self._resolve)
            out.target = st[2].target.dist(self._resolve)
        elif kind in (abi.SSM_OBSERVE, abi.SSM_WEIGHT):
            out.value = Expr.lift(st[1]).operand(self._resolve)
            out.dist = st[2].dist(self._resolve)
        elif _general(st[2]):
            out.kind = abi.SSM_ASSIGN_EXPR
            out.col = self._resolve(st[1])
            prog, lens = xprogram([st[2]], self._resolve)
            if lens[0] > abi.SSM_XPROG_MAX:
                raise ValueError(f"{st[1]}: a program of {lens[0]} instructions (at most {abi.SSM_XPROG_MAX})")
            out.prog_len = lens[0]
            for k in range(lens[0]):
                out.prog[k] = prog[k]
        else:
            out.col = self._resolve(st[1])
            out.value = Expr.lift(st[2]).operand(self._resolve)

    @property
    def spec(self) -> abi.SsmSpec:
        """The wsmc_ssm_spec (built once; the builder's statements lowered over local indices)."""
        if self._spec is not None:
            return self._spec
        if not 1 <= len(self.cols) <= abi.SSM_MAX_COLS:
            raise ValueError(f"1..{abi.SSM_MAX_COLS} columns")
        if len(self._init) > abi.SSM_MAX_INIT or len(self._step) > abi.SSM_MAX_STMTS:
            raise ValueError(f"at most {abi.SSM_MAX_INIT} init and {abi.SSM_MAX_STMTS} step statements")
        sp = abi.SsmSpec()
        sp.n_cols = len(self.cols)
        for k, name in enumerate(self.cols):
            b = name.encode()
            if len(b) >= abi.SSM_NAME_MAX:
                raise ValueError(f"column name {name!r} longer than {abi.SSM_NAME_MAX - 1} bytes")
            sp.col_names[k].value = b
        sp.n_init, sp.n_step = len(self._init), len(self._step)
        for k, st in enumerate(self._init):
            self._lower(st, sp.init[k])
        for k, st in enumerate(self._step):
            self._lower(st, sp.step[k])
        used = -1
        for q in range(sp.n_init + sp.n_step):
            s = sp.init[q] if q < sp.n_init else sp.step[q - sp.n_init]
            ops = list(s.dist.mu) + [s.dist.scale, s.value] + list(s.target.mu) + [s.target.scale]
            for o in ops:
                for k in range(2):
                    if o.col[k] == abi.OPERAND_DATA:
                        used = max(used, o.comp[k])
            for k in range(s.prog_len):
                if s.prog[k].op == abi.X_COL and s.prog[k].col == abi.OPERAND_DATA:
                    used = max(used, s.prog[k].comp)
        sp.data_dim = used + 1 if self._data_dim is None else int(self._data_dim)
        self._spec = sp
        return sp

    def check(self) -> None:
        """wsmc_ssm_spec_check (host only): raises WSMCError(WSMC_EARG) with the reason"""
        abi.check(abi.load_library().wsmc_ssm_spec_check(C.byref(self.spec)))

    def shape_difference(self, other: "SSM") -> str | None:
        """wsmc_ssm_spec_same_shape (host only): None when the two specs differ in their numbers
        alone (what one batch of Context.ssm_run_batch may hold), else the library's message, which
        names the first differing field"""
        L = abi.load_library()
        if L.wsmc_ssm_spec_same_shape(C.byref(self.spec), C.byref(other.spec)) == abi.WSMC_OK:
            return None
        return L.wsmc_last_error().decode()

    def same_shape(self, other: "SSM") -> bool:
        """True when `other` differs from this spec in its numbers alone: operand constants and
        coefficients, dist parameters, program constants (shape_difference says where it does not)"""
        return self.shape_difference(other) is None

    def table(self, data, T: int | None = None) -> np.ndarray:
        """the run's data as the T x data_dim table the C entry point takes (a spec that reads no
        data takes its horizon from T, or from len(data))"""
        dd = self.spec.data_dim
        if dd == 0:
            return np.empty((len(data) if T is None else int(T), 0))
        return np.ascontiguousarray(np.asarray(data, dtype=np.float64).reshape(-1, dd))

    # ---- the executable definition ----
    def statements(self, backend, data, ess_perc_min: float = 1.0, scheme: int = abi.RESAMPLE_STRATIFIED,
                   wait: bool = True, T: int | None = None, trace: bool = False, smooth: bool = False,
                   record: bool = False):
        """Issue the spec's statements one by one on `backend` (a Context or the tests' Oracle: any
        object with the operator methods), each `sample` / `observe` followed by its Resample, the
        step's data folded into constants: a data slot of an operand is removed and its value
        becomes c0, a data read of a program becomes a constant. This is what wsmc_ssm_run
        computes. wait=True returns (flags, ESS%) of the Resample after each step's last observe;
        wait=False leaves every Resample asynchronous and returns None. trace=True (with wait)
        also takes backend.weighted_moments of every column and backend.log_evidence() between each
        step's last observe and its Resample and returns (flags, ESS%, SsmTrace): the definition
        of what Context.ssm_run(trace=True) returns. smooth=True (with wait) also keeps every
        column's values at each trace point in a column of their own, `name@t` (an exact copy, a -0.0
        included), which the Resamples that follow gather like any other, and reads them after the
        last step: the result gains an SsmSmooth as its last member, the definition of what
        Context.ssm_run(smooth=True) returns. record=True (with wait) also downloads every column and
        the log-weights at each trace point: the result gains an SsmRecord as its last member, what
        backward_definition draws from and what Context.ssm_run(backward=M) logs on the device."""
        if record and not wait:
            raise ValueError("record=True needs wait=True (the trace point is a synchronisation)")
        if trace and not wait:
            raise ValueError("trace=True needs wait=True (the trace point is a synchronisation)")
        if smooth and not wait:
            raise ValueError("smooth=True needs wait=True (the trace point is a synchronisation)")
        sp = self.spec
        tab = self.table(data, T)
        T = len(tab)
        if smooth and T * len(self.cols) + len(self.cols) > STORE_COLUMNS:
            raise ValueError(f"smooth=True: {T} steps of {len(self.cols)} columns need {T * len(self.cols) + len(self.cols)} "
                             f"store columns (at most {STORE_COLUMNS})")
        ids = [backend.col_create(name, 1) for name in self.cols]

        # every statement is built once (ids mapped, data slots removed); a step only writes its
        # data values into the slots listed in `patch`: (object, field, data column)
        def fold_operand(o, patch):
            return _fold_operand(o, ids, patch)

        def fold_dist(d, patch):
            return _fold_dist(d, ids, patch)

        def prepare(s):
            """(call, patch): call(waited) issues the statement and its Resample"""
            patch = []
            out = ids[s.col] if s.kind not in (abi.SSM_OBSERVE, abi.SSM_WEIGHT) else -1
            if s.kind == abi.SSM_SAMPLE:
                d = fold_dist(s.dist, patch)

                def call(waited):
                    backend.sample(out, d)
                    backend.resample(ess_perc_min, scheme, wait=False)
            elif s.kind == abi.SSM_SAMPLE_IMPORTANCE:
                d = fold_dist(s.dist, patch)
                tg = fold_dist(s.target, patch)

                def call(waited):
                    backend.sample_importance(out, d, tg)
                    backend.resample(ess_perc_min, scheme, wait=False)
            elif s.kind == abi.SSM_WEIGHT:
                d = fold_dist(s.dist, patch)
                x = [fold_operand(s.value, patch)]

                def call(waited):
                    backend.weight(d, x)
                    backend.resample(ess_perc_min, scheme, wait=False)
            elif s.kind == abi.SSM_ASSIGN:
                e = [fold_operand(s.value, patch)]

                def call(waited):
                    backend.assign(out, e)
            elif s.kind == abi.SSM_ASSIGN_EXPR:
                prog, lens = _fold_prog(s, ids, patch)

                def call(waited):
                    backend.assign_expr(out, prog, lens)
            else:
                d = fold_dist(s.dist, patch)
                x = [fold_operand(s.value, patch)]

                def call(waited, at=None):
                    backend.observe(d, x)
                    if at is not None:
                        at()
                    return backend.resample(ess_perc_min, scheme, wait=waited)
            return call, patch

        for q in range(sp.n_init):
            prepare(sp.init[q])[0](False)
        last = max(q for q in range(sp.n_step) if sp.step[q].kind == abi.SSM_OBSERVE)
        step = [prepare(sp.step[q]) for q in range(sp.n_step)]
        flags, ess = [], []
        if trace:
            S = len(self.cols)
            mean, var, lev = np.empty((T, S)), np.empty((T, S)), np.empty(T)
            exprs = [Operand.column(ids[k]) for k in range(S)]

        hist = []   # smooth: step t's history columns, in the spec's order
        rec_cols, rec_lw = [], []   # record: the columns and the log-weights at each trace point

        def point(t):
            if trace:
                m, cv = backend.weighted_moments(exprs)
                mean[t], var[t] = m, np.diagonal(cv)
                lev[t] = backend.log_evidence()
            if smooth:
                hs = [backend.col_create(f"{name}@{t}", 1) for name in self.cols]
                for h, i in zip(hs, ids):   # a copy, bit for bit: the affine form 0.0 + 1.0 x would turn a -0.0 into 0.0
                    copy = (abi.XInst * 1)()
                    copy[0].op, copy[0].col, copy[0].comp = abi.X_COL, i, 0
                    backend.assign_expr(h, copy, [1])
                hist.append(hs)
            if record:
                rec_cols.append(np.stack([backend.col_download(i) for i in ids]))
                rec_lw.append(backend.weights_download())

        for t in range(T):
            row = tab[t]
            for q, (call, patch) in enumerate(step):
                for obj, field, j in patch:
                    setattr(obj, field, row[j])
                if (trace or smooth or record) and q == last:
                    r = call(True, lambda: point(t))
                else:
                    r = call(wait and q == last)
                if wait and q == last:
                    flags.append(bool(r[0]))
                    ess.append(float(r[1]))
        out = (flags, np.array(ess)) if wait else None
        if trace:
            tr = SsmTrace(np.array(ess), {c: mean[:, k].copy() for k, c in enumerate(self.cols)},
                          {c: var[:, k].copy() for k, c in enumerate(self.cols)}, lev)
            out = (flags, tr.ess, tr)
        if smooth:
            n_cols = len(self.cols)
            paths = {c: np.stack([backend.col_download(hist[t][k]) for t in range(T)]) for k, c in enumerate(self.cols)}
            smean, svar = np.empty((T, n_cols)), np.empty((T, n_cols))
            for t in range(T):
                m, cv = backend.weighted_moments([Operand.column(h) for h in hist[t]])
                smean[t], svar[t] = m, np.diagonal(cv)
            sm = SsmSmooth(paths, {c: smean[:, k].copy() for k, c in enumerate(self.cols)},
                           {c: svar[:, k].copy() for k, c in enumerate(self.cols)}, backend.weights_download())
            out = out + (sm,)
        if record:
            out = out + (SsmRecord(np.stack(rec_cols), np.stack(rec_lw)),)
        return out

    # ---- backward simulation ----
    def backward_terms(self) -> list:
        """The step statements whose log-density enters the backward weight of forward filtering,
        backward simulation, as indices into `step`: wsmc_ssm_spec_backward's rule, restated here.
        Every column starts tainted (it holds the previous trace point's value); a SAMPLE's term is
        included iff its dist reads a tainted column, an importance SAMPLE's target's iff it does
        once the column holds the successor's value, an OBSERVE's or WEIGHT's iff its dist or value
        does; an assignment is tainted iff its right-hand side is. Raises ValueError with the
        library's reason for a spec backward simulation is not defined for."""
        self.check()
        sp = self.spec
        S, n = sp.n_cols, sp.n_step
        name = lambda k: self.cols[k]
        if sp.step[n - 1].kind != abi.SSM_OBSERVE:
            raise ValueError("ssm backward: the step's last statement is not its last OBSERVE (the trace point)")
        drawn = [0] * S
        writes = [0] * S
        for q in range(n):
            s = sp.step[q]
            if s.kind in (abi.SSM_OBSERVE, abi.SSM_WEIGHT):
                continue
            writes[s.col] += 1
            drawn[s.col] += s.kind in (abi.SSM_SAMPLE, abi.SSM_SAMPLE_IMPORTANCE)
        for k in range(S):
            if drawn[k] and writes[k] > 1:
                raise ValueError(f"ssm backward: column {name(k)} is written by a SAMPLE and by another statement of the step")
        tainted, written, state, included = (1 << S) - 1, 0, 0, []
        for q in range(n):
            s = sp.step[q]
            if s.kind == abi.SSM_SAMPLE:
                r = _dist_reads(s.dist)
                state |= r & ~written
                if r & tainted:
                    included.append(q)
                tainted &= ~(1 << s.col)
                written |= 1 << s.col
            elif s.kind == abi.SSM_SAMPLE_IMPORTANCE:
                state |= _dist_reads(s.dist) & ~written   # the draw reads the proposal before the store
                tainted &= ~(1 << s.col)
                written |= 1 << s.col
                r = _dist_reads(s.target)
                state |= r & ~written
                if r & tainted:
                    included.append(q)
            elif s.kind in (abi.SSM_ASSIGN, abi.SSM_ASSIGN_EXPR):
                if s.kind == abi.SSM_ASSIGN:
                    r = _operand_reads(s.value)
                else:
                    r = 0
                    for k in range(s.prog_len):
                        if s.prog[k].op == abi.X_COL and s.prog[k].col >= 0:
                            r |= 1 << s.prog[k].col
                state |= r & ~written
                tainted = tainted | (1 << s.col) if r & tainted else tainted & ~(1 << s.col)
                written |= 1 << s.col
            else:
                r = _dist_reads(s.dist) | _operand_reads(s.value)
                state |= r & ~written
                if r & tainted:
                    included.append(q)
        for k in range(S):
            if state & tainted & (1 << k):
                raise ValueError(f"ssm backward: state column {name(k)} still holds the previous step's value at the end of the "
                                 "step (a static parameter or a deterministic carry-over: the transition is a Dirac)")
        return included

    def backward_definition(self, make_backend, record, data, M: int, seed: int, T: int | None = None) -> SsmBackward:
        """Forward filtering, backward simulation, operator by operator: the definition of what
        Context.ssm_backward and Context.ssm_run(backward=M) return. make_backend(n, seed) gives a
        fresh context (a Context or the tests' Oracle); record is the filter's SsmRecord.
        Trajectory m = 0 .. M-1, going t = T-1 down to 0 on a scratch backend of n particles and
        seed `seed`: the weights are log_weights[t]; for t < T-1 the columns are cols[t] and step
        t+1's statements are issued in order with data row t+1 folded in and z = cols[t+1][:,
        idx[t+1][m]] the successor's row: a SAMPLE as weight(dist, z[col]) if included, then
        assign(col, z[col]); an importance SAMPLE as assign(col, z[col]), then weight(target, col) if
        included; an assignment as it is; an OBSERVE or WEIGHT as weight(dist, value) if included;
        no Resample. Then set_op_counter(t M + m) and sample_particles(1) give idx[t][m]. paths
        gathers the record through idx; mean / var are weighted_moments of each row on an
        M-particle backend with fresh weights. A draw that fails (exp_norm of the weights is NaN)
        raises WSMCError(WSMC_ESTATE)."""
        included = set(self.backward_terms())
        sp = self.spec
        tab = self.table(data, T)
        T, M, S = len(tab), int(M), len(self.cols)
        cols, lw = record.cols, record.log_weights
        if M < 1:
            raise ValueError("M: at least one trajectory")
        if cols.shape[:2] != (T, S):
            raise ValueError(f"record: {cols.shape[0]} steps of {cols.shape[1]} columns, the call has {T} of {S}")
        n = cols.shape[2]
        idx = np.empty((T, M), dtype=np.int32)
        for m in range(M):
            be = make_backend(n, seed)
            ids = [be.col_create(name, 1) for name in self.cols]
            stmts = []   # (kind, included, out column, the folded parts, patch)
            for q in range(sp.n_step):
                s, patch = sp.step[q], []
                if s.kind == abi.SSM_SAMPLE:
                    parts = (_fold_dist(s.dist, ids, patch),)
                elif s.kind == abi.SSM_SAMPLE_IMPORTANCE:
                    parts = (_fold_dist(s.target, ids, patch),)
                elif s.kind == abi.SSM_ASSIGN:
                    parts = ([_fold_operand(s.value, ids, patch)],)
                elif s.kind == abi.SSM_ASSIGN_EXPR:
                    parts = _fold_prog(s, ids, patch)
                else:
                    parts = (_fold_dist(s.dist, ids, patch), [_fold_operand(s.value, ids, patch)])
                out = ids[s.col] if s.kind not in (abi.SSM_OBSERVE, abi.SSM_WEIGHT) else -1
                stmts.append((s.kind, q in included, int(s.col), out, parts, patch))
            for t in range(T - 1, -1, -1):
                be.weights_upload(lw[t])
                if t < T - 1:
                    for k in range(S):
                        be.col_upload(ids[k], cols[t][k])
                    z, row = cols[t + 1][:, idx[t + 1][m]], tab[t + 1]
                    for kind, inc, col, out, parts, patch in stmts:
                        for obj, field, j in patch:
                            setattr(obj, field, row[j])
                        if kind == abi.SSM_SAMPLE:
                            if inc:
                                be.weight(parts[0], [Operand.const(z[col])])
                            be.assign(out, [Operand.const(z[col])])
                        elif kind == abi.SSM_SAMPLE_IMPORTANCE:
                            be.assign(out, [Operand.const(z[col])])
                            if inc:
                                be.weight(parts[0], [Operand.column(out)])
                        elif kind == abi.SSM_ASSIGN:
                            be.assign(out, parts[0])
                        elif kind == abi.SSM_ASSIGN_EXPR:
                            be.assign_expr(out, parts[0], parts[1])
                        elif inc:
                            be.weight(parts[0], parts[1])
                be.set_op_counter(t * M + m)
                try:
                    idx[t][m] = be.sample_particles(1, True)[0]
                except RuntimeError as e:   # a Context's WSMCError, or the oracle's own error with the code
                    code = e.code if isinstance(e, abi.WSMCError) else abi.WSMC_ESTATE if f"({abi.WSMC_ESTATE})" in str(e) else None
                    if code != abi.WSMC_ESTATE:
                        raise
                    raise abi.WSMCError(abi.WSMC_ESTATE, f"ssm backward: exp_norm of the weights is NaN at step {t} "
                                                         f"of trajectory {m}") from None
            if hasattr(be, "close"):
                be.close()
        paths = np.stack([cols[t][:, idx[t]] for t in range(T)])   # [T, S, M]
        mean, var = np.empty((T, S)), np.empty((T, S))
        be = make_backend(M, seed)
        ids = [be.col_create(name, 1) for name in self.cols]
        exprs = [Operand.column(i) for i in ids]
        for t in range(T):
            for k in range(S):
                be.col_upload(ids[k], paths[t][k])
            mu, cv = be.weighted_moments(exprs)
            mean[t], var[t] = mu, np.diagonal(cv)
        if hasattr(be, "close"):
            be.close()
        return SsmBackward(idx, {c: paths[:, k, :] for k, c in enumerate(self.cols)}, _by_name(mean, self.cols),
                           _by_name(var, self.cols), record)

    # ---- conditional SMC (particle Gibbs) ----
    def conditional_terms(self) -> list:
        """The columns a conditional run pins to its reference trajectory, by name in the spec's
        order: wsmc_ssm_spec_conditional's rule, restated here. They are the columns a SAMPLE of
        `step` writes. Raises ValueError with the library's reason for a spec a conditional run is
        not defined for: one with an importance SAMPLE or a WEIGHT (pinning an importance Sample
        needs its weight term at the pinned value), one whose `init` holds anything but SAMPLE and
        assignments, and everything backward_terms refuses."""
        self.check()
        sp = self.spec
        for where, stmts, n in (("init", sp.init, sp.n_init), ("step", sp.step, sp.n_step)):
            for q in range(n):
                kind = stmts[q].kind
                if kind == abi.SSM_SAMPLE_IMPORTANCE:
                    raise ValueError(f"ssm conditional: statement {q} of {where} is an importance SAMPLE (pinning it needs its "
                                     "weight term at the pinned value)")
                if kind == abi.SSM_WEIGHT:
                    raise ValueError(f"ssm conditional: statement {q} of {where} is a WEIGHT (guided specs are not supported)")
                if where == "init" and kind == abi.SSM_OBSERVE:
                    raise ValueError(f"ssm conditional: statement {q} of init is an OBSERVE (init may hold SAMPLE and "
                                     "assignments only: it is not pinned)")
        try:
            self.backward_terms()
        except ValueError as e:
            raise ValueError(f"ssm conditional: {e}") from None
        drawn = {int(sp.step[q].col) for q in range(sp.n_step) if sp.step[q].kind == abi.SSM_SAMPLE}
        return [c for k, c in enumerate(self.cols) if k in drawn]

    def reference_table(self, reference, T: int) -> np.ndarray:
        """a conditional run's reference trajectory as the [T, n_cols] table the C entry point
        takes: an array of that shape, or column name -> [T] (a column that is not given is 0.0;
        entries of columns that are not pinned are ignored)"""
        S = len(self.cols)
        if isinstance(reference, dict):
            ref = np.zeros((int(T), S))
            for name, v in reference.items():
                ref[:, self.cols.index(name)] = np.asarray(v, dtype=np.float64).reshape(int(T))
            return ref
        ref = np.ascontiguousarray(np.asarray(reference, dtype=np.float64))
        if ref.shape != (int(T), S):
            raise ValueError(f"reference: shape {ref.shape}, the run has {T} steps of {S} columns")
        return ref

    def conditional_definition(self, make_backend, data, n: int, seed: int, reference, ess_perc_min: float,
                               T: int | None = None, trace: bool = False):
        """Conditional SMC, operator by operator: the definition of what Context.ssm_run_conditional
        computes for one filter. make_backend(n, seed) gives a fresh context (a Context or the
        tests' Oracle). It is statements(..., record=True) with two changes; particle n-1 is the
        reference particle.
        Pin: in `step` (never in `init`), right after a `sample` of step t, col_download of its
        column, the last entry set to reference[t][column], col_upload.
        Conditional Resample, in place of every Resample: read get_state()'s op counter r,
        weights_download() and every column; resample(ess_perc_min, STRATIFIED, wait=True); if it
        ran (get_state()'s n_resamples grew: a Resample that meets unchanged weights, as after a
        `sample`, does nothing and reports the previous flag), upload the saved weights to a scratch backend of the same n and seed,
        set_op_counter(r) and idx = sample_particles(n, True) there; idx[n-1] = n-1;
        col_upload(k, saved[k][idx]) for every column. So the decision, the ESS, the evidence and
        the reset weights are the ordinary Resample's and the ancestors are n independent draws
        with the last slot forced.
        Returns (flags, ESS%, SsmRecord, SsmFinal), with trace=True (flags, ESS%, SsmTrace,
        SsmRecord, SsmFinal)."""
        self.conditional_terms()
        sp = self.spec
        tab = self.table(data, T)
        T, S, n = len(tab), len(self.cols), int(n)
        ref = self.reference_table(reference, T)
        be = make_backend(n, seed)
        ids = [be.col_create(name, 1) for name in self.cols]
        end = SsmFinal(None, None, np.zeros(n, dtype=np.int32), 0, None)

        def resample():
            before = be.get_state()
            r = before["op_counter"]
            w = be.weights_download()
            saved = [be.col_download(i) for i in ids]
            ran, ess = be.resample(ess_perc_min, abi.RESAMPLE_STRATIFIED, wait=True)
            if be.get_state()["n_resamples"] > before["n_resamples"]:
                scratch = make_backend(n, seed)
                scratch.weights_upload(w)
                scratch.set_op_counter(r)
                idx = np.asarray(scratch.sample_particles(n, True), dtype=np.int64)
                if hasattr(scratch, "close"):
                    scratch.close()
                idx[n - 1] = n - 1
                for i, v in zip(ids, saved):
                    be.col_upload(i, v[idx])
                end.last_ancestors = idx.astype(np.int32)
                end.n_resamples += 1
            return bool(ran), float(ess)

        def prepare(s):
            """(kind, column, the folded parts, patch) of a statement"""
            patch = []
            if s.kind == abi.SSM_SAMPLE:
                parts = (_fold_dist(s.dist, ids, patch),)
            elif s.kind == abi.SSM_ASSIGN:
                parts = ([_fold_operand(s.value, ids, patch)],)
            elif s.kind == abi.SSM_ASSIGN_EXPR:
                parts = _fold_prog(s, ids, patch)
            else:
                parts = (_fold_dist(s.dist, ids, patch), [_fold_operand(s.value, ids, patch)])
            return int(s.kind), int(s.col), parts, patch

        def issue(kind, col, parts, pin=None, at=None):
            """the statement, then its Resample's (flag, ESS%) if it has one"""
            if kind == abi.SSM_SAMPLE:
                be.sample(ids[col], parts[0])
                if pin is not None:
                    v = be.col_download(ids[col])
                    v[n - 1] = pin[col]
                    be.col_upload(ids[col], v)
                return resample()
            if kind == abi.SSM_ASSIGN:
                be.assign(ids[col], parts[0])
            elif kind == abi.SSM_ASSIGN_EXPR:
                be.assign_expr(ids[col], parts[0], parts[1])
            else:
                be.observe(parts[0], parts[1])
                if at is not None:
                    at()
                return resample()
            return None

        for q in range(sp.n_init):
            kind, col, parts, _ = prepare(sp.init[q])
            issue(kind, col, parts)
        step = [prepare(sp.step[q]) for q in range(sp.n_step)]
        last = sp.n_step - 1   # (conditional_terms: the step ends in its last OBSERVE)
        flags, ess = [], []
        mean, var, lev = np.empty((T, S)), np.empty((T, S)), np.empty(T)
        exprs = [Operand.column(i) for i in ids]
        rec_cols, rec_lw = [], []

        def point(t):
            if trace:
                m, cv = be.weighted_moments(exprs)
                mean[t], var[t] = m, np.diagonal(cv)
                lev[t] = be.log_evidence()
            rec_cols.append(np.stack([be.col_download(i) for i in ids]))
            rec_lw.append(be.weights_download())

        for t in range(T):
            row = tab[t]
            for q, (kind, col, parts, patch) in enumerate(step):
                for obj, field, j in patch:
                    setattr(obj, field, row[j])
                r = issue(kind, col, parts, pin=ref[t], at=(lambda: point(t)) if q == last else None)
                if q == last:
                    flags.append(r[0])
                    ess.append(r[1])
                    end.last_resampled = r[0]
        end.cols = {c: be.col_download(ids[k]) for k, c in enumerate(self.cols)}
        end.log_weights = be.weights_download()
        end.log_evidence = be.log_evidence()
        if hasattr(be, "close"):
            be.close()
        out = (flags, np.array(ess))
        if trace:
            out = out + (SsmTrace(np.array(ess), _by_name(mean, self.cols), _by_name(var, self.cols), lev),)
        return out + (SsmRecord(np.stack(rec_cols), np.stack(rec_lw)), end)


class SsmFinal:
    """What a filter leaves at its end (SSM.conditional_definition's last member; row b of
    Context.ssm_run_conditional(state=True)'s arrays): `cols` (name -> [n]), `log_weights` [n],
    `last_ancestors` [n] int32 (the ancestors of the last Resample that ran, zeros if none did),
    `n_resamples`, `log_evidence` and `last_resampled`, the decision of the last step's last Resample."""

    def __init__(self, cols, log_weights, last_ancestors, n_resamples, log_evidence, last_resampled=False):
        self.cols, self.log_weights, self.last_ancestors = cols, log_weights, last_ancestors
        self.n_resamples, self.log_evidence, self.last_resampled = n_resamples, log_evidence, last_resampled


_M64 = 2**64 - 1


def pg_seeds(seed: int, sweep: int, chains: int):
    """The seeds of particle_gibbs' sweep `sweep`: (seeds, bw_seeds), [chains] uint64 each, the
    filters' and their backward passes'. A pure function: seed number i = 2 (sweep chains + b) +
    role (role 0 the filter's, 1 the backward pass's, b the chain) is the splitmix64 output
    mix(seed + (i + 1) 0x9E3779B97F4A7C15 mod 2^64), mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
    z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31. mix is a bijection and the multiplier is
    odd, so for one seed and one chain count the values are distinct across sweeps, chains and the
    two roles."""
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    out = np.empty((2, int(chains)), dtype=np.uint64)
    for b in range(int(chains)):
        for role in range(2):
            i = 2 * (int(sweep) * int(chains) + b) + role
            out[role, b] = mix((int(seed) + (i + 1) * 0x9E3779B97F4A7C15) & _M64)
    return out[0], out[1]


def particle_gibbs(ctx, spec, data, n: int, sweeps: int, seed: int, chains: int = 1, ess_perc_min: float = 0.5,
                   reference=None):
    """Particle Gibbs with backward sampling for a fixed spec, one device call a sweep. Sweep 0 is
    ctx.ssm_run_batch(backward=1) (an unconditional filter and one backward trajectory per chain)
    unless `reference` ([chains, T, n_cols], or name -> [chains, T]) starts the chains; every later
    sweep is one ctx.ssm_run_conditional(backward=1) on the previous sweep's trajectories, whose
    backward paths become the next reference. Sweep j draws from pg_seeds(seed, j, chains).
    Returns (trajectories, log_evidence): column name -> [sweeps, chains, T], and [sweeps, chains],
    each sweep's filter's log evidence estimate. The spec's numbers are the caller's to change
    between calls (a parameter update); within one call they are fixed."""
    sweeps, chains = int(sweeps), int(chains)
    if sweeps < 1 or chains < 1:
        raise ValueError("particle_gibbs: at least one sweep and one chain")
    T, S = len(spec.table(data)), len(spec.cols)
    traj = np.empty((sweeps, chains, T, S))
    logev = np.empty((sweeps, chains))
    ref = None
    if reference is not None:
        ref = np.stack([spec.reference_table({k: np.asarray(v)[b] for k, v in reference.items()} if isinstance(reference, dict)
                                             else np.asarray(reference)[b], T) for b in range(chains)])
    for j in range(sweeps):
        seeds, bw_seeds = pg_seeds(seed, j, chains)
        if ref is None:
            res = ctx.ssm_run_batch(spec, data, n, seeds, ess_perc_min=ess_perc_min, backward=1, backward_seeds=bw_seeds)
        else:
            res = ctx.ssm_run_conditional(spec, data, n, seeds, ref, ess_perc_min=ess_perc_min, backward=1,
                                          backward_seeds=bw_seeds)
        ref = np.stack([np.stack([res.backward[b].paths[c][:, 0] for c in spec.cols], axis=1) for b in range(chains)])
        traj[j], logev[j] = ref, res.log_evidence
    return {c: traj[..., k].copy() for k, c in enumerate(spec.cols)}, logev

"""Low-level context: one particle shard on one GPU, driven through the C ABI.

Each method is a thin, typed wrapper of one include/wsmc.h entry point. The same method
set ("the context protocol") is what the high-level operators in ``transformers.py``
call, so they are agnostic of how a context is implemented; tests drive the CPU oracle
through the identical protocol to compare results bit for bit.
"""
from __future__ import annotations

import ctypes as C
import sys
import math

import numpy as np

from . import abi
from .abi import Dist, Operand, RunTiming, State, check, load_library
from .ssm import (TRACE_PARTS, SsmRecord, SsmSmooth, SsmTrace, backward_buffers, backward_by_name, batch_arguments, smooth_buffers,
                  smooth_by_name, smooth_parts, trace_buffers, trace_by_name, trace_parts)

_D = C.POINTER(C.c_double)
_I32P = C.POINTER(C.c_int32)


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(_D)


def _operands4(exprs) -> C.Array:
    ops = list(exprs) if isinstance(exprs, (list, tuple)) else [exprs]
    arr = (Operand * 4)()
    for k in range(4):
        arr[k] = ops[k] if k < len(ops) else ops[0]
    return arr


class SsmBatchResult:
    """What Context.ssm_run_batch returns: [B] arrays log_evidence, n_resamples, last_resampled;
    ess [B, T] when the trace was asked for; cols (name -> [B, n]), log_weights and last_ancestors
    [B, n] when the state was (None otherwise); with trace=True also mean and var (name -> [B, T])
    and log_evidence_trace [B, T], each filter's SsmTrace rows; with smooth also paths (name ->
    [B, T, n]), smean and svar (name -> [B, T]), each filter's SsmSmooth."""
    log_evidence = n_resamples = last_resampled = ess = cols = log_weights = last_ancestors = None
    mean = var = log_evidence_trace = None
    paths = smean = svar = None
    backward = None   # with backward=M: a list of B SsmBackward


class Context:
    """A shard of ``n_particles`` particles on HIP device ``device`` (SMCState's storage)."""

    is_oracle = False

    def __init__(self, n_particles: int, seed: int = 42, device: int = 0):
        self._L = load_library()
        h = C.c_void_p()
        check(self._L.wsmc_create(C.byref(h), int(n_particles), int(device), int(seed) & (2**64 - 1)))
        self._h = h
        self.n = int(n_particles)
        self.seed = int(seed)
        self.device = int(device)
        self.world = 1
        self.rank = 0

    @classmethod
    def multi(cls, n_particles: int, n_gpus: int, seed: int = 42, devices=None,
              transport: int = abi.TRANSPORT_RCCL) -> "Context":
        """One handle over n_gpus shards (wsmc_create_multi): every call fans out to the
        shards; host arrays cover all n_particles."""
        self = cls.__new__(cls)
        self._L = load_library()
        h = C.c_void_p()
        devs = None
        if devices is not None:
            devs = (C.c_int32 * n_gpus)(*[int(d) for d in devices])
        check(self._L.wsmc_create_multi(C.byref(h), int(n_particles), int(n_gpus),
                                        C.cast(devs, _I32P) if devs is not None else None,
                                        int(seed) & (2**64 - 1), int(transport)))
        self._h = h
        self.n = int(n_particles)
        self.seed = int(seed)
        self.device = int(devices[0]) if devices is not None else 0
        self.world = 1
        self.rank = 0
        return self

    # ---- lifetime ----
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.wsmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self) -> None:
        check(self._L.wsmc_sync(self._h))

    # ---- multi-GPU ----
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(load_library().wsmc_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, uid: bytes, world: int, rank: int, global_offset: int, global_n: int) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        check(self._L.wsmc_comm_init(self._h, buf, int(world), int(rank), int(global_offset), int(global_n)))
        self.world, self.rank = int(world), int(rank)

    def comm_init_host(self, allgather, world: int, rank: int, global_offset: int, global_n: int) -> None:
        """Shard this context with a host-side record exchange: ``allgather(list_of_u64)`` must
        return every rank's list in rank order (e.g. wsmc.hostcomm.HostComm.allgather)."""
        def _exchange(_user, mine, words, out):
            try:
                nb = 8 * int(words)
                recs = allgather(C.string_at(mine, nb))        # raw u64 words of this rank
                for r, rec in enumerate(recs):
                    if len(rec) != nb:   # the ranks are at different exchanges: a desync
                        sys.stderr.write(f"wsmc host exchange: rank {rank} sent {nb} B, rank {r} {len(rec)} B\n")
                        return 1
                    C.memmove(C.addressof(out.contents) + r * nb, rec, nb)
                return 0
            except Exception as e:   # the reason goes to stderr; the ABI call fails with ERCCL
                sys.stderr.write(f"wsmc host exchange: rank {rank}: {type(e).__name__}: {e}\n")
                return 1
        self._exchange_cb = abi.EXCHANGE_FN(_exchange)   # keep alive as long as the context
        check(self._L.wsmc_comm_init_host(self._h, C.cast(self._exchange_cb, C.c_void_p), None, int(world),
                                          int(rank), int(global_offset), int(global_n)))
        self.world, self.rank = int(world), int(rank)

    def comm_set_timeout(self, seconds: float) -> None:
        """wsmc_comm_set_timeout: abort the communicator when a stream wait exceeds `seconds`."""
        check(self._L.wsmc_comm_set_timeout(self._h, float(seconds)))

    def comm_info(self) -> dict:
        """wsmc_comm_info: shards, world/rank, the RCCL communicator's own rank count
        (ncclCommCount), transport, shard mode, and each shard's device and size."""
        ci = abi.CommInfo()
        check(self._L.wsmc_comm_info(self._h, C.byref(ci)))
        k = min(int(ci.shards), 8)
        return {"shards": int(ci.shards), "world": int(ci.world), "rank": int(ci.rank),
                "rccl_ranks": int(ci.rccl_ranks),
                "transport": {abi.TRANSPORT_RCCL: "rccl", abi.TRANSPORT_HOST: "host"}.get(int(ci.transport), "none"),
                "shard_mode": "exact" if ci.shard_mode == abi.SHARD_EXACT else "island",
                "devices": [int(ci.devices[g]) for g in range(k)],
                "shard_n": [int(ci.shard_n[g]) for g in range(k)]}

    @staticmethod
    def device_count() -> int:
        n = C.c_int32()
        check(load_library().wsmc_device_count(C.byref(n)))
        return int(n.value)

    def comm_set_shard_mode(self, mode: int) -> None:
        """abi.SHARD_ISLAND (default) or abi.SHARD_EXACT: sharded Resample over the whole
        population, bit-identical to one context holding every particle (include/wsmc.h)."""
        check(self._L.wsmc_comm_set_shard_mode(self._h, int(mode)))

    # ---- store (AbstractParticleStore) ----
    def col_find(self, name: str) -> int:
        c = C.c_int32()
        check(self._L.wsmc_col_find(self._h, name.encode(), C.byref(c)))
        return int(c.value)

    def col_create(self, name: str, dim: int = 1) -> int:
        c = C.c_int32()
        check(self._L.wsmc_col_create(self._h, name.encode(), int(dim), C.byref(c)))
        return int(c.value)

    def col_dim(self, col: int) -> int:
        d = C.c_int32()
        check(self._L.wsmc_col_info(self._h, int(col), None, 0, C.byref(d)))
        return int(d.value)

    def col_names(self) -> list[str]:
        n = C.c_int32()
        check(self._L.wsmc_col_count(self._h, C.byref(n)))
        out = []
        buf = C.create_string_buffer(256)
        for k in range(n.value):
            check(self._L.wsmc_col_info(self._h, k, buf, 256, None))
            out.append(buf.value.decode())
        return out

    def col_download(self, col: int) -> np.ndarray:
        d = self.col_dim(col)
        a = np.empty(d * self.n)
        check(self._L.wsmc_col_download(self._h, int(col), _dptr(a)))
        return a.reshape(d, self.n) if d > 1 else a

    def col_upload(self, col: int, values) -> None:
        d = self.col_dim(col)
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(d * self.n))
        check(self._L.wsmc_col_upload(self._h, int(col), _dptr(v)))

    def store_resample(self, indices) -> None:
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int32))
        check(self._L.wsmc_store_resample(self._h, idx.ctypes.data_as(_I32P)))

    def store_set_lazy(self, lazy: bool) -> None:
        """Lazy genealogy (default) or the eager ColumnStore gather of every column."""
        check(self._L.wsmc_store_set_lazy(self._h, 1 if lazy else 0))

    def store_materialize(self) -> None:
        """Bring every column up to date (one trace over the Resample log)."""
        check(self._L.wsmc_store_materialize(self._h))

    def store_info(self) -> dict:
        e = C.c_int64()
        st = C.c_int32()
        check(self._L.wsmc_store_info(self._h, C.byref(e), C.byref(st)))
        return {"log_entries": e.value, "stale_columns": st.value}

    # ---- weights / state ----
    def weights_download(self) -> np.ndarray:
        a = np.empty(self.n)
        check(self._L.wsmc_weights_download(self._h, _dptr(a)))
        return a

    def weights_upload(self, w) -> None:
        a = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(self.n))
        check(self._L.wsmc_weights_upload(self._h, _dptr(a)))

    def log_evidence(self) -> float:
        v = C.c_double()
        check(self._L.wsmc_log_evidence(self._h, C.byref(v)))
        return float(v.value)

    # ---- analysis reductions (src/utils.jl) ----
    def weighted_moments(self, exprs, want_cov: bool = True):
        """Means (and uncorrected covariance) of up to 4 operand expressions under
        exp_norm(weights): expectation / @E and describe's mean / std."""
        ex = list(exprs) if isinstance(exprs, (list, tuple)) else [exprs]
        d = len(ex)
        arr = (Operand * 4)()
        for k in range(4):
            arr[k] = ex[k] if k < d else ex[0]
        mean = np.zeros(d)
        cov = np.zeros(d * d)
        check(self._L.wsmc_weighted_moments(self._h, arr, d, _dptr(mean), _dptr(cov) if want_cov else None))
        return mean, (cov.reshape(d, d) if want_cov else None)

    def col_minmax(self, col: int, comp: int = 0):
        mn, mx = C.c_double(), C.c_double()
        check(self._L.wsmc_col_minmax(self._h, int(col), int(comp), C.byref(mn), C.byref(mx)))
        return float(mn.value), float(mx.value)

    def ess(self) -> float:
        v = C.c_double()
        check(self._L.wsmc_ess(self._h, C.byref(v)))
        return float(v.value)

    def weighted_median(self, col: int, comp: int = 0) -> float:
        """StatsBase.quantile(v, Weights(w), 0.5) of a column component (describe's median)."""
        v = C.c_double()
        check(self._L.wsmc_weighted_median(self._h, int(col), int(comp), C.byref(v)))
        return float(v.value)

    def histogram(self, col: int, comp: int = 0) -> np.ndarray:
        """describe's 8-bin weighted sparkline as levels 1..8 (src/utils.jl:120-141)."""
        lv = np.zeros(8, dtype=np.int32)
        check(self._L.wsmc_histogram(self._h, int(col), int(comp), lv.ctypes.data_as(C.POINTER(C.c_int32))))
        return lv

    def sample_particles(self, n: int, replace: bool = True) -> np.ndarray:
        """sample(state, n; replace) indices (0-based), src/utils.jl:92-118."""
        out = np.zeros(max(int(n), 0), dtype=np.int64)
        check(self._L.wsmc_sample_particles(self._h, int(n), int(bool(replace)),
                                            out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def col_gather_rows(self, col: int, idx) -> np.ndarray:
        """getcol(store, c)[idx] on the device: [n] (scalar column) or [dim][n]."""
        ix = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
        dim = self.col_dim(col)
        out = np.zeros((dim, len(ix)))
        check(self._L.wsmc_col_gather_rows(self._h, int(col), ix.ctypes.data_as(C.POINTER(C.c_int64)), len(ix),
                                           _dptr(out)))
        return out[0] if dim == 1 else out

    def get_state(self) -> dict:
        s = State()
        check(self._L.wsmc_get_state(self._h, C.byref(s)))
        return dict(resampled=int(s.resampled), weights_changed=int(s.weights_changed), depth=int(s.depth),
                    n_terms=int(s.n_terms), last_ess_perc=float(s.last_ess_perc),
                    op_counter=int(s.op_counter), n_resamples=int(s.n_resamples))

    def set_depth(self, d: int) -> None:
        check(self._L.wsmc_set_depth(self._h, int(d)))

    def set_op_counter(self, op: int) -> None:
        check(self._L.wsmc_set_op_counter(self._h, int(op)))

    def last_ancestors(self) -> np.ndarray:
        a = np.empty(self.n, dtype=np.int32)
        check(self._L.wsmc_last_ancestors(self._h, a.ctypes.data_as(_I32P)))
        return a

    # ---- operators ----
    def assign(self, out: int, exprs) -> None:
        check(self._L.wsmc_assign(self._h, int(out), _operands4(exprs)))

    def assign_expr(self, out: int, prog, lens) -> None:
        """wsmc_assign_expr: prog a ctypes XInst array (wsmc.dsl.xprogram), lens the
        per-component program lengths"""
        ln = (C.c_int32 * 4)(*(list(lens) + [0] * (4 - len(lens))))
        check(self._L.wsmc_assign_expr(self._h, int(out), prog, ln))

    def sample(self, out: int, dist: Dist) -> None:
        check(self._L.wsmc_sample(self._h, int(out), C.byref(dist)))

    def sample_importance(self, out: int, proposal: Dist, target: Dist) -> None:
        check(self._L.wsmc_sample_importance(self._h, int(out), C.byref(proposal), C.byref(target)))

    def observe(self, dist: Dist, x) -> None:
        check(self._L.wsmc_observe(self._h, C.byref(dist), _operands4(x)))

    def weight(self, dist: Dist, x) -> None:
        check(self._L.wsmc_weight(self._h, C.byref(dist), _operands4(x)))

    def resample(self, ess_perc_min: float, scheme: int = abi.RESAMPLE_STRATIFIED, wait: bool = True):
        """Resample.apply!; returns (resampled, ESS%). wait=False leaves the decision on the
        device (no host round trip; the gather and weight reset are gated there) and returns
        None; get_state() folds it in later."""
        if not wait:
            check(self._L.wsmc_resample(self._h, float(ess_perc_min), int(scheme), None, None))
            return None
        r = C.c_int32()
        e = C.c_double()
        check(self._L.wsmc_resample(self._h, float(ess_perc_min), int(scheme), C.byref(r), C.byref(e)))
        return bool(r.value), float(e.value)

    def move(self, proposal: int, targets, step: float, lo=None, hi=None, target_depth: int = -1,
             diversity: float = math.nan, wait: bool = True):
        """Move.apply!; returns the accepted count. wait=False: asynchronous (returns None; a
        PosDefException surfaces at the next synchronizing call)."""
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.int32))
        d = len(t)
        lo_a = None if lo is None else np.ascontiguousarray(np.asarray(lo, float).reshape(d))
        hi_a = None if hi is None else np.ascontiguousarray(np.asarray(hi, float).reshape(d))
        acc = C.c_int64()
        rc = self._L.wsmc_move(self._h, int(proposal), t.ctypes.data_as(_I32P), d, float(step),
                               None if lo_a is None else _dptr(lo_a), None if hi_a is None else _dptr(hi_a),
                               int(target_depth), float(diversity), C.byref(acc) if wait else None)
        if rc == abi.WSMC_ENOTPD:
            raise np.linalg.LinAlgError(self._L.wsmc_last_error().decode())
        check(rc)
        return int(acc.value) if wait else None

    def move_gated(self, proposal: int, targets, step: float, lo=None, hi=None, target_depth: int = -1,
                   diversity: float = math.nan) -> None:
        """Move.apply! inside `if resampled` decided on the device (wsmc_move_gated): runs only
        if the last Resample resampled; consumes its two op counters either way."""
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.int32))
        d = len(t)
        lo_a = None if lo is None else np.ascontiguousarray(np.asarray(lo, float).reshape(d))
        hi_a = None if hi is None else np.ascontiguousarray(np.asarray(hi, float).reshape(d))
        rc = self._L.wsmc_move_gated(self._h, int(proposal), t.ctypes.data_as(_I32P), d, float(step),
                                     None if lo_a is None else _dptr(lo_a), None if hi_a is None else _dptr(hi_a),
                                     int(target_depth), float(diversity))
        if rc == abi.WSMC_ENOTPD:
            raise np.linalg.LinAlgError(self._L.wsmc_last_error().decode())
        check(rc)

    def move_block(self, moves, gated: bool = False, wait: bool = False):
        """A statement block of consecutive Moves (wsmc_move_block): `moves` is a list of
        (proposal, targets, step) or (proposal, targets, step, lo, hi[, target_depth]); the
        same results as calling move / move_gated for each in order. wait=True returns the
        accepted counts (a list), else None (asynchronous)."""
        n = len(moves)
        specs = (abi.MoveSpec * max(n, 1))()
        for m, mv in enumerate(moves):
            proposal, targets, step = mv[0], mv[1], mv[2]
            lo = mv[3] if len(mv) > 3 else None
            hi = mv[4] if len(mv) > 4 else None
            depth = mv[5] if len(mv) > 5 else -1
            t = [int(x) for x in np.asarray(targets).reshape(-1)]
            if not 1 <= len(t) <= 4:
                raise ValueError("a Move has 1..4 targets")
            sp = specs[m]
            sp.proposal, sp.d, sp.step, sp.target_depth = int(proposal), len(t), float(step), int(depth)
            sp.bounded = 0 if (lo is None and hi is None) else 1
            for k in range(4):
                sp.targets[k] = t[k] if k < len(t) else -1
                sp.lo[k] = float(lo[k]) if lo is not None and k < len(t) else -math.inf
                sp.hi[k] = float(hi[k]) if hi is not None and k < len(t) else math.inf
        acc = (C.c_int64 * max(n, 1))()
        rc = self._L.wsmc_move_block(self._h, n, specs, 1 if gated else 0, acc if wait else None)
        if rc == abi.WSMC_ENOTPD:
            raise np.linalg.LinAlgError(self._L.wsmc_last_error().decode())
        check(rc)
        return [int(acc[m]) for m in range(n)] if wait else None

    def score(self, target_depth: int) -> np.ndarray:
        out = np.empty(self.n)
        check(self._L.wsmc_score(self._h, int(target_depth), _dptr(out)))
        return out

    def marginal_diversity(self, targets) -> float:
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.int32))
        v = C.c_double()
        check(self._L.wsmc_marginal_diversity(self._h, t.ctypes.data_as(_I32P), len(t), C.byref(v)))
        return float(v.value)

    # ---- fused runners ----
    def run_stats(self) -> dict:
        """The fused run's Resample statistics (wsmc_debug_run_stats): steps whose statistics
        were recomputed against the exact reference point (cumulative), and where they are taken."""
        st = (C.c_int64 * 4)()
        check(self._L.wsmc_debug_run_stats(self._h, st))
        return {"missed_steps": st[0], "qstat_mode": st[1], "replays": st[2], "batch_statistics": st[3]}

    def weight_stores(self) -> dict:
        """The fused run's weight rows, counted by the propagate launches on the device
        (wsmc_debug_weight_stores, cumulative): the launches with the Resample statistics that
        stored their row, that recomputed the previous row, their number, and the launches without
        the statistics (which always store)."""
        st = (C.c_int64 * 4)()
        check(self._L.wsmc_debug_weight_stores(self._h, st))
        return {"stored": st[0], "recomputed": st[1], "qs_launches": st[2], "plain_launches": st[3]}

    def ssm2d_routes(self) -> dict:
        """ssm2d_run's calls by route (wsmc_debug_ssm2d_routes, cumulative): the fused runs, and the
        runs issued as statements because the context held a column that is not the run's."""
        st = (C.c_int64 * 2)()
        check(self._L.wsmc_debug_ssm2d_routes(self._h, st))
        return {"fused_runs": st[0], "statement_runs": st[1]}

    def ssm2d_run(self, obs, x0=(0.0, 0.0), v0=(1.0, 0.0), q_var=0.1, r_var=0.5, ess_perc_min=0.5,
                  scheme: int = abi.RESAMPLE_STRATIFIED, keep_history: bool = True,
                  want_evidence: bool = True):
        o = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1, 2))
        x0a = np.asarray(x0, dtype=np.float64)
        v0a = np.asarray(v0, dtype=np.float64)
        ev = C.c_double()
        check(self._L.wsmc_ssm2d_run(self._h, _dptr(o), len(o), _dptr(x0a), _dptr(v0a), float(q_var),
                                     float(r_var), float(ess_perc_min), int(scheme), int(bool(keep_history)),
                                     C.byref(ev) if want_evidence else None))
        return float(ev.value) if want_evidence else None

    def lgssm1d_run(self, data, a=0.9, q=1.0, r=0.5, x0_std=1.0, ess_perc_min=1.0,
                    scheme: int = abi.RESAMPLE_STRATIFIED, want_evidence: bool = True, ess_trace: bool = False):
        """The 1D linear-Gaussian SSM of models.lgssm1d_statements as one call (wsmc_lgssm1d_run):
        the same column, weights, ancestors, state and RNG positions. Returns the log evidence
        (None without want_evidence), or (evidence, trace) with ess_trace: the ESS% of every
        step's post-Observe Resample."""
        d = np.ascontiguousarray(np.asarray(data, dtype=np.float64).reshape(-1))
        ev = C.c_double()
        tr = np.empty(len(d)) if ess_trace else None
        check(self._L.wsmc_lgssm1d_run(self._h, _dptr(d), len(d), float(a), float(q), float(r), float(x0_std),
                                       float(ess_perc_min), int(scheme), C.byref(ev) if want_evidence else None,
                                       _dptr(tr) if ess_trace else None))
        e = float(ev.value) if want_evidence else None
        return (e, tr) if ess_trace else e

    def lgssm_stats(self) -> dict:
        """wsmc_debug_lgssm's counters: the persistent kernel's particle cap, the runs it took, the
        runs that went through the statement route, the segments launched (cumulative), and the
        last run's host bookkeeping and whole-call seconds."""
        st = (C.c_int64 * 6)()
        check(self._L.wsmc_debug_lgssm(self._h, -1, st))
        return {"cap": st[0], "persistent_runs": st[1], "statement_runs": st[2], "segments": st[3],
                "bookkeeping_s": st[4] / 1e6, "call_s": st[5] / 1e6}

    def set_lgssm_segment(self, steps: int) -> None:
        """Steps per launch of the persistent LGSSM kernel (0 restores the default)."""
        if steps < 0:
            raise ValueError("steps must be >= 0")
        check(self._L.wsmc_debug_lgssm(self._h, int(steps), None))

    def ssm_run(self, spec, data, ess_perc_min=1.0, scheme: int = abi.RESAMPLE_STRATIFIED,
                want_evidence: bool = True, ess_trace: bool = False, T: int | None = None, trace=False, smooth=False,
                backward: int = 0, backward_seed: int = 0, record: bool = False):
        """A scalar state-space model (wsmc.SSM) as one call (wsmc_ssm_run): the same columns,
        weights, ancestors, state, tape and RNG positions as spec.statements(self, data, ...).
        data: T values, or T rows of the spec's data columns (a spec that reads no data takes T).
        Returns the log evidence (None without want_evidence), or (evidence, trace) with
        ess_trace: the ESS% of the Resample after each step's last observe.
        trace=True (wsmc_ssm_run_traced) returns (evidence, SsmTrace): per step the ESS%, every
        column's filtered mean and variance and the cumulative log evidence, bit for bit those of
        spec.statements(self, data, trace=True); everything else the run leaves is the untraced
        run's. trace may also name the parts wanted: a subset of ("ess", "mean", "var",
        "log_evidence"); the others are None.
        smooth=True (wsmc_ssm_run_smoothed) returns (evidence, SsmSmooth), with trace as well
        (evidence, SsmTrace, SsmSmooth): the final particles' trajectories and the smoothed moments,
        bit for bit those of spec.statements(self, data, smooth=True). smooth may name the parts
        wanted: a subset of ("paths", "mean", "var"). A smoothed run has the persistent route only:
        what would send ssm_run through the statements raises WSMCError(WSMC_EARG) here.
        backward=M (wsmc_ssm_run_backward) returns (evidence, SsmBackward), with trace as well
        (evidence, SsmTrace, SsmBackward): M trajectories drawn by forward filtering, backward
        simulation from backward_seed, bit for bit spec.backward_definition over the record of
        spec.statements(self, data, record=True); record=True keeps that record in
        SsmBackward.record. Everything the run leaves on the context is ssm_run(trace=True)'s. The
        persistent route only, and not together with smooth (two calls)."""
        tab = spec.table(data, T)
        ev = C.c_double()
        sparts = smooth_parts(smooth)
        if backward:
            if int(backward) < 0:
                raise ValueError("backward: the number of trajectories")
            if sparts or ess_trace:
                raise ValueError("backward and smooth / ess_trace: make two calls (the ESS% is in trace=(\"ess\",))")
            steps, S = len(tab), len(spec.cols)
            buf, out = trace_buffers(trace_parts(trace), (steps,), S)
            bbuf, bo = backward_buffers(steps, S, self.n, int(backward), record=record)
            check(self._L.wsmc_ssm_run_backward(self._h, C.byref(spec.spec), _dptr(tab) if tab.size else None, steps,
                                                float(ess_perc_min), int(scheme), C.byref(ev) if want_evidence else None,
                                                C.byref(out), int(backward), int(backward_seed) & (2**64 - 1), C.byref(bo)))
            tr = (SsmTrace(*trace_by_name(buf, spec.cols)),) if trace else ()
            return ((float(ev.value) if want_evidence else None),) + tr + (backward_by_name(bbuf, spec.cols),)
        if record:
            raise ValueError("record=True needs backward=M (the record is the backward pass's)")
        if sparts and ess_trace:
            raise ValueError("ess_trace and smooth: ask for the ESS% with trace=(\"ess\",)")
        if trace or sparts:
            if ess_trace:
                raise ValueError("ess_trace and trace: the trace holds the ESS% (SsmTrace.ess)")
            steps, S = len(tab), len(spec.cols)
            buf, out = trace_buffers(trace_parts(trace), (steps,), S)
            head = (self._h, C.byref(spec.spec), _dptr(tab) if tab.size else None, steps, float(ess_perc_min), int(scheme),
                    C.byref(ev) if want_evidence else None, C.byref(out))
            if sparts:
                sbuf, so = smooth_buffers(sparts, (steps,), S, self.n)
                check(self._L.wsmc_ssm_run_smoothed(*head, C.byref(so)))
                sm = SsmSmooth(*smooth_by_name(sbuf, spec.cols), self.weights_download())
            else:
                check(self._L.wsmc_ssm_run_traced(*head))
            tr = SsmTrace(*trace_by_name(buf, spec.cols))
            res = ((float(ev.value) if want_evidence else None),) + ((tr,) if trace else ()) + ((sm,) if sparts else ())
            return res
        tr = np.empty(len(tab)) if ess_trace else None
        check(self._L.wsmc_ssm_run(self._h, C.byref(spec.spec), _dptr(tab) if tab.size else None, len(tab),
                                   float(ess_perc_min), int(scheme), C.byref(ev) if want_evidence else None,
                                   _dptr(tr) if ess_trace else None))
        e = float(ev.value) if want_evidence else None
        return (e, tr) if ess_trace else e

    def ssm_backward(self, spec, data, record, M: int, seed: int, T: int | None = None):
        """Forward filtering, backward simulation over a record the caller holds (wsmc_ssm_backward):
        M trajectories as an SsmBackward, bit for bit spec.backward_definition(make_backend, record,
        data, M, seed). record: an SsmRecord (spec.statements(..., record=True), or
        ssm_run(backward=M, record=True)'s). This context gives the device and the stream; its
        particles and state are not touched."""
        tab = spec.table(data, T)
        steps, S = len(tab), len(spec.cols)
        if record.cols.shape[:2] != (steps, S):
            raise ValueError(f"record: {record.cols.shape[0]} steps of {record.cols.shape[1]} columns, the call has {steps} of {S}")
        n = record.cols.shape[2]
        bbuf, bo = backward_buffers(steps, S, n, int(M))
        check(self._L.wsmc_ssm_backward(self._h, C.byref(spec.spec), _dptr(tab) if tab.size else None, steps, _dptr(record.cols),
                                        _dptr(record.log_weights), n, int(M), int(seed) & (2**64 - 1), C.byref(bo)))
        bw = backward_by_name(bbuf, spec.cols)
        bw.record = record
        return bw

    def ssm_backward_stats(self) -> dict:
        """wsmc_debug_ssm_backward's figures of the last backward pass on this context: device seconds
        of the run's segments (0 for ssm_backward), of the backward kernel and of the rows kernel, the
        bytes of the record and the outputs, and the segments this context has launched on the
        backward-recording kernels (cumulative; no other run launches them)."""
        st = (C.c_int64 * 5)()
        check(self._L.wsmc_debug_ssm_backward(self._h, st))
        return {"segments_s": st[0] / 1e6, "backward_s": st[1] / 1e6, "rows_s": st[2] / 1e6, "bytes": int(st[3]),
                "recording_segments": int(st[4])}

    def ssm_stats(self) -> dict:
        """wsmc_debug_ssm's counters: the persistent kernel's particle cap for 1..4 columns, the runs
        it took, the runs that went through the statement route, the segments launched
        (cumulative), and the last run's host bookkeeping and whole-call seconds."""
        st = (C.c_int64 * 9)()
        check(self._L.wsmc_debug_ssm(self._h, -1, st))
        return {"cap": {S: int(st[S - 1]) for S in range(1, 5)}, "persistent_runs": st[4], "statement_runs": st[5],
                "segments": st[6], "bookkeeping_s": st[7] / 1e6, "call_s": st[8] / 1e6}

    def set_ssm_segment(self, steps: int) -> None:
        """Steps per launch of the persistent SSM kernel (0 restores the default)."""
        if steps < 0:
            raise ValueError("steps must be >= 0")
        check(self._L.wsmc_debug_ssm(self._h, int(steps), None))

    def ssm_run_batch(self, specs, data, n: int, seeds, ess_perc_min=1.0, scheme: int = abi.RESAMPLE_STRATIFIED,
                      ess_trace: bool = False, state: bool = False, T: int | None = None,
                      trace: bool = False, smooth=False, backward: int = 0, backward_seeds=None,
                      record: bool = False) -> "SsmBatchResult":
        """B = len(seeds) independent filters of n particles in one call (wsmc_ssm_run_batch), one
        persistent workgroup each: filter b is, bit for bit, ssm_run(spec b, table b) on a fresh
        Context(n, seed=seeds[b]). This context gives the device and the stream; its own particles
        and state are not touched.
        specs: one wsmc.SSM, or a list of B of one shape (SSM.same_shape: only numbers differ).
        data: one table (T values or T rows), or a list / 3-D array of B tables of one length.
        Returns an SsmBatchResult: log_evidence, n_resamples, last_resampled ([B] each), with
        ess_trace `ess` [B, T], with state `cols` (name -> [B, n]), `log_weights` [B, n] and
        `last_ancestors` [B, n] (row b is zeros while filter b has not resampled). trace=True
        (wsmc_ssm_run_batch_traced) also fills `ess`, `mean` / `var` (name -> [B, T]) and
        `log_evidence_trace` [B, T]: row b is ssm_run(trace=True)'s SsmTrace of filter b.
        smooth=True, or a subset of ("paths", "mean", "var") (wsmc_ssm_run_batch_smoothed), fills
        `paths` (name -> [B, T, n]), `smean` and `svar` (name -> [B, T]): row b is
        ssm_run(smooth=True)'s SsmSmooth of filter b (its log_weights are `log_weights` with state).
        backward=M with backward_seeds [B] (wsmc_ssm_run_batch_backward; not with smooth) fills
        `backward`, a list of B SsmBackward: filter b's is ssm_run(backward=M,
        backward_seed=backward_seeds[b])'s on a fresh Context(n, seed=seeds[b]), with its record
        when record=True."""
        sparts = smooth_parts(smooth)
        if backward and sparts:
            raise ValueError("backward and smooth: make two calls")
        if backward and (int(backward) < 0 or backward_seeds is None or len(backward_seeds) != len(seeds)):
            raise ValueError("backward: the number of trajectories, and one backward seed per filter")
        if record and not backward:
            raise ValueError("record=True needs backward=M (the record is the backward pass's)")
        spec_list, tabs, seeds_a = batch_arguments(specs, data, n, seeds, T)   # (before any device call)
        B, first, steps = len(seeds_a), spec_list[0], len(tabs[0])
        tab = np.ascontiguousarray(np.stack(tabs)) if tabs[0].size else None
        arr = (abi.SsmSpec * len(spec_list))()
        for k, s in enumerate(spec_list):
            C.memmove(C.byref(arr[k]), C.byref(s.spec), C.sizeof(abi.SsmSpec))
        S = len(first.cols)
        res = SsmBatchResult()
        res.log_evidence = np.empty(B)
        res.n_resamples = np.empty(B, dtype=np.int64)
        res.last_resampled = np.empty(B, dtype=np.int32)
        out = abi.SsmBatchOut()
        out.log_evidence = _dptr(res.log_evidence)
        out.n_resamples = res.n_resamples.ctypes.data_as(C.POINTER(C.c_int64))
        out.last_resampled = res.last_resampled.ctypes.data_as(_I32P)
        tbuf, tr = trace_buffers(TRACE_PARTS if trace else (), (B, steps), S)
        if ess_trace:   # (with the trace as well: one buffer for both)
            res.ess = tbuf["ess"] if trace else np.empty((B, steps))
            out.ess_trace = _dptr(res.ess)
        if state:
            cols = np.empty((B, S, int(n)))
            res.log_weights = np.empty((B, int(n)))
            res.last_ancestors = np.empty((B, int(n)), dtype=np.int32)
            out.cols = _dptr(cols)
            out.log_weights = _dptr(res.log_weights)
            out.last_ancestors = res.last_ancestors.ctypes.data_as(_I32P)
        args = (self._h, arr, len(spec_list), _dptr(tab) if tab is not None else None, len(tabs), steps, int(n), B,
                seeds_a.ctypes.data_as(C.POINTER(C.c_uint64)), float(ess_perc_min), int(scheme), C.byref(out))
        if backward:
            bbuf, bo = backward_buffers(steps, S, int(n), int(backward), lead=(B,), record=record)
            bseeds = np.ascontiguousarray(np.asarray([int(s) & (2**64 - 1) for s in backward_seeds], dtype=np.uint64))
            check(self._L.wsmc_ssm_run_batch_backward(*args, C.byref(tr), int(backward), bseeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      C.byref(bo)))
            res.backward = [backward_by_name({k: v[b] for k, v in bbuf.items()}, first.cols) for b in range(B)]
        elif sparts:
            sbuf, so = smooth_buffers(sparts, (B, steps), S, int(n))
            check(self._L.wsmc_ssm_run_batch_smoothed(*args, C.byref(tr), C.byref(so)))
            res.paths, res.smean, res.svar = smooth_by_name(sbuf, first.cols)
        elif trace:
            check(self._L.wsmc_ssm_run_batch_traced(*args, C.byref(tr)))
        else:
            check(self._L.wsmc_ssm_run_batch(*args))
        if trace:
            res.ess, res.mean, res.var, res.log_evidence_trace = trace_by_name(tbuf, first.cols)
        res.last_resampled = res.last_resampled.astype(bool)
        if state:
            res.cols = {name: cols[:, k, :] for k, name in enumerate(first.cols)}
        return res

    def ssm_run_conditional(self, specs, data, n: int, seeds, reference, ess_perc_min=0.5, trace: bool = False,
                            backward: int = 0, backward_seeds=None, record: bool = False, state: bool = False,
                            T: int | None = None) -> "SsmBatchResult":
        """B = len(seeds) conditional SMC filters in one call (wsmc_ssm_run_conditional), one
        persistent workgroup each: filter b is, bit for bit, spec.conditional_definition(make_backend,
        table b, n, seeds[b], reference[b], ess_perc_min) with particle n-1 pinned to its reference
        trajectory and independent ancestor draws with the last slot forced. reference: an array
        [B, T, n_cols] in the spec's column order, or column name -> [B, T] (entries of columns
        that are not pinned are ignored). specs, data, trace and state as in ssm_run_batch, whose
        SsmBatchResult this returns. backward=M with backward_seeds [B] fills `backward`, a list of
        B SsmBackward drawn over each filter's record (with record=True the record itself); with
        backward=0 and record=True `backward` holds B SsmRecord. One sweep of particle Gibbs with
        backward sampling is this call with backward=1 (wsmc.particle_gibbs)."""
        M = int(backward)
        if M < 0 or (M and (backward_seeds is None or len(backward_seeds) != len(seeds))):
            raise ValueError("backward: the number of trajectories, and one backward seed per filter")
        spec_list, tabs, seeds_a = batch_arguments(specs, data, n, seeds, T)   # (before any device call)
        B, first, steps = len(seeds_a), spec_list[0], len(tabs[0])
        S, n = len(first.cols), int(n)
        if isinstance(reference, dict):
            reference = {k: np.asarray(v, dtype=np.float64).reshape(B, steps) for k, v in reference.items()}
            ref = np.stack([first.reference_table({k: v[b] for k, v in reference.items()}, steps) for b in range(B)])
        else:
            ref = np.ascontiguousarray(np.asarray(reference, dtype=np.float64))
            if ref.shape != (B, steps, S):
                raise ValueError(f"reference: shape {ref.shape}, the call has {B} filters of {steps} steps of {S} columns")
        tab = np.ascontiguousarray(np.stack(tabs)) if tabs[0].size else None
        arr = (abi.SsmSpec * len(spec_list))()
        for k, s in enumerate(spec_list):
            C.memmove(C.byref(arr[k]), C.byref(s.spec), C.sizeof(abi.SsmSpec))
        res = SsmBatchResult()
        res.log_evidence = np.empty(B)
        res.n_resamples = np.empty(B, dtype=np.int64)
        res.last_resampled = np.empty(B, dtype=np.int32)
        out = abi.SsmBatchOut()
        out.log_evidence = _dptr(res.log_evidence)
        out.n_resamples = res.n_resamples.ctypes.data_as(C.POINTER(C.c_int64))
        out.last_resampled = res.last_resampled.ctypes.data_as(_I32P)
        tbuf, tr = trace_buffers(TRACE_PARTS if trace else (), (B, steps), S)
        if state:
            cols = np.empty((B, S, n))
            res.log_weights = np.empty((B, n))
            res.last_ancestors = np.empty((B, n), dtype=np.int32)
            out.cols = _dptr(cols)
            out.log_weights = _dptr(res.log_weights)
            out.last_ancestors = res.last_ancestors.ctypes.data_as(_I32P)
        if M:
            bbuf, bo = backward_buffers(steps, S, n, M, lead=(B,), record=record)
            bseeds = np.ascontiguousarray(np.asarray([int(s) & (2**64 - 1) for s in backward_seeds], dtype=np.uint64))
        else:   # the record alone, if asked for
            bbuf = {"particles": np.empty((B, steps, S, n)), "log_weights": np.empty((B, steps, n))} if record else {}
            bo, bseeds = abi.SsmBackwardOut(), None
            for p, a in bbuf.items():
                setattr(bo, p, _dptr(a))
        check(self._L.wsmc_ssm_run_conditional(
            self._h, arr, len(spec_list), _dptr(tab) if tab is not None else None, len(tabs), steps, n, B,
            seeds_a.ctypes.data_as(C.POINTER(C.c_uint64)), float(ess_perc_min), _dptr(ref), C.byref(out), C.byref(tr), M,
            bseeds.ctypes.data_as(C.POINTER(C.c_uint64)) if M else None, C.byref(bo)))
        if M:
            res.backward = [backward_by_name({k: v[b] for k, v in bbuf.items()}, first.cols) for b in range(B)]
        elif record:
            res.backward = [SsmRecord(bbuf["particles"][b], bbuf["log_weights"][b]) for b in range(B)]
        if trace:
            res.ess, res.mean, res.var, res.log_evidence_trace = trace_by_name(tbuf, first.cols)
        res.last_resampled = res.last_resampled.astype(bool)
        if state:
            res.cols = {name: cols[:, k, :] for k, name in enumerate(first.cols)}
        return res

    def ssm_conditional_stats(self) -> dict:
        """wsmc_debug_ssm_conditional's figures of the last conditional batch on this context: device
        seconds of its segments, of the backward kernel and of the rows kernel, the bytes of the record,
        the references and the outputs, and the segments this context has launched on the conditional
        kernels (cumulative; no other run launches them)."""
        st = (C.c_int64 * 5)()
        check(self._L.wsmc_debug_ssm_conditional(self._h, st))
        return {"segments_s": st[0] / 1e6, "backward_s": st[1] / 1e6, "rows_s": st[2] / 1e6, "bytes": int(st[3]),
                "conditional_segments": int(st[4])}

    def ssm_smooth_stats(self) -> dict:
        """wsmc_debug_ssm_smooth's figures of the last smoothed run or batch on this context: device
        seconds of its segments, of the trace-back and of the rows kernel, and the bytes of the log."""
        st = (C.c_int64 * 4)()
        check(self._L.wsmc_debug_ssm_smooth(self._h, st))
        return {"segments_s": st[0] / 1e6, "traceback_s": st[1] / 1e6, "rows_s": st[2] / 1e6, "log_bytes": int(st[3])}

    def ssm_batch_stats(self) -> dict:
        """wsmc_debug_ssm_batch's figures: the last batch's resident workgroups per CU, the device's
        CU count (known before the first batch), the segments it launched and its whole-call seconds."""
        st = (C.c_int64 * 4)()
        check(self._L.wsmc_debug_ssm_batch(self._h, -1, st))
        return {"blocks_per_cu": int(st[0]), "cus": int(st[1]), "segments": int(st[2]), "call_s": st[3] / 1e6}

    def set_ssm_batch_segment(self, steps: int) -> None:
        """Steps per launch of ssm_run_batch on this context (0 restores the default)."""
        if steps < 0:
            raise ValueError("steps must be >= 0")
        check(self._L.wsmc_debug_ssm_batch(self._h, int(steps), None))

    def set_timing(self, enabled: bool) -> None:
        check(self._L.wsmc_run_set_timing(self._h, int(bool(enabled))))

    def debug_kernel_bench(self, kernel: int, mode: int = 0, iters: int = 50) -> float:
        v = C.c_double()
        check(self._L.wsmc_debug_kernel_bench(self._h, int(kernel), int(mode), int(iters), C.byref(v)))
        return float(v.value)

    def debug_exact(self, cap: int = -1, ctr: int = -1) -> dict:
        """Exact-sharded fused run: set the neighbour block / trace window sizes (> 0 sets, 0
        restores the defaults, < 0 keeps) and return the last run's statistics."""
        st = (C.c_int64 * 6)()
        check(self._L.wsmc_debug_exact(self._h, int(cap), int(ctr), st))
        return {"need": st[0], "excursion": st[1], "eager_reruns": st[2], "cap": st[3],
                "history_traces": st[4], "no_windows": st[5]}

    def debug_inject_failure(self, shard: int, nth: int) -> None:
        """Test hook: shard `shard` fails its nth next record exchange (include/wsmc.h)."""
        check(self._L.wsmc_debug_inject_failure(self._h, int(shard), int(nth)))

    def timing(self) -> dict:
        t = RunTiming()
        check(self._L.wsmc_run_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in RunTiming._fields_}


def device_count() -> int:
    n = C.c_int32()
    check(load_library().wsmc_device_count(C.byref(n)))
    return int(n.value)

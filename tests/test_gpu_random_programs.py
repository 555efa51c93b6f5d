"""Seeded random statement programs on the GPU against the CPU oracle, bit for bit
(tests/progfuzz.py; the corpus' coverage is asserted by tests/test_random_programs.py).

The oracle is eager, so one answer serves every way of driving the device: `chatty` (every call
waited for, the whole state compared after every statement: almost every statement batch holds one
statement, a fault is located), `quiet` (nothing waited for, no reads, one comparison at the end:
the batches grow to their caps, the Resamples and Moves stay on the stream) and `reads` (the
program's own reads and waits), each with the lazy and the eager store, at N = 1 (one particle),
65 (one past a wave), 1001 (odd, several blocks) and 5002 (even: two particles a thread in the
compiled batches). The directed `caps` programs take the full cross; the `mixed` and `moves` seeds
a Latin square over it, so every (mode, store, N) is met by several seeds."""
import os
import pathlib
import subprocess
import sys

import pytest

import progfuzz as pf
import wsmc
from oracle import Oracle
from wsmc import abi

pytestmark = pytest.mark.gpu
REPO = pathlib.Path(__file__).resolve().parents[1]

MODE_NAMES = ("chatty", "quiet", "reads")
STORE_N = [(lazy, n) for lazy in (True, False) for n in pf.SIZES]


def latin(seed, j, dm, ds):
    """(seed mod 3, seed mod 8) runs over every (mode, store, N) once per 24 seeds; j shifts it by
    (dm, ds), chosen so that the 18 + 12 seeds below meet every combination three times or more"""
    lazy, n = STORE_N[(seed + ds * j) % 8]
    return MODE_NAMES[(seed + dm * j) % 3], lazy, n


def cases():
    out = []
    for seed in pf.CAPS_SEEDS:
        for mode in MODE_NAMES:
            for lazy, n in STORE_N:
                out.append(("caps", seed, mode, lazy, n))
    for seed in pf.MIXED_SEEDS:
        out += [("mixed", seed) + latin(seed, j, 2, 1) for j in range(3)]
    for seed in pf.MOVES_SEEDS:
        out += [("moves", seed) + latin(seed, j, 0, 4) for j in range(2)]
    for seed in pf.EDGE_SEEDS:
        out += [("edge", seed, mode, lazy, n) for mode in MODE_NAMES for lazy in (True, False) for n in (65, 1001)]
    return out


def case_id(c):
    profile, seed, mode, lazy, n = c
    name = pf.caps_name(seed) if profile == "caps" else pf.EDGE_NAMES[seed] if profile == "edge" else str(seed)
    return f"{profile}-{name}-{mode}-{'lazy' if lazy else 'eager'}-{n}"


CASES = cases()


def run_case(profile, seed, mode, lazy, n):
    """one program on a fresh context and a fresh oracle; the compiled statement batches and Move
    blocks stay compiled (none fails to compile, none runs on the interpreter)"""
    before, mv_before = abi.jit_stats(), abi.mv_jit_stats()
    cs = pf.ctx_seed(seed, profile)
    g, o = wsmc.Context(n, seed=cs), Oracle(n, seed=cs)
    try:
        g.store_set_lazy(lazy)
        pf.differential(g, o, pf.gen(seed, profile), mode, pf.info(seed, profile, mode, n, lazy))
    finally:
        g.close()
        o.close()
    after = abi.jit_stats()
    for b, a in ((before, after), (mv_before, abi.mv_jit_stats())):
        assert a["failed"] == 0 and a["interpreted"] == b["interpreted"], (b, a)
    if profile == "caps" and mode == "quiet" and lazy:
        # progfuzz.batch_model (which the CPU test's cap conditions rest on) against the library: the
        # batches it predicts from the program text are the batches launched
        batches, _ = pf.batch_model(pf.gen(seed, profile))
        assert after["launched"] - before["launched"] == len(batches), (after, before, batches)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_program_matches_the_oracle(gpu_available, case):
    run_case(*case)


def test_every_combination_is_met_by_several_seeds():
    met = {}
    for profile, seed, mode, lazy, n in CASES:
        if profile in ("mixed", "moves"):
            met.setdefault((mode, lazy, n), set()).add((profile, seed))
    assert len(met) == 24 and min(len(v) for v in met.values()) >= 3, {k: len(v) for k, v in met.items()}


CHILD = r"""
import sys
sys.path[:0] = [{pkg!r}, {orc!r}, {tests!r}]
import progfuzz as pf
import wsmc
from wsmc import abi
from oracle import Oracle
for profile, seed in {programs!r}:
    cs = pf.ctx_seed(seed, profile)
    g, o = wsmc.Context(1001, seed=cs), Oracle(1001, seed=cs)
    pf.differential(g, o, pf.gen(seed, profile), "quiet", pf.info(seed, profile, "quiet", 1001))
    g.close()
st, mv = abi.jit_stats(), abi.mv_jit_stats()
print("EWJIT", st["launched"], st["interpreted"])
print("MVJIT", mv["launched"], mv["interpreted"])
"""
INTERP_PROGRAMS = ([("mixed", s) for s in (0, 3, 7, 13)] + [("moves", s) for s in (1, 4, 8)] +
                   [("caps", s) for s in pf.CAPS_SEEDS])


def test_interpreter_kernels_match_the_oracle(gpu_available):
    """the statement-batch and Move interpreter kernels (the fallback of a signature that does not
    compile) on the same programs, in a child process with the run-time compiler switched off"""
    code = CHILD.format(pkg=str(REPO / "weightedsampling.jl_amd"), orc=str(REPO / "oracle"), tests=str(REPO / "tests"),
                        programs=INTERP_PROGRAMS)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "WSMC_DIAG_NO_JIT": "1"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    for tag in ("EWJIT", "MVJIT"):
        line = [x for x in r.stdout.splitlines() if x.startswith(tag)][0]
        launched, interpreted = map(int, line.split()[1:])
        assert launched == 0 and interpreted > 0, line


@pytest.mark.parametrize("seed", [2, 5, 11, 17])
@pytest.mark.parametrize("shard_mode", ["island", "exact"])
def test_multi_device_handle_matches_the_sharded_oracle(gpu_available, seed, shard_mode):
    """two shards on the one device behind one handle: island shards against the sharded oracle,
    exact shards against the exact-sharded one (a Move's autoRW moments sum per shard)"""
    n, exact = 1001, shard_mode == "exact"
    cs = pf.ctx_seed(seed, "mixed")
    g = wsmc.Context.multi(n, 2, seed=cs, devices=[0, 0], transport=abi.TRANSPORT_HOST)
    if exact:
        g.comm_set_shard_mode(abi.SHARD_EXACT)
    o = Oracle(n, seed=cs, shards=2, exact=exact)
    try:
        pf.differential(g, o, pf.for_shards(pf.gen(seed, "mixed"), exact), "reads",
                        f"two {shard_mode} shards: " + pf.info(seed, "mixed", "reads", n), sharded=True)
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("first,second,mode,lazy", [(("mixed", 4), ("moves", 2), "quiet", True),
                                                    (("moves", 5), ("mixed", 9), "reads", True),
                                                    (("mixed", 10), ("mixed", 15), "quiet", False)])
def test_two_programs_on_one_context(gpu_available, first, second, mode, lazy):
    """a second program after the first without a reset: the stream positions, the tape, the
    counters and the lazy log continue"""
    n = 1001
    prog = pf.gen(first[1], first[0]) + pf.gen(second[1], second[0], prefix="b_")
    g, o = wsmc.Context(n, seed=77), Oracle(n, seed=77)
    try:
        g.store_set_lazy(lazy)
        pf.differential(g, o, prog, mode, f"{first} then {second}, mode={mode} lazy={lazy} N={n}")
    finally:
        g.close()
        o.close()


# ---- the minimised programs of what the random programs found ----------------------------------
def _o(c0=0.0, *terms):
    return pf.Opnd(float(c0), tuple(terms))


def _normal(mu, sd=1.0):
    return pf.DistSpec(abi.FAM_NORMAL, 1, (mu,), _o(sd))


def _iso(dim):
    return pf.DistSpec(abi.FAM_MVNORMAL_ISO, dim, tuple(_o(0.1 * k) for k in range(dim)), _o(0.8))


DIRECTED = {
    # A Sample or weight term that found no room in the open batch (here: va and vb hold 8 of the
    # kEwPre = 10 preloaded components, v3 needs 3 more) launches the batch and is staged again. It
    # was staged into the slot it held before the launch, ops[nops_before], while the new batch
    # recorded ops[0]: the launched statement's stale term, its columns renumbered to the new
    # batch's slots, ran in its place (wsmc_sample and weigh in csrc/wsmc_api.hip). Seen only on
    # compiled and interpreted batches of two or more statements: a batch of one replays the call.
    "restaged_statement": [
        pf.Stmt("sample", out="x0", dim=1, dist=_normal(_o(0.2))),
        pf.Stmt("sample", out="va", dim=4, dist=_iso(4)),
        pf.Stmt("sample", out="vb", dim=4, dist=_iso(4)),
        pf.Stmt("sample", out="v3", dim=3, dist=_iso(3)),
        pf.Stmt("assign_expr", out="f", dim=1, trees=((abi.X_ADD, ("col", "x0", 0), ("c", 1.0)),)),   # launches
        pf.Stmt("observe", dist=_normal(_o(0.0, ("va", 3, 1.0), ("vb", 3, 1.0))), x=(_o(0.3),)),
        pf.Stmt("observe", dist=_normal(_o(0.0, ("v3", 0, 1.0))), x=(_o(-0.4),)),                     # restaged
        pf.Stmt("sample", out="y", dim=1, dist=_normal(_o(0.0, ("v3", 1, 1.0), ("x0", 0, 0.5)))),
    ],
    # A Sample whose distribution reads no column leaves its output unstored while the lazy store
    # is on (the values stay in the batch's rows, a VirtCol entry is written when read). The
    # reader looked for the entry before the batch was launched on its behalf (here: the seventh
    # statement of a full batch), found none, and then read the never-written buffer from memory.
    "unstored_output_read_after_launch": [
        pf.Stmt("sample", out="x0", dim=1, dist=_normal(_o(0.2), 1.5)),
    ] + [pf.Stmt("sample", out=f"p{j}", dim=1, dist=_normal(_o(0.1 * j))) for j in range(5)] + [
        pf.Stmt("observe", dist=_normal(_o(0.0, ("x0", 0, 1.0))), x=(_o(0.3),)),                     # the 7th
        pf.Stmt("sample", out="q", dim=1, dist=_normal(_o(0.25))),
        pf.Stmt("assign", out="t", dim=1, exprs=(_o(1.0, ("x0", 0, 0.5)),)),
        pf.Stmt("resample", ess=1.0, scheme=abi.RESAMPLE_STRATIFIED, wait=False),
        pf.Stmt("sample", out="q2", dim=1, dist=_normal(_o(-0.3))),
    ] + [pf.Stmt("assign", out=f"u{j}", dim=1, exprs=(_o(0.5, ("p0", 0, 1.0)),)) for j in range(4)] + [
        # p0 is read through the ancestors by the open batch: its Sample launches the batch, and reads q2
        pf.Stmt("sample", out="p0", dim=1, dist=_normal(_o(0.0, ("q2", 0, 1.0)))),
        pf.Stmt("sample", out="q3", dim=1, dist=_normal(_o(0.7))),
    ] + [pf.Stmt("assign", out=f"w{j}", dim=1, exprs=(_o(0.5, ("p1", 0, 1.0)),)) for j in range(4)] + [
        pf.Stmt("assign", out="w4", dim=1, exprs=(_o(0.0, ("q3", 0, 2.0)),)),    # the 7th, an Assign, reads q3
    ],
    # Compiling this batch (an Exponential Observe with a column scale, then a LogNormal Weight with
    # column parameters: statements 21-22 of `mixed` seed 0) for two particles a thread took the
    # run-time compiler down in its post-RA scheduler, and the process with it: a batch's kernels for
    # one and for two particles a thread are one translation unit, so this happens at every N, before
    # anything is launched. Batches with a WSMC_FEAT_EXT family compile one particle a thread now
    # (csrc/wsmc_jit.hip ew_single); without that this case ends the test process.
    "ext_pair_compile": [
        pf.Stmt("col_upload", out="b", kind="bit", dim=1, vseed=11),
        pf.Stmt("col_upload", out="s", kind="pos", dim=1, vseed=12),
        pf.Stmt("observe", dist=pf.DistSpec(abi.FAM_EXPONENTIAL, 1, (_o(0.0),), _o(1.054, ("b", 0, 0.5), ("b", 0, 0.5))),
                x=(_o(3.322),)),
        pf.Stmt("weight", dist=pf.DistSpec(abi.FAM_LOGNORMAL, 1, (_o(0.654, ("b", 0, 0.5)),), _o(0.231)),
                x=(_o(0.25, ("s", 0, 0.5)),)),
        pf.Stmt("resample", ess=0.5, scheme=abi.RESAMPLE_STRATIFIED, wait=False),
        pf.Stmt("sample", out="y", dim=1, dist=pf.DistSpec(abi.FAM_LAPLACE, 1, (_o(0.0, ("s", 0, 1.0)),), _o(0.7))),
        pf.Stmt("observe", dist=_normal(_o(0.0, ("y", 0, 1.0))), x=(_o(0.1),)),
    ],
}


@pytest.mark.parametrize("n", [65, 1001, 5002])
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_program_matches_the_oracle(gpu_available, name, lazy, n):
    g, o = wsmc.Context(n, seed=91), Oracle(n, seed=91)
    try:
        g.store_set_lazy(lazy)
        pf.differential(g, o, DIRECTED[name], "quiet", f"directed {name} lazy={lazy} N={n}")
    finally:
        g.close()
        o.close()

"""The random-program corpus on the CPU oracle (tests/progfuzz.py): what the seed lists of
tests/test_gpu_random_programs.py cover, so that the GPU test cannot quietly go vacuous; the
generator's determinism; exact sharding against the single population; and the comparer's teeth."""
import math

import numpy as np
import pytest

import progfuzz as pf
from oracle import Oracle
from wsmc import abi

N = 1001


def corpus():
    return ([("mixed", s) for s in pf.MIXED_SEEDS] + [("moves", s) for s in pf.MOVES_SEEDS] +
            [("caps", s) for s in pf.CAPS_SEEDS] + [("edge", s) for s in pf.EDGE_SEEDS])


@pytest.fixture(scope="module")
def oracle_runs():
    """every corpus program run once on the oracle: (profile, seed) -> (program, outcomes, final state)"""
    out = {}
    for profile, seed in corpus():
        prog = pf.gen(seed, profile)
        o = Oracle(N, seed=pf.ctx_seed(seed, profile))
        flags = []   # SMCState.resampled after each statement: whether a gated block ran
        res = pf.run(o, prog, "chatty", on_step=lambda i, s, r: flags.append(o.get_state()["resampled"]))
        res = [r + (f,) for r, f in zip(res, flags)]
        out[profile, seed] = (prog, res, o.log_evidence(), o.weights_download())
        o.close()
    return out


def test_programs_stay_short(oracle_runs):
    for (profile, seed), (prog, _, _, _) in oracle_runs.items():
        n = sum(1 for s in prog if s.op != "read")
        assert n <= pf.MAX_STATEMENTS, (profile, seed, n)


def test_corpus_covers_the_vocabulary(oracle_runs):
    cov = None
    for prog, _, _, _ in oracle_runs.values():
        cov = pf.static_coverage(prog, cov)
    fams = set(pf.FAMILIES)
    assert len(fams) == 23
    missing = fams - cov["sample"]
    assert not missing, f"families never drawn by a Sample: {[pf.FAMILIES[f] for f in sorted(missing)]}"
    missing = (fams - set(pf.VECTOR_FAMILIES)) - cov["weigh"]
    assert not missing, f"scalar families never scored by an Observe / Weight: {[pf.FAMILIES[f] for f in sorted(missing)]}"
    for fam, dims in ((abi.FAM_MVNORMAL_ISO, (2, 3, 4)), (abi.FAM_MVNORMAL, (2, 3))):
        for d in dims:
            assert (fam, d) in cov["dims"], f"{pf.FAMILIES[fam]} never drawn at dim {d}"
    missing = set(pf.XOPS_ALL) - cov["xops"]
    assert not missing, f"WSMC_X_* opcodes in no expression: {sorted(missing)}"
    assert cov["forms"] == set(pf.OPERAND_FORMS), f"operand forms: {cov['forms']}"
    assert cov["schemes"] == set(pf.SCHEMES), f"resampling schemes: {cov['schemes']}"
    want = {"move", "move_gated", "move_block", "bounded", "unbounded", "d1", "d2", "d3", "d4", "RW", "autoRW"}
    assert want <= cov["moves"], f"Move forms missing: {want - cov['moves']}"
    assert cov["reads"] == set(pf.READ_KINDS), f"read kinds missing: {set(pf.READ_KINDS) - cov['reads']}"


def test_corpus_outcomes(oracle_runs):
    """the Resamples go both ways, the Moves move, and no `mixed` program degenerates"""
    flags, accepted, notpd, moves = [], 0, 0, 0
    for (profile, seed), (prog, res, ev, w) in oracle_runs.items():
        for i, (s, r) in enumerate(zip(prog, res)):
            if s.op == "resample":
                assert r[0] == "ok", (profile, seed, s, r)
                flags.append(r[1][0])
            elif s.op in ("move", "move_block"):
                if (s.op == "move" and not math.isnan(s.diversity)) or (s.op == "move_block" and s.gated and
                                                                        not res[i - 1][2]):
                    continue   # behind a gate that may have kept it from running
                moves += 1
                if r[0] == "err":
                    assert r[1] == abi.WSMC_ENOTPD, (profile, seed, s, r)
                    notpd += 1
                else:
                    accepted += (max(r[1]) if isinstance(r[1], list) else r[1]) > 0
            elif s.op not in ("sample_particles", "move_gated"):
                assert r[0] == "ok", f"unexpected error {r} in {profile} seed {seed} at {s!r}"
        if profile == "mixed":
            assert not math.isnan(ev), f"mixed seed {seed} ends with NaN evidence"
            assert not np.all(np.isneginf(w)), f"mixed seed {seed} ends with every weight -inf"
    frac = sum(flags) / len(flags)
    assert len(flags) >= 60 and 0.2 <= frac <= 0.8, f"{sum(flags)} of {len(flags)} Resamples resampled"
    assert moves >= 60, moves
    assert accepted >= 0.9 * moves, f"{accepted} of {moves} Moves accepted a particle"
    assert notpd <= 0.05 * moves, f"{notpd} of {moves} Moves were not positive definite"


def test_the_degenerate_case_is_directed(oracle_runs):
    prog, res, ev, w = oracle_runs["edge", 0]
    errs = [(s.op, r[1]) for s, r in zip(prog, res) if r[0] == "err"]
    assert errs == [("sample_particles", abi.WSMC_ESTATE)], errs
    assert math.isnan(ev) or np.isnan(w).any()


def _batches(name):
    prog = pf.gen(pf.CAPS_NAMES.index(name), "caps")
    return pf.batch_model(prog)


@pytest.mark.parametrize("name", pf.CAPS_NAMES)
def test_caps_programs_reach_their_cap(name):
    """each directed program reaches the cap it is named for and goes one past it, by
    progfuzz.batch_model's restatement of csrc/wsmc_api.hip's batching rules"""
    batches, events = _batches(name)
    ev = {e for e, _ in events}
    if name == "kEwOps":      # 5 and 6 statements launched by the next stretch, the 7th by "full" (kEwOps = 6)
        assert [b["nops"] for b in batches if b["why"] == "assign_expr"][1:4:1][:2] == [5, 6], batches
        full = [b for b in batches if b["why"] == "full"]
        assert len(full) == 1 and full[0]["nops"] == pf.K_OPS, batches
        assert batches[batches.index(full[0]) + 1]["nops"] >= 1
    elif name == "kEwSlots":
        # the statements read 15, 16 and 17 distinct columns, but every slot needs an LDS row of its
        # own (ew_remap :269-271), so a batch holds at most kEwRows = 12 < kEwSlots = 16 columns:
        # the row (or preload) cap launches the batch first and `nslots == kEwSlots` (:268) never binds
        reads = []
        prog = pf.gen(pf.CAPS_NAMES.index(name), "caps")
        cur = set()
        for s in prog:
            if s.op == "assign_expr":
                reads.append(len(cur))
                cur = set()
            elif s.op == "observe" and len(s.dist.cols()) > 1:
                cur |= set(s.dist.cols()) | {n for o in s.x for n in o.cols()}
        reads.append(len(cur))
        assert sorted(reads)[-3:] == [15, 16, 17], reads
        assert max(b["nslots"] for b in batches) == pf.K_PRE, batches
        assert "slots_full" not in ev and "pre_full" in ev
        assert sum(1 for b in batches if b["why"] == "stage") >= 3
    elif name == "kEwRows":   # 11 and 12 rows held; the 13th (an output) goes unstaged and its reader launches
        rows = sorted(b["nrows"] for b in batches if b["npre"] == pf.K_PRE)
        assert rows == [11, 12, 12], batches
        assert "unstaged_output" in ev and "reads_unstaged" in ev
        assert any(b["why"] == "stage" and b["nrows"] == pf.K_ROWS for b in batches)
    elif name == "kEwPre":    # 9 and 10 preloaded components; the 11th fails for a weight term and for an Assign
        pre = [b["npre"] for b in batches if b["why"] in ("assign_expr", "stage")]
        assert {9, 10} <= set(pre), batches
        assert any(b["why"] == "stage" and b["npre"] == 8 for b in batches), batches   # va + vb held, v3 refused
        assert "pre_full" in ev and "unstaged_read" in ev
    elif name == "ntab4":
        b = [b for b in batches if b["why"] == "ntab"]
        assert len(b) == 1 and b[0]["ntab"] == 4 and b[0]["nops"] == 4, batches
    elif name == "lagged_write":
        assert [b["why"] for b in batches].count("lagged_write") == 2, batches
    elif name == "anc_row":
        # a second lagged read joins a batch that holds an ancestor row (the no-op Resample between
        # them leaves the batch open). The launch condition itself (`b->anc != ind.row`, wsmc_assign :2174) needs
        # a second row, and every call that logs one (wsmc_resample past :2562, wsmc_store_resample)
        # launches the batch first: no program reaches it
        assert "second_lagged_read_same_row" in ev, events
        assert not any(b["why"] == "anc_row" for b in batches)
        assert sum(1 for b in batches if b["anc"] is not None) >= 2
    elif name == "seventh_lagged":
        full = [b for b in batches if b["why"] == "full"]
        assert len(full) == 1 and full[0]["anc"] is not None and full[0]["nrows"] == pf.K_ROWS, batches
        last = batches[batches.index(full[0]) + 1]
        assert last["ntab"] == 1 and last["anc"] is not None and last["why"] == "resample", batches


def test_every_cap_and_flush_condition_is_named():
    assert {"kEwOps", "kEwSlots", "kEwRows", "kEwPre"} <= set(pf.CAPS_NAMES)       # csrc/wsmc_ew.h:68-71
    assert {"kEwOps", "anc_row", "ntab4", "lagged_write"} <= set(pf.CAPS_NAMES)    # wsmc_api.hip wsmc_assign :2173-2176
    assert [pf.caps_name(s) for s in pf.CAPS_SEEDS] == pf.CAPS_NAMES


def test_generation_is_deterministic():
    for profile, seed in corpus():
        a, b = pf.gen(seed, profile), pf.gen(seed, profile)
        assert a == b and [repr(s) for s in a] == [repr(s) for s in b], (profile, seed)
    assert pf.gen(1, "mixed") != pf.gen(2, "mixed")


def _snapshot(o):
    return ([o.col_download(c) for c in range(len(o.col_names()))], o.weights_download(), o.get_state(),
            o.log_evidence())


def test_oracle_runs_are_deterministic():
    for profile, seed in [("mixed", 0), ("mixed", 5), ("moves", 1), ("caps", 3)]:
        prog = pf.gen(seed, profile)
        snaps = []
        for _ in range(2):
            o = Oracle(N, seed=pf.ctx_seed(seed, profile))
            res = pf.run(o, prog, "chatty")
            snaps.append((_snapshot(o), [r for r in res]))
        assert pf.same_value(snaps[0][0], snaps[1][0]), (profile, seed)
        for a, b in zip(snaps[0][1], snaps[1][1]):
            assert a[0] == b[0] and pf.same_value(a[1], b[1]), (profile, seed)


def test_exact_sharding_equals_one_population():
    """README: exact mode "covers the statement operators": up to its first Move (sharded autoRW
    moments sum per shard) every corpus program gives the single population's bits on
    two exact shards, after every statement"""
    checked = 0
    for profile, seed in corpus():
        prog = pf.gen(seed, profile)
        cut = next((i for i, s in enumerate(prog) if s.op.startswith("move")), len(prog))
        prog = pf.for_shards(prog[:cut], exact=True)
        cs = pf.ctx_seed(seed, profile)
        pf.differential(Oracle(N, seed=cs, shards=2, exact=True), Oracle(N, seed=cs), prog, "chatty",
                        f"exact shards vs one population: {profile} seed {seed}")
        checked += len(prog)
    assert checked > 400


@pytest.mark.parametrize("what", ["column", "weight", "op_counter"])
def test_the_comparer_has_teeth(what):
    """one particle of one column moved by one ulp (or one weight, or the op counter by one) after
    one chosen statement: `differential` reports exactly that statement"""
    prog = pf.gen(2, "mixed")
    at = 9
    assert prog[at].op != "read"

    def fault(i, g):
        if i != at:
            return
        if what == "column":
            c = g.col_find("x0")
            v = g.col_download(c)
            v[N // 3] = np.nextafter(v[N // 3], np.inf)
            g.col_upload(c, v)
        elif what == "weight":
            w = g.weights_download()
            w[N - 1] = np.nextafter(w[N - 1], -np.inf)
            g.weights_upload(w)
        else:
            g.set_op_counter(g.get_state()["op_counter"] + 1)

    cs = pf.ctx_seed(2, "mixed")
    pf.differential(Oracle(N, seed=cs), Oracle(N, seed=cs), prog, "chatty", "no fault")
    with pytest.raises(pf.Mismatch) as e:
        pf.differential(Oracle(N, seed=cs), Oracle(N, seed=cs), prog, "chatty",
                        pf.info(2, "mixed", "chatty", N), hook=fault)
    assert e.value.index == at, str(e.value)
    msg = str(e.value)
    assert f"statement {at}: {prog[at]!r}" in msg and "--seed 2 --profile mixed --mode chatty --n 1001" in msg
    assert {"column": "column x0", "weight": "weights", "op_counter": "state.op_counter"}[what] in msg
    # the quiet mode sees it too, at the end
    with pytest.raises(pf.Mismatch) as e:
        pf.differential(Oracle(N, seed=cs), Oracle(N, seed=cs), prog[:at + 1], "quiet", "quiet", hook=fault)
    assert e.value.index == at + 1


def test_a_waited_call_that_returns_nothing_is_a_difference():
    """None stands for "not waited for" only where the device was told not to wait"""
    class Silent:
        def __init__(self, o):
            self._o = o

        def __getattr__(self, k):
            return getattr(self._o, k)

        def resample(self, ess, scheme=0, wait=True):
            self._o.resample(ess, scheme, wait=True)
            return None

    prog = pf.gen(2, "mixed")
    first = next(i for i, s in enumerate(prog) if s.op == "resample")
    cs = pf.ctx_seed(2, "mixed")
    with pytest.raises(pf.Mismatch) as e:
        pf.differential(Silent(Oracle(N, seed=cs)), Oracle(N, seed=cs), prog, "chatty", "silent")
    assert e.value.index == first, str(e.value)
    pf.differential(Silent(Oracle(N, seed=cs)), Oracle(N, seed=cs), prog, "quiet", "silent")   # told not to wait
    assert not pf.same_value(None, 1.0) and pf.same_value(None, None)

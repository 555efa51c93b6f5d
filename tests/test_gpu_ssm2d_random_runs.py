"""Seeded random fused 2D-SSM runs (wsmc_ssm2d_run) against the CPU oracle issuing the same model
statement by statement, bit for bit (tests/ssm2dfuzz.py; what the corpus covers is asserted on the
CPU by tests/test_ssm2d_random_runs.py, which also holds the oracle's answer to a second CPU
statement and to arithmetic that shares no header with either).

Every `mixed` seed runs synchronously (the evidence returned, everything compared after every run)
and asynchronously (nothing read until the last run); eight of them as two island shards and as
two exact shards on the one device; every directed case synchronously, the sequences on one
context (grow_T, shorter_run_after_longer, param_switch, async_mix) also asynchronously. The route
of every run (fused, or issued as statements by the library because the context holds a column
that is not the run's: Case.routes) is asserted by ssm2dfuzz.differential.

The counters. On one unsharded context whose runs take the Resample statistics in the propagate
(run_stats()["qstat_mode"] != 0), a synchronous fused run's growth of `missed_steps` and `replays`
is held to ssm2dfuzz.predict_misses, which restates the guess from the oracle's weights alone. The
relation the code implies is not equality (ssm2dfuzz.counter_bounds has the derivation from
k_rs_fill_fused, wsmc_ssm2d_run and fold_run): a miss is counted per step of the guessed run, and
that run is the oracle's only up to its first miss, after which its statistics are taken against a
reference point above the canonical one until the whole run is re-done on the exact path. With
every step determined: no predicted miss <=> both counters stay; a first predicted miss at step k
<=> 1 <= missed <= T - k + 1 (equality with the prediction when k = T) and replays grows by
exactly one. Measured on an MI355X: in every one of this file's 94 synchronous fused runs (46 of
them with a predicted miss, up to 9 in a run) the count equalled the prediction's; the steps after
a first miss are nonetheless not held to it.

Seconds a test on an MI355X (device and oracle sides together): qstat_edge_2999999 2.4,
qstat_edge_3000000 2.3 (T = 3: their oracle side takes 1.5 s); mixed-14 (262145 particles, three
runs) 0.98 synchronous and 0.46 asynchronous, mixed-29 (262145) 0.37 and 0.17, mixed-2 0.65; every
other test under 0.35; the file 11.4 s."""
import pytest

import ssm2dfuzz as sf

pytestmark = pytest.mark.gpu

# two shards need two particles; sizes 2 .. 70001, both store modes, one to three runs
SHARDED_SEEDS = (1, 2, 4, 7, 9, 11, 12, 13)


@pytest.fixture(scope="module")
def cases(gpu_available):
    return {c.name: c for c in sf.corpus()}


def check_counters(case, stats):
    """every synchronous run's counters against the prediction (the module docstring's relation)"""
    out = []
    for k, (run, st, pred, route) in enumerate(zip(case.runs, stats, sf.predict_misses(case), case.routes())):
        if not st["qstat_mode"] or route != "fused":
            continue        # (a run issued as statements: the batches' own guesses, recomputed in place, no replay)
        (lo, hi), (rlo, rhi) = sf.counter_bounds(run, pred)
        print(f"{case.name} run {k}: T={run.T} predicted misses {pred['miss']} undetermined {pred['undetermined']}: "
              f"missed_steps +{st['missed']} replays +{st['replays']}")
        assert lo <= st["missed"] <= hi, (case.name, k, pred, st)
        assert rlo <= st["replays"] <= rhi, (case.name, k, pred, st)
        assert (st["missed"] > 0) == (st["replays"] == 1), (case.name, k, st)
        out.append((len(pred["miss"]), st["missed"]))
    return out


@pytest.mark.parametrize("seed", sf.MIXED_SEEDS)
def test_mixed_sync(cases, seed):
    c = cases[f"mixed-{seed}"]
    check_counters(c, sf.differential(c, "hip", "sync"))


@pytest.mark.parametrize("seed", sf.MIXED_SEEDS)
def test_mixed_async(cases, seed):
    sf.differential(cases[f"mixed-{seed}"], "hip", "async")


@pytest.mark.parametrize("drive", ["island2", "exact2"])
@pytest.mark.parametrize("seed", SHARDED_SEEDS)
def test_mixed_two_shards(cases, seed, drive):
    sf.differential(cases[f"mixed-{seed}"], "hip", drive)


@pytest.mark.parametrize("name", sf.DIRECTED)
def test_directed_sync(cases, name):
    c = cases[name]
    stats = sf.differential(c, "hip", "sync")
    check_counters(c, stats)
    if name in ("param_switch", "grow_T"):
        assert len(stats) == len(c.runs)  # (compared after every run: differential's sync drive)
    if name.startswith("qstat_edge"):
        assert [st["qstat_mode"] for st in stats] == [2 if c.N >= 3_000_000 else 1]


@pytest.mark.parametrize("name", sf.SEQUENCES)
def test_sequences_async(cases, name):
    sf.differential(cases[name], "hip", "async")

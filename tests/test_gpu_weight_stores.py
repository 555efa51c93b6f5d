"""The fused 2D-SSM run's lazy weight rows: bit for bit the statement
oracle, and the rows stored and recomputed as the oracle's resample flags say.

A one-GPU run in statistics mode 1 stores step t's weights (t >= 2, k_ssm2d_prop QS) only when
something will read them: the next propagate after a step that did not resample, and the
trace-back at t = T. A step after a "not" step whose own predecessor resampled finds no stored row
and recomputes it from the x it loads anyway. The propagate launches count, on the device, what
they stored and recomputed (Context.weight_stores); the expected counts are derived here from the
oracle's flags alone:

    a launch at step t in 2..T stores      iff t == T or step t-1 did not resample
    a launch at step t in 3..T recomputes  iff step t-1 did not resample and step t-2 did

Step 1 never resamples on this model (every particle starts at the same state, so its weights are
equal and ESS = N), so a forced run stores at t = 2 and t = T and a run that never resamples at
every t in 2..T.

Shapes: N = 1001 (a ragged last pair), 2050 (a ragged third tile), 4096 (whole tiles); T = 12;
history kept and not. The pinned mixed case (seed 2, ess_perc_min 0.3, models.ssm2d_data(12, seed=2))
has the flags N N N R N R R R N R N R at every N: all four transitions, R R N at steps 7-9 (step 10
recomputes, as do steps 6 and 12), and step 12 resamples; its first 11 observations end on a step
that does not. It was picked on the CPU oracle among the sequences on which no step's guessed
reference point misses (a carried bound often straddles an integer): a miss re-does the run on the
exact path, which stores every row, and the comparison would then say nothing about the lazy rows.
The tests assert that no replay happened wherever the decisions depend on the statistics; a run
that never resamples (ess_perc_min 0) always misses somewhere, its replay is what is compared, and
its counts are those of the guessed pass (whose decisions cannot differ: ESS < 0 never holds).
"""
import functools
import math

import numpy as np
import pytest

import wsmc
from wsmc import abi, models
from oracle import Oracle
from test_gpu_parity import assert_same_state

pytestmark = pytest.mark.gpu

T = 12
NS = [1001, 2050, 4096]
MIX_SEED, MIX_ESS, MIX_DATA = 2, 0.3, 2
DATA = 42   # models.ssm2d_data's own seed


@functools.lru_cache(maxsize=None)
def oracle_run(N, seed, ess, steps, scheme=abi.RESAMPLE_STRATIFIED, shards=1, data=DATA):
    """the statement oracle after one run over the first `steps` observations, and its flags
    (computed once a case; the tests only read it)"""
    o = Oracle(N, seed=seed, shards=shards) if shards > 1 else Oracle(N, seed=seed)
    flags = models.ssm2d_statements(o, models.ssm2d_data(T, seed=data)[:steps], ess_perc_min=ess, scheme=scheme)
    return o, tuple(bool(f) for f in flags)


def expected_counts(flags):
    """(stored, recomputed) over the launches of steps 2..T under the lazy rule; flags[t-1] is step t"""
    n = len(flags)
    f = (None,) + tuple(flags)
    stored = sum(1 for t in range(2, n + 1) if t == n or not f[t - 1])
    recomputed = sum(1 for t in range(3, n + 1) if not f[t - 1] and f[t - 2])
    return stored, recomputed


def assert_same(g, o, keep, steps):
    """weights, every column (history included when kept), the last ancestors, the evidence, the
    state flags"""
    if keep:
        assert_same_state(g, o)
    else:
        np.testing.assert_array_equal(g.col_download(g.col_find("x")), o.col_download(o.col_find("x_%d" % (steps + 1))))
        for n in ("v", "dv"):
            np.testing.assert_array_equal(g.col_download(g.col_find(n)), o.col_download(o.col_find(n)), err_msg=n)
        np.testing.assert_array_equal(g.weights_download(), o.weights_download())
        sg, so = g.get_state(), o.get_state()
        for k in ("resampled", "n_resamples", "op_counter"):
            assert sg[k] == so[k], k
    np.testing.assert_array_equal(g.last_ancestors(), o.last_ancestors())
    eg, eo = g.log_evidence(), o.log_evidence()
    assert eg == eo or (math.isnan(eg) and math.isnan(eo))


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


def run_and_check(N, seed, ess, steps, keep, data=DATA, replay_free=True):
    o, flags = oracle_run(N, seed, ess, steps, data=data)
    g = wsmc.Context(N, seed=seed)
    rs0, ws0 = g.run_stats(), g.weight_stores()
    ev = g.ssm2d_run(models.ssm2d_data(T, seed=data)[:steps], ess_perc_min=ess, keep_history=keep)
    rs1, ws = g.run_stats(), delta(g.weight_stores(), ws0)
    assert ev == o.log_evidence()
    assert_same(g, o, keep, steps)
    assert rs1["qstat_mode"] == 1
    replays = rs1["replays"] - rs0["replays"]
    if replay_free:   # what was compared is the lazy pass itself, not a replay on the exact path
        assert replays == 0
    stored, recomputed = expected_counts(flags)
    print(f"N={N} ess={ess} T={steps} flags={''.join('RN'[not f] for f in flags)} counts={ws} "
          f"expected stored={stored} recomputed={recomputed} replays={replays}")
    # (a replay is `steps` launches without the statistics)
    assert ws == {"stored": stored, "recomputed": recomputed, "qs_launches": steps - 1,
                  "plain_launches": 1 + replays * steps}
    g.close()
    return flags


def assert_pinned_pattern(N):
    """the pattern conditions on the oracle's flags alone (no device): all four transitions, a
    "not" step after two resampling steps with a step after it (the recompute), step T once on a
    resampling step (T = 12) and once on one that is not (the first 11 observations)"""
    _, f = oracle_run(N, MIX_SEED, MIX_ESS, T, data=MIX_DATA)
    assert {(a, b) for a, b in zip(f, f[1:])} == {(True, True), (True, False), (False, False), (False, True)}
    assert any(f[k - 2] and f[k - 1] and not f[k] for k in range(2, T - 1))   # R R N, then a step
    assert expected_counts(f)[1] >= 1
    assert f[T - 1] is True
    _, f11 = oracle_run(N, MIX_SEED, MIX_ESS, T - 1, data=MIX_DATA)
    assert f11 == f[:T - 1] and f11[-1] is False
    assert expected_counts(f11)[1] >= 1


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("steps", [T, T - 1], ids=["ends_resampled", "ends_not"])
@pytest.mark.parametrize("N", NS)
def test_mixed_sequence(gpu_available, N, steps, keep):
    assert_pinned_pattern(N)           # first: the run below cannot pass by never recomputing
    flags = run_and_check(N, MIX_SEED, MIX_ESS, steps, keep, data=MIX_DATA)
    assert flags[-1] is (steps == T)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("N", NS)
def test_never_resamples(gpu_available, N, keep):
    """ess_perc_min 0: every step from 3 on reads the row its predecessor stored"""
    flags = run_and_check(N, 7, 0.0, T, keep, replay_free=False)
    assert not any(flags)
    assert expected_counts(flags) == (T - 1, 0)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("N", NS)
def test_always_resamples(gpu_available, N, keep):
    """ess_perc_min 1: step 1 cannot resample (equal weights), every later step does; the rows of
    steps 3..T-1 are never stored"""
    flags = run_and_check(N, 7, 1.0, T, keep)
    assert flags == (False,) + (True,) * (T - 1)
    assert expected_counts(flags) == (2, 0)


@pytest.mark.parametrize("N", NS)
def test_outlier_replay_starts_from_a_lazy_runs_weights(gpu_available, N):
    """A lazy run leaves canonical weights; the next run's outlier observation misses the guess,
    and its replay starts from them."""
    obs = models.ssm2d_data(T)
    bad = obs.copy()
    bad[5] += (40.0, -25.0)
    g, o = wsmc.Context(N, seed=21), Oracle(N, seed=21)
    g.ssm2d_run(obs, ess_perc_min=0.5, keep_history=True)
    before = g.run_stats()
    ev = g.ssm2d_run(bad, ess_perc_min=0.5, keep_history=True)
    st = g.run_stats()
    for ob in (obs, bad):
        models.ssm2d_statements(o, ob, ess_perc_min=0.5)
    assert ev == o.log_evidence()
    assert_same(g, o, True, T)
    assert st["replays"] - before["replays"] == 1
    g.close()


@pytest.mark.parametrize("ess", [1.0, MIX_ESS])
@pytest.mark.parametrize("N", NS)
def test_back_to_back_asynchronous_runs(gpu_available, N, ess):
    """the second run's step 1 reads (and saves) the canonical weights the first one left"""
    obs = models.ssm2d_data(T)
    g, o = wsmc.Context(N, seed=MIX_SEED), Oracle(N, seed=MIX_SEED)
    for _ in range(2):
        assert g.ssm2d_run(obs, ess_perc_min=ess, keep_history=True, want_evidence=False) is None
    sg = g.get_state()
    wg = g.weights_download()
    for _ in range(2):
        models.ssm2d_statements(o, obs, ess_perc_min=ess)
    so = o.get_state()
    for k in ("resampled", "weights_changed", "n_resamples", "op_counter"):
        assert sg[k] == so[k], k
    np.testing.assert_array_equal(wg, o.weights_download())
    assert_same(g, o, True, T)
    g.close()


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("ess", [1.0, MIX_ESS])
@pytest.mark.parametrize("N", NS)
def test_island_shards_store_every_row(gpu_available, N, ess, keep):
    """two island shards on one device: k_rs_qfix reads the weights on a miss, so every step
    stores them (the counts are the first shard's)"""
    o, _ = oracle_run(N, MIX_SEED, ess, T, shards=2)
    g = wsmc.Context.multi(N, 2, seed=MIX_SEED, devices=[0, 0], transport=abi.TRANSPORT_HOST)
    ws0 = g.weight_stores()
    ev = g.ssm2d_run(models.ssm2d_data(T), ess_perc_min=ess, keep_history=keep)
    ws = delta(g.weight_stores(), ws0)
    assert ev == o.log_evidence()
    assert_same(g, o, keep, T)
    assert ws == {"stored": T - 1, "recomputed": 0, "qs_launches": T - 1, "plain_launches": 1}
    g.close()


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("ess", [1.0, MIX_ESS])
@pytest.mark.parametrize("N", NS)
def test_multinomial_stores_every_row(gpu_available, N, ess, keep):
    """the multinomial scheme's own statistics kernel reads the weights: no lazy launch at all"""
    o, _ = oracle_run(N, MIX_SEED, ess, T, scheme=abi.RESAMPLE_MULTINOMIAL)
    g = wsmc.Context(N, seed=MIX_SEED)
    ws0 = g.weight_stores()
    ev = g.ssm2d_run(models.ssm2d_data(T), ess_perc_min=ess, scheme=abi.RESAMPLE_MULTINOMIAL, keep_history=keep)
    ws = delta(g.weight_stores(), ws0)
    assert ev == o.log_evidence()
    assert_same(g, o, keep, T)
    assert ws == {"stored": 0, "recomputed": 0, "qs_launches": 0, "plain_launches": T}
    g.close()

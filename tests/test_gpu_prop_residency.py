"""The fused 2D-SSM run after the propagate's scalar diet: bit for bit the
statement oracle on every path the change touches.

The one-GPU propagate that takes the Resample statistics (k_ssm2d_prop QS) no longer carries the
island decision path or the first-step / exact-shard operands, issues its ancestor pair, previous
decision and previous max slots ahead of the log table's barrier, and loads the ancestor pair of
a ragged last particle without a branch. Shapes: under one 1024-particle tile, whole tiles, and
an odd N with a ragged last pair and a partial tile; forced and gated resampling (ess 0.5 carries
weights and the max-slot bound through steps that do not resample); an outlier observation whose
guess misses (the replay: the plain propagate, k_rs_sums_t and the fill); the state read straight
after an asynchronous run; two island shards on one device (the templated decision path).
Every case runs at both residencies of that propagate: 4 blocks a CU (what a population up to one
round of blocks gets) and 3 (larger ones; 44 KB of unused dynamic LDS a block), forced at these
small sizes with WSMC_PROP_BLOCKS, which the library reads at every run.
"""
import math

import numpy as np
import pytest

import wsmc
from wsmc import abi, models
from oracle import Oracle

pytestmark = pytest.mark.gpu

T = 8


@pytest.fixture(autouse=True, params=[4, 3], ids=["blocks4", "blocks3"])
def prop_blocks(request, monkeypatch):
    monkeypatch.setenv("WSMC_PROP_BLOCKS", str(request.param))
    return request.param


def assert_same(g, o):
    """every column, the weights, the last ancestors, the evidence and the state"""
    assert g.col_names() == o.col_names()
    for name in g.col_names():
        np.testing.assert_array_equal(g.col_download(g.col_find(name)), o.col_download(o.col_find(name)),
                                      err_msg=f"column {name}")
    np.testing.assert_array_equal(g.weights_download(), o.weights_download())
    np.testing.assert_array_equal(g.last_ancestors(), o.last_ancestors())
    assert_same_state(g.get_state(), o.get_state())
    eg, eo = g.log_evidence(), o.log_evidence()
    assert eg == eo or (math.isnan(eg) and math.isnan(eo))


def assert_same_state(sg, so):
    for k in ("resampled", "weights_changed", "depth", "n_terms", "op_counter", "n_resamples"):
        assert sg[k] == so[k], k
    assert sg["last_ess_perc"] == so["last_ess_perc"] or (math.isnan(sg["last_ess_perc"])
                                                          and math.isnan(so["last_ess_perc"]))


@pytest.mark.parametrize("N", [1023, 4096, 5001])
@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_fused_run_matches_statements(gpu_available, N, ess):
    obs = models.ssm2d_data(T)
    g, o = wsmc.Context(N, seed=19), Oracle(N, seed=19)
    before = g.run_stats()
    ev = g.ssm2d_run(obs, ess_perc_min=ess, keep_history=True)
    st = g.run_stats()
    flags = models.ssm2d_statements(o, obs, ess_perc_min=ess)
    assert ev == o.log_evidence()
    assert_same(g, o)
    assert g.get_state()["n_resamples"] == sum(flags)
    if ess == 0.5:
        assert not all(flags[1:])      # some steps carry their weights into the next bound
    # forced resampling on the model's own data: the guesses hold (the bound is the log-mean plus
    # the density's maximum, tight), so what is compared is the QS propagate's own result and not a
    # replay's. A carried bound (ess 0.5) is looser and may legitimately straddle an integer.
    if st["qstat_mode"] and ess == 1.0:
        assert st["replays"] == before["replays"]
    g.close()


def test_outlier_step_misses_the_guess_and_replays(gpu_available):
    N = 4096
    obs = models.ssm2d_data(T).copy()
    obs[4] += (40.0, -25.0)            # no particle near it: the step's max lies far below the bound
    g, o = wsmc.Context(N, seed=19), Oracle(N, seed=19)
    before = g.run_stats()
    ev = g.ssm2d_run(obs, ess_perc_min=1.0, keep_history=True)
    st = g.run_stats()
    models.ssm2d_statements(o, obs, ess_perc_min=1.0)
    assert ev == o.log_evidence()
    assert_same(g, o)
    if st["qstat_mode"]:
        assert st["missed_steps"] - before["missed_steps"] >= 1
        assert st["replays"] - before["replays"] == 1
    g.close()


@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_state_straight_after_an_asynchronous_run(gpu_available, ess):
    N = 4096
    obs = models.ssm2d_data(T)
    g, o = wsmc.Context(N, seed=23), Oracle(N, seed=23)
    assert g.ssm2d_run(obs, ess_perc_min=ess, keep_history=True, want_evidence=False) is None
    sg = g.get_state()                 # the first call after the enqueue: folds the run in
    models.ssm2d_statements(o, obs, ess_perc_min=ess)
    assert_same_state(sg, o.get_state())
    assert_same(g, o)
    g.close()


@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_two_island_shards_on_one_device(gpu_available, ess):
    """Island shards take the previous step's decision inside the propagate, from the
    all-gathered records: the ISL instantiation."""
    G, n = 2, 2048
    N = G * n
    obs = models.ssm2d_data(T)
    g = wsmc.Context.multi(N, G, seed=29, devices=[0] * G, transport=abi.TRANSPORT_HOST)
    ev = g.ssm2d_run(obs, ess_perc_min=ess, keep_history=True)
    o = Oracle(N, seed=29, shards=G)
    models.ssm2d_statements(o, obs, ess_perc_min=ess)
    assert ev == o.log_evidence()
    assert_same(g, o)
    g.close()

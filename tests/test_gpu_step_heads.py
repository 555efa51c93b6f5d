"""The fused 2D-SSM step kernels after their loads were taken out from under branches
(DESIGN.md §3): bit for bit the statement oracle at the sizes where a clamped load can go wrong.

The propagate (k_ssm2d_prop QS) gathers x and v through the ancestors, and reads the weight pair
of a step that follows no resample, from clamped indices under no branch: threads past N and a
ragged second particle read particle 0 and store nothing. The fill's tile blocks (k_rs_fill_fused)
load a thread's four q as two 16-B loads from a clamped quad, with the first group line and the
first tile partial of the group from clamped addresses. Sizes: the smallest population (one
particle: a ragged pair, every other lane clamped), 3 (a ragged pair in the second thread), 1025
(a second tile that holds one particle), 2047 and 3073 (a ragged last pair and quad at the end of
a tile and at the start of one). Forced resampling (ess 1.0) and gated (0.5: the steps that do not
resample carry the weights and the max-slot bound). An outlier observation at N = 1025 misses the
guess and replays on the exact path.

The fill's recomputed-q loads (load_tile_qw, populations from 3M particles) are reached by no
small test: tests/test_gpu_parity.py::test_ssm2d_fused_recomputed_q_matches_port covers them.
"""
import math

import numpy as np
import pytest

import wsmc
from wsmc import models
from oracle import Oracle

pytestmark = pytest.mark.gpu

T = 6
SIZES = [1, 3, 1025, 2047, 3073]


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


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("ess", [1.0, 0.5])
def test_fused_run_matches_statements(gpu_available, N, ess):
    obs = models.ssm2d_data(T)
    g, o = wsmc.Context(N, seed=31), Oracle(N, seed=31)
    ev = g.ssm2d_run(obs, ess_perc_min=ess, keep_history=True)
    flags = models.ssm2d_statements(o, obs, ess_perc_min=ess)
    assert ev == o.log_evidence() or (math.isnan(ev) and math.isnan(o.log_evidence()))
    assert_same(g, o)
    assert g.get_state()["n_resamples"] == sum(flags)
    g.close()


def test_outlier_step_misses_the_guess_and_replays(gpu_available):
    N = 1025
    obs = models.ssm2d_data(T).copy()
    obs[3] += (40.0, -25.0)            # no particle near it: the step's max lies far below the bound
    g, o = wsmc.Context(N, seed=31), Oracle(N, seed=31)
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

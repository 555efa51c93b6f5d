"""The calls that read the state, on the GPU, against the CPU oracle (tests/readedge.py's corpus):
wsmc_col_minmax, wsmc_weighted_median, wsmc_histogram, wsmc_weighted_moments, wsmc_ess,
wsmc_log_evidence, wsmc_marginal_diversity, wsmc_sample_particles and wsmc_col_gather_rows, bit for
bit through `view(np.uint64)`: a NaN matches any NaN, -0.0 is distinct from 0.0, an error must be
the same status on both sides, and the op counter must agree after every read, refused ones
included. After the list the device's state, weights and columns must be the oracle's, which must
be what it was before the list. tests/test_read_edges.py holds the oracle itself to the definitions.

One test is one (N, weight kind, state): one context and one oracle, every value entry uploaded in
turn into the same columns and the read list run under readedge.compare (from N = 524289 on one
test is one value entry, so that a test stays within a few seconds including the oracle's side).
The sharded leg is one handle over shards on the one device, island and exact, against the sharded
oracle: ragged splits, one-particle shards, the special value and all the live weight on rank 0 only
and on the last rank only; there weighted_moments is held to progfuzz._moments_close (the shards
sum in rank order; a component that is not finite must be the same NaN or infinity) and everything else stays bit for bit.

Every refusal the corpus triggers (a sample size of 0 or above N, weights that do not normalise) is
decided on the host in csrc/wsmc_api.hip before a kernel sees the arguments, and col_gather_rows
gets the indices sample_particles returned (and checks them against N on the host).

    python tests/readedge.py --values V --weights W --n N --state S --backend hip [--shards K --mode exact]

replays one cell and prints the first differing read with both bit patterns."""
import re

import pytest

import readedge as rd
import wsmc
from oracle import Oracle
from wsmc import abi

pytestmark = pytest.mark.gpu

HIP_FAILURE = re.compile(rf"(ok|err|status) {abi.WSMC_EHIP} !=|^after the reads: .*HIP")
PER_VALUE = 524289          # from here on a test is one value entry
CELLS = [(n, w, "fresh") for n in rd.SIZES if n < PER_VALUE for w in rd.weight_entries(n)] + \
        [(n, w, "lazy_stale") for n in rd.LAZY_SIZES for w in rd.weight_entries(n)]
BIG_CELLS = [(n, w, v) for n in rd.SIZES if n >= PER_VALUE for w in rd.weight_entries(n) for v in rd.value_entries(n, w)]


def run_cells(g, o, n, wname, state, vnames, sharded=False, shards=1, mode="island", lw=None):
    rd.prepare(g)
    rd.prepare(o)
    for vname in vnames:
        d = rd.differential(g, o, vname, wname, n, state, sharded=sharded, lw=lw)
        if d and HIP_FAILURE.search(d):   # the runtime reported a failure: nothing more on this device
            pytest.exit(f"{vname} x {wname} at N = {n} ({state}): {d}", returncode=3)
        assert d is None, f"{vname} x {wname} at N = {n} ({state}): {d}\n  replay: {rd.replay(vname, wname, n, state, shards, mode)}"


@pytest.mark.parametrize("n,wname,state", CELLS, ids=[f"{n}-{w}-{s}" for n, w, s in CELLS])
def test_reads_match_the_oracle(gpu_available, n, wname, state):
    g, o = wsmc.Context(n, seed=1), Oracle(n, seed=1)
    try:
        run_cells(g, o, n, wname, state, rd.value_entries(n, wname))
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("n,wname,vname", BIG_CELLS, ids=[f"{n}-{w}-{v}" for n, w, v in BIG_CELLS])
def test_reads_match_the_oracle_past_the_grid_caps(gpu_available, n, wname, vname):
    """N = 524289: k_hist strides; 1048577: K drops to 42; 2097153: k_rs_max strides"""
    g, o = wsmc.Context(n, seed=1), Oracle(n, seed=1)
    try:
        run_cells(g, o, n, wname, "fresh", [vname])
    finally:
        g.close()
        o.close()


# ---- shards ---------------------------------------------------------------------------------------------------
SPLITS = [(2049, 2), (4099, 3), (4, 3)]     # 1024 / 1025; ragged; one-particle shards
SHARD_VALUES = ["ordinary", "neg_zero", "zero_among", "two_values", "adjacent", "on_edges", "ties_by_weight", "offset",
                "all_equal", "all_equal_but_one@0", "all_equal_but_one@last", "one_nan@0", "one_nan@last",
                "pos_inf@0", "pos_inf@last", "neg_inf@0", "neg_inf@last", "both_inf@0", "both_inf@last"]
SHARD_WEIGHTS = ["flat", "gaussian", "half_dead", "one_live@0", "one_live@last", "live_on_rank0", "live_on_last_rank",
                 "all_neg_inf", "one_nan@0", "one_nan@last", "q_boundary", "median_tie"]
SHARD_CELLS = [(n, k, mode, w) for n, k in SPLITS for mode in ("island", "exact") for w in SHARD_WEIGHTS]


@pytest.mark.parametrize("n,k,mode,wname", SHARD_CELLS, ids=[f"{n}/{k}-{m}-{w}" for n, k, m, w in SHARD_CELLS])
def test_sharded_reads_match_the_sharded_oracle(gpu_available, n, k, mode, wname):
    exact = mode == "exact"
    lw = None
    if wname.startswith("live_on"):
        lw = rd.live_on_rank(n, k, 0 if wname == "live_on_rank0" else k - 1)
    vnames = rd.REFUSED_VALUES if wname.partition("@")[0] in rd.NO_ANSWER else SHARD_VALUES
    g = wsmc.Context.multi(n, k, seed=1, devices=[0] * k, transport=abi.TRANSPORT_HOST)
    o = Oracle(n, seed=1, shards=k, exact=exact)
    try:
        if exact:
            g.comm_set_shard_mode(abi.SHARD_EXACT)
        run_cells(g, o, n, "gaussian" if lw is not None else wname, "fresh", vnames, sharded=True, shards=k, mode=mode, lw=lw)
    finally:
        g.close()
        o.close()

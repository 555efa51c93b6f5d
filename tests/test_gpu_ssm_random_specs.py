"""Seeded random scalar-SSM specs through the fused run (wsmc_ssm_run) against the CPU oracle
issuing the same spec statement by statement, bit for bit (tests/ssmfuzz.py; what the corpus
covers and how its runs come out is asserted on the CPU by tests/test_ssm_random_specs.py).

N = 65 gives two particles a thread with one particle in the second wave's first thread, 1001 two
a thread over 8 waves, 2049 three a thread with five waves that own no particle, 1 a lone particle:
the smallest shapes that differ in kind. Every `mixed` seed runs at (1001, ess 0.5, stratified, the
default segment) and once more with the four axes rotated by the seed; every directed case at 65
and 2049, forced (1.0) and gated (0.5) resampling; `full` also at the four-column cap and one past
it (the statement route); prog97, a multinomial run, four seeds and the thresholds specs through
the library's statement route."""
import pytest

import ssmfuzz as sf
import wsmc
from wsmc import abi

pytestmark = pytest.mark.gpu

STRAT, SYST, MULT = abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL
STATEMENT_SEEDS = (3, 6, 14, 23)


def rotated(seed):
    """(N, ess, scheme, segment) of a seed's second run: over the 24 seeds every value of every axis
    is met eight times or more (tests/test_ssm_random_specs.py asserts at least four)"""
    return ((1, 65, 2049)[(seed // 2) % 3], (1.0, 0.5)[(seed // 3) % 2], (STRAT, SYST)[(seed + seed // 4) % 2],
            (1, 5, None)[(seed + seed // 3) % 3])


MIXED = [(s, 1001, 0.5, STRAT, None) for s in sf.MIXED_SEEDS] + [(s,) + rotated(s) for s in sf.MIXED_SEEDS]
DIRECTED = [(name, n, ess) for name in sf.DIRECTED if name != "pre_state" for n in (65, 2049) for ess in (1.0, 0.5)]


def _id(c):
    return "-".join("default" if v is None else str(v) for v in c)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sf.corpus()}


@pytest.fixture(scope="module")
def cap(gpu_available):
    g = wsmc.Context(1, seed=sf.SEED)
    c = g.ssm_stats()["cap"]
    g.close()
    assert c[1] >= c[2] >= c[3] >= c[4] >= 2049
    return c


@pytest.mark.parametrize("case", MIXED, ids=_id)
def test_mixed_seed(cap, cases, case):
    seed, n, ess, scheme, segment = case
    sf.differential(cases[f"mixed-{seed}"], n, ess, scheme, segment, "persistent")


@pytest.mark.parametrize("case", DIRECTED, ids=_id)
def test_directed(cap, cases, case):
    name, n, ess = case
    c = cases[name]
    flags, state = sf.differential(c, n, ess, STRAT, 5, c.route(n, STRAT, cap))
    if name == "prog96":
        assert c.route(n, STRAT, cap) == "persistent"
    if name == "prog97":
        assert c.route(n, STRAT, cap) == "statements"
    if name == "init_observe" and ess == 1.0:
        assert state["n_resamples"] == 2 + sum(flags) and all(flags)
    if name == "no_init":
        assert state["depth"] == 3 * sf.T and state["op_counter"] == 3 * sf.T


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("n", ["cap", "cap+1"])
def test_full_at_the_cap(cap, cases, n, ess):
    n = cap[4] + (n == "cap+1")
    sf.differential(cases["full"], n, ess, STRAT, None, "persistent" if n <= cap[4] else "statements")


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("n", [65, 2049])
def test_pre_state(gpu_available, n, ess):
    sf.run_pre_state(n, ess)


def test_statement_route_multinomial(cap, cases):
    sf.differential(cases["observe_first"], 65, 0.5, MULT, None, "statements")


@pytest.mark.parametrize("name", [f"mixed-{s}" for s in STATEMENT_SEEDS] + sf.THRESHOLDS)
def test_statement_route(cap, cases, name):
    """a foreign column on both sides: the library issues the statements itself"""
    sf.differential(cases[name], 65, 0.5, STRAT, None, "statements")

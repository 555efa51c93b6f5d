"""Seeded random fused 1D-LGSSM runs (wsmc_lgssm1d_run, kernel k_lgssm_segment) against the CPU oracle
issuing the same model statement by statement, bit for bit (tests/lgssmfuzz.py; what the corpus
covers is asserted on the CPU by tests/test_lgssm_random_runs.py, which also holds the oracle's
answer to arithmetic that shares no header with it).

Every `mixed` seed and every directed case runs twice on fresh contexts: once with the case's
segment lengths and once at the library's default, both against the oracle, so the bits are the
same whatever the launch boundaries. After every run the column, the weights, every state field,
the last ancestors, both evidences, the ESS trace (where asked for) and score(d) at depths 0, 1,
the run's middle, its end and -1 are compared: the last checks the tape the host writes while the
device runs. The route of every run (the persistent workgroup, or the statements issued by the
library: Case.routes) and its segment count are asserted from lgssm_stats() by
lgssmfuzz.differential. The non-finite cases are ordinary inputs that the argument check admits
and the oracle defines; nothing here expects a fault.

The independent check (tests/test_independent_math.py, case (f)) restates every step of seven
cases' first runs, and of `cap` at r = 0.3, q = 0.07, with numpy alone."""
import pytest

import lgssmfuzz as lf
from test_lgssm_random_runs import INDEPENDENT, independent_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cap(gpu_available):
    c = lf.device_cap()
    assert c >= 4097      # the corpus's sizes up to 4097 are meant for the persistent route
    return c


@pytest.fixture(scope="module")
def cases(gpu_available):
    return {c.name: c for c in lf.corpus()}


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "unsegmented"])
@pytest.mark.parametrize("seed", lf.MIXED_SEEDS)
def test_mixed(cases, cap, seed, segmented):
    c = cases[f"mixed-{seed}"]
    assert len(lf.differential(c, "hip", segmented, cap)) == len(c.runs)


@pytest.mark.parametrize("segmented", [True, False], ids=["segmented", "unsegmented"])
@pytest.mark.parametrize("name", lf.DIRECTED)
def test_directed(cases, cap, name, segmented):
    c = cases[name]
    assert len(lf.differential(c, "hip", segmented, cap)) == len(c.runs)


@pytest.mark.parametrize("name", INDEPENDENT + ["cap"])
def test_parameters_match_reference_math(cases, cap, name):
    from test_independent_math import run_lgssm_checked
    c = cases[name]
    args = independent_args(c, **(dict(r=0.3, q=0.07) if name == "cap" else {}))
    args["n"] = c.n(cap)
    n_rs, ties = run_lgssm_checked("hip", **args)
    print(f"{name}: {n_rs} steps resampled, {ties} ancestor ties")
    assert n_rs >= 1 and ties <= 2       # (a step's own allowance: test_resample_reference.check_against_reference)

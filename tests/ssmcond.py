"""Shared by tests/test_ssm_conditional.py and tests/test_gpu_ssm_conditional.py: the specs and
references the conditional runs are tested on, and particle Gibbs as a loop over the definitions
(SSM.statements / SSM.conditional_definition, then SSM.backward_definition) on the CPU oracle.
"""
import numpy as np

import ssmfuzz as sf   # noqa: F401  (puts the package and the oracle on sys.path)
import wsmc
from oracle import Oracle
from wsmc import Col, Normal, models
from wsmc.dsl import Data
from wsmc.ssm import SSM, assign, observe, sample

# the five shipped non-guided specs: (make, data, the pinned columns)
SHIPPED = {
    "lgssm1d_spec": (models.lgssm1d_spec, models.lgssm1d_data, ["x"]),
    "sv": (models.sv, models.sv_data, ["h"]),
    "poisson_count": (models.poisson_count, models.poisson_count_data, ["x"]),
    "kitagawa": (models.kitagawa, models.kitagawa_data, ["x"]),
    "local_trend": (models.local_trend, models.local_trend_data, ["v", "x"]),
}


def two_observes():
    """a step with two OBSERVEs and so a Resample between them"""
    x = Col("x")
    return (SSM(cols=["x"]).init(sample("x", Normal(0.0, 1.0)))
            .step(sample("x", Normal(x * 0.9, 1.0)), observe(Data(0), Normal(x, 2.0)), observe(Data(0), Normal(x * 0.5, 1.0))))


def chained_samples():
    """the pinned column v is read by a later SAMPLE's operands in the same step, and by an assignment"""
    v, x = Col("v"), Col("x")
    return (SSM(cols=["v", "x", "s", "u"]).init(sample("v", Normal(0.0, 1.0)), sample("x", Normal(0.0, 1.0)), assign("u", x * 0.0))
            .step(sample("v", Normal(v * 0.5 + x * 0.1, 1.0)), sample("x", Normal(v, 0.5)), assign("s", v + x * 2.0),
                  sample("u", Normal(Col("s") * 0.1, 1.0)), observe(Data(0), Normal(x + Col("u") * 0.1, 0.7))))


def reference(ssm, T, seed, B=None):
    """a fixed reference [T, n_cols] ([B, T, n_cols] with B), every column filled: the run must
    ignore the entries of the columns it does not pin"""
    rng = np.random.Generator(np.random.Philox(seed))
    return rng.standard_normal(((B,) if B else ()) + (T, len(ssm.cols))) * 1.5


def definition(ssm, data, n, seed, ref, ess, M=0, bw_seed=0, trace=False):
    """one conditional filter and its backward pass by the definitions on the oracle:
    (flags, ESS%, SsmTrace or None, SsmRecord, SsmFinal, SsmBackward or None)"""
    r = ssm.conditional_definition(Oracle, data, n, seed, ref, ess, trace=trace)
    flags, ess_tr, tr, rec, end = (r[0], r[1], r[2], r[3], r[4]) if trace else (r[0], r[1], None, r[2], r[3])
    bw = ssm.backward_definition(Oracle, rec, data, M, bw_seed) if M else None
    return flags, ess_tr, tr, rec, end, bw


def definition_gibbs(ssm, data, n, sweeps, seed, chains=1, ess=0.5, ref=None):
    """wsmc.particle_gibbs as a loop over the definitions on the oracle:
    (column name -> [sweeps, chains, T], log evidence [sweeps, chains])"""
    T, S = len(ssm.table(data)), len(ssm.cols)
    traj, logev = np.empty((sweeps, chains, T, S)), np.empty((sweeps, chains))
    ref = None if ref is None else np.array(ref, dtype=np.float64)
    for j in range(sweeps):
        seeds, bw_seeds = wsmc.pg_seeds(seed, j, chains)
        nxt = np.empty((chains, T, S))
        for b in range(chains):
            if ref is None:
                o = Oracle(n, seed=int(seeds[b]))
                rec = ssm.statements(o, data, ess, record=True)[-1]
                logev[j, b] = o.log_evidence()
                o.close()
            else:
                rec, end = ssm.conditional_definition(Oracle, data, n, int(seeds[b]), ref[b], ess)[-2:]
                logev[j, b] = end.log_evidence
            bw = ssm.backward_definition(Oracle, rec, data, 1, int(bw_seeds[b]))
            nxt[b] = np.stack([bw.paths[c][:, 0] for c in ssm.cols], axis=1)
        ref = traj[j] = nxt
    return {c: traj[..., k].copy() for k, c in enumerate(ssm.cols)}, logev

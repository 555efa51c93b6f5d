"""The batched fused run (wsmc_ssm_run_batch, csrc/wsmc_ssm_batch.hip): B independent filters in one
call, one persistent workgroup each. Filter b is compared, bit for bit, with the CPU oracle issuing
spec b's statements one by one on Oracle(n, seed=seeds[b]): every column, the log-weights, the last
ancestors, the evidence, the ESS trace (NaNs by position), the number of resamples and the last
decision. A mismatch names the filter, then the step, or the column and the particle.

A filter that never resampled has a last-ancestors row of zeros: what wsmc_last_ancestors gives on
a fresh context and what the oracle's fresh state holds (not the identity).

Shapes: T <= 40; n = 1 (a lone particle), 65 (one particle in the second wave), 1001 (two a
thread), 2049 (three a thread, waves that own nothing), the cap of the column count; B = 1, a few,
and more than the device holds resident (from ssm_batch_stats()'s CU count).
"""
import math

import numpy as np
import pytest

import ssmfuzz as sf
import wsmc
from wsmc import abi, dsl, models
from wsmc.dsl import Col, Data, Normal
from wsmc.ssm import SSM, assign, observe, sample
from oracle import Oracle

pytestmark = pytest.mark.gpu

STRAT, SYST, MULT = abi.RESAMPLE_STRATIFIED, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MULTINOMIAL
T = 24


def bits_equal(a, b):
    """elementwise: the same bits, or NaN on both sides"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def reference(spec, data, n, seed, ess, scheme, horizon=None):
    """filter b's definition: the spec's statements on a fresh oracle"""
    o = Oracle(n, seed=seed)
    _, trace = spec.statements(o, data, ess_perc_min=ess, scheme=scheme, T=horizon)
    st = o.get_state()
    r = {"cols": {name: o.col_download(o.col_find(name)) for name in spec.cols}, "w": o.weights_download(),
         "anc": o.last_ancestors(), "ev": o.log_evidence(), "ess": np.asarray(trace),
         "nres": st["n_resamples"], "last": bool(st["resampled"])}
    o.close() if hasattr(o, "close") else None
    return r


def check_filter(res, b, ref, what=""):
    """filter b of a batch's result against its reference"""
    tag = f"{what} filter b={b}"
    if res.ess is not None:
        ok = bits_equal(res.ess[b], ref["ess"])
        assert ok.all(), f"{tag}: ESS trace differs first at step {int(np.argmin(ok))}: {res.ess[b][np.argmin(ok)]!r} != {ref['ess'][np.argmin(ok)]!r}"
    assert int(res.n_resamples[b]) == ref["nres"], f"{tag}: n_resamples {int(res.n_resamples[b])} != {ref['nres']}"
    assert bool(res.last_resampled[b]) == ref["last"], f"{tag}: last decision {bool(res.last_resampled[b])} != {ref['last']}"
    if res.cols is not None:
        for name, col in ref["cols"].items():
            ok = bits_equal(res.cols[name][b], col)
            assert ok.all(), f"{tag}: column {name} differs first at particle {int(np.argmin(ok))}: {res.cols[name][b][np.argmin(ok)]!r} != {col[np.argmin(ok)]!r}"
        ok = bits_equal(res.log_weights[b], ref["w"])
        assert ok.all(), f"{tag}: log-weights differ first at particle {int(np.argmin(ok))}"
        ok = res.last_ancestors[b] == ref["anc"]
        assert ok.all(), f"{tag}: last ancestors differ first at particle {int(np.argmin(ok))}"
    assert bits_equal(res.log_evidence[b], ref["ev"]).all(), f"{tag}: log evidence {res.log_evidence[b]!r} != {ref['ev']!r}"


def run_batch(g, specs, data, n, seeds, ess, scheme=STRAT, horizon=None):
    return g.ssm_run_batch(specs, data, n, seeds, ess_perc_min=ess, scheme=scheme, ess_trace=True, state=True, T=horizon)


@pytest.fixture(scope="module")
def ctx(gpu_available):
    g = wsmc.Context(16, seed=1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def caps(ctx):
    return ctx.ssm_stats()["cap"]


# ---- 1. one filter: the batch, the single run and the oracle ----------------------------------
MODELS = {name: (make(), gen(40)) for name, (make, gen) in models.SSM_MODELS.items()}


@pytest.mark.parametrize("ess", [1.0, 0.5])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_filter_is_the_single_run(ctx, name, ess):
    spec, data = MODELS[name]
    seed = 42
    res = run_batch(ctx, spec, data, 1000, [seed], ess)
    ref = reference(spec, data, 1000, seed, ess, STRAT)
    check_filter(res, 0, ref, name)
    g = wsmc.Context(1000, seed=seed)
    ev, trace = g.ssm_run(spec, data, ess_perc_min=ess, ess_trace=True)
    assert g.ssm_stats()["persistent_runs"] == 1
    assert bits_equal(ev, res.log_evidence[0]).all()
    assert bits_equal(trace, res.ess[0]).all()
    for cname in spec.cols:
        assert bits_equal(g.col_download(g.col_find(cname)), res.cols[cname][0]).all(), cname
    assert bits_equal(g.weights_download(), res.log_weights[0]).all()
    np.testing.assert_array_equal(g.last_ancestors(), res.last_ancestors[0])
    st = g.get_state()
    assert st["n_resamples"] == res.n_resamples[0] and bool(st["resampled"]) == bool(res.last_resampled[0])
    g.close()


# ---- 2. per-filter parameters and seeds --------------------------------------------------------
SV_PARAMS = [(-1.0, 0.95, 0.25), (-0.5, 0.9, 0.3), (0.2, 0.97, 0.15), (-2.0, 0.8, 0.5), (0.0, 0.99, 0.1)]
SV_SEEDS = [42, 7, 2**63 + 5, 0, 123456789]
SV_SPECS = [models.sv(*p) for p in SV_PARAMS]
SV_DATA = models.sv_data(T)


@pytest.mark.parametrize("scheme", [STRAT, SYST])
@pytest.mark.parametrize("ess", [0.5, 1.0])
@pytest.mark.parametrize("n", [1, 65, 1001, 2049])
def test_per_filter_parameters_and_seeds(ctx, n, ess, scheme):
    refs = [reference(SV_SPECS[b], SV_DATA, n, SV_SEEDS[b], ess, scheme) for b in range(5)]
    try:
        for segment in (1, 5, 0):
            ctx.set_ssm_batch_segment(segment)
            res = run_batch(ctx, SV_SPECS, SV_DATA, n, SV_SEEDS, ess, scheme)
            st = ctx.ssm_batch_stats()
            assert st["segments"] == (-(-T // segment) if segment else 1)
            assert st["blocks_per_cu"] >= 1 and st["cus"] >= 1
            for b in range(5):
                check_filter(res, b, refs[b], f"segment {segment}")
    finally:
        ctx.set_ssm_batch_segment(0)
    if n >= 65 and ess == 1.0:
        assert all(r["nres"] == T for r in refs)
    # the filters do differ
    assert len({float(r["ev"]) for r in refs}) == 5


# ---- 3. a block's result does not depend on its place or its neighbours -------------------------
def test_block_independence(ctx):
    n, ess = 1001, 0.5
    same = (models.sv(-1.0, 0.95, 0.25), 42)
    others = [(models.sv(-0.5, 0.9 + 0.01 * k, 0.2 + 0.02 * k), 100 + k) for k in range(4)]
    order = [same, others[0], others[1], same, others[2], others[3], same]
    ref_same = reference(same[0], SV_DATA, n, same[1], ess, STRAT)
    ref_other = [reference(s, SV_DATA, n, seed, ess, STRAT) for s, seed in others]
    for what, seq in (("forward", order), ("reversed", order[::-1])):
        res = run_batch(ctx, [s for s, _ in seq], SV_DATA, n, [seed for _, seed in seq], ess)
        for b, (s, seed) in enumerate(seq):
            ref = ref_same if s is same[0] else ref_other[[o[0] for o in others].index(s)]
            check_filter(res, b, ref, what)
        for b in (3, 6):
            for cname in same[0].cols:
                assert bits_equal(res.cols[cname][0], res.cols[cname][b]).all()
            assert bits_equal(res.ess[0], res.ess[b]).all() and bits_equal(res.log_weights[0], res.log_weights[b]).all()


# ---- 4. more filters than the device holds resident -------------------------------------------
def test_more_filters_than_resident_blocks_at_the_cap(ctx, caps):
    """n = cap(1): one workgroup a CU by LDS; 2 CUs + 3 filters queue behind one another"""
    cus = ctx.ssm_batch_stats()["cus"]
    assert cus >= 1
    n, B, steps = caps[1], 2 * cus + 3, 4
    spec, data = models.lgssm1d_spec(), models.lgssm1d_data(steps)
    res = run_batch(ctx, spec, data, n, list(range(B)), 1.0)
    st = ctx.ssm_batch_stats()
    assert st["blocks_per_cu"] == 1 and B > st["blocks_per_cu"] * st["cus"]
    for b in range(B):
        check_filter(res, b, reference(spec, data, n, b, 1.0, STRAT), "cap")


def test_many_small_filters(ctx):
    cus = ctx.ssm_batch_stats()["cus"]
    n, B, steps = 65, 8 * cus + 1, 6
    spec, data = models.local_trend(), models.local_trend_data(steps)
    res = run_batch(ctx, spec, data, n, list(range(B)), 0.5)
    for b in range(B):
        check_filter(res, b, reference(spec, data, n, b, 0.5, STRAT), "small")


# ---- 5. data ------------------------------------------------------------------------------------
def test_shared_table_and_per_filter_tables(ctx):
    n, ess = 1001, 0.5
    spec, seeds = models.local_trend(), [3, 4, 5, 6]
    y = models.local_trend_data(T)
    y2, y3 = models.local_trend_data(T, seed=9), y[::-1].copy()
    shared = run_batch(ctx, spec, y, n, seeds, ess)
    tables = run_batch(ctx, spec, [y, y2, y.copy(), y3], n, seeds, ess)
    for b, d in enumerate([y, y2, y, y3]):
        check_filter(tables, b, reference(spec, d, n, seeds[b], ess, STRAT), "tables")
        check_filter(shared, b, reference(spec, y, n, seeds[b], ess, STRAT), "shared")
    for b in (0, 2):
        assert bits_equal(shared.log_weights[b], tables.log_weights[b]).all()
    for b in (1, 3):
        assert not bits_equal(shared.log_weights[b], tables.log_weights[b]).all()


@pytest.mark.parametrize("name", ["nodata", "wide_data"])
def test_no_table_and_a_wide_table(ctx, name):
    """data_dim = 0 with a null table; a four-column table of which only columns 3 and 1 are read
    (the others hold 1e300 and NaN)"""
    case = sf.gen(name, "directed")
    seeds = [11, 12, 13]
    res = run_batch(ctx, case.ssm, case.data, 65, seeds, 0.5, horizon=case.T)
    for b, seed in enumerate(seeds):
        check_filter(res, b, reference(case.ssm, case.data, 65, seed, 0.5, STRAT, case.T), name)


# ---- 6. families: the log-Gamma and the extended variant, neighbouring blocks on other branches --
def test_poisson_count_variant(ctx):
    specs = [models.poisson_count(a, s) for a, s in ((0.9, 0.3), (0.7, 0.5), (0.95, 0.1))]
    data = models.poisson_count_data(T)
    res = run_batch(ctx, specs, data, 1001, [1, 2, 3], 0.5)
    for b in range(3):
        check_filter(res, b, reference(specs[b], data, 1001, b + 1, 0.5, STRAT), "poisson_count")


def test_ext_variant(ctx):
    mk = lambda a, th, sg: (SSM(cols=["x"])
                            .init(sample("x", dsl.Laplace(0.0, 1.0)))
                            .step(sample("x", dsl.Laplace(Col("x") * a, th)),
                                  observe(Data(0), dsl.Cauchy(Col("x"), sg))))
    specs = [mk(0.9, 0.5, 0.7), mk(0.5, 1.0, 0.2), mk(0.99, 0.1, 2.0)]
    data = models.lgssm1d_data(T)
    res = run_batch(ctx, specs, data, 1001, [1, 2, 3], 1.0)
    for b in range(3):
        check_filter(res, b, reference(specs[b], data, 1001, b + 1, 1.0, STRAT), "ext")


def test_sampler_branches_differ_between_blocks(ctx):
    """Poisson rates on both sides of the inversion / PTRS threshold and Gamma shapes on both sides
    of the boost, as per-filter constants: whole blocks, not lanes, take different branches"""
    pois = lambda rate: (SSM(cols=["k", "x"])
                         .init(sample("x", Normal(0.0, 1.0)))
                         .step(sample("k", dsl.Poisson(rate)),
                               sample("x", Normal(Col("x") * 0.9, 0.5)),
                               observe(Col("k"), dsl.Poisson(rate * 1.25)),
                               observe(Data(0), Normal(Col("x"), 1.0))))
    gam = lambda shape: (SSM(cols=["g", "x"])
                         .init(sample("x", Normal(0.0, 1.0)))
                         .step(sample("g", dsl.Gamma(shape, 1.5)),
                               sample("x", Normal(Col("x") * 0.9, 0.5)),
                               observe(Col("g"), dsl.Gamma(shape * 1.1, 1.5)),
                               observe(Data(0), Normal(Col("x"), 1.0))))
    data = models.lgssm1d_data(T)
    for what, specs in (("poisson", [pois(r) for r in (0.5, 9.99, 10.0, 300.0)]), ("gamma", [gam(a) for a in (0.2, 1.0, 50.0)])):
        seeds = list(range(20, 20 + len(specs)))
        assert all(specs[0].same_shape(s) for s in specs)
        res = run_batch(ctx, specs, data, 65, seeds, 0.5)
        for b, s in enumerate(specs):
            check_filter(res, b, reference(s, data, 65, seeds[b], 0.5, STRAT), what)


# ---- 7. a filter that dies between two that live ------------------------------------------------
def test_a_dying_filter_between_two_healthy_ones(ctx):
    case = sf.gen("partial_support", "directed")   # data[20] = -100: the OBSERVE is -inf for every particle
    healthy = case.data.copy()
    healthy[sf.PARTIAL_ALL_AT] = 0.5
    tables, seeds = [healthy, case.data, healthy.copy()], [5, 6, 7]
    res = run_batch(ctx, case.ssm, tables, 1001, seeds, 1.0, horizon=case.T)
    for b in range(3):
        check_filter(res, b, reference(case.ssm, tables[b], 1001, seeds[b], 1.0, STRAT, case.T), "dying")
    assert np.isnan(res.ess[1][sf.PARTIAL_ALL_AT:]).all() and not np.isnan(res.ess[1][:sf.PARTIAL_ALL_AT]).any()
    assert np.isneginf(res.log_weights[1]).all() and res.n_resamples[1] == sf.PARTIAL_ALL_AT
    assert not np.isnan(res.ess[0]).any() and not np.isnan(res.ess[2]).any()
    assert math.isfinite(res.log_evidence[0]) and math.isfinite(res.log_evidence[2])


# ---- 8. random specs ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1001, 65])
@pytest.mark.parametrize("seed", range(6))
def test_random_specs(ctx, seed, n):
    case = sf.gen(seed, "mixed")
    ess = (1.0, 0.5)[seed % 2]
    seeds = [sf.SEED, sf.SEED + 1 + seed, 1000 + seed]
    res = run_batch(ctx, case.ssm, case.data, n, seeds, ess, horizon=case.T)
    for b in range(3):
        check_filter(res, b, reference(case.ssm, case.data, n, seeds[b], ess, STRAT, case.T), case.name)


@pytest.mark.parametrize("name", ["full", "prog96"])
def test_directed_specs(ctx, caps, name):
    case = sf.gen(name, "directed")
    n = caps[4] if name == "full" else 65
    seeds = [sf.SEED, 9]
    res = run_batch(ctx, case.ssm, case.data, n, seeds, 0.5, horizon=case.T)
    for b in range(2):
        check_filter(res, b, reference(case.ssm, case.data, n, seeds[b], 0.5, STRAT, case.T), name)


# ---- 9. the context the call goes through is untouched ------------------------------------------
def test_the_context_is_untouched(gpu_available):
    n = 1000
    g, o = wsmc.Context(n, seed=42), Oracle(n, seed=42)

    def first_half(c):
        r = models.resolver(c)
        x, v = c.col_create("x", 1), c.col_create("v", 1)
        c.sample(x, Normal(0.0, 1.0).dist(r))
        c.resample(0.5, STRAT, wait=False)
        c.sample(v, Normal(Col("x") * 0.5, 0.3).dist(r))
        c.resample(0.5, STRAT, wait=False)
        c.observe(Normal(Col("x"), 0.4).dist(r), models._const([0.3]))
        c.resample(0.9, STRAT, wait=False)   # its decision is still on the device when the batch runs
        c.sample(x, Normal(Col("x") + Col("v"), 0.2).dist(r))   # an open statement batch

    def second_half(c):
        r = models.resolver(c)
        c.resample(0.9, STRAT, wait=False)
        c.observe(Normal(Col("x"), 0.4).dist(r), models._const([-0.2]))
        c.resample(0.9, STRAT, wait=False)
        c.sample(c.col_find("v"), Normal(Col("v"), 0.1).dist(r))

    first_half(g)
    before = g.ssm_stats()
    spec, data = MODELS["sv"]
    res = run_batch(g, spec, data, 1001, [1, 2], 0.5)
    assert g.ssm_stats() == before
    second_half(g)
    first_half(o)
    second_half(o)
    assert sf.compare(g, o) is None, sf.compare(g, o)
    assert g.col_names() == ["x", "v"]
    for b, seed in enumerate((1, 2)):
        check_filter(res, b, reference(spec, data, 1001, seed, 0.5, STRAT), "beside a program")
    g.close()


# ---- 10. refusals -------------------------------------------------------------------------------
def _raw(g, specs, n_specs, tab, n_tables, steps, n, B, seeds, ess=0.5, scheme=STRAT, out=True):
    import ctypes as C
    arr = (abi.SsmSpec * len(specs))()
    for k, s in enumerate(specs):
        C.memmove(C.byref(arr[k]), C.byref(s.spec), C.sizeof(abi.SsmSpec))
    sd = (C.c_uint64 * max(1, len(seeds)))(*seeds) if seeds is not None else None
    o = abi.SsmBatchOut()
    ev = np.empty(max(B, 1))
    o.log_evidence = ev.ctypes.data_as(C.POINTER(C.c_double))
    t = None if tab is None else np.ascontiguousarray(tab, dtype=np.float64)
    rc = g._L.wsmc_ssm_run_batch(g._h, arr, n_specs, None if t is None else t.ctypes.data_as(C.POINTER(C.c_double)), n_tables,
                                 steps, n, B, sd, ess, scheme, C.byref(o) if out else None)
    return rc, g._L.wsmc_last_error().decode()


def test_refusals(ctx, caps):
    sv, y = MODELS["sv"]
    y = y[:T]
    big = sf.gen("prog97", "directed")
    bad = SSM.from_spec(type(sv.spec).from_buffer_copy(bytes(sv.spec)))
    bad.spec.step[0].dist.family = 15   # the reserved family: wsmc_ssm_spec_check refuses it
    other = models.local_trend()
    cases = [
        ("above the cap", lambda: _raw(ctx, [sv], 1, y, 1, T, caps[2] + 1, 2, [1, 2]), "cap"),
        ("multinomial", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, [1, 2], scheme=MULT), "multinomial"),
        ("unknown scheme", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, [1, 2], scheme=7), "scheme"),
        ("97 instructions", lambda: _raw(ctx, [big.ssm], 1, big.data, 1, big.T, 65, 2, [1, 2]), "program instructions"),
        ("B < 1", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 0, [1]), "B < 1"),
        ("T < 1", lambda: _raw(ctx, [sv], 1, y, 1, 0, 100, 2, [1, 2]), "T < 1"),
        ("n < 1", lambda: _raw(ctx, [sv], 1, y, 1, T, 0, 2, [1, 2]), "n < 1"),
        ("n_specs", lambda: _raw(ctx, [sv, sv], 2, y, 1, T, 100, 3, [1, 2, 3]), "n_specs"),
        ("n_tables", lambda: _raw(ctx, [sv], 1, np.concatenate([y, y]), 2, T, 100, 3, [1, 2, 3]), "n_tables"),
        ("null seeds", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, None), "seeds"),
        ("null out", lambda: _raw(ctx, [sv], 1, y, 1, T, 100, 2, [1, 2], out=False), "out"),
        ("null data", lambda: _raw(ctx, [sv], 1, None, 1, T, 100, 2, [1, 2]), "data"),
        ("a refused spec", lambda: _raw(ctx, [sv, sv, bad], 3, y, 1, T, 100, 3, [1, 2, 3]), "spec 2"),
        ("another shape", lambda: _raw(ctx, [sv, other], 2, y, 1, T, 100, 2, [1, 2]), "spec 1 differs from spec 0 in shape"),
    ]
    for what, call, word in cases:
        rc, msg = call()
        assert rc == abi.WSMC_EARG, (what, rc, msg)
        assert word in msg, (what, msg)
    # a multi-device handle (two host-transport shards on one device)
    m = wsmc.Context.multi(128, 2, seed=1, devices=[0, 0], transport=abi.TRANSPORT_HOST)
    rc, msg = _raw(m, [sv], 1, y, 1, T, 100, 2, [1, 2])
    assert rc == abi.WSMC_EARG and "multi-device" in msg, msg
    m.close()
    # afterwards the context still runs a statement and a batch
    x = ctx.col_create("after", 1)
    ctx.assign(x, models._const([1.5]))
    assert (ctx.col_download(x) == 1.5).all()
    res = run_batch(ctx, sv, y, 65, [1, 2], 0.5)
    for b in range(2):
        check_filter(res, b, reference(sv, y, 65, b + 1, 0.5, STRAT), "after the refusals")

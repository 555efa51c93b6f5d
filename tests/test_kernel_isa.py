"""The order of loads, waits and Philox multiplies in the fused 2D-SSM step kernels.

Read from the device assembly the build saves next to the kernels' resource listing
(weightedsampling.jl_amd/build/wsmc_kernels.s, tools/kres.py isa_events): the vector-memory loads,
the s_waitcnt that name vmcnt and the v_mad_u64_u32 of a kernel, in the order of the text. In a
launch whose blocks all run in one resident round every wave is in the same phase at the same time,
so a memory round trip that sits serially in a wave's chain is idle time for the whole GPU: these
checks hold the step kernels to the round trips their data dependences need.
"""
import importlib.util
import pathlib

import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("kres", REPO / "tools" / "kres.py")
kres = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kres)

PROP_1M = "k_ssm2d_propILi0ELi1ELi512ELb1ELb0EE"    # <MODE 0, IT 1, NT 512, QS, not ISL>
FILLS = ("k_rs_fill_fusedILi0ELb0EE", "k_rs_fill_fusedILi0ELb1EE")
# Philox4x32-10 for two particles is 2 x 10 rounds x 2 products = 40 32x32->64 products. Two of
# them (the first round's product of the counter word that holds the run's op number, the same
# for both particles and every thread) are scalar multiplies, so 38 are v_mad_u64_u32. The whole
# draw of both particles was hoisted (nothing less was needed to fit the registers): all of them.
PHILOX_VECTOR_MULTIPLIES = 38


@pytest.fixture(scope="module")
def isa():
    if not kres.ISA.exists():
        pytest.fail(f"{kres.ISA} is missing: build() saves it beside the kernels' resource listing")
    return kres.ISA


def gathers(ev):
    """indices of the 16-B loads after the first full wait (the table's barrier): the weight pair
    of a step that follows no resample, then the x and v pairs of both particles"""
    first_wait = next(i for i, (k, t) in enumerate(ev) if k == "wait" and "vmcnt(0)" in t)
    idx = [i for i, (k, t) in enumerate(ev) if i > first_wait and k == "load" and "global_load_dwordx4" in t]
    return idx


def test_every_philox_multiply_precedes_the_wait_for_the_gathers(isa):
    ev = kres.isa_events(PROP_1M, path=isa)
    g = gathers(ev)
    assert len(g) >= 4                  # x and v of two particles (and the weight pair, the observation)
    last_gather = g[-1]
    wait = next(i for i, (k, _) in enumerate(ev) if i > last_gather and k == "wait")
    mads = [i for i, (k, _) in enumerate(ev) if k == "mad"]
    assert len(mads) == PHILOX_VECTOR_MULTIPLIES
    assert all(i < wait for i in mads)
    # stronger, and what the source arranges: they precede the gathers' issue too, under the first
    # hop (the ancestor pair, the previous max slots, the table entry)
    assert all(i < g[0] for i in mads)


def test_no_wait_separates_the_gathers(isa):
    ev = kres.isa_events(PROP_1M, path=isa)
    g = gathers(ev)
    assert not [t for k, t in ev[g[0]:g[-1] + 1] if k == "wait"]


def narrow_runs(ev):
    """Address operands from which a kernel loads the entries at offsets 8, 16 and 24 all three
    8 bytes at a time: a thread's four q or w loaded one by one.

    The plain rule "no global_load_dwordx2 with offset:8, offset:16 or offset:24" cannot hold in
    these kernels whatever the q and w loads are: the record and overflow blocks read single
    fields of structures at those offsets (Decision.mean at 8, two fields of the exact-shard plan
    at 8 and 24, a group line's maximum at 8, parts of an all-gathered line at 16). Those read at
    most two of the three offsets from one address; the parent's q and w loads read all three."""
    by_addr = {}
    for k, t in ev:
        if k != "load" or not t.startswith("global_load_dwordx2"):
            continue
        ops = [o.strip() for o in t.split(None, 1)[1].split(",")]
        last = ops[-1].split()
        off = next((w for w in last if w.startswith("offset:")), "offset:0")
        addr = (ops[1], last[0])        # the vector address and `off` or the scalar base
        by_addr.setdefault(addr, set()).add(off)
    rest = {"offset:8", "offset:16", "offset:24"}
    return {a: sorted(o) for a, o in by_addr.items() if rest <= o}


def wide_pairs(ev):
    """adjacent 16-B loads of one quad: offsets 0 and 16 from one address"""
    n = 0
    for (k0, t0), (k1, t1) in zip(ev, ev[1:]):
        if k0 == k1 == "load" and t0.startswith("global_load_dwordx4") and t1.startswith("global_load_dwordx4"):
            a0, a1 = t0.split(",")[1].strip(), t1.split(",")[1].strip()
            offs = {("offset:16" in t0), ("offset:16" in t1)}
            n += a0 == a1 and offs == {True, False}
    return n


@pytest.mark.parametrize("name", FILLS)
def test_fill_loads_q_and_w_16_bytes_at_a_time(isa, name):
    ev = kres.isa_events(name, path=isa)
    assert not narrow_runs(ev)
    assert wide_pairs(ev) >= 2          # the tile blocks' quad and the overflow chunks'


def test_isa_events_reads_only_its_kernel(isa):
    ev = kres.isa_events(PROP_1M, path=isa)
    assert {k for k, _ in ev} == {"load", "wait", "mad"}
    with pytest.raises(KeyError):
        kres.isa_events("k_ssm2d_prop", path=isa)      # several instantiations match

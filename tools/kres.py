"""Residency of the library's kernels from the compiler's resource listing.

    python tools/kres.py [--listing FILE] [--block THREADS] [--blocks GRID] [name-part ...]
    python tools/kres.py --block 512 --blocks 977 k_ssm2d_propILi0ELi1ELi512     # the 1M propagate

The build saves hipcc's -Rpass-analysis=kernel-resource-usage remarks for csrc/wsmc_kernels.hip as
weightedsampling.jl_amd/build/wsmc_kernels.resources.txt. Printed per kernel: its registers, LDS
and scratch, the waves a SIMD admits, the blocks a CU admits and, with --blocks, the rounds a
launch of that many blocks takes on the 256 CUs of an MI355X.

The rule for the scalar registers is measured, not the compiler's: a SIMD admits
min(8, floor(800 / (ceil(sgpr / 16) * 16 + 16))) waves, that is 8 up to 80 SGPRs, 7 from 82 to 96
and 6 from 98, one fewer than the compiler's own "Occupancy" line in the upper bands.
"""
from __future__ import annotations

import argparse
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
LISTING = ROOT / "weightedsampling.jl_amd" / "build" / "wsmc_kernels.resources.txt"
ISA = LISTING.with_name("wsmc_kernels.s")   # the build's device assembly of csrc/wsmc_kernels.hip
CUS = 256               # MI355X
SIMDS_PER_CU = 4
VGPRS_PER_SIMD = 512    # per lane, wave64 (unified with the AGPRs)
LDS_PER_CU = 160 * 1024

_FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
           "Occupancy [waves/SIMD]": "compiler_occupancy", "SGPRs Spill": "sgpr_spills",
           "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "lds"}


def parse(path=LISTING) -> dict:
    """{mangled kernel name: {sgprs, vgprs, agprs, scratch, sgpr_spills, vgpr_spills, lds, ...}}"""
    out, cur = {}, None
    for line in pathlib.Path(path).read_text().splitlines():
        m = re.match(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+)\s*$", line)
        if m and cur is not None and m.group(1) in _FIELDS:
            cur[_FIELDS[m.group(1)]] = int(m.group(2))
    return {k: v for k, v in out.items() if "sgprs" in v}


def waves_by_sgprs(sgprs: int) -> int:
    return min(8, 800 // (-(-sgprs // 16) * 16 + 16))


def waves_by_vgprs(vgprs: int) -> int:
    return min(8, VGPRS_PER_SIMD // max(8, -(-vgprs // 8) * 8))


def waves_per_simd(sgprs: int, vgprs: int = 0) -> int:
    return min(waves_by_sgprs(sgprs), waves_by_vgprs(vgprs))


def blocks_per_cu(block_threads: int, sgprs: int, vgprs: int = 0, lds: int = 0) -> int:
    """Blocks of block_threads threads (wave64) one CU admits."""
    waves = -(-block_threads // 64)
    n = waves_per_simd(sgprs, vgprs) * SIMDS_PER_CU // waves
    if lds > 0:
        n = min(n, LDS_PER_CU // lds)
    return n


def rounds(blocks: int, per_cu: int) -> float:
    return blocks / (CUS * per_cu)


def find(res: dict, *parts: str) -> dict:
    """The one kernel whose mangled name holds every part."""
    hit = [k for k in res if all(p in k for p in parts)]
    if len(hit) != 1:
        raise KeyError(f"{parts}: {len(hit)} kernels match")
    return res[hit[0]]


_VMEM_LOAD = re.compile(r"(global|buffer|flat|scratch)_load_\w+")


def isa_events(*parts: str, path=ISA) -> list:
    """The memory schedule of the one kernel whose mangled name holds every part, in the order of
    the assembly text: ("load", text) for each vector-memory load, ("wait", text) for each
    s_waitcnt that names vmcnt, ("mad", text) for each v_mad_u64_u32 (a Philox round has two)."""
    lines = pathlib.Path(path).read_text().splitlines()
    heads = [(i, ln.split(":", 1)[0]) for i, ln in enumerate(lines)
             if ln.startswith("_Z") and ":" in ln and all(p in ln.split(":", 1)[0] for p in parts)]
    if len(heads) != 1:
        raise KeyError(f"{parts}: {len(heads)} kernels match")
    out = []
    for ln in lines[heads[0][0] + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        t = ln.split(";", 1)[0].strip()
        op = t.split(None, 1)[0] if t else ""
        if _VMEM_LOAD.fullmatch(op):
            out.append(("load", t))
        elif op == "s_waitcnt" and "vmcnt(" in t:
            out.append(("wait", t))
        elif op == "v_mad_u64_u32":
            out.append(("mad", t))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--listing", default=str(LISTING))
    ap.add_argument("--block", type=int, default=256, help="threads a block")
    ap.add_argument("--blocks", type=int, default=0, help="blocks of the launch: prints its rounds")
    ap.add_argument("parts", nargs="*", help="print the kernels whose mangled name holds one of these")
    ap.add_argument("--isa", action="store_true", help="print the loads, vmcnt waits and 64-bit multiplies of the one "
                    "kernel whose name holds every part, in order")
    a = ap.parse_args()
    if a.isa:
        for kind, text in isa_events(*a.parts):
            print(f"{kind:5s} {text}")
        return
    for name, r in parse(a.listing).items():
        if a.parts and not any(p in name for p in a.parts):
            continue
        v = r["vgprs"] + r.get("agprs", 0)
        b = blocks_per_cu(a.block, r["sgprs"], v, r["lds"])
        line = (f"{name[:64]:64s} sgpr {r['sgprs']:>3} (spill {r['sgpr_spills']:>2}) vgpr {r['vgprs']:>3} lds {r['lds']:>6} "
                f"scratch {r['scratch']:>3} | waves/SIMD {waves_per_simd(r['sgprs'], v)} blocks/CU({a.block}) {b}")
        if a.blocks and b:
            line += f" | {a.blocks} blocks = {rounds(a.blocks, b):.2f} rounds"
        print(line)


if __name__ == "__main__":
    main()

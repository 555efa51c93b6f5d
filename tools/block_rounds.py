"""Rounds of workgroups in the fused 2D-SSM run, from the block clocks of a diagnostic build.

    python tools/build_variant.py diag -DWSMC_DIAG_BUILD
    WSMC_LIB=tools/variants/diag/libwsmc.so python tools/block_rounds.py [--particles N] [--steps T] [--ess E]

A diagnostic build's propagate, fill and trace-back store each block's start and end on the
100 MHz constant clock (csrc/wsmc_kernels.hip, WSMC_BLK_CLOCK); the buffer holds the last launch
of each kernel. Printed per kernel, as one JSON line: the blocks launched, the largest number
alive at once, how many started only after the first block had ended (a second round), and the
launch's span first start -> last end. One clock tick is 10 ns, so blocks that end and start
within the same tick are counted as overlapping.
"""
import argparse
import ctypes as C
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "weightedsampling.jl_amd"))
import wsmc  # noqa: E402

KINDS = ("propagate", "fill", "traceback", "propagate_plain")   # (plain: the steps without the statistics, the first)
MAX_BLOCKS = 16384


def rounds(clk: np.ndarray) -> dict:
    """clk: [n][2] start / end ticks of the blocks that ran."""
    t0, t1 = clk[:, 0].astype(np.int64), clk[:, 1].astype(np.int64)
    # sweep: a block that ends at a tick is still alive for the blocks that start at it
    ev = np.concatenate([np.stack([t0, np.zeros_like(t0)], 1), np.stack([t1, np.ones_like(t1)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    alive = np.cumsum(np.where(ev[:, 1] == 0, 1, -1))
    return {"blocks": int(len(clk)), "max_alive": int(alive.max()),
            "started_after_first_end": int((t0 > t1.min()).sum()),
            "span_us": round(float(t1.max() - t0.min()) / 100.0, 2),
            "median_block_us": round(float(np.median(t1 - t0)) / 100.0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3, help="runs before the one that is read (warm-up)")
    a = ap.parse_args()
    L = wsmc.load_library()
    if not hasattr(L, "wsmc_diag_block_clocks"):
        raise SystemExit("not a diagnostic build: build one with -DWSMC_DIAG_BUILD and select it with WSMC_LIB")
    L.wsmc_diag_block_clocks.argtypes = [C.c_int, C.c_void_p, C.c_int]
    L.wsmc_diag_block_clocks.restype = C.c_int
    obs = wsmc.models.ssm2d_data(a.steps)
    g = wsmc.Context(a.particles, seed=123, device=0)
    for _ in range(a.runs):
        g.ssm2d_run(obs, ess_perc_min=a.ess, keep_history=True)
    g.sync()
    if L.wsmc_diag_block_clocks(0, None, -1) != 0:
        raise SystemExit("could not reset the block clocks")
    g.ssm2d_run(obs, ess_perc_min=a.ess, keep_history=True)
    g.sync()
    for kind, name in enumerate(KINDS):
        buf = np.zeros((MAX_BLOCKS, 2), dtype=np.uint64)
        if L.wsmc_diag_block_clocks(kind, buf.ctypes.data_as(C.c_void_p), MAX_BLOCKS) != 0:
            raise SystemExit("could not read the block clocks")
        ran = buf[buf[:, 1] != 0]
        out = {"kernel": name, "particles": a.particles, "steps": a.steps, "ess": a.ess}
        out.update(rounds(ran) if len(ran) else {"blocks": 0})
        print(json.dumps(out), flush=True)
    g.close()


if __name__ == "__main__":
    main()

"""The shared-impulse FIR path on the north-star shape with ONE impulse bank: 4096 chains x (16 biquads + 4096 taps),
DSP_FORMAT 6, every chain's DSP_FIR pointing at the same bank.

Times device-resident blocks of 64 / 128 / 256 / 1024 frames with "fir_shared" 1 and 0 ALTERNATED in one process (the same runtime, the
option flipped between rounds), each block call bracketed by device events on the caller's stream (median of `--steps` calls per
round), and prints the device memory the program holds either way (a fresh runtime each, hipMemGetInfo before / after its first
block).  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (`--quick`: one round, fewer steps).
One JSON line at the end.

    python tools/fir_shared_bench.py [--steps 50] [--rounds 3] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avdsp_amd import progbuilder as pb      # noqa: E402
from avdsp_amd import runtime as rt          # noqa: E402

C, S, T = 4096, 16, 4096
BLOCKS = (64, 128, 256, 1024)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--blocks", type=str, default=",".join(map(str, BLOCKS)), help="block lengths, comma-separated")
    ap.add_argument("--no-memory", action="store_true", help="skip the device-memory figures")
    ap.add_argument("--fir-rows", type=int, default=0, help='"fir_rows": row tiles of fir_tile AND fir_shared (0: by the launch rule)')
    a = ap.parse_args()
    blocks = [int(v) for v in a.blocks.split(",")]
    if a.quick:
        a.steps, a.rounds = 10, 1
    import torch
    from avdsp_amd import devmem as dm
    prog = pb.synth_program(6, C, S, T, fir_banks=1)
    x = pb.lcg_input(max(blocks), C, True, seed=3)
    xd = dm.to_device(x)
    yd = torch.zeros_like(xd)
    st = torch.cuda.current_stream().cuda_stream

    mem = {}
    for shared in (() if a.no_memory else (1, 0)):      # device memory of the program either way
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        r = rt.Runtime(6, prog)
        r.set_option("fir_shared", shared)
        r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, 64, st)
        torch.cuda.synchronize()
        mem[shared] = (free0 - torch.cuda.mem_get_info()[0]) / 1e6
        r.release()

    r = rt.Runtime(6, prog)
    r.set_option("fir_rows", a.fir_rows)
    res = {B: {1: [], 0: []} for B in blocks}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for _ in range(a.rounds):
        for B in blocks:
            for shared in (1, 0):
                r.set_option("fir_shared", shared)
                for _w in range(3):
                    r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                for e0, e1 in ev:
                    e0.record()
                    r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                    e1.record()
                torch.cuda.synchronize()
                assert r.get_option("fir_shared_chains") == (C if shared else 0)
                res[B][shared].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    r.release()
    out = {"program": f"{C} chains x ({S} biquads + {T} taps), one bank, format 6", "steps": a.steps, "rounds": a.rounds,
           "us_per_block": {}, "device_mb": {f"fir_shared_{k}": round(v, 1) for k, v in mem.items()}}
    for B in blocks:
        on, off = min(res[B][1]), min(res[B][0])
        out["us_per_block"][str(B)] = {"fir_shared_1": round(on, 1), "fir_shared_0": round(off, 1), "rounds_1": [round(v, 1) for v in res[B][1]],
                                      "rounds_0": [round(v, 1) for v in res[B][0]]}
        print(f"{B:5d} frames: fir_shared 1 {on:8.1f} us   0 {off:8.1f} us   ({off / on:.2f}x)")
    if mem:
        print(f"device memory: fir_shared 1 {mem[1]:.1f} MB, 0 {mem[0]:.1f} MB")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

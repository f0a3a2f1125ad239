"""Dressed finishes on the chain kernels against the interpreter ("chain_finish" 1 / 0): microseconds per
device-resident block of the REWgenericEQ shape at scale,

    TPDF_CALC;  4096 x (LOAD_GAIN -> 16 biquads -> SAT0DB_TPDF -> STORE)

in DSP_FORMAT 2, 4 and 6 at blocks of 1024 and 256 frames.  One process, one loaded program per format; the two settings alternate
(`--rounds` times: set the option, two warm-up calls that also make the plans, then `--steps` calls each bracketed by device events on
the caller's stream), and a setting's figure is the median over all its timed calls.  One JSON line at the end.

    python tools/finish_bench.py [--steps 20] [--rounds 3] [--formats 2,4,6] [--blocks 1024,256] [--chains 4096] [--sections 16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avdsp_amd import encoder as enc         # noqa: E402
from avdsp_amd import progbuilder as pb      # noqa: E402
from avdsp_amd import runtime as rt          # noqa: E402

FPEAK, F48000 = 74, 5


def eq_program(fmt: int, chains: int, sections: int):
    """inputs at IO chains .., outputs at IO 0 .."""
    def build(L):
        banks = []
        for c in range(chains):
            if c % 256 == 0:
                L.dsp_PARAM()                            # (a PARAM section holds 65535 words at the most)
            banks.append(L.dspBiquad_Sections(sections))
            for k in range(sections):
                L.dsp_Filter2ndOrder(FPEAK, 60.0 + 3.0 * (c % 500) + 900.0 * k, 0.9, 1.02 if k % 2 else 0.97)
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for c in range(chains):
            L.dsp_LOAD_GAIN_Fixed(chains + c, 0.5)
            L.dsp_BIQUADS(banks[c])
            L.dsp_SAT0DB_TPDF()
            L.dsp_STORE(c)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=2 * chains, capacity=chains * (sections * 8 + 16) + 4096)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="2,4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--sections", type=int, default=16)
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    C = a.chains
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            r = rt.Runtime(fmt, eq_program(fmt, C, a.sections), fs=48000, random=1, dither=24)
            xd = dm.to_device(pb.lcg_input(max(blocks), C, fmt == 6, seed=3))
            yd = torch.zeros_like(xd)
            for B in blocks:
                us = {0: [], 1: []}
                chains = {}
                for _ in range(a.rounds):
                    for opt in (0, 1):
                        r.set_option("chain_finish", opt)
                        chains[opt] = r.core_info()["chains"]
                        for _ in range(2):
                            r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                        torch.cuda.synchronize()
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                        for e0, e1 in ev:
                            e0.record()
                            r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                            e1.record()
                        torch.cuda.synchronize()
                        us[opt] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                m0, m1 = statistics.median(us[0]), statistics.median(us[1])
                lines.append(dict(format=fmt, chains=C, sections=a.sections, block=B,
                                  chain_finish_0_us=round(m0, 1), chain_finish_1_us=round(m1, 1),
                                  chain_finish_0_gsamples_s=round(C * B / m0 / 1e3, 2), chain_finish_1_gsamples_s=round(C * B / m1 / 1e3, 2),
                                  lowered_chains={str(k): v for k, v in chains.items()}, calls_per_setting=len(us[0])))
                print(lines[-1], flush=True)
            r.release()
            del xd, yd
    finally:
        rt.Runtime.set_global_option("chain_finish", 0)
    print(json.dumps(dict(tool="finish_bench", lines=lines)))


if __name__ == "__main__":
    main()

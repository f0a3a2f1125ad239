"""Delay lines on the chain kernels against the interpreter ("chain_delay" 1 / 0): microseconds per device-resident
block of the reference's crossover shape at scale,

    TPDF_CALC;  4096 x (LOAD_GAIN -> 16 biquads -> DELAY 1000 us -> SAT0DB_TPDF_GAIN -> STORE)

with "chain_finish" 1, in DSP_FORMAT 2, 4 and 6 at blocks of 1024 and 256 frames -- and the same program WITHOUT the DELAY opcode
under "chain_finish" 1: the difference to "chain_delay" 1 is what the hand-over block and chain_tail cost.  One process, two loaded
programs per format; the three settings alternate (`--rounds` times: select, two warm-up calls that also make the plans, then `--steps`
calls each bracketed by device events on the caller's stream), and a setting's figure is the median over all its timed calls.  One
JSON line at the end.

    python tools/delay_bench.py [--steps 20] [--rounds 3] [--formats 2,4,6] [--blocks 1024,256] [--chains 4096] [--sections 16] [--us 1000]
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


def crossover_program(fmt: int, chains: int, sections: int, us: int):
    """inputs at IO chains .., outputs at IO 0 ..; us 0: no DELAY opcode"""
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
            if us:
                L.dsp_DELAY_FixedMicroSec(us)
            L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
            L.dsp_STORE(c)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=2 * chains, capacity=chains * (sections * 8 + 24) + 4096)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="2,4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--sections", type=int, default=16)
    ap.add_argument("--us", type=int, default=1000)
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    from ctypes import c_float
    enc.lib().dsp_SAT0DB_TPDF_GAIN_Fixed.argtypes = [c_float]
    C = a.chains
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            delayed = rt.Runtime(fmt, crossover_program(fmt, C, a.sections, a.us), fs=48000, random=1, dither=24)
            plain = rt.Runtime(fmt, crossover_program(fmt, C, a.sections, 0), fs=48000, random=1, dither=24)
            for r in (delayed, plain):
                r.set_option("chain_finish", 1)
            xd = dm.to_device(pb.lcg_input(max(blocks), C, fmt == 6, seed=3))
            yd = torch.zeros_like(xd)
            settings = (("chain_delay_0", delayed, 0), ("chain_delay_1", delayed, 1), ("no_delay", plain, 0))
            for B in blocks:
                us = {name: [] for name, _, _ in settings}
                chains = {}
                for _ in range(a.rounds):
                    for name, r, opt in settings:
                        r.set_option("chain_delay", opt)
                        chains[name] = r.core_info()["chains"]
                        for _ in range(2):
                            r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                        torch.cuda.synchronize()
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                        for e0, e1 in ev:
                            e0.record()
                            r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                            e1.record()
                        torch.cuda.synchronize()
                        us[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                med = {name: statistics.median(v) for name, v in us.items()}
                lines.append(dict(format=fmt, chains=C, sections=a.sections, block=B, delay_us=a.us, delay_samples=delayed.delay_info()[1],
                                  **{f"{name}_us": round(m, 1) for name, m in med.items()},
                                  **{f"{name}_min_us": round(min(us[name]), 1) for name in us},
                                  tail_and_hand_over_us=round(med["chain_delay_1"] - med["no_delay"], 1),
                                  lowered_chains=chains, calls_per_setting=len(us["no_delay"])))
                print(lines[-1], flush=True)
            delayed.release()
            plain.release()
            del xd, yd
    finally:
        rt.Runtime.set_global_option("chain_delay", 0)
        rt.Runtime.set_global_option("chain_finish", 0)
    print(json.dumps(dict(tool="delay_bench", lines=lines)))


if __name__ == "__main__":
    main()

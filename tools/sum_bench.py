"""Sum heads on the chain kernels against the interpreter ("chain_sum" 1 / 0): microseconds per device-resident block of
the reference's crossover2x2lfe core at scale,

    TPDF_CALC;  1024 x ( 2 x ( LOAD_GAIN, 6 biquads, STORE_MEM )                                                the prefilter trunks
                         2 x ( LOAD_GAIN, COPYXY, 4 biquads, SAT0DB_TPDF, DELAY, STORE,
                               SWAPXY, 4 biquads, GAIN, SAT0DB_TPDF_GAIN, STORE )                               the two-way forks
                         LOAD_MEM, LOAD_MEM, ADDXY, 4 biquads, SAT0DB, DELAY, STORE )                           the LFE bus

7168 chains, with "chain_mem", "chain_finish", "chain_delay" and "chain_ways" 1, in DSP_FORMAT 2, 4 and 6 at blocks of 1024 and 256
frames.  Three settings: "chain_sum" 1; "chain_sum" 0, where the one LFE chain of each group sends the whole core to the interpreter;
and the same program without the LFE chains, which the chain kernels take without the option -- what the buses cost on top.  One
process, two loaded programs per format; the settings alternate (`--rounds` times: select, a first call that also makes the plans, a
warm-up call, then `--steps` calls each bracketed by device events on the caller's stream), and a setting's figure is the median over
all its timed calls.  A setting whose first call lasts more than `--slow-ms` is measured by that one call and left out of the later
rounds; every line says how many calls stand behind each figure.  One JSON line at the end.

    python tools/sum_bench.py [--steps 20] [--rounds 3] [--formats 2,4,6] [--blocks 1024,256] [--groups 1024] [--us 294]
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
OPTIONS = ("chain_mem", "chain_finish", "chain_delay", "chain_ways")


def bank(L, sections, c):
    b = L.dspBiquad_Sections(sections)
    for k in range(sections):
        L.dsp_Filter2ndOrder(FPEAK, 60.0 + 3.0 * (c % 500) + 900.0 * (k % 16), 0.9, 1.02 if k % 2 else 0.97)
    return b


def lfe_program(fmt: int, groups: int, us: int, lfe: bool = True):
    """inputs at IO 5 * groups .. (two per group), outputs at IO 0 .. (five per group, the fifth the LFE bus's)"""
    nout = 5 * groups

    def build(L):
        banks, mems = [], []
        for g in range(groups):
            if g % 32 == 0:
                L.dsp_PARAM()                                # (a PARAM section holds 65535 words at the most)
            mems.append((L.dspMem_Location(), L.dspMem_Location()))
            banks.append([bank(L, n, 7 * g + j) for j, n in enumerate((6, 6, 4, 4, 4, 4, 4))])
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for g in range(groups):
            b, io = banks[g], nout + 2 * g
            for s in range(2):
                L.dsp_LOAD_GAIN_Fixed(io + s, 1.0)
                L.dsp_BIQUADS(b[s])
                L.dsp_STORE_MEM(mems[g][s])
            for s in range(2):
                L.dsp_LOAD_GAIN_Fixed(io + s, 1.0)
                L.dsp_COPYXY()
                L.dsp_BIQUADS(b[2 + 2 * s])
                L.dsp_SAT0DB_TPDF()
                L.dsp_DELAY_FixedMicroSec(us)
                L.dsp_STORE(5 * g + 2 * s)
                L.dsp_SWAPXY()
                L.dsp_BIQUADS(b[3 + 2 * s])
                L.dsp_GAIN_Fixed(0.8)
                L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.8)
                L.dsp_STORE(5 * g + 2 * s + 1)
            if lfe:
                L.dsp_LOAD_MEM(mems[g][0])
                L.dsp_LOAD_MEM(mems[g][1])
                L.dsp_ADDXY()
                L.dsp_BIQUADS(b[6])
                L.dsp_SAT0DB()
                L.dsp_DELAY_FixedMicroSec(us)
                L.dsp_STORE(5 * g + 4)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=nout + 2 * groups, capacity=groups * 1024 + 8192)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="2,4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--us", type=int, default=294)
    ap.add_argument("--slow-ms", type=float, default=2000.0)
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    from ctypes import c_float, c_int
    L = enc.lib()
    L.dsp_SAT0DB_TPDF_GAIN_Fixed.argtypes = [c_float]
    L.dsp_LOAD_MEM.argtypes = [c_int]
    L.dsp_STORE_MEM.argtypes = [c_int]
    G = a.groups
    nin, nout = 2 * G, 5 * G
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            full = rt.Runtime(fmt, lfe_program(fmt, G, a.us), fs=48000, random=1, dither=24)
            bare = rt.Runtime(fmt, lfe_program(fmt, G, a.us, lfe=False), fs=48000, random=1, dither=24)
            for r in (full, bare):
                for key in OPTIONS:
                    r.set_option(key, 1)
            xd = dm.to_device(pb.lcg_input(max(blocks), nin, fmt == 6, seed=3))
            yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
            settings = (("chain_sum_1", full, 1), ("no_lfe", bare, 1), ("chain_sum_0", full, 0))

            def call(r, B):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r.run_block_device(xd.data_ptr(), nin, nout, yd.data_ptr(), nout, 0, B, st)
                e1.record()
                return e0, e1
            for B in blocks:
                us = {name: [] for name, _, _ in settings}
                chains, slow, info = {}, set(), None
                for _ in range(a.rounds):
                    for name, r, opt in settings:
                        if name in slow:
                            continue
                        r.set_option("chain_sum", opt)
                        chains[name] = r.core_info()["chains"]
                        if name == "chain_sum_1":
                            info = r.sum_info()
                        # the first call also makes the plans: a setting whose first call lasts more than --slow-ms (the interpreter on a
                        # core with memory words) is measured by that one call and left out of the later rounds
                        w0, w1 = call(r, B)
                        torch.cuda.synchronize()
                        if w0.elapsed_time(w1) > a.slow_ms:
                            slow.add(name)
                            us[name].append(w0.elapsed_time(w1) * 1e3)
                            print(f"# format {fmt} block {B} {name}: one call of {us[name][0] / 1e6:.2f} s", flush=True)
                            continue
                        call(r, B)
                        ev = [call(r, B) for _ in range(a.steps)]
                        torch.cuda.synchronize()
                        us[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                        print(f"# format {fmt} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                med = {name: statistics.median(v) for name, v in us.items()}
                lines.append(dict(format=fmt, groups=G, block=B, delay_us=a.us,
                                  **{f"{name}_us": round(m, 1) for name, m in med.items()},
                                  **{f"{name}_min_us": round(min(us[name]), 1) for name in us},
                                  over_no_lfe=round(med["chain_sum_1"] / med["no_lfe"], 3), speedup=round(med["chain_sum_0"] / med["chain_sum_1"], 2),
                                  sum_info=info, lowered_chains=chains, calls={name: len(v) for name, v in us.items()}))
                print(lines[-1], flush=True)
            full.release()
            bare.release()
            del xd, yd
    finally:
        for key in OPTIONS + ("chain_sum",):
            rt.Runtime.set_global_option(key, 0)
    print(json.dumps(dict(tool="sum_bench", lines=lines)))


if __name__ == "__main__":
    main()

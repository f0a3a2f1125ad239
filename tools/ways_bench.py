"""Two-way forks on the chain kernels against the interpreter ("chain_ways" 1 / 0): microseconds per device-resident block
of the two-way crossover at scale,

    TPDF_CALC;  2048 x ( LOAD_GAIN, COPYXY, 8 biquads, SAT0DB_TPDF, DELAY 1000 us, STORE,
                         SWAPXY, 8 biquads, GAIN, SAT0DB_TPDF_GAIN, STORE )                                     4096 ways

with "chain_finish" 1 and "chain_delay" 1, in DSP_FORMAT 2, 4 and 6 at blocks of 1024 and 256 frames -- and the floor: the same program
without the GAIN, written as 4096 independent chains (each way with a LOAD_GAIN of its own), which the chain kernels take without the
option.  The floor is NOT the same program (no GAIN): it stands for the cost of the work a fork should add nothing to.  One process,
two loaded programs per format; the three settings alternate (`--rounds` times: select, two warm-up calls that also make the plans,
then `--steps` calls each bracketed by device events on the caller's stream), and a setting's figure is the median over all its timed
calls.  A setting whose second warm-up call lasts more than `--slow-ms` is measured by that one call and left out of the later rounds;
every line says how many calls stand behind each figure.  One JSON line at the end.

    python tools/ways_bench.py [--steps 20] [--rounds 3] [--formats 2,4,6] [--blocks 1024,256] [--forks 2048] [--sections 8] [--us 1000]
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


def filters(L, sections, c):
    for k in range(sections):
        L.dsp_Filter2ndOrder(FPEAK, 60.0 + 3.0 * (c % 500) + 900.0 * (k % 16), 0.9, 1.02 if k % 2 else 0.97)


def banks_of(L, n, sections):
    banks = []
    for c in range(n):
        if c % 128 == 0:
            L.dsp_PARAM()                                # (a PARAM section holds 65535 words at the most)
        banks.append(L.dspBiquad_Sections(sections))
        filters(L, sections, c)
    return banks


def fork_program(fmt: int, forks: int, sections: int, us: int):
    """inputs at IO 2 * forks .., outputs at IO 0 ..: way A of fork f stores IO 2 f, way B IO 2 f + 1"""
    nout = 2 * forks

    def build(L):
        banks = banks_of(L, nout, sections)
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for f in range(forks):
            L.dsp_LOAD_GAIN_Fixed(nout + f, 0.5)
            L.dsp_COPYXY()
            L.dsp_BIQUADS(banks[2 * f])
            L.dsp_SAT0DB_TPDF()
            L.dsp_DELAY_FixedMicroSec(us)
            L.dsp_STORE(2 * f)
            L.dsp_SWAPXY()
            L.dsp_BIQUADS(banks[2 * f + 1])
            L.dsp_GAIN_Fixed(0.7)
            L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
            L.dsp_STORE(2 * f + 1)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=nout + forks, capacity=nout * (sections * 8 + 48) + 4096)


def floor_program(fmt: int, forks: int, sections: int, us: int):
    """the same inputs, outputs and banks; every way a chain of its own, no GAIN"""
    nout = 2 * forks

    def build(L):
        banks = banks_of(L, nout, sections)
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for f in range(forks):
            L.dsp_LOAD_GAIN_Fixed(nout + f, 0.5)
            L.dsp_BIQUADS(banks[2 * f])
            L.dsp_SAT0DB_TPDF()
            L.dsp_DELAY_FixedMicroSec(us)
            L.dsp_STORE(2 * f)
            L.dsp_LOAD_GAIN_Fixed(nout + f, 0.5)
            L.dsp_BIQUADS(banks[2 * f + 1])
            L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
            L.dsp_STORE(2 * f + 1)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=nout + forks, capacity=nout * (sections * 8 + 48) + 4096)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="2,4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--forks", type=int, default=2048)
    ap.add_argument("--sections", type=int, default=8)
    ap.add_argument("--us", type=int, default=1000)
    ap.add_argument("--slow-ms", type=float, default=20.0)
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    from ctypes import c_float
    enc.lib().dsp_SAT0DB_TPDF_GAIN_Fixed.argtypes = [c_float]
    F = a.forks
    nout = 2 * F
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            fork = rt.Runtime(fmt, fork_program(fmt, F, a.sections, a.us), fs=48000, random=1, dither=24)
            flat = rt.Runtime(fmt, floor_program(fmt, F, a.sections, a.us), fs=48000, random=1, dither=24)
            for r in (fork, flat):
                r.set_option("chain_finish", 1)
                r.set_option("chain_delay", 1)
            xd = dm.to_device(pb.lcg_input(max(blocks), F, fmt == 6, seed=3))
            yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
            settings = (("chain_ways_1", fork, 1), ("floor", flat, 0), ("chain_ways_0", fork, 0))
            for B in blocks:
                us = {name: [] for name, _, _ in settings}
                chains, slow, info = {}, set(), None
                for _ in range(a.rounds):
                    for name, r, opt in settings:
                        if name in slow:
                            continue
                        r.set_option("chain_ways", opt)
                        chains[name] = r.core_info()["chains"]
                        if name == "chain_ways_1":
                            info = r.ways_info()
                        # two warm-up calls that also make the plans; the second is timed: a setting whose call lasts more than
                        # --slow-ms is measured by that one call and left out of the later rounds
                        r.run_block_device(xd.data_ptr(), F, nout, yd.data_ptr(), nout, 0, B, st)
                        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        w0.record()
                        r.run_block_device(xd.data_ptr(), F, nout, yd.data_ptr(), nout, 0, B, st)
                        w1.record()
                        torch.cuda.synchronize()
                        if w0.elapsed_time(w1) > a.slow_ms:
                            slow.add(name)
                            us[name].append(w0.elapsed_time(w1) * 1e3)
                            print(f"# format {fmt} block {B} {name}: one call of {us[name][0] / 1e6:.2f} s", flush=True)
                            continue
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                        for e0, e1 in ev:
                            e0.record()
                            r.run_block_device(xd.data_ptr(), F, nout, yd.data_ptr(), nout, 0, B, st)
                            e1.record()
                        torch.cuda.synchronize()
                        us[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                        print(f"# format {fmt} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                med = {name: statistics.median(v) for name, v in us.items()}
                lines.append(dict(format=fmt, forks=F, sections=a.sections, block=B, delay_us=a.us,
                                  **{f"{name}_us": round(m, 1) for name, m in med.items()},
                                  **{f"{name}_min_us": round(min(us[name]), 1) for name in us},
                                  over_floor=round(med["chain_ways_1"] / med["floor"], 3), speedup=round(med["chain_ways_0"] / med["chain_ways_1"], 2),
                                  ways_info=info, lowered_chains=chains, calls={name: len(v) for name, v in us.items()}))
                print(lines[-1], flush=True)
            fork.release()
            flat.release()
            del xd, yd
    finally:
        for key in ("chain_ways", "chain_delay", "chain_finish"):
            rt.Runtime.set_global_option(key, 0)
    print(json.dumps(dict(tool="ways_bench", lines=lines)))


if __name__ == "__main__":
    main()

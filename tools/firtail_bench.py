"""Handed FIR chains against the interpreter ("fir_tail" 1 / 0): microseconds per device-resident block of a convolution
channel written the way the reference's programs end their channels,

    TPDF_CALC;  C x (LOAD_GAIN -> 16 biquads -> FIR of T taps -> DELAY 1000 us -> SAT0DB_TPDF_GAIN -> STORE)

with "chain_finish" 1 and "chain_delay" 1, in DSP_FORMAT 4 and 6 at blocks of 1024 and 256 frames.

  --mode compare   "fir_tail" 0 (the interpreter) and 1 alternate in one process (`--rounds` times: two warm-up calls that also make the
                   plans, then up to `--steps` calls each bracketed by device events on the caller's stream; a setting whose calls have
                   taken `--budget-ms` in a round stops that round early, after three calls at the least -- the interpreter's blocks are
                   long); a setting's figure is the median over all its timed calls.
                   --root DIR takes the package (and its library) of ANOTHER checkout, e.g. the parent commit's, which knows no
                   "fir_tail": then only the setting "parent" is measured, in this process of its own.
  --mode overhead  the same program against its plain twin (SAT0DB, no DELAY: fir_tile stores itself) at the north-star shape: the
                   difference is what the hand-over block and chain_tail cost.  With --timers the kernel timers (dspRuntimeKernelTime) of
                   a further run of each say where it goes.

One JSON line at the end.

    python tools/firtail_bench.py --mode compare [--chains 1024] [--taps 1024] [--formats 4,6] [--blocks 1024,256] [--steps 20] [--rounds 3]
    python tools/firtail_bench.py --mode overhead [--chains 4096] [--taps 4096] [--blocks 1024] [--timers]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

from avdsp_amd import progbuilder as pb      # noqa: E402
from avdsp_amd import runtime as rt          # noqa: E402



OP_TPDF_CALC, OP_SAT0DB_TPDF_GAIN, OP_DELAY = 7, 45, 47
FACTOR_48000 = 206158430                     # (unsigned)(2^32 / 10^6 x 48000): samples = us x factor >> 32


def channel_program(fmt: int, chains: int, sections: int, taps: int, us: int, dressed: bool):
    """inputs at IO chains .., outputs at IO 0 ..; every chain has a bank and an impulse of its own, in a PARAM of its own (the
    layout of progbuilder.synth_program, written with its ProgramWriter: the encoder's dsp_FIR keeps a region's end in 16 bits and
    cannot address an impulse beyond the first 65535 words).  dressed False: the plain twin -- SAT0DB, no DELAY"""
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + chains * (16 + sections * 8 + 8 + taps + 3 + 8 + 24))
    h = pb.lcg_taps_all(chains, taps)
    pw.core()
    pw._head(OP_TPDF_CALC, 3)                                  # dsp_TPDF_CALC(0): the default width, an 8-byte result word
    pw._w(0)
    pw._w(pw._data_aligned8(2))
    for c in range(chains):
        pw.param()
        bank = pw.biquad_bank(pb.synth_sections(c, sections, pb.F48000, pb.F48000))
        imp = pw.fir_impulses([h[c]])
        pw.load_gain_fixed(chains + c, 0.5)
        pw.biquads(bank, sections)
        pw.fir(imp, taps)
        if dressed:
            pw._head(OP_DELAY, 4)                              # dsp_DELAY_FixedMicroSec(us): [us, line, no parameter]
            pw._w(us)
            pw._w(pw.data_counter)
            pw.data_counter += 1 + ((us * FACTOR_48000) >> 32)
            pw._w(0)
            pw._head(OP_SAT0DB_TPDF_GAIN, 3)                   # dsp_SAT0DB_TPDF_GAIN_Fixed(0.9): the gain behind the opcode
            pw._w(2)
            pw._param_value(0.9)
        else:
            pw.sat0db()
        pw.store(c)
    return pw.end_of_code()


def timed_calls(r, torch, xd, yd, C, B, st, steps, budget_ms):
    for _ in range(2):
        r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
    torch.cuda.synchronize()
    out, spent = [], 0.0
    while len(out) < steps and (len(out) < 3 or spent < budget_ms):
        n = 1 if spent / max(len(out), 1) > 5.0 else min(10, steps - len(out))       # (long blocks one by one)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        out += [m * 1e3 for m in ms]
        spent += sum(ms)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("compare", "overhead"), default="compare")
    ap.add_argument("--root", type=str, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--budget-ms", type=float, default=1500.0)
    ap.add_argument("--formats", type=str, default="4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--taps", type=int, default=None)
    ap.add_argument("--sections", type=int, default=16)
    ap.add_argument("--us", type=int, default=1000)
    ap.add_argument("--timers", action="store_true")
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    overhead = a.mode == "overhead"
    C = a.chains or (4096 if overhead else 1024)
    T = a.taps or (4096 if overhead else 1024)
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    has_tail = hasattr(rt.Runtime, "fir_tail_info")
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            dressed = rt.Runtime(fmt, channel_program(fmt, C, a.sections, T, a.us, True), fs=48000, random=1, dither=24)
            dressed.set_option("chain_finish", 1)
            dressed.set_option("chain_delay", 1)
            plain = rt.Runtime(fmt, channel_program(fmt, C, a.sections, T, a.us, False), fs=48000, random=1, dither=24) if overhead else None
            xd = dm.to_device(pb.lcg_input(max(blocks), C, fmt == 6, seed=3))
            yd = torch.zeros_like(xd)
            if overhead:
                settings = (("fir_tail_1", dressed, 1), ("plain_twin", plain, None))
            elif has_tail:
                settings = (("fir_tail_0", dressed, 0), ("fir_tail_1", dressed, 1))
            else:
                settings = (("parent", dressed, None),)
            for B in blocks:
                us = {name: [] for name, _, _ in settings}
                chains, handed = {}, {}
                for _ in range(a.rounds):
                    for name, r, opt in settings:
                        if opt is not None:
                            r.set_option("fir_tail", opt)
                        chains[name] = r.core_info()["chains"]
                        handed[name] = r.fir_tail_info()[0] if has_tail else 0
                        us[name] += timed_calls(r, torch, xd, yd, C, B, st, a.steps, a.budget_ms)
                line = dict(mode=a.mode, format=fmt, chains=C, sections=a.sections, taps=T, block=B, delay_us=a.us,
                            **{f"{name}_us": round(statistics.median(v), 1) for name, v in us.items()},
                            **{f"{name}_min_us": round(min(v), 1) for name, v in us.items()},
                            **{f"{name}_calls": len(v) for name, v in us.items()},
                            lowered_chains=chains, handed_chains=handed)
                if overhead:
                    line["tail_and_hand_over_us"] = round(statistics.median(us["fir_tail_1"]) - statistics.median(us["plain_twin"]), 1)
                    if a.timers:
                        for name, r, _ in settings:
                            r.set_option("profile", 1)
                            for _ in range(2):
                                r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                            torch.cuda.synchronize()
                            for kind in range(3):
                                r.kernel_time(kind)
                            for _ in range(a.steps):
                                r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, B, st)
                            torch.cuda.synchronize()
                            for kind, what in ((0, "cascade"), (1, "fir"), (2, "pass_and_tail")):
                                ms, n = r.kernel_time(kind)
                                line[f"{name}_{what}_us_per_launch"] = round(ms * 1e3 / max(n, 1), 1)
                                line[f"{name}_{what}_launches"] = n
                            r.set_option("profile", 0)
                elif has_tail:
                    line["speedup"] = round(statistics.median(us["fir_tail_0"]) / statistics.median(us["fir_tail_1"]), 2)
                lines.append(line)
                print(line, flush=True)
            dressed.release()
            if plain is not None:
                plain.release()
            del xd, yd
    finally:
        for key in ("fir_tail",) if has_tail else ():
            rt.Runtime.set_global_option(key, 0)
        rt.Runtime.set_global_option("chain_delay", 0)
        rt.Runtime.set_global_option("chain_finish", 0)
    print(json.dumps(dict(tool="firtail_bench", lines=lines)))


if __name__ == "__main__":
    main()

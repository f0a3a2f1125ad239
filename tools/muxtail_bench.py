"""Dressed finishes and delay lines behind LOAD_MUX heads on the chain kernels against the interpreter ("mux_tail" 1 / 0, DESIGN.md
4.2i): microseconds per device-resident block of the array shape,

    TPDF_CALC;  O x (LOAD_MUX of I inputs -> 16 biquads -> DELAY 1000 us -> SAT0DB_TPDF_GAIN -> STORE)

with "chain_finish" 1 and "chain_delay" 1, in DSP_FORMAT 2, 4 and 6 at blocks of 1024 and 256 frames.

  (a) a ladder of shapes O x I from 64 x 8 up, "mux_tail" 1 against 0 alternating in one process.  Where an interpreter block would take
      more than 5 s a 64-frame call is measured and scaled (`est` 1 in its line: an estimate, to be quoted as one); once a block is
      estimated at more than `--give-up` seconds the interpreter is not run on the larger shapes at all.  A library from before the
      option runs the same programs on the interpreter: `--parent` (with AVDSP_LIB naming that library, in a process of its own)
      measures it -- the option is then never set.
  (b) at the last shape of the ladder, the step under "mux_tail" 1 beside two plain twins -- the same program without the mixer (LOAD_GAIN
      heads: 4.2g's program) and the same program ending in a plain SAT0DB without the delay (4.2e's program) -- and the kernel timers
      (dspRuntimeKernelTime) of a further 20 blocks each: the stage (kind 7), the cascades (0), chain_tail and passthrough (2),
      dither_block (3).
  (c) sectionless chains only, LOAD_MUX -> DELAY -> SAT0DB_TPDF -> STORE: what the stage's hand-over stores cost, with shared lists
      (mux_tile) and with private lists (mux_plain), beside the same chains without the delay (which the stage finishes itself).

Every call between two device events on the caller's stream, the settings alternating (`--rounds` times `--steps` calls each), medians.
Raw lines go to profiles/muxtail_bench.txt (appended), one JSON line at the end.

    python tools/muxtail_bench.py [--parts a,b,c] [--steps 20] [--rounds 3] [--formats 2,4,6] [--blocks 1024,256] [--ladder 64x8,256x16,1024x32,4096x64] [--parent]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avdsp_amd import encoder as enc         # noqa: E402
from avdsp_amd import progbuilder as pb      # noqa: E402
from avdsp_amd import runtime as rt          # noqa: E402

FPEAK, F48000 = 74, 5
PROBE, SLOW_S = 64, 5.0
KINDS = (("cascade_us", 0), ("tail_and_pass_us", 2), ("dither_us", 3), ("mux_us", 7))


def array_program(fmt, O, I, sections=16, us=1000, finish="tpdf_gain", mux="shared"):
    """inputs at IO O .., outputs at IO 0 ..; mux: "shared" (every list names the I inputs in order: one mix group), "private" (8 of
    them, drawn per chain), None (LOAD_GAIN of input o % I); us 0: no DELAY opcode; finish: "tpdf_gain", "tpdf" or "sat" """
    import numpy as np
    rng = np.random.default_rng(7)
    per_chain = (2 * I + 4 if mux else 0) + sections * 8 + 16

    def build(L):
        banks, tables = [], []
        for o in range(O):
            if o % max(1, 40000 // per_chain) == 0:
                L.dsp_PARAM()                            # (a PARAM section holds 65535 words at the most)
            if mux:
                ios = range(I) if mux == "shared" else [int(v) for v in rng.integers(0, I, 8)]
                tables.append(L.dspLoadMux_Inputs(len(ios)))
                for io in ios:
                    L.dspLoadMux_Data(O + io, float(rng.uniform(-1.0, 1.0)) / I ** 0.5)
            if sections:
                banks.append(L.dspBiquad_Sections(sections))
                for k in range(sections):
                    L.dsp_Filter2ndOrder(FPEAK, 60.0 + 3.0 * (o % 500) + 900.0 * k, 0.9, 1.02 if k % 2 else 0.97)
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for o in range(O):
            if mux:
                L.dsp_LOAD_MUX(tables[o])
            else:
                L.dsp_LOAD_GAIN_Fixed(O + o % I, 0.5)
            if sections:
                L.dsp_BIQUADS(banks[o])
            if us:
                L.dsp_DELAY_FixedMicroSec(us)
            if finish == "tpdf_gain":
                L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
            elif finish == "tpdf":
                L.dsp_SAT0DB_TPDF()
            else:
                L.dsp_SAT0DB()
            L.dsp_STORE(o)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=O + I, capacity=O * (per_chain + 16) + 4096)


class Bench:
    def __init__(self, steps, rounds):
        import torch
        from avdsp_amd import devmem as dm
        self.torch, self.dm, self.steps, self.rounds = torch, dm, steps, rounds
        self.st = torch.cuda.current_stream().cuda_stream

    def buffers(self, fmt, frames, I, O):
        xd = self.dm.to_device(pb.lcg_input(frames, I, fmt == 6, seed=3))
        yd = self.torch.zeros((frames, O), dtype=xd.dtype, device="cuda")
        return xd, yd

    def call(self, r, xd, yd, B):
        r.run_block_device(xd.data_ptr(), xd.shape[1], yd.shape[1], yd.data_ptr(), yd.shape[1], 0, B, self.st)

    def wall(self, r, xd, yd, B):
        t0 = time.time()
        self.call(r, xd, yd, B)
        self.torch.cuda.synchronize()
        return time.time() - t0

    def timed(self, r, xd, yd, B, n):
        ev = [(self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            self.call(r, xd, yd, B)
            e1.record()
        self.torch.cuda.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]

    def alternate(self, settings, xd, yd, B):
        """settings: (name, runtime, options to set first).  -> {name: dict(us, min_us, calls, est, chains)}; a setting whose block is
        estimated over SLOW_S from a PROBE-frame call is not run whole"""
        us = {name: [] for name, _, _ in settings}
        info = {}
        for _ in range(self.rounds):
            for name, r, opts in settings:
                if info.get(name, {}).get("est") or info.get(name, {}).get("slow"):      # (an interpreter block of seconds: one round)
                    continue
                for k, v in opts:
                    r.set_option(k, v)
                try:
                    chains = r.core_info()["chains"]
                except rt.AvdspError:
                    chains = 0
                self.wall(r, xd, yd, min(PROBE, B))                  # (with the plan's making)
                probe = self.wall(r, xd, yd, min(PROBE, B))
                if probe * B / min(PROBE, B) > SLOW_S:
                    info[name] = dict(us=round(probe * B / min(PROBE, B) * 1e6, 1), est=1, calls=0, chains=chains)
                    continue
                one = self.wall(r, xd, yd, B)
                n = max(3, min(self.steps, int(2.0 / max(one, 1e-6))))
                us[name] += self.timed(r, xd, yd, B, n)
                info[name] = dict(est=0, chains=chains, slow=int(one > 0.3))
        for name, v in us.items():
            if v:
                info[name].update(us=round(statistics.median(v), 1), min_us=round(min(v), 1), calls=len(v))
        return info

    def kernel_times(self, r, xd, yd, B, n=20):
        r.set_option("profile", 1)
        try:
            for _, k in KINDS:
                r.kernel_time(k)
            for _ in range(n):
                self.call(r, xd, yd, B)
            self.torch.cuda.synchronize()
            out = {}
            for key, k in KINDS:
                ms, launches = r.kernel_time(k)
                out[key] = round(ms * 1e3 / n, 1) if launches else None
            return out
        finally:
            r.set_option("profile", 0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=str, default="a,b,c")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="2,4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--ladder", type=str, default="64x8,256x16,1024x32,4096x64")
    ap.add_argument("--give-up", type=float, default=20.0, help="seconds per interpreter block beyond which larger shapes are not given to the interpreter")
    ap.add_argument("--parent", action="store_true", help='a library from before "mux_tail": the option is never set (part a only)')
    a = ap.parse_args()
    from ctypes import c_float, c_int
    for name, args in (("dsp_SAT0DB_TPDF_GAIN_Fixed", [c_float]), ("dsp_LOAD_MUX", [c_int]), ("dspLoadMux_Inputs", [c_int]), ("dspLoadMux_Data", [c_int, c_float])):
        getattr(enc.lib(), name).argtypes = args
    b = Bench(a.steps, a.rounds)
    blocks = [int(v) for v in a.blocks.split(",")]
    formats = [int(v) for v in a.formats.split(",")]
    ladder = [tuple(int(v) for v in s.split("x")) for s in a.ladder.split(",")]
    parts = a.parts.split(",") if not a.parent else ["a"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    raw = open(os.path.join(ROOT, "profiles", "muxtail_bench.txt"), "a")
    lines = []

    def emit(**line):
        lines.append(line)
        print(line, flush=True)
        raw.write(json.dumps(line) + "\n")
        raw.flush()

    def loaded(fmt, prog):
        r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
        r.set_option("chain_finish", 1)
        r.set_option("chain_delay", 1)
        return r

    try:
        for fmt in formats:
            slow = False
            if "a" in parts:
                for O, I in ladder:
                    r = loaded(fmt, array_program(fmt, O, I))
                    xd, yd = b.buffers(fmt, max(blocks), I, O)
                    settings = [("parent", r, [])] if a.parent else ([] if slow else [("mux_tail_0", r, [("mux_tail", 0)])]) + [("mux_tail_1", r, [("mux_tail", 1)])]
                    for B in blocks:
                        res = b.alternate(settings, xd, yd, B)
                        emit(part="a", format=fmt, outputs=O, inputs=I, block=B, **res)
                        slow = slow or any(v.get("est") and v["us"] * 1024 / B > a.give_up * 1e6 for v in res.values())
                    r.release()
                    del xd, yd
            if "b" in parts:
                O, I = ladder[-1]
                progs = (("mux_tail_1", array_program(fmt, O, I)), ("no_mixer", array_program(fmt, O, I, mux=None)), ("plain_sat_no_delay", array_program(fmt, O, I, us=0, finish="sat")))
                rs = [(name, loaded(fmt, p), [("mux_tail", 1)] if name == "mux_tail_1" else []) for name, p in progs]
                xd, yd = b.buffers(fmt, max(blocks), I, O)
                for B in blocks:
                    res = b.alternate(rs, xd, yd, B)
                    for name, r, _ in rs:
                        res[name].update(b.kernel_times(r, xd, yd, B))
                    emit(part="b", format=fmt, outputs=O, inputs=I, block=B, **res)
                for _, r, _ in rs:
                    r.release()
                del xd, yd
            if "c" in parts:
                O, I = ladder[-1]
                for lists in ("shared", "private"):
                    if fmt == 2 and lists == "private":
                        continue                              # (format 2 has no mux_tile: both are mux_plain)
                    progs = (("handed", array_program(fmt, O, I, sections=0, finish="tpdf", mux=lists)), ("stage_finished", array_program(fmt, O, I, sections=0, us=0, finish="tpdf", mux=lists)))
                    rs = [(name, loaded(fmt, p), [("mux_tail", 1)]) for name, p in progs]
                    xd, yd = b.buffers(fmt, max(blocks), I, O)
                    for B in blocks:
                        res = b.alternate(rs, xd, yd, B)
                        for name, r, _ in rs:
                            res[name].update(b.kernel_times(r, xd, yd, B), tail_info=list(r.mux_tail_info()), groups=r.mux_info()["groups"])
                        emit(part="c", format=fmt, outputs=O, inputs=I, lists=lists, block=B, **res)
                    for _, r, _ in rs:
                        r.release()
                    del xd, yd
    finally:
        if not a.parent:
            rt.Runtime.set_global_option("mux_tail", 0)
        rt.Runtime.set_global_option("chain_delay", 0)
        rt.Runtime.set_global_option("chain_finish", 0)
    print(json.dumps(dict(tool="muxtail_bench", parent=bool(a.parent), lines=lines)))


if __name__ == "__main__":
    main()

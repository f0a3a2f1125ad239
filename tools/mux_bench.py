"""A mixing matrix in front of the chains (LOAD_MUX chain heads): microseconds per device-resident block, DSP_FORMAT 6.

    4096 outputs x 64 inputs x 16 sections          (shared lists: one mix group, mux_tile)
    the same with a 4096-tap FIR behind the cascade
    4096 outputs x 1024 inputs x 16 sections
    1024 outputs with private 8-entry lists over 64 inputs x 16 sections   (no group: mux_plain)

at blocks of 1024 and 256 frames, every block call bracketed by device events on the caller's stream (median of `--steps` calls, the
bench's method), then the stage's own kernel time (dspRuntimeKernelTime kind 7) and the cascade's (kind 0) from a second pass with
the kernel timers on -- beside the same cascade without a mixer (synth_program, 4096 x 16: DESIGN.md 4.1's cfg3).  A library that
does not lower LOAD_MUX runs these programs on the interpreter: the same script measures that (chains = 0 in its lines); calls that
take long get fewer steps, and a block estimated to take more than 5 s is NOT run: its figure is a 64-frame call scaled to the block
length (steps 0 in its line -- an estimate, to be quoted as one).  A commit from before synth_mixer_program cannot run this script as it
is: to measure it, build that commit's library and put this file and this commit's avdsp_amd/progbuilder.py beside it (that is how the
parent's column of profiles/mux_mixer.md was made); --generic on this library is the other way to see the interpreter.  One JSON line
at the end.

    python tools/mux_bench.py [--steps 30] [--shapes a,b,c,d] [--blocks 1024,256] [--generic]
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

from avdsp_amd import progbuilder as pb      # noqa: E402
from avdsp_amd import runtime as rt          # noqa: E402

SHAPES = {
    "a": dict(name="4096x64 s16", outputs=4096, inputs=64, sections=16, taps=0, lists="shared"),
    "b": dict(name="4096x64 s16 fir4096", outputs=4096, inputs=64, sections=16, taps=4096, lists="shared"),
    "c": dict(name="4096x1024 s16", outputs=4096, inputs=1024, sections=16, taps=0, lists="shared"),
    "d": dict(name="1024 private8 s16", outputs=1024, inputs=64, sections=16, taps=0, lists="private"),
}
KIND_BIQUAD, KIND_FIR, KIND_MUX = 0, 1, 7


PROBE = 64                                 # frames of the call that decides whether whole blocks can be timed
SLOW_S = 5.0                               # a block estimated to take longer is not run: the probe's figure is the result


def time_blocks(r, xd, yd, in_stride, in_base, out_stride, B, steps, st, torch):
    """median microseconds of a block call.  A short call first: where a block would take seconds (a mixer on the interpreter), its
    time scaled to the block is reported instead (steps 0), and no whole block is run."""
    def wall(frames):
        t0 = time.time()
        r.run_block_device(xd.data_ptr(), in_stride, in_base, yd.data_ptr(), out_stride, 0, frames, st)
        torch.cuda.synchronize()
        return time.time() - t0
    first = wall(min(PROBE, B))                            # (with the plan's making)
    probe = wall(min(PROBE, B))
    if probe * B / min(PROBE, B) > SLOW_S:
        return probe * B / min(PROBE, B) * 1e6, 0, first
    wall(B)
    one = wall(B)
    n = max(3, min(steps, int(2.0 / max(one, 1e-6))))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        r.run_block_device(xd.data_ptr(), in_stride, in_base, yd.data_ptr(), out_stride, 0, B, st)
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev), n, first


def kernel_times(r, xd, yd, in_stride, in_base, out_stride, B, st, torch, n=10):
    r.set_option("profile", 1)
    try:
        for k in (KIND_BIQUAD, KIND_FIR, KIND_MUX):
            r.kernel_time(k)
        for _ in range(n):
            r.run_block_device(xd.data_ptr(), in_stride, in_base, yd.data_ptr(), out_stride, 0, B, st)
        torch.cuda.synchronize()
        out = {}
        for key, k in (("cascade_us", KIND_BIQUAD), ("fir_us", KIND_FIR), ("mux_us", KIND_MUX)):
            ms, launches = r.kernel_time(k)
            out[key] = round(ms * 1e3 / n, 1) if launches else None
        return out
    finally:
        r.set_option("profile", 0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", type=str, default="a,b,c,d")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--generic", action="store_true", help='"generic" 1: every core on the interpreter (what a library without the lowering does)')
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    # the cascade alone: cfg3's 4096 chains x 16 biquads behind a LOAD_GAIN
    C = 4096
    r = rt.Runtime(6, pb.synth_program(6, C, 16))
    xd = dm.to_device(pb.lcg_input(max(blocks), C, True, seed=3))
    yd = torch.zeros_like(xd)
    for B in blocks:
        us, n, _ = time_blocks(r, xd, yd, C, C, C, B, a.steps, st, torch)
        kt = kernel_times(r, xd, yd, C, C, C, B, st, torch)
        lines.append(dict(shape="cascade alone 4096 s16", block=B, chains=C, us_per_block=round(us, 1), steps=n, **kt))
        print(lines[-1], flush=True)
    r.release()
    del xd, yd

    for key in a.shapes.split(","):
        sh = SHAPES[key]
        O, I = sh["outputs"], sh["inputs"]
        try:
            prog = pb.synth_mixer_program(6, O, I, sh["sections"], ntaps=sh["taps"], lists=sh["lists"], entries=8)
            r = rt.Runtime(6, prog)
            if a.generic:
                r.set_option("generic", 1)
            chains = r.core_info()["chains"]
            info = r.mux_info() if hasattr(r, "mux_info") and hasattr(r.L, "dspRuntimeMuxInfo") else {}
            xd = dm.to_device(pb.lcg_input(max(blocks), I, True, seed=5))
            yd = torch.zeros((max(blocks), O), dtype=torch.float32, device="cuda")
            for B in blocks:
                us, n, first = time_blocks(r, xd, yd, I, O, O, B, a.steps, st, torch)
                kt = kernel_times(r, xd, yd, I, O, O, B, st, torch, n=min(10, n)) if chains and n else {}
                lines.append(dict(shape=sh["name"], block=B, chains=chains, groups=info.get("groups"), us_per_block=round(us, 1), steps=n,
                                  first_call_ms=round(first * 1e3, 1), **kt))
                print(lines[-1], flush=True)
            r.release()
            del xd, yd
        except Exception as e:                              # a shape a library cannot run is a result too
            lines.append(dict(shape=sh["name"], error=str(e)[:200]))
            print(lines[-1], flush=True)
            rt.lib().dspRuntimeRelease()
    print(json.dumps(dict(tool="mux_bench", format=6, generic=bool(a.generic), lines=lines)))


if __name__ == "__main__":
    main()

"""Memory-word trees with a DSP_FIR in a trunk or in the branches ("mem_fir" 1 beside "chain_mem" 1): microseconds per
device-resident block of the two programs a convolution engine is bought for, at scale --

    crossover     TPDF_CALC;  T x ( LOAD_GAIN -> 8 biquads -> STORE_MEM m;  W x (LOAD_MEM m -> FIR of `taps` -> SAT0DB -> STORE) )
    crossover_t   the same with every way ending  DELAY us -> SAT0DB_TPDF_GAIN -> STORE  ("fir_tail" 1: handed FIR branches)
    room          TPDF_CALC;  T x ( LOAD_GAIN -> 8 biquads -> FIR of `taps` -> STORE_MEM m;
                                    W x (LOAD_MEM m -> 8 biquads -> DELAY us -> SAT0DB_TPDF_GAIN -> STORE) )

-- each against the program a user has to write today to stay on the chain kernels ("unshared": the trunk's sections, and for `room`
its FIR, repeated in every way -- W x T independent chains).  That one is NOT the same program: between trunk and way the tree narrows
the accumulator to a 32-bit word and widens it again, the unshared chain does not, so its outputs differ in bits from the tree's; it
stands for the cost of the work, not for its result.  With --ladder the tree programs also run with "mem_fir" 0 (the interpreter) up a
ladder of sizes, one call per cell, until a call exceeds --stop-ms.  One process; the settings alternate (`--rounds` times: two warm-up
calls that also make the plans, then `--steps` calls each bracketed by device events on the caller's stream), a setting's figure is
the median over all its timed calls; with --timers the kernel timers (dspRuntimeKernelTime) of one more call are read per kind.  Raw
lines as they come, one JSON line at the end.

    python tools/firtree_bench.py [--steps 20] [--rounds 3] [--formats 4,6] [--blocks 1024,256] [--trees 1024] [--ways 3] [--taps 4096] [--timers] [--ladder]

--shard RANK WORLD ("shard_trees" 1): the tree programs alone, one shard on this GPU -- dspRuntimeSetShard(RANK, WORLD), the
core cut at tree boundaries -- against the whole core on the same library, alternating in the same way; the windows stay the whole
block's.  `linear` is whole / (WORLD x shard).
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

KINDS = dict(cascade=0, fir=1, tail=2, stage=7)          # AVDSP_KERNEL_BIQUAD, _FIR, _PASS (passthrough and chain_tail), _MUX (mem_stage)


OP_TPDF_CALC, OP_LOAD_MEM, OP_STORE_MEM, OP_SAT0DB_TPDF_GAIN, OP_DELAY = 7, 39, 40, 45, 47
FACTOR_48000 = 206158430                     # (unsigned)(2^32 / 10^6 x 48000): samples = us x factor >> 32


def program(fmt: int, kind: str, shared: bool, trees: int, ways: int, sections: int, taps: int, us: int):
    """inputs at IO trees * ways .., outputs at IO 0 ..; shared: the tree, else the unshared chains.  Every chain has its bank and its
    impulse in a PARAM of its own in front of its opcodes, a tree its memory word in the trunk's (written with progbuilder's
    ProgramWriter: the encoder's dsp_FIR keeps a region's end in 16 bits and cannot address an impulse beyond the first 65535 words)"""
    nout = trees * ways
    room, tailed = kind == "room", kind != "crossover"
    nfir = trees if room else nout
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=256 + trees * (ways + 1) * (64 + 2 * sections * 8) + (nout if not shared else nfir) * (taps + 16))
    h = pb.lcg_taps_all(nfir, taps)
    secs = lambda c: pb.synth_sections(c, sections, pb.F48000, pb.F48000)
    pw.core()
    pw._head(OP_TPDF_CALC, 3)                                  # dsp_TPDF_CALC(0): the default width, an 8-byte result word
    pw._w(0)
    pw._w(pw._data_aligned8(2))
    for t in range(trees):
        word = 0
        if shared:
            pw.param()
            bank = pw.biquad_bank(secs(t))
            imp = pw.fir_impulses([h[t]]) if room else None
            word = pw._w(0)                                    # dspMem_Location(): two free words of the PARAM
            pw._w(0)
            pw.load_gain_fixed(nout + t, 0.5)
            pw.biquads(bank, sections)
            if room:
                pw.fir(imp, taps)
            base = pw._head(OP_STORE_MEM, 2)
            pw._w(word - base)
        for w in range(ways):
            c = t * ways + w
            pw.param()
            if shared:
                if room:
                    bank = pw.biquad_bank(secs(trees + c))
                else:
                    imp = pw.fir_impulses([h[c]])
                base = pw._head(OP_LOAD_MEM, 2)
                pw._w(word - base)
                if room:
                    pw.biquads(bank, sections)
                else:
                    pw.fir(imp, taps)
            else:
                # (room: trunk sections, FIR, way sections is no chain the lowering takes -- all the sections, then the trunk's FIR)
                both = secs(t) + (secs(trees + c) if room else [])
                bank = pw.biquad_bank(both)
                imp = pw.fir_impulses([h[t] if room else h[c]])
                pw.load_gain_fixed(nout + t, 0.5)
                pw.biquads(bank, len(both))
                pw.fir(imp, taps)
            if tailed:
                pw._head(OP_DELAY, 4)                          # dsp_DELAY_FixedMicroSec(us): [us, line, no parameter]
                pw._w(us)
                pw._w(pw.data_counter)
                pw.data_counter += 1 + ((us * FACTOR_48000) >> 32)
                pw._w(0)
                pw._head(OP_SAT0DB_TPDF_GAIN, 3)               # dsp_SAT0DB_TPDF_GAIN_Fixed(0.9): the gain behind the opcode
                pw._w(2)
                pw._param_value(0.9)
            else:
                pw.sat0db()
            pw.store(c)
    return pw.end_of_code()


def time_calls(r, args, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        r.run_block_device(*args)
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--kinds", type=str, default="crossover,crossover_t,room")
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--ways", type=int, default=3)
    ap.add_argument("--sections", type=int, default=8)
    ap.add_argument("--taps", type=int, default=4096)
    ap.add_argument("--us", type=int, default=1000)
    ap.add_argument("--timers", action="store_true")
    ap.add_argument("--ladder", action="store_true", help="mem_fir 1 against mem_fir 0 from 16 trees x 128 taps up, one call per cell")
    ap.add_argument("--stop-ms", type=float, default=1000.0)
    ap.add_argument("--shard", type=int, nargs=2, metavar=("RANK", "WORLD"), help="one shard of the tree programs (shard_trees 1) against the whole core")
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    options = ("chain_mem", "mem_fir", "fir_tail", "chain_delay", "chain_finish") + (("shard_trees",) if a.shard else ())
    rank, world = a.shard or (0, 1)

    def loaded(fmt, kind, shared, T, taps, mem_fir=1):
        r = rt.Runtime(fmt, program(fmt, kind, shared, T, a.ways, a.sections, taps, a.us), fs=48000, random=1, dither=24)
        for key in options:
            r.set_option(key, mem_fir if key == "mem_fir" else 1)
        return r

    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            for kind in a.kinds.split(","):
                if a.shard:
                    T = a.trees
                    nout = T * a.ways
                    r = loaded(fmt, kind, True, T, a.taps)
                    xd = dm.to_device(pb.lcg_input(max(blocks), T, fmt == 6, seed=3))
                    yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
                    settings = (("whole", (0, 1)), ("shard", (rank, world)))
                    for B in blocks:
                        args = (xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                        us = {name: [] for name, _ in settings}
                        cuts, chains = {}, {}
                        for _ in range(a.rounds):
                            for name, (k, n) in settings:
                                r.set_shard(k, n)
                                s = r.shard_info()
                                cuts[name], chains[name] = (s["first_chain"], s["nchains"]), r.core_info()["chains"]
                                r.run_block_device(*args)
                                r.run_block_device(*args)
                                torch.cuda.synchronize()
                                us[name] += time_calls(r, args, a.steps)
                                print(f"# format {fmt} {kind} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                        med = {name: statistics.median(v) for name, v in us.items()}
                        lines.append(dict(format=fmt, kind=kind, trees=T, ways=a.ways, sections=a.sections, taps=a.taps, block=B, delay_us=a.us, shard=[rank, world],
                                          **{f"{name}_us": round(m, 1) for name, m in med.items()}, **{f"{name}_min_us": round(min(v), 1) for name, v in us.items()},
                                          linear=round(med["whole"] / (world * med["shard"]), 3), first_chain_and_chains=cuts, lowered_chains=chains,
                                          calls={name: len(v) for name, v in us.items()}))
                        print(lines[-1], flush=True)
                    r.set_shard(0, 1)
                    r.release()
                    del xd, yd
                    continue
                if a.ladder:
                    T, taps = 16, 128
                    while True:
                        nout = T * a.ways
                        xd = dm.to_device(pb.lcg_input(max(blocks), T, fmt == 6, seed=3))
                        yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
                        r = loaded(fmt, kind, True, T, taps)
                        cell = dict(format=fmt, kind=kind, trees=T, ways=a.ways, taps=taps)
                        for B in blocks:
                            args = (xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                            for opt in (1, 0):
                                r.set_option("mem_fir", opt)
                                chains = r.core_info()["chains"]
                                r.run_block_device(*args)                  # (makes the plan)
                                cell[f"mem_fir_{opt}_block_{B}_us"] = round(time_calls(r, args, 1)[0], 1)
                                cell[f"mem_fir_{opt}_chains"] = chains
                        r.release()
                        lines.append(cell)
                        print(cell, flush=True)
                        if max(cell[f"mem_fir_0_block_{B}_us"] for B in blocks) > a.stop_ms * 1e3 or (T >= a.trees and taps >= a.taps):
                            break
                        T, taps = min(2 * T, a.trees), min(2 * taps, a.taps)
                    continue
                T = a.trees
                nout = T * a.ways
                tree, flat = loaded(fmt, kind, True, T, a.taps), loaded(fmt, kind, False, T, a.taps)
                xd = dm.to_device(pb.lcg_input(max(blocks), T, fmt == 6, seed=3))
                yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
                settings = (("mem_fir_1", tree), ("unshared", flat))
                for B in blocks:
                    args = (xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                    us = {name: [] for name, _ in settings}
                    for _ in range(a.rounds):
                        for name, r in settings:
                            r.run_block_device(*args)
                            r.run_block_device(*args)
                            torch.cuda.synchronize()
                            us[name] += time_calls(r, args, a.steps)
                            print(f"# format {fmt} {kind} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                    line = dict(format=fmt, kind=kind, trees=T, ways=a.ways, sections=a.sections, taps=a.taps, block=B, delay_us=a.us,
                                **{f"{name}_us": round(statistics.median(v), 1) for name, v in us.items()},
                                **{f"{name}_min_us": round(min(v), 1) for name, v in us.items()},
                                mem_fir_info=tree.mem_fir_info(), mem_info=tree.mem_info(), fir_tail_info=tree.fir_tail_info(),
                                lowered_chains={name: r.core_info()["chains"] for name, r in settings}, calls={name: len(v) for name, v in us.items()})
                    if a.timers:
                        for name, r in settings:
                            r.set_option("profile", 1)
                            for k in KINDS.values():
                                r.kernel_time(k)
                            r.run_block_device(*args)
                            torch.cuda.synchronize()
                            read = {what: r.kernel_time(k) for what, k in KINDS.items()}      # (total ms, launches) per kind; a read resets
                            line[f"{name}_timers_us"] = {what: [round(ms * 1e3, 1), n] for what, (ms, n) in read.items()}
                            r.set_option("profile", 0)
                    lines.append(line)
                    print(line, flush=True)
                tree.release()
                flat.release()
                del xd, yd
    finally:
        rt.lib().dspRuntimeSetShard(0, 1)
        for key in options:
            rt.Runtime.set_global_option(key, 0)
    print(json.dumps(dict(tool="firtree_bench", lines=lines)))


if __name__ == "__main__":
    main()

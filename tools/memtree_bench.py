"""Memory words on the chain kernels against the interpreter ("chain_mem" 1 / 0): microseconds per device-resident
block of the crossover at scale,

    TPDF_CALC;  1024 x ( LOAD_GAIN -> 8 biquads -> STORE_MEM m;
                         3 x (LOAD_MEM m -> 8 biquads -> DELAY 1000 us -> SAT0DB_TPDF_GAIN -> STORE) )          4096 chains

with "chain_finish" 1 and "chain_delay" 1, in DSP_FORMAT 2, 4 and 6 at blocks of 1024 and 256 frames -- and the program a user had to
write to stay on the chain kernels without the option, 3072 independent chains of LOAD_GAIN -> 16 biquads (the trunk's eight repeated
in front of the way's eight) -> DELAY -> SAT0DB_TPDF_GAIN -> STORE ("unshared").  That one is NOT the same program: between trunk and
way the tree narrows the accumulator to a 32-bit word and widens it again, the 16-section cascade does not, so its outputs differ in
bits from the tree's; it stands for the cost of the work, not for its result.  One process, two loaded programs per format; the three
settings alternate (`--rounds` times: select, two warm-up calls that also make the plans, then `--steps` calls each bracketed by
device events on the caller's stream), and a setting's figure is the median over all its timed calls.  A setting whose second warm-up
call lasts more than `--slow-ms` is measured by that one call and left out of the later rounds (the interpreter walks this program's
frames in turn, one wave: seconds per block); every line says how many calls stand behind each figure.  One JSON line at the end.

    python tools/memtree_bench.py [--steps 20] [--rounds 3] [--formats 2,4,6] [--blocks 1024,256] [--trees 1024] [--ways 3] [--sections 8] [--us 1000]

--shard RANK WORLD ("shard_trees" 1): the tree program alone, one shard of it on this GPU -- dspRuntimeSetShard(RANK, WORLD),
the core cut at tree boundaries -- against the whole core on the same library, alternating in the same way; the windows stay the
whole block's (they only have to cover the shard's IOs).  `linear` is whole / (WORLD x shard): 1.0 would be a shard that costs its
share of the whole.  --with-off adds the same shard with "shard_trees" 0 -- the core whole on the interpreter, as every rank ran it
before the option --, measured like the other slow settings; meant for a small --trees.
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


def filters(L, sections, c, first=0):
    for k in range(first, first + sections):
        L.dsp_Filter2ndOrder(FPEAK, 60.0 + 3.0 * (c % 500) + 900.0 * (k % 16), 0.9, 1.02 if k % 2 else 0.97)


def tree_program(fmt: int, trees: int, ways: int, sections: int, us: int):
    """inputs at IO trees * ways .., outputs at IO 0 .."""
    nout = trees * ways

    def build(L):
        trunks, branches, words = [], [], []
        for t in range(trees):
            if t % 64 == 0:
                L.dsp_PARAM()                            # (a PARAM section holds 65535 words at the most)
            trunks.append(L.dspBiquad_Sections(sections))
            filters(L, sections, t)
            for w in range(ways):
                branches.append(L.dspBiquad_Sections(sections))
                filters(L, sections, t * ways + w, sections)
            words.append(L.dspMem_Location())
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for t in range(trees):
            L.dsp_LOAD_GAIN_Fixed(nout + t, 0.5)
            L.dsp_BIQUADS(trunks[t])
            L.dsp_STORE_MEM(words[t])
            for w in range(ways):
                L.dsp_LOAD_MEM(words[t])
                L.dsp_BIQUADS(branches[t * ways + w])
                L.dsp_DELAY_FixedMicroSec(us)
                L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
                L.dsp_STORE(t * ways + w)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=nout + trees, capacity=trees * (ways + 1) * (sections * 8 + 32) + 4096)


def unshared_program(fmt: int, trees: int, ways: int, sections: int, us: int):
    """the same inputs and outputs; way w of tree t repeats the trunk's sections in front of its own"""
    nout = trees * ways

    def build(L):
        banks = []
        for c in range(nout):
            if c % 128 == 0:
                L.dsp_PARAM()
            banks.append(L.dspBiquad_Sections(2 * sections))
            filters(L, sections, c // ways)
            filters(L, sections, c, sections)
        L.dsp_CORE()
        L.dsp_TPDF_CALC(0)
        for c in range(nout):
            L.dsp_LOAD_GAIN_Fixed(nout + c // ways, 0.5)
            L.dsp_BIQUADS(banks[c])
            L.dsp_DELAY_FixedMicroSec(us)
            L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
            L.dsp_STORE(c)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=nout + trees, capacity=nout * (sections * 16 + 32) + 4096)


def shard_mode(a) -> None:
    """one shard of the tree program against the whole core"""
    import torch
    from avdsp_amd import devmem as dm
    rank, world = a.shard
    T, W = a.trees, a.ways
    nout = T * W
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    options = ("chain_mem", "chain_delay", "chain_finish", "shard_trees")
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            r = rt.Runtime(fmt, tree_program(fmt, T, W, a.sections, a.us), fs=48000, random=1, dither=24)
            for key in options:
                r.set_option(key, 1)
            xd = dm.to_device(pb.lcg_input(max(blocks), T, fmt == 6, seed=3))
            yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
            settings = [("whole", (0, 1), 1), ("shard", (rank, world), 1)] + ([("shard_trees_0", (rank, world), 0)] if a.with_off else [])
            for B in blocks:
                args = (xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                us = {name: [] for name, _, _ in settings}
                slow, cuts, chains = set(), {}, {}
                for _ in range(a.rounds):
                    for name, (k, n), opt in settings:
                        if name in slow:
                            continue
                        r.set_option("shard_trees", opt)
                        r.set_shard(k, n)
                        s = r.shard_info()
                        cuts[name], chains[name] = (s["first_chain"], s["nchains"]), r.core_info()["chains"]
                        r.run_block_device(*args)
                        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        w0.record()
                        r.run_block_device(*args)
                        w1.record()
                        torch.cuda.synchronize()
                        if w0.elapsed_time(w1) > a.slow_ms:
                            slow.add(name)
                            us[name].append(w0.elapsed_time(w1) * 1e3)
                            print(f"# format {fmt} block {B} {name}: one call of {us[name][0] / 1e6:.3f} s", flush=True)
                            continue
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                        for e0, e1 in ev:
                            e0.record()
                            r.run_block_device(*args)
                            e1.record()
                        torch.cuda.synchronize()
                        us[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                        print(f"# format {fmt} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                med = {name: statistics.median(v) for name, v in us.items()}
                lines.append(dict(format=fmt, trees=T, ways=W, sections=a.sections, block=B, delay_us=a.us, shard=[rank, world],
                                  **{f"{name}_us": round(m, 1) for name, m in med.items()},
                                  **{f"{name}_min_us": round(min(us[name]), 1) for name in us},
                                  linear=round(med["whole"] / (world * med["shard"]), 3), first_chain_and_chains=cuts, lowered_chains=chains,
                                  calls={name: len(v) for name, v in us.items()}))
                print(lines[-1], flush=True)
            r.set_shard(0, 1)
            r.release()
            del xd, yd
    finally:
        rt.lib().dspRuntimeSetShard(0, 1)
        for key in options:
            rt.Runtime.set_global_option(key, 0)
    print(json.dumps(dict(tool="memtree_bench", mode="shard", lines=lines)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="2,4,6")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--ways", type=int, default=3)
    ap.add_argument("--sections", type=int, default=8)
    ap.add_argument("--us", type=int, default=1000)
    ap.add_argument("--slow-ms", type=float, default=20.0)
    ap.add_argument("--shard", type=int, nargs=2, metavar=("RANK", "WORLD"), help="one shard of the tree program (shard_trees 1) against the whole core")
    ap.add_argument("--with-off", action="store_true", help="with --shard: the same shard with shard_trees 0 too (the interpreter)")
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    from ctypes import c_float, c_int
    L = enc.lib()
    L.dsp_SAT0DB_TPDF_GAIN_Fixed.argtypes = [c_float]
    L.dsp_LOAD_MEM.argtypes = [c_int]
    L.dsp_STORE_MEM.argtypes = [c_int]
    if a.shard:
        return shard_mode(a)
    T, W = a.trees, a.ways
    nout = T * W
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            tree = rt.Runtime(fmt, tree_program(fmt, T, W, a.sections, a.us), fs=48000, random=1, dither=24)
            flat = rt.Runtime(fmt, unshared_program(fmt, T, W, a.sections, a.us), fs=48000, random=1, dither=24)
            for r in (tree, flat):
                r.set_option("chain_finish", 1)
                r.set_option("chain_delay", 1)
            xd = dm.to_device(pb.lcg_input(max(blocks), T, fmt == 6, seed=3))
            yd = dm.to_device(pb.lcg_input(max(blocks), nout, fmt == 6, seed=4))
            settings = (("chain_mem_1", tree, 1), ("unshared", flat, 0), ("chain_mem_0", tree, 0))
            for B in blocks:
                us = {name: [] for name, _, _ in settings}
                chains, slow, info = {}, set(), None
                for _ in range(a.rounds):
                    for name, r, opt in settings:
                        if name in slow:
                            continue
                        r.set_option("chain_mem", opt)
                        chains[name] = r.core_info()["chains"]
                        if name == "chain_mem_1":
                            info = r.mem_info()
                        # two warm-up calls that also make the plans; the second is timed: a setting whose call lasts more than
                        # --slow-ms (the interpreter on this program: one wave walks the frames in turn, seconds per block) is
                        # measured by that one call and left out of the later rounds
                        r.run_block_device(xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        w0.record()
                        r.run_block_device(xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                        w1.record()
                        torch.cuda.synchronize()
                        if w0.elapsed_time(w1) > a.slow_ms:
                            slow.add(name)
                            us[name].append(w0.elapsed_time(w1) * 1e3)
                            print(f"# format {fmt} block {B} {name}: one call of {us[name][0] / 1e6:.2f} s", flush=True)
                            continue
                        steps = a.steps
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                        for e0, e1 in ev:
                            e0.record()
                            r.run_block_device(xd.data_ptr(), T, nout, yd.data_ptr(), nout, 0, B, st)
                            e1.record()
                        torch.cuda.synchronize()
                        us[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                        print(f"# format {fmt} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                med = {name: statistics.median(v) for name, v in us.items()}
                lines.append(dict(format=fmt, trees=T, ways=W, sections=a.sections, block=B, delay_us=a.us,
                                  **{f"{name}_us": round(m, 1) for name, m in med.items()},
                                  **{f"{name}_min_us": round(min(us[name]), 1) for name in us},
                                  gsamples_per_s={name: round(nout * B / m / 1e3, 4) for name, m in med.items()},
                                  mem_info=info, lowered_chains=chains, calls={name: len(v) for name, v in us.items()}))
                print(lines[-1], flush=True)
            tree.release()
            flat.release()
            del xd, yd
    finally:
        for key in ("chain_mem", "chain_delay", "chain_finish"):
            rt.Runtime.set_global_option(key, 0)
    print(json.dumps(dict(tool="memtree_bench", lines=lines)))


if __name__ == "__main__":
    main()

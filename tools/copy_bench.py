"""LOAD_STORE lists beside the chain kernels against the interpreter ("chain_copy" 1 / 0): microseconds per
device-resident block of

    (a)  LOAD_STORE of 2048 pairs;  TPDF_CALC;  1024 x ( LOAD_GAIN -> 8 biquads -> STORE_MEM m;
                                                        3 x (LOAD_MEM m -> 8 biquads -> DELAY 1000 us -> SAT0DB_TPDF_GAIN -> STORE) )
         -- tools/memtree_bench.py's program with every trunk's input copied to two monitor outputs in front of it -- with "chain_copy" 1
         ("list_copy_1"), with "chain_copy" 0 ("list_copy_0": the whole core on the interpreter), and the same program without the list
         ("no_list"), which needs no "chain_copy": the difference to "list_copy_1" is the price of the list;
    (b)  a core that is a LOAD_STORE of 4096 pairs and nothing else, "chain_copy" 1 ("pairs_copy_1") and 0 ("pairs_copy_0"),

with "chain_mem", "chain_finish" and "chain_delay" 1, in DSP_FORMAT 6 and 2 at blocks of 1024 and 256 frames.  One process; the
settings of a cell alternate (`--rounds` times: two warm-up calls that also make the plans, then `--steps` calls each bracketed by
device events on the caller's stream), and a setting's figure is the median over all its timed calls.  A setting whose second warm-up
call lasts more than `--slow-ms` is measured by that one call and left out of the later rounds (the interpreter walks program (a)'s
frames in turn, one wave: seconds per block); every line says how many calls stand behind each figure.  One JSON line at the end.

    python tools/copy_bench.py [--steps 20] [--rounds 3] [--formats 6,2] [--blocks 1024,256] [--trees 1024] [--pairs 4096]
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
WAYS, SECTIONS, US = 3, 8, 1000


def filters(L, sections, c, first=0):
    for k in range(first, first + sections):
        L.dsp_Filter2ndOrder(FPEAK, 60.0 + 3.0 * (c % 500) + 900.0 * (k % 16), 0.9, 1.02 if k % 2 else 0.97)


def tree_program(fmt: int, trees: int, with_list: bool):
    """outputs of the ways at IO 0 .., inputs at IO trees * WAYS .., the monitor outputs behind them"""
    nout = trees * WAYS

    def build(L):
        trunks, branches, words = [], [], []
        for t in range(trees):
            if t % 64 == 0:
                L.dsp_PARAM()                            # (a PARAM section holds 65535 words at the most)
            trunks.append(L.dspBiquad_Sections(SECTIONS))
            filters(L, SECTIONS, t)
            for w in range(WAYS):
                branches.append(L.dspBiquad_Sections(SECTIONS))
                filters(L, SECTIONS, t * WAYS + w, SECTIONS)
            words.append(L.dspMem_Location())
        L.dsp_CORE()
        if with_list:
            L.dsp_LOAD_STORE()
            for t in range(trees):
                L.dspLoadStore_Data(nout + t, nout + trees + 2 * t)
                L.dspLoadStore_Data(nout + t, nout + trees + 2 * t + 1)
        L.dsp_TPDF_CALC(0)
        for t in range(trees):
            L.dsp_LOAD_GAIN_Fixed(nout + t, 0.5)
            L.dsp_BIQUADS(trunks[t])
            L.dsp_STORE_MEM(words[t])
            for w in range(WAYS):
                L.dsp_LOAD_MEM(words[t])
                L.dsp_BIQUADS(branches[t * WAYS + w])
                L.dsp_DELAY_FixedMicroSec(US)
                L.dsp_SAT0DB_TPDF_GAIN_Fixed(0.9)
                L.dsp_STORE(t * WAYS + w)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=nout + 3 * trees, capacity=trees * (WAYS + 1) * (SECTIONS * 8 + 32) + 4 * trees + 4096)


def pairs_program(fmt: int, pairs: int):
    """input IO pairs + k to output IO k"""
    def build(L):
        L.dsp_CORE()
        L.dsp_LOAD_STORE()
        for k in range(pairs):
            L.dspLoadStore_Data(pairs + k, k)
    return enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=2 * pairs, capacity=2 * pairs + 4096)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", type=str, default="6,2")
    ap.add_argument("--blocks", type=str, default="1024,256")
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--slow-ms", type=float, default=20.0)
    a = ap.parse_args()
    import torch
    from avdsp_amd import devmem as dm
    from ctypes import c_float, c_int
    L = enc.lib()
    L.dsp_SAT0DB_TPDF_GAIN_Fixed.argtypes = [c_float]
    L.dsp_LOAD_MEM.argtypes = [c_int]
    L.dsp_STORE_MEM.argtypes = [c_int]
    L.dspLoadStore_Data.argtypes = [c_int, c_int]
    T, P = a.trees, a.pairs
    nout = T * WAYS
    blocks = [int(v) for v in a.blocks.split(",")]
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    try:
        for fmt in [int(v) for v in a.formats.split(",")]:
            listed = rt.Runtime(fmt, tree_program(fmt, T, True), fs=48000, random=1, dither=24)
            bare = rt.Runtime(fmt, tree_program(fmt, T, False), fs=48000, random=1, dither=24)
            alone = rt.Runtime(fmt, pairs_program(fmt, P), fs=48000, random=1, dither=24)
            for r in (listed, bare, alone):
                for key in ("chain_mem", "chain_finish", "chain_delay"):
                    r.set_option(key, 1)
            # (a): input window [nout, nout + T), output window [0, nout + 3 T); (b): input window [P, 2 P), output window [0, P)
            cells = (("a", (("list_copy_1", listed, 1), ("no_list", bare, 0), ("list_copy_0", listed, 0)), (T, nout, nout + 3 * T, 0)),
                     ("b", (("pairs_copy_1", alone, 1), ("pairs_copy_0", alone, 0)), (P, P, P, 0)))
            for cell, settings, (in_stride, in_base, out_stride, out_base) in cells:
                xd = dm.to_device(pb.lcg_input(max(blocks), in_stride, fmt == 6, seed=3))
                yd = dm.to_device(pb.lcg_input(max(blocks), out_stride, fmt == 6, seed=4))
                for B in blocks:
                    us = {name: [] for name, _, _ in settings}
                    chains, copies, slow = {}, {}, set()

                    def call(r):
                        r.run_block_device(xd.data_ptr(), in_stride, in_base, yd.data_ptr(), out_stride, out_base, B, st)
                    for _ in range(a.rounds):
                        for name, r, opt in settings:
                            if name in slow:
                                continue
                            r.set_option("chain_copy", opt)
                            chains[name], copies[name] = r.core_info()["chains"], r.copy_info()
                            call(r)
                            w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            w0.record()
                            call(r)
                            w1.record()
                            torch.cuda.synchronize()
                            if w0.elapsed_time(w1) > a.slow_ms:
                                slow.add(name)
                                us[name].append(w0.elapsed_time(w1) * 1e3)
                                print(f"# format {fmt} cell {cell} block {B} {name}: one call of {us[name][0] / 1e6:.2f} s", flush=True)
                                continue
                            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                            for e0, e1 in ev:
                                e0.record()
                                call(r)
                                e1.record()
                            torch.cuda.synchronize()
                            us[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
                            print(f"# format {fmt} cell {cell} block {B} {name}: {len(us[name])} calls, median {statistics.median(us[name]):.1f} us", flush=True)
                    med = {name: statistics.median(v) for name, v in us.items()}
                    lines.append(dict(format=fmt, cell=cell, block=B, trees=T if cell == "a" else 0, pairs=2 * T if cell == "a" else P,
                                      **{f"{name}_us": round(m, 1) for name, m in med.items()},
                                      **{f"{name}_min_us": round(min(us[name]), 1) for name in us},
                                      lowered_chains=chains, copy_info=copies, calls={name: len(v) for name, v in us.items()}))
                    print(lines[-1], flush=True)
                del xd, yd
            for r in (listed, bare, alone):
                r.release()
    finally:
        for key in ("chain_copy", "chain_mem", "chain_delay", "chain_finish"):
            rt.Runtime.set_global_option(key, 0)
    print(json.dumps(dict(tool="copy_bench", lines=lines)))


if __name__ == "__main__":
    main()

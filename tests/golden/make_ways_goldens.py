#!/usr/bin/env python3
"""Generate tests/golden/ways_f2.npz, ways_f4.npz and ways_f6.npz from the COMPILED REFERENCE: two-way COPYXY / SWAPXY forks and runs of
GAIN / NEGX over 200 frames in blocks of 64, cores outer in blocks.  Core 1, behind a TPDF_CALC: the crossOver2ways
shape (LOAD_GAIN, COPYXY, BIQUADS, SAT0DB_TPDF, DELAY, STORE, SWAPXY, BIQUADS, GAIN, SAT0DB_TPDF_GAIN, STORE -- crossover2x2lfe.c:48-60)
with the delay behind the SAT0DB slot, and again with the delays in front of it in both ways; a trunk of one word.  Core 2: a LOAD_MEM
fork of that word, and chains with runs of one and of four operations.  Runs only where oracle/_ref has been built
(oracle/build_ref.sh); the fixtures are data -- program words, seeded inputs, the reference runtime's outputs, its final state area and
its program words behind the header.

    python tests/golden/make_ways_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import ways_programs as wp            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER, HEAD = 200, 64, 17, 24, 12


def cores():
    return [wp.core([wp.fork(wp.head(0.8), wp.way(nsec=2, finish="tpdf", slot="B", us=1000), wp.way(nsec=2, ops=[("gain", 0.7)], finish="tpdf_gain", gain=0.9)),
                     wp.fork(wp.head(0.6), wp.way(nsec=1, slot="A", us=63, finish="tpdf"), wp.way(nsec=3, ops=[("gain", -0.55)], slot="A", form="param", us=400, max_us=1000, finish="tpdf_gain", gain=1.1)),
                     wp.trunk("a", 1, 0.9)], calc=0),
            wp.core([wp.fork(wp.head(key="a"), wp.way(nsec=1), wp.way(nsec=0, ops=["neg"], finish="none")),
                     wp.chain(nsec=2, ops=[("gain", 0.53)], load_gain=None), wp.chain(nsec=0, ops=[("gain", 1.3), "neg", ("gain", -0.77), "neg"], stores=2)])]


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (2, 4, 6):
        prog, nin, nout, words = wp.program(fmt, cores())
        prog = prog.copy()
        x = pb.lcg_input(FRAMES, nin, fmt == 6, seed=SEED)
        rc, out, buf = po.run_reference(fmt, prog, x, nout, wp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
        assert rc >= 0, rc
        total = int(prog[1])
        state, after = buf[rc:rc + int(prog[2])], buf[HEAD:total]
        np.savez_compressed(os.path.join(OUT, f"ways_f{fmt}.npz"), prog=prog, out=out, state=state, words=after, x=x, rc=np.int64(rc),
                            mem=np.array(sorted(words.values()), dtype=np.int64),
                            meta=np.array([fmt, 48000, 1, DITHER, BLOCK, wp.IN, nout], dtype=np.int64))
        print(f"  ways_f{fmt}: rc={rc} out={out.shape} state={state.shape} words={after.shape}")


if __name__ == "__main__":
    main()

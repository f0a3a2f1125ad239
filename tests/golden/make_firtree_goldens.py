#!/usr/bin/env python3
"""Generate tests/golden/firtree_f4.npz and firtree_f6.npz from the COMPILED REFERENCE: a DSP_FIR in a trunk and in branches of a
memory-word tree over 200 frames in blocks of 64, cores outer in blocks.  Core 1: a trunk of 2 sections and a 31-tap
FIR, and three branches of its word -- 1 section and a 63-tap FIR; a 63-tap FIR alone; no FIR.  Core 2: branches of the same word,
which nobody there writes -- a 63-tap FIR alone, and 1 section with a 15-tap FIR: they see core 1's last frame of the block.  Runs only
where oracle/_ref has been built (oracle/build_ref.sh); the fixtures are data -- program words, seeded inputs, the reference runtime's
outputs, its final state area and its program words behind the header.

    python tests/golden/make_firtree_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import firtree_programs as tp         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER, HEAD = 200, 64, 11, 24, 12


def cores():
    return [tp.core([tp.trunk("a", 2, 31, 0.7), tp.branch("a", nsec=1, taps=63), tp.branch("a", nsec=0, taps=63, finish="none"), tp.branch("a", nsec=0, taps=0)]),
            tp.core([tp.branch("a", nsec=0, taps=63, stores=2), tp.branch("a", nsec=1, taps=15)])]


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (4, 6):
        prog, nin, nout, words = tp.program(fmt, cores())
        prog = prog.copy()
        x = pb.lcg_input(FRAMES, nin, fmt == 6, seed=SEED)
        rc, out, buf = po.run_reference(fmt, prog, x, nout, tp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
        assert rc >= 0, rc
        total = int(prog[1])
        state, after = buf[rc:rc + int(prog[2])], buf[HEAD:total]
        np.savez_compressed(os.path.join(OUT, f"firtree_f{fmt}.npz"), prog=prog, out=out, state=state, words=after, x=x, rc=np.int64(rc),
                            mem=np.array(sorted(words.values()), dtype=np.int64),
                            meta=np.array([fmt, 48000, 1, DITHER, BLOCK, tp.IN, nout], dtype=np.int64))
        print(f"  firtree_f{fmt}: rc={rc} out={out.shape} state={state.shape} words={after.shape}")


if __name__ == "__main__":
    main()

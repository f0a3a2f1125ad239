#!/usr/bin/env python3
"""Generate tests/golden/firtail_f4.npz and firtail_f6.npz from the COMPILED REFERENCE: one channel written the way the reference's
programs end theirs -- TPDF_CALC; LOAD_GAIN, 3 biquads, FIR of 100 taps, DELAY 1000 us, SAT0DB_TPDF_GAIN, STORE -- over 300 frames in
blocks of 64, in DSP_FORMAT 4 and 6.  Runs only where oracle/_ref has been built (oracle/build_ref.sh); the fixtures
are data -- program words, seeded inputs, the reference runtime's outputs and final state.

    python tests/golden/make_firtail_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import firtail_programs as fp         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER = 300, 64, 5, 24


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (4, 6):
        prog, nin, nout = fp.program(fmt, [fp.core([fp.chain(3, 100, "A", "fixed", 1000, finish="tpdf_gain", gain=0.9, load_gain=0.5)], calc=0)])
        x = pb.lcg_input(FRAMES, nin, fmt == 6, seed=SEED)
        rc, out, buf = po.run_reference(fmt, prog, x, nout, fp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
        assert rc >= 0, rc
        state = buf[rc:rc + int(prog[2])]
        np.savez_compressed(os.path.join(OUT, f"firtail_f{fmt}.npz"), prog=prog, x=x, out=out, state=state,
                            meta=np.array([fmt, 48000, 1, DITHER, BLOCK, fp.IN, nout, rc], dtype=np.int64))
        print(f"  firtail_f{fmt}: rc={rc} out={out.shape} state={state.shape}")


if __name__ == "__main__":
    main()

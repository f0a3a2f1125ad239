#!/usr/bin/env python3
"""Generate tests/golden/muxtail_f2.npz, muxtail_f4.npz and muxtail_f6.npz from the COMPILED REFERENCE: the shape of the reference's
generic DAC program (dspprogs/oktodac.c, dspDACStereoDsp4channels) -- four cores of LOAD_MUX(2), 12 biquads, SAT0DB, DELAY(parameter,
max 5000 us, default 0), STORE, STORE -- over 300 frames in blocks of 64.  Two variants: "a" as authored (every line
bypassed), "b" with the microsecond words edited to 2100, 1000, 63 and 5000 us and SAT0DB_TPDF_GAIN in the SAT0DB slot behind a head
TPDF_CALC.  Runs only where oracle/_ref has been built (oracle/build_ref.sh); the fixtures are data -- program words, seeded inputs,
the reference runtime's outputs and final state.

    python tests/golden/make_muxtail_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import muxtail_programs as mp         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER = 300, 64, 7, 24
EDITED_US = (2100, 1000, 63, 5000)


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (2, 4, 6):
        saved = {}
        for variant, finish in (("a", "sat"), ("b", "tpdf_gain")):
            prog, nin, nout = mp.program(fmt, mp.reference_shape_cores(finish))
            prog = prog.copy()
            if variant == "b":
                for word, us in zip(mp.us_words(prog), EDITED_US):
                    prog[word] = (int(prog[word]) & 0xFFFF0000) | us
                mp.resealed(prog)
            x = pb.lcg_input(FRAMES, nin, fmt == 6, seed=SEED)
            rc, out, buf = po.run_reference(fmt, prog, x, nout, mp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
            assert rc >= 0, rc
            state = buf[rc:rc + int(prog[2])]
            saved.update({f"prog_{variant}": prog, f"out_{variant}": out, f"state_{variant}": state, "x": x,
                          f"rc_{variant}": np.int64(rc),
                          "meta": np.array([fmt, 48000, 1, DITHER, BLOCK, mp.IN, nout], dtype=np.int64)})
            print(f"  muxtail_f{fmt} {variant}: rc={rc} out={out.shape} state={state.shape}")
        np.savez_compressed(os.path.join(OUT, f"muxtail_f{fmt}.npz"), **saved)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/copy_f2.npz, copy_f4.npz and copy_f6.npz from the COMPILED REFERENCE: DSP_LOAD_STORE lists beside chains
 over 200 frames in blocks of 64.  Two variants: "a", one core -- a head
list with a forwarded pair and two writers of one IO in front of the TPDF_CALC, two trunks, a list behind a trunk, a branch, a plain
chain, a list at the end that reads an earlier list's destination; "b", a core of pairs alone (the same head list) in front of a core
with one chain.  Runs only where oracle/_ref has been built (oracle/build_ref.sh); the fixtures are data -- program words, seeded
inputs, the reference runtime's outputs, its final state area and its program words behind the header.

    python tests/golden/make_copy_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import copy_programs as cp            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER, HEAD = 200, 64, 9, 24, 12
IN = cp.IN
HEAD_LIST = [(IN + 4, 20), (IN + 5, 21), (IN + 6, 24), (20, 25), (IN + 7, 26), (IN + 5, 26), (IN, 27)]      # 25 takes IN + 4; 26 is written twice


def cores_of(variant):
    if variant == "a":
        items = [cp.trunk("l", 2, 0.7), cp.trunk("r", 0, None), cp.copies([(IN + 8, 28)]), cp.branch("l", nsec=1, finish="sat"),
                 cp.plain(nsec=2, finish="sat"), cp.copies([(28, 29), (IN + 9, 30)])]
        return [cp.core(items, calc=0, head=[cp.copies(HEAD_LIST)])]
    return [cp.core([cp.copies(HEAD_LIST)]), cp.core([cp.plain(nsec=1, finish="sat")])]


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (2, 4, 6):
        saved = {}
        for variant in ("a", "b"):
            cores = cores_of(variant)
            prog, nin, nout = cp.program(fmt, cores)
            in_stride, out_stride = cp.windows(cores, nin, nout)
            x = pb.lcg_input(FRAMES, in_stride, fmt == 6, seed=SEED)
            rc, out, buf = po.run_reference(fmt, prog, x, out_stride, IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
            assert rc >= 0, rc
            total = int(prog[1])
            state, after = buf[rc:rc + int(prog[2])], buf[HEAD:total]
            live = {}
            for c in cores:
                live.update(cp.resolve(cp.all_pairs(c)))
            saved.update({f"prog_{variant}": prog, f"out_{variant}": out, f"state_{variant}": state, f"words_{variant}": after, f"x_{variant}": x,
                          f"rc_{variant}": np.int64(rc), f"live_{variant}": np.array(sorted(live.items()), dtype=np.int64),
                          f"meta_{variant}": np.array([fmt, 48000, 1, DITHER, BLOCK, IN, out_stride, nout], dtype=np.int64)})
            print(f"  copy_f{fmt} {variant}: rc={rc} out={out.shape} state={state.shape} words={after.shape} live={len(live)}")
        np.savez_compressed(os.path.join(OUT, f"copy_f{fmt}.npz"), **saved)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/memtree_f2.npz, memtree_f4.npz and memtree_f6.npz from the COMPILED REFERENCE: memory words between trunks and
branches over 300 frames in blocks of 64.  Two variants: "a", one core behind a head TPDF_CALC with trees (trunks of
2, 0 and 17 sections; branches with and without sections, delayed, dressed, stored twice, one not adjacent), ordinary chains between
them and branches of two words nobody writes, which the program holds non-zero values in; "b", the oktodac_diy arrangement -- trunks
in core 1, their branches in cores 2 and 3, cores outer in blocks, so that the branches see the trunks' last frame of the block -- with
a tree local to core 3.  Runs only where oracle/_ref has been built (oracle/build_ref.sh); the fixtures are data -- program words,
seeded inputs, the reference runtime's outputs, its final state area and its program words behind the header.

    python tests/golden/make_memtree_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import memtree_programs as mp         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER, HEAD = 300, 64, 7, 24, 12


def cores_of(variant):
    if variant == "a":
        items = [mp.trunk("a", 2, 0.7), mp.branch("a", nsec=3, slot="A", form="param", us=2100, finish="tpdf_gain"),
                 mp.plain(nsec=2, finish="tpdf"), mp.branch("a", nsec=0, finish="sat", stores=2), mp.trunk("b", 0, None),
                 mp.branch("w0", nsec=1, finish="gain"), mp.branch("b", nsec=0, slot="B", us=63, finish="tpdf"), mp.branch("a", nsec=17, finish="none"),
                 mp.trunk("c", 17, 0.5), mp.branch("c", nsec=0, finish="tpdf_gain"), mp.plain(nsec=0, slot="A", us=1000, finish="sat", load_gain=None),
                 mp.branch("w1", nsec=0, slot="A", us=1000, finish="sat"), mp.branch("c", nsec=16, slot="B", form="param", us=1000, finish="sat"),
                 mp.trunk("d", 1)]
        return [mp.core(items, calc=0)]
    return [mp.core([mp.trunk("l", 5, 0.7), mp.trunk("r", 0, None), mp.trunk("s", 17, 0.6)], calc=0),
            mp.core([mp.branch("l", nsec=4, slot="A", form="param", us=2100, finish="tpdf"), mp.branch("r", nsec=0, slot="B", us=21, finish="tpdf_gain"),
                     mp.plain(nsec=2, finish="tpdf_gain"), mp.branch("l", nsec=0, finish="none")]),
            mp.core([mp.branch("s", nsec=1, finish="gain"), mp.trunk("m", 2), mp.branch("r", nsec=16, slot="A", us=1000, finish="sat", stores=2),
                     mp.branch("m", nsec=3, finish="tpdf"), mp.branch("m", nsec=0, slot="A", form="param", us=63, finish="sat")])]


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (2, 4, 6):
        saved = {}
        for variant in ("a", "b"):
            prog, nin, nout, words = mp.program(fmt, cores_of(variant))
            prog = prog.copy()
            if variant == "a":
                mp.set_word(prog, words["w0"], 0.31, fmt)
                mp.set_word(prog, words["w1"], -0.24, fmt)
            x = pb.lcg_input(FRAMES, nin, fmt == 6, seed=SEED)
            rc, out, buf = po.run_reference(fmt, prog, x, nout, mp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
            assert rc >= 0, rc
            total = int(prog[1])
            state, after = buf[rc:rc + int(prog[2])], buf[HEAD:total]
            saved.update({f"prog_{variant}": prog, f"out_{variant}": out, f"state_{variant}": state, f"words_{variant}": after, f"x_{variant}": x,
                          f"rc_{variant}": np.int64(rc), f"mem_{variant}": np.array(sorted(words.values()), dtype=np.int64),
                          f"meta_{variant}": np.array([fmt, 48000, 1, DITHER, BLOCK, mp.IN, nout], dtype=np.int64)})
            print(f"  memtree_f{fmt} {variant}: rc={rc} out={out.shape} state={state.shape} words={after.shape}")
        np.savez_compressed(os.path.join(OUT, f"memtree_f{fmt}.npz"), **saved)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/sum_f2.npz, sum_f4.npz and sum_f6.npz from the COMPILED REFERENCE: sum heads over 200 frames in
blocks of 64, cores outer in blocks.  Core 1: tests/sum_programs.py's lfe_core(), the opcode sequence of crossover2x2lfe.c's core.
Core 2: two trunks, a three-term bus with one SUBXY (a - b ... + w), and buses of two constant words -- CASES below: in format 2 values
whose sum and difference wrap, in formats 4 and 6 +Inf and -Inf under ADDXY, one NaN operand on either side under ADDXY and under
SUBXY, and both operands NaN; some with a DELAY in slot A, whose line keeps to_sp of the sum.  Runs only where oracle/_ref has been
built (oracle/build_ref.sh); the fixtures are data -- program words, seeded inputs, the reference runtime's outputs, its final state
area and its program words behind the header.

    python tests/golden/make_sum_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from oracle import pyoracle as po                # noqa: E402
from tests import sum_programs as sp             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, SEED, DITHER, HEAD = 200, 64, 23, 24, 12

PINF, NINF, ONE, M3 = 0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000, 0xC008000000000000
NAN_A, NAN_B = 0x7FF8123400000000, 0xFFFA567800000000           # two quiet NaNs: payloads that survive the way to a float, signs apart
# (first word, second word, operation): X is the second word, Y the first
FLOAT_CASES = [(PINF, NINF, "ADDXY"), (NINF, NINF, "SUBXY"), (NAN_A, ONE, "ADDXY"), (ONE, NAN_A, "ADDXY"), (NAN_B, M3, "SUBXY"), (M3, NAN_B, "SUBXY"),
               (NAN_A, NAN_B, "ADDXY"), (NAN_B, NAN_A, "ADDXY"), (NAN_A, NAN_B, "SUBXY"), (NAN_B, NAN_A, "SUBXY")]
BOTH_NAN = [6, 7, 8, 9]
# (the int64 model: sums and differences that wrap, the low words telling them apart)
INT_CASES = [(0x7FFFFFFFFFFFFFFF, 0x0000000012345679, "ADDXY"), (0x7FFFFFFF0BADF00D, 0x8000000000000000, "SUBXY"), (0x0123456789ABCDEF, 0xF0F0F0F0F0F0F0F0, "ADDXY"),
             (0x0400000000001111, 0x0200000000003333, "SUBXY")]


def cases(fmt):
    return INT_CASES if fmt == 2 else FLOAT_CASES


def cores(fmt):
    """the constant buses: finish "none" (the float models store the sum's float as it is), every third with a line in slot A"""
    items = [sp.trunk("a", 1, 0.9), sp.trunk("b", 0, None), sp.bus(["a", "b", "w"], ["SUBXY", "ADDXY"], nsec=2, finish="tpdf")]
    for k, (_, _, op) in enumerate(cases(fmt)):
        items.append(sp.bus([f"u{k}", f"v{k}"], [op], nsec=0, finish="none", **(dict(slot="A", us=63) if k % 3 == 0 else {})))
    return [sp.lfe_core(), sp.core(items)]


def program(fmt):
    prog, nin, nout, words = sp.program(fmt, cores(fmt))
    prog = prog.copy()
    sp.set_word(prog, words["w"], -0.37, fmt)
    for k, (u, v, _) in enumerate(cases(fmt)):
        sp.set_word_bits(prog, words[f"u{k}"], u, fmt)
        sp.set_word_bits(prog, words[f"v{k}"], v, fmt)
    return prog, nin, nout, words


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (2, 4, 6):
        prog, nin, nout, words = program(fmt)
        x = pb.lcg_input(FRAMES, nin, fmt == 6, seed=SEED)
        rc, out, buf = po.run_reference(fmt, prog, x, nout, sp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
        assert rc >= 0, rc
        total = int(prog[1])
        state, after = buf[rc:rc + int(prog[2])], buf[HEAD:total]
        np.savez_compressed(os.path.join(OUT, f"sum_f{fmt}.npz"), prog=prog, out=out, state=state, words=after, x=x, rc=np.int64(rc),
                            mem=np.array(sorted(words.values()), dtype=np.int64),
                            meta=np.array([fmt, 48000, 1, DITHER, BLOCK, sp.IN, nout], dtype=np.int64))
        print(f"  sum_f{fmt}: rc={rc} out={out.shape} state={state.shape} words={after.shape}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/lowered_f2.npz, lowered_f4.npz and lowered_f6.npz from the COMPILED REFERENCE: the programs of
tests/lowered_programs.py's PINNED seeds (plain, LOAD_MUX, tree and pairs cores in one program; together the seeds hold
every form of lowered_programs.FORMS) over 200 frames in blocks of 64, cores outer in blocks, 48 kHz, random 1, dither 24.  Runs only
where oracle/_ref has been built (oracle/build_ref.sh); the reference runtime must load every program (its dspRuntimeInit checks header,
checksum and maxOpcode).  The fixtures are data -- per seed the program words, the input block (8-bit values, see input_block()), the
reference runtime's outputs, its final state area and the program words behind the header that it changed (index and value).

    python tests/golden/make_lowered_goldens.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po                # noqa: E402
from tests import lowered_programs as lp         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FRAMES, BLOCK, DITHER, HEAD = 200, 64, 24, lp.HEAD


def input_block(fmt, seed):
    """(the 8-bit values the fixture stores, the samples they stand for: value << 23 as int, value / 2^8 as float)"""
    v = np.random.default_rng(31000 + seed).integers(-128, 128, (FRAMES, lp.IN_STRIDE)).astype(np.int8)
    return v, samples_of(fmt, v)


def samples_of(fmt, v):
    return (v.astype(np.float32) / np.float32(256.0)) if fmt == 6 else (v.astype(np.int32) << 23)


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    for fmt in (2, 4, 6):
        data = dict(meta=np.array([fmt, 48000, 1, DITHER, BLOCK, lp.IN, FRAMES], dtype=np.int64), seeds=np.array(lp.PINNED[fmt], dtype=np.int64))
        forms = set()
        for seed in lp.PINNED[fmt]:
            prog, in_stride, out_stride, desc = lp.random_lowered_program(seed, fmt)
            v, x = input_block(fmt, seed)
            rc, out, buf = po.run_reference(fmt, prog, x, out_stride, lp.IN, 0, fs=48000, random=1, dither=DITHER, block=BLOCK, want_state=True)
            assert rc >= 0, (seed, fmt, rc)
            total = int(prog[1])
            changed = HEAD + np.nonzero(buf[HEAD:total] != prog[HEAD:total])[0]          # the program words the run changed (memory words)
            data.update({f"prog_{seed}": prog, f"x_{seed}": v, f"out_{seed}": out, f"state_{seed}": buf[rc:rc + int(prog[2])], f"words_at_{seed}": changed, f"words_{seed}": buf[changed],
                         f"rc_{seed}": np.int64(rc)})
            forms |= set().union(*[c["forms"] for c in desc["cores"]])
            print(f"  lowered_f{fmt} seed {seed}: rc={rc} out={out.shape} words={len(prog)} cores={[(c['cls'], c['chains']) for c in desc['cores']]}")
        path = os.path.join(OUT, f"lowered_f{fmt}.npz")
        np.savez_compressed(path, **data)
        print(f"  lowered_f{fmt}.npz: {os.path.getsize(path)} bytes, forms missing: {sorted(set(lp.FORMS) - forms)}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of the mixer programs (LOAD_MUX chain heads) from the COMPILED REFERENCE.

Runs only where oracle/_ref exists (oracle/build_ref.sh).  Every case of tests/mux_recipes.mixer_cases() goes through
pyoracle.run_reference -- the reference runtime itself, two blocks of ragged size -- and leaves its outputs and its whole state
area in tests/golden/<name>.npz, with tests/golden/mux_manifest.json naming the cases.  Data only:  python tests/golden/make_mux_goldens.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po                                   # noqa: E402
from tests.mux_recipes import mixer_cases, mixer_input, mixer_program   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    if not po.have_ref():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh first")
    manifest, total = [], 0
    for case in mixer_cases():
        fmt = case["fmt"]
        prog = mixer_program(case["program"])
        x = mixer_input(case["input"], fmt)
        rc, out, buf = po.run_reference(fmt, prog, x, case["out_stride"], case["in_base"], case["out_base"],
                                        block=case["block"], want_state=True)
        assert rc >= 0, (case["name"], rc)
        state = buf[rc:rc + int(prog[2])]
        path = os.path.join(OUT, case["name"] + ".npz")
        np.savez_compressed(path, out=out, state=state)
        total += os.path.getsize(path)
        manifest.append(dict(case, init_rc=rc, prog_sha=sha(prog), in_sha=sha(x), out_sha=sha(out), state_sha=sha(state)))
        print(f"  {case['name']}: rc={rc} out={out.shape} state={state.shape}")
    with open(os.path.join(OUT, "mux_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(f"{len(manifest)} cases, {total / 1024:.0f} KB")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Sweep (GPU box): seeded programs over the whole grammar that the seven opt-in options lower (tests/lowered_programs.py, DESIGN.md
4.2m) -- plain, LOAD_MUX, tree and pairs cores side by side -- played in ragged blocks with a drawn event between blocks (the other block
call, an in-place call, an option toggled off and on, another kernel, a live parameter edit, a checkpoint into a fresh runtime, a
reset, a shard) against the oracle: outputs, state area and program words after every block, word for word.
python tests/dev/gpu_lowered_sweep.py LO HI [FORMATS, e.g. 2,4,6]
(tests/test_gpu_lowered_sweep.py runs a slice of the seeds in the -m gpu suite)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from avdsp_amd import runtime as rt            # noqa: E402
from tests import lowered_programs as lp       # noqa: E402


def options_back():
    """every option the player touches back at its default, and the library's device state released"""
    for key in lp.OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    for key, _, default in lp.IMPLS:
        rt.Runtime.set_global_option(key, default)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def run(lo, hi, formats=(2, 4, 6)):
    """seeds lo .. hi-1; returns (runs, list of mismatch descriptions)"""
    bad, n = [], 0
    try:
        for seed in range(lo, hi):
            for fmt in formats:
                bad += lp.play(seed, fmt, device=True)
                n += 1
    finally:
        options_back()
    return n, bad


if __name__ == "__main__":
    fmts = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (2, 4, 6)
    import time
    n, bad = 0, []
    for seed in range(int(sys.argv[1]), int(sys.argv[2])):                  # seed by seed: a line each, with its time
        t0 = time.time()
        k, b = run(seed, seed + 1, fmts)
        n, bad = n + k, bad + b
        for m in b:
            print("MISMATCH", m, flush=True)
        print(f"seed {seed}: {k} runs, {len(b)} bad, {time.time() - t0:.2f} s", flush=True)
    print("runs", n, "bad", len(bad))

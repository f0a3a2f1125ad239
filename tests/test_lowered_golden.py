"""The oracle pinned to the COMPILED REFERENCE on the programs of tests/lowered_programs.py (no GPU):
tests/golden/lowered_f{2,4,6}.npz hold what the reference runtime made of the PINNED seeds (tests/golden/make_lowered_goldens.py: 200
frames in blocks of 64, cores outer; the reference runtime loaded every program) -- the oracle reproduces outputs, final state and
program words bit for bit, and the generator still makes the stored words, so the fixtures and the device sweep cannot drift apart."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import lowered_programs as lp
from tests.golden.make_lowered_goldens import samples_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(fmt, seed) for fmt in sorted(lp.PINNED) for seed in lp.PINNED[fmt]]


def fixture(fmt):
    return np.load(os.path.join(GOLDEN, f"lowered_f{fmt}.npz"))


@pytest.mark.parametrize("fmt, seed", CASES)
def test_oracle_reproduces_the_reference_on_lowered_programs(fmt, seed):
    g = fixture(fmt)
    f, fs, random, dither, block, in_base, frames = [int(v) for v in g["meta"]]
    assert f == fmt and seed in g["seeds"].tolist()
    prog, want = g[f"prog_{seed}"], g[f"out_{seed}"]
    x = samples_of(fmt, g[f"x_{seed}"])
    assert x.shape == (frames, lp.IN_STRIDE) and x.dtype == po.sample_dtype(fmt)
    o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
    assert o.rc == int(g[f"rc_{seed}"])
    out = o.run_block(x, want.shape[1], in_base, 0, block=block)
    assert (out.view(np.uint32) == want.view(np.uint32)).all(), np.nonzero((out.view(np.uint32) != want.view(np.uint32)).any(axis=0))[0][:8]
    assert (o.state == g[f"state_{seed}"]).all(), np.nonzero(o.state != g[f"state_{seed}"])[0][:8]
    total = int(prog[1])
    after = prog.copy()
    after[g[f"words_at_{seed}"]] = g[f"words_{seed}"]                            # (the fixture holds the words the reference run changed)
    assert (o.buf[lp.HEAD:total] == after[lp.HEAD:total]).all(), np.nonzero(o.buf[lp.HEAD:total] != after[lp.HEAD:total])[0][:8]


@pytest.mark.parametrize("fmt, seed", CASES)
def test_the_generator_still_makes_the_pinned_words(fmt, seed):
    prog, _, out_stride, _ = lp.random_lowered_program(seed, fmt)
    g = fixture(fmt)
    assert len(prog) == len(g[f"prog_{seed}"]) and (prog == g[f"prog_{seed}"]).all() and out_stride == g[f"out_{seed}"].shape[1]


def test_the_pinned_seeds_hold_every_form():
    forms = set().union(*[c["forms"] for fmt, seed in CASES for c in lp.random_lowered_program(seed, fmt)[3]["cores"]])
    assert forms == set(lp.FORMS), sorted(set(lp.FORMS) - forms)
    assert all(os.path.getsize(os.path.join(GOLDEN, f"lowered_f{fmt}.npz")) < (1 << 20) for fmt in lp.PINNED)

"""The oracle against the reference runtime on DSP_LOAD_STORE lists beside chains ("chain_copy"): variant "a", one core
with a head list (a forwarded pair, two writers of one IO) in front of the TPDF_CALC, two trunks, a list behind a trunk, a branch, a
plain chain and a list at the end; variant "b", a core of pairs alone in front of a core with one chain.  tests/golden/copy_f{2,4,6}.npz
hold the programs, the inputs and what the compiled reference made of them (tests/golden/make_copy_goldens.py); the oracle -- which the
GPU tests are held to -- must reproduce the outputs, the final state area and the program words behind the header bit for bit, and
the live pairs the host's resolution names must be what the reference's frame shows.  CPU only."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR

HEAD = 12


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_oracle_reproduces_the_reference_on_copy_lists(fmt, variant):
    g = np.load(os.path.join(GOLDEN_DIR, f"copy_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, out_stride, nout = (int(v) for v in g[f"meta_{variant}"])
    assert f == fmt and (out_stride, nout) == ((31, 2) if variant == "a" else (28, 1))
    prog = g[f"prog_{variant}"]
    o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
    assert o.rc == int(g[f"rc_{variant}"])
    x, want = g[f"x_{variant}"], g[f"out_{variant}"]
    out = np.concatenate([o.run_block(x[a:a + block], out_stride, in_base) for a in range(0, len(x), block)])
    assert out.shape == want.shape
    assert (np.ascontiguousarray(out).view(np.uint32) == want.view(np.uint32)).all()
    assert (o.state == g[f"state_{variant}"]).all()
    assert (o.buf[HEAD:int(prog[1])] == g[f"words_{variant}"]).all()
    # the reference itself: every live pair's column is its source's input column word for word (no mask, no conversion), the
    # forwarded pair and the last of two writers among them; columns nobody writes stay zero
    live = {int(d): int(s) for d, s in g[f"live_{variant}"]}
    assert len(live) == (9 if variant == "a" else 6) and live[25] == in_base + 4 and live[26] == in_base + 5
    for d, s in live.items():
        assert (want.view(np.uint32)[:, d] == x.view(np.uint32)[:, s - in_base]).all(), (d, s)
    untouched = [c for c in range(nout, out_stride) if c not in live]
    assert untouched and not want.view(np.uint32)[:, untouched].any()

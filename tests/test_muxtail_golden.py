"""The oracle against the reference runtime on the shape of the reference's generic DAC program ("mux_tail"): four cores
of LOAD_MUX(2), 12 biquads, SAT0DB, DELAY(parameter), STORE, STORE -- as authored (0 us: every line bypassed), and with edited delays
and SAT0DB_TPDF_GAIN in the SAT0DB slot.  tests/golden/muxtail_f{2,4,6}.npz hold the programs, the input and what the compiled reference
made of them (tests/golden/make_muxtail_goldens.py); the oracle -- which the GPU tests are held to -- must reproduce outputs and the final
state area bit for bit.  CPU only."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_oracle_reproduces_the_reference_on_the_dac_program_shape(fmt, variant):
    g = np.load(os.path.join(GOLDEN_DIR, f"muxtail_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, nout = (int(v) for v in g["meta"])
    assert f == fmt and nout == 8
    o = po.OracleProgram(fmt, g[f"prog_{variant}"], fs=fs, random=random, dither=dither)
    assert o.rc == int(g[f"rc_{variant}"])
    x, want = g["x"], g[f"out_{variant}"]
    out = np.concatenate([o.run_block(x[a:a + block], nout, in_base) for a in range(0, len(x), block)])
    assert out.shape == want.shape and np.abs(want.astype(np.float64)).max() > 0
    assert (np.ascontiguousarray(out).view(np.uint32) == want.view(np.uint32)).all()
    assert (o.state == g[f"state_{variant}"]).all()
    if variant == "b":                                         # the delays do something: the two variants differ
        assert (g["out_a"].view(np.uint32) != want.view(np.uint32)).any()

"""The oracle against the reference runtime on a channel that ends the way handed FIR chains do ("fir_tail"):
TPDF_CALC; LOAD_GAIN, biquads, FIR, DELAY, SAT0DB_TPDF_GAIN, STORE.  tests/golden/firtail_f{4,6}.npz hold the program, the input and
what the compiled reference made of them (tests/golden/make_firtail_goldens.py); the oracle -- which the GPU tests are held to -- must
reproduce outputs and the final state area bit for bit.  CPU only."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR


@pytest.mark.parametrize("fmt", [4, 6])
def test_oracle_reproduces_the_reference_on_a_handed_fir_channel(fmt):
    g = np.load(os.path.join(GOLDEN_DIR, f"firtail_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, nout, rc = (int(v) for v in g["meta"])
    assert f == fmt
    o = po.OracleProgram(fmt, g["prog"], fs=fs, random=random, dither=dither)
    assert o.rc == rc
    x = g["x"]
    out = np.concatenate([o.run_block(x[a:a + block], nout, in_base) for a in range(0, len(x), block)])
    assert out.shape == g["out"].shape and np.abs(g["out"].astype(np.float64)).max() > 0
    assert (np.ascontiguousarray(out).view(np.uint32) == g["out"].view(np.uint32)).all()
    assert (o.state == g["state"]).all()

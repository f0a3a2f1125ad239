"""The oracle against the reference runtime on a DSP_FIR in a trunk and in branches of a memory-word tree ("mem_fir"):
core 1, a trunk of 2 sections and a 31-tap FIR and three branches of its word (1 section + a 63-tap FIR; a 63-tap FIR alone; no FIR);
core 2, branches of that word, which nobody there writes (a 63-tap FIR alone, stored twice; 1 section + a 15-tap FIR), cores outer in
blocks.  tests/golden/firtree_f{4,6}.npz hold the program, the input and what the compiled reference made of them
(tests/golden/make_firtree_goldens.py); the oracle -- which the GPU tests are held to -- must reproduce the outputs, the final state
area and the program words behind the header bit for bit.  CPU only.

The first test is a pin of the ORACLE alone: it loads no library and sets no option, so it passes on any commit that has the fixture --
unlike the other new tests it does not fail where "mem_fir" is unknown.  The second one does: it asks the library what "mem_fir" makes
of the fixture's program."""
import os

import numpy as np
import pytest

from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR

HEAD = 12


@pytest.mark.parametrize("fmt", [4, 6])
def test_oracle_reproduces_the_reference_on_fir_trees(fmt):
    g = np.load(os.path.join(GOLDEN_DIR, f"firtree_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, nout = (int(v) for v in g["meta"])
    assert f == fmt and nout == 6 and len(g["x"]) == 200
    prog = g["prog"]
    o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
    assert o.rc == int(g["rc"])
    x, want = g["x"], g["out"]
    out = np.concatenate([o.run_block(x[a:a + block], nout, in_base) for a in range(0, len(x), block)])
    assert out.shape == want.shape and (np.abs(want.astype(np.float64)).max(axis=0) > 0).all()
    assert (np.ascontiguousarray(out).view(np.uint32) == want.view(np.uint32)).all()
    assert (o.state == g["state"]).all()
    after = o.buf[HEAD:int(prog[1])]
    assert (after == g["words"]).all()
    # of the program words only the memory word has changed: the trunk's FIR sum of the last frame
    changed = np.nonzero(after != prog[HEAD:int(prog[1])])[0] + HEAD
    mem = set(int(w) for w in g["mem"]) | set(int(w) + 1 for w in g["mem"])
    assert len(changed) >= 1 and set(changed.tolist()) <= mem


@pytest.mark.parametrize("fmt", [4, 6])
def test_the_fixture_program_is_what_mem_fir_lowers(fmt):
    """host-only: both cores of the fixture's program go to the chain kernels under "chain_mem" and "mem_fir", and not without the latter"""
    g = np.load(os.path.join(GOLDEN_DIR, f"firtree_f{fmt}.npz"))
    try:
        r = rt.Runtime(fmt, g["prog"].copy(), fs=48000, random=1, dither=24)
        r.set_option("chain_mem", 1)
        assert [r.mem_info(k) for k in (0, 1)] == [(0, 0, 0)] * 2
        r.set_option("mem_fir", 1)
        assert [r.core_info(k) for k in (0, 1)] == [dict(chains=4, max_sections=2, max_taps=63), dict(chains=2, max_sections=1, max_taps=63)]
        assert [r.mem_fir_info(k) for k in (0, 1)] == [(1, 2, 0), (0, 2, 0)] and [r.mem_info(k) for k in (0, 1)] == [(1, 3, 0), (0, 2, 2)]
    finally:
        for key in ("mem_fir", "chain_mem"):
            rt.Runtime.set_global_option(key, 0)
        rt.lib().dspRuntimeRelease()

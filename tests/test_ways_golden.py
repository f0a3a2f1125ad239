"""The oracle against the reference runtime on two-way COPYXY / SWAPXY forks and runs of GAIN / NEGX ("chain_ways"): core
1, the crossOver2ways shape with the delay behind the SAT0DB slot and again with delays in front of it in both ways, and a trunk; core
2, a LOAD_MEM fork of the trunk's word and chains with runs of one and of four operations, cores outer in blocks.
tests/golden/ways_f{2,4,6}.npz hold the program, the input and what the compiled reference made of them
(tests/golden/make_ways_goldens.py); the oracle -- which the GPU tests are held to -- must reproduce the outputs, the final state area
and the program words behind the header bit for bit.  CPU only.

The first test is a pin of the ORACLE alone: it loads no library and sets no option, so it passes on any commit that has the fixture
and the builder.  The others fail where "chain_ways" is unknown: they ask the library what the option makes of the fixture's program."""
import os

import numpy as np
import pytest

from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import ways_programs as wp
from tests.golden.make_ways_goldens import cores
from tests.golden_recipes import GOLDEN_DIR

HEAD = 12
FMTS = [2, 4, 6]


@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_reproduces_the_reference_on_forks_and_way_operations(fmt):
    g = np.load(os.path.join(GOLDEN_DIR, f"ways_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, nout = (int(v) for v in g["meta"])
    assert f == fmt and nout == 9 and len(g["x"]) == 200
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
    # of the program words only the memory word has changed: the trunk's accumulator of the last frame
    changed = np.nonzero(after != prog[HEAD:int(prog[1])])[0] + HEAD
    mem = set(int(w) for w in g["mem"]) | set(int(w) + 1 for w in g["mem"])
    assert len(changed) >= 1 and set(changed.tolist()) <= mem


@pytest.mark.parametrize("fmt", FMTS)
def test_the_builder_still_makes_the_stored_words(fmt):
    g = np.load(os.path.join(GOLDEN_DIR, f"ways_f{fmt}.npz"))
    prog, nin, nout, words = wp.program(fmt, cores())
    assert (prog == g["prog"]).all() and nin == g["x"].shape[1] and nout == g["out"].shape[1] and sorted(words.values()) == g["mem"].tolist()


@pytest.mark.parametrize("fmt", FMTS)
def test_the_fixture_program_is_what_chain_ways_lowers(fmt):
    """host-only: both cores of the fixture's program go to the chain kernels under "chain_ways" (with the options of what stands in the
    ways), and neither without it"""
    g = np.load(os.path.join(GOLDEN_DIR, f"ways_f{fmt}.npz"))
    keys = ("chain_finish", "chain_delay", "chain_mem")
    try:
        r = rt.Runtime(fmt, g["prog"].copy(), fs=48000, random=1, dither=24)
        for key in keys:
            r.set_option(key, 1)
        assert [r.ways_info(k) for k in (0, 1)] == [(0, 0)] * 2
        r.set_option("chain_ways", 1)
        assert [r.core_info(k) for k in (0, 1)] == [dict(chains=5, max_sections=3, max_taps=0), dict(chains=4, max_sections=2, max_taps=0)], r.last_error()
        assert [r.ways_info(k) for k in (0, 1)] == [(2, 2), (1, 3)] == [wp.counts(c)[0] for c in cores()]
        assert r.delay_info(0) == (3, 47) and r.finish_info(0) == (4, 1) and r.mem_info(0) == (1, 0, 0) and r.mem_info(1) == (0, 2, 2)
    finally:
        for key in keys + ("chain_ways",):
            rt.Runtime.set_global_option(key, 0)
        rt.lib().dspRuntimeRelease()

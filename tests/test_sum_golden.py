"""The oracle against the reference runtime on sum heads ("chain_sum"): core 1, the opcode sequence of
crossover2x2lfe.c's core (tests/sum_programs.py, lfe_core); core 2, two trunks, a three-term bus with one SUBXY and buses of two
constant words -- in format 2 sums and differences that wrap, in formats 4 and 6 +Inf and -Inf, one NaN operand on either side under
ADDXY and SUBXY, and both operands NaN --, cores outer in blocks.  tests/golden/sum_f{2,4,6}.npz hold the program, the input and what
the compiled reference made of them (tests/golden/make_sum_goldens.py); the oracle -- which the GPU tests are held to -- must reproduce
the outputs, the final state area and the program words behind the header bit for bit.  CPU only.

The first test is a pin of the ORACLE alone: it loads no library and sets no option.  The last fails where "chain_sum" is unknown: it
asks the library what the option makes of the fixture's program."""
import os

import numpy as np
import pytest

from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import sum_programs as sp
from tests.golden.make_sum_goldens import cases, cores, program
from tests.golden_recipes import GOLDEN_DIR

HEAD = 12
FMTS = [2, 4, 6]


@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_reproduces_the_reference_on_sum_heads(fmt):
    g = np.load(os.path.join(GOLDEN_DIR, f"sum_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, nout = (int(v) for v in g["meta"])
    assert f == fmt and nout == 6 + len(cases(fmt)) and len(g["x"]) == 200
    prog = g["prog"]
    o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
    assert o.rc == int(g["rc"])
    x, want = g["x"], g["out"]
    out = np.concatenate([o.run_block(x[a:a + block], nout, in_base) for a in range(0, len(x), block)])
    assert out.shape == want.shape
    got, ref = np.ascontiguousarray(out).view(np.uint32), want.view(np.uint32)
    assert (got == ref).all(), np.nonzero((got != ref).any(axis=0))[0].tolist()
    assert (ref[:, :6] != 0).any(axis=0).all()                 # (the LFE core's outputs and the three-term bus carry signal)
    assert (o.state == g["state"]).all()
    after = o.buf[HEAD:int(prog[1])]
    assert (after == g["words"]).all()
    # of the program words only the trunks' memory words have changed: a sum head writes none
    changed = np.nonzero(after != prog[HEAD:int(prog[1])])[0] + HEAD
    mem = set(int(w) for w in g["mem"]) | set(int(w) + 1 for w in g["mem"])
    assert len(changed) >= 1 and set(changed.tolist()) <= mem


def test_the_constant_cases_reach_inf_and_nan():
    """what the fixture's constant buses store in format 6, the float itself: the default NaN where the infinities cancel, a lone NaN
    operand's payload whichever side it stands on, and of two NaNs X's -- the second word's (the first operand of the reference's SSE
    instruction)"""
    g = np.load(os.path.join(GOLDEN_DIR, "sum_f6.npz"))
    a, b, d = 0x7FC091A0, 0xFFD2B3C0, 0xFFC00000              # NAN_A and NAN_B as floats, the default NaN
    bits = g["out"][:, 6:].view(np.uint32)
    assert bits[3:].tolist() == [[d, d, a, a, b, b, b, a, b, a]] * 197
    assert bits[:3, [0, 3, 6, 9]].tolist() == [[0] * 4] * 3     # (the lines of 3 samples in slot A)


@pytest.mark.parametrize("fmt", FMTS)
def test_the_builder_still_makes_the_stored_words(fmt):
    g = np.load(os.path.join(GOLDEN_DIR, f"sum_f{fmt}.npz"))
    prog, nin, nout, words = program(fmt)
    assert (prog == g["prog"]).all() and nin == g["x"].shape[1] and nout == g["out"].shape[1] and sorted(words.values()) == g["mem"].tolist()


@pytest.mark.parametrize("fmt", FMTS)
def test_the_fixture_program_is_what_chain_sum_lowers(fmt):
    """host-only: both cores of the fixture's program go to the chain kernels under "chain_sum" (with the options of what stands behind
    the heads), and neither without it"""
    g = np.load(os.path.join(GOLDEN_DIR, f"sum_f{fmt}.npz"))
    keys = ("chain_finish", "chain_delay", "chain_mem", "chain_ways")
    try:
        r = rt.Runtime(fmt, g["prog"].copy(), fs=48000, random=1, dither=24)
        for key in keys:
            r.set_option(key, 1)
        assert [r.mem_info(k) for k in (0, 1)] == [(0, 0, 0)] * 2
        r.set_option("chain_sum", 1)
        n = len(cases(fmt))
        assert [r.sum_info(k) for k in (0, 1)] == [(1, 2), (1 + n, 3 + 2 * n)] == [sp.counts(c)[0] for c in cores(fmt)], r.last_error()
        assert [r.core_info(k)["chains"] for k in (0, 1)] == [7, 3 + n] and r.ways_info(0) == (2, 2)
        assert r.mem_info(0) == (2, 1, 0) and r.mem_info(1) == (2, 1 + n, 0)
    finally:
        for key in keys + ("chain_sum",):
            rt.Runtime.set_global_option(key, 0)
        rt.lib().dspRuntimeRelease()

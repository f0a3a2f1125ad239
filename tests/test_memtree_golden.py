"""The oracle against the reference runtime on memory words between trunks and branches ("chain_mem"): variant "a", one
core with trees, ordinary chains and branches of words nobody writes (given non-zero values in the program); variant "b", the
oktodac_diy arrangement, trunks in core 1 and their branches in cores 2 and 3, cores outer in blocks.  tests/golden/memtree_f{2,4,6}.npz
hold the programs, the inputs and what the compiled reference made of them (tests/golden/make_memtree_goldens.py); the oracle -- which
the GPU tests are held to -- must reproduce the outputs, the final state area and the program words behind the header bit for bit.
CPU only."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR

HEAD = 12


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_oracle_reproduces_the_reference_on_memory_trees(fmt, variant):
    g = np.load(os.path.join(GOLDEN_DIR, f"memtree_f{fmt}.npz"))
    f, fs, random, dither, block, in_base, nout = (int(v) for v in g[f"meta_{variant}"])
    assert f == fmt and nout == (11 if variant == "a" else 9)
    prog = g[f"prog_{variant}"]
    o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
    assert o.rc == int(g[f"rc_{variant}"])
    x, want = g[f"x_{variant}"], g[f"out_{variant}"]
    out = np.concatenate([o.run_block(x[a:a + block], nout, in_base) for a in range(0, len(x), block)])
    assert out.shape == want.shape and (np.abs(want.astype(np.float64)).max(axis=0) > 0).sum() >= nout - 1
    assert (np.ascontiguousarray(out).view(np.uint32) == want.view(np.uint32)).all()
    assert (o.state == g[f"state_{variant}"]).all()
    after = o.buf[HEAD:int(prog[1])]
    assert (after == g[f"words_{variant}"]).all()
    # the memory words among them: every trunk has left its last frame (the words nobody writes keep what the program gave them)
    changed = np.nonzero(after != prog[HEAD:int(prog[1])])[0] + HEAD
    mem = set(int(w) for w in g[f"mem_{variant}"]) | set(int(w) + 1 for w in g[f"mem_{variant}"])
    assert len(changed) >= 4 and set(changed.tolist()) <= mem

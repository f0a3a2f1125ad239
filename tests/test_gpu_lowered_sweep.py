"""A slice of tests/dev/gpu_lowered_sweep.py in the -m gpu suite: seeded programs over the whole grammar that the seven
opt-in options lower -- plain, LOAD_MUX, tree and pairs cores side by side in one program -- in ragged blocks with an event between
blocks, against the oracle bit for bit after every block: the whole output block over a sentinel, the whole state area, the program
words behind the header.  tests/test_lowered_programs.py (no GPU) shows that every core of these seeds is on the chain kernels with the
options on and on the interpreter with them off, and which pairs of forms the seeds hold."""
import pytest

from tests import lowered_programs as lp
from tests.dev import gpu_lowered_sweep as sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options_back():
    yield
    sweep.options_back()


@pytest.mark.parametrize("name, fmt, seeds", lp.GPU_CASES, ids=[c[0] for c in lp.GPU_CASES])
def test_lowered_programs_match_the_oracle(name, fmt, seeds):
    runs, bad = 0, []
    for s in seeds:
        f, seed = (fmt, s) if fmt else s
        n, b = sweep.run(seed, seed + 1, (f,))
        runs, bad = runs + n, bad + b
    assert runs == len(seeds) and not bad, "\n".join(bad)

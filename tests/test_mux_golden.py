"""The oracle against the compiled reference on the mixer programs (LOAD_MUX chain heads; tests/golden/make_mux_goldens.py made the
vectors): outputs and the whole state area, bit for bit, every case of the manifest -- and the manifest holds every case of the recipe."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR
from tests.mux_recipes import mixer_cases, mixer_input, mixer_program

with open(os.path.join(GOLDEN_DIR, "mux_manifest.json")) as _f:
    MANIFEST = json.load(_f)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_manifest_holds_every_case():
    want = mixer_cases()
    assert [c["name"] for c in MANIFEST] == [c["name"] for c in want]
    assert len({c["name"] for c in want}) == len(want)
    for got, c in zip(MANIFEST, want):
        assert all(got[k] == v for k, v in c.items()), c["name"]
    # the dimensions the cases must span
    progs = [c["program"] for c in want]
    for fmt in (2, 4, 6):
        mine = [p for p in progs if p["fmt"] == fmt]
        assert {p["entries"] for p in mine} == {1, 3, 17, 64, 200}
        assert {p["lists"] for p in mine} == {"shared", "shuffled", "twice", "private"}
        assert {p["sections"] for p in mine} == {0, 2, 17}
        assert {p["sat"] for p in mine} == {0, 1}
        assert {bool(p["taps"]) for p in mine} == ({False} if fmt == 2 else {False, True})
    assert all(0 < c["block"] < c["input"]["frames"] and c["input"]["frames"] % c["block"] for c in want)      # two ragged blocks
    assert any(c["input"]["kind"] == "special" for c in want)


@pytest.mark.parametrize("case", MANIFEST, ids=lambda c: c["name"])
def test_oracle_reproduces_reference_on_mixers(case):
    fmt = case["fmt"]
    prog = mixer_program(case["program"])
    x = mixer_input(case["input"], fmt)
    assert sha(prog) == case["prog_sha"], "program recipe drifted from the one the golden was made with"
    assert sha(x) == case["in_sha"]
    o = po.OracleProgram(fmt, prog)
    assert o.rc == case["init_rc"]
    out = o.run_block(x, case["out_stride"], case["in_base"], case["out_base"], block=case["block"])
    g = np.load(os.path.join(GOLDEN_DIR, case["name"] + ".npz"))
    assert (out.view(np.uint32) == g["out"].view(np.uint32)).all(), f"{case['name']}: output differs from the reference's"
    assert (o.state == g["state"]).all(), f"{case['name']}: state area differs from the reference's"
    assert sha(out) == case["out_sha"] and sha(o.state) == case["state_sha"]

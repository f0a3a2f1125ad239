"""The plans of a tree core's slices ("shard_trees"), without a GPU.  tests/csrc/shard_trees_layout_driver.cpp holds the
shapes of tests/shard_tree_programs.py as chain descriptors, cuts each with avdsp_amd/csrc/avdsp_shard_cut.h for 2, 3 and 8 ranks and
lays out every rank's slice with avdsp_amd/csrc/avdsp_plan_layout.h, built against the two headers alone with AddressSanitizer and
UBSan and run as a program of its own (the way tests/test_firtree_layout.py builds its driver).  Every index of every slice's tables
lies inside what the plan allocates, no branch whose trunk is in the core is laid out as a branch of a constant word, and the C rule
cuts where avdsp_amd/sharding.py tree_shard_bounds() does."""
import json
import os
import shutil
import subprocess

import pytest

from avdsp_amd import sharding as sh
from tests import shard_tree_programs as stp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("shardtreeslayout")
    flags = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    # whether the sanitizers can be built and run here at all is asked of a trivial program; the driver itself must then build
    probe_src, probe = str(tmp / "probe.cpp"), str(tmp / "probe")
    with open(probe_src, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    p = subprocess.run(flags + ["-o", probe, probe_src], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([probe], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).returncode != 0:
        pytest.skip("sanitizer build not available here: " + p.stderr[-300:])
    exe = str(tmp / "shard_trees_layout_driver")
    cmd = flags + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
                   os.path.join(ROOT, "tests", "csrc", "shard_trees_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the layout driver does not build:\n" + r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name", sorted(stp.SHAPES))
def test_every_slice_lays_out_inside_its_buffers(driver, name):
    r = subprocess.run([driver, name], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    t = json.loads(r.stdout)
    items = stp.SHAPES[name][0]()
    assert t["chains"] == len(items) and t["tree_of"] == stp.tree_of(items)          # the driver's shape is the programs' shape
    assert t["refused"] == 0 and t["error"] == "" and t["bad_indices"] == 0 and t["misclassified"] == 0
    for world in stp.WORLDS:
        w = t["worlds"][str(world)]
        assert w["bounds"] == sh.tree_shard_bounds(t["tree_of"], world)
        # a constant word in a slice is one the core does not write: the branches of "w" keys
        lo_hi = list(zip(w["bounds"], w["bounds"][1:]))
        assert w["constant"] == [len({it["key"] for it in items[a:b] if it["kind"] == "branch" and it["key"].startswith("w")}) for a, b in lo_hi]
    assert t["slices"] == sum(b > a for world in stp.WORLDS for a, b in zip(t["worlds"][str(world)]["bounds"], t["worlds"][str(world)]["bounds"][1:]))

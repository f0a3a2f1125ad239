"""What "mem_fir"  adds to a chain plan's host-side tables (avdsp_amd/csrc/avdsp_plan_layout.h), without a GPU: a FIR
in a trunk -- its row, the `fir_trunk` list, a cascade that feeds the ring instead of handing over -- and in a branch -- a column and a
phase-1 cascade that feeds the ring, or, for a FIR alone, a ring feed of mem_stage and the kLoadFed load mode --, the `fir`, `fir_plain`
and `fir_hand` lists, the hand-over rows, every index against what the plan allocates, and every refusal.
tests/csrc/firtree_layout_driver.cpp is built against that header alone with AddressSanitizer and UBSan and run as a program of its
own (the way tests/test_memtree_layout.py builds its driver); what it prints is compared with literal values that follow from the rules."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, GAIN, RAW, FED = 0, 1, 2, 5            # AVDSP_LOAD_PLAIN, _GAIN; kLoadRaw, kLoadFed (device-side only)
ROW, SAMPLE, WORD = 0, 1, 2                   # MemTree::src


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("firtreelayout")
    flags = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    # whether the sanitizers can be built and run here at all is asked of a trivial program; the driver itself must then build
    probe_src, probe = str(tmp / "probe.cpp"), str(tmp / "probe")
    with open(probe_src, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    p = subprocess.run(flags + ["-o", probe, probe_src], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([probe], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).returncode != 0:
        pytest.skip("sanitizer build not available here: " + p.stderr[-300:])
    exe = str(tmp / "firtree_layout_driver")
    cmd = flags + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
                   os.path.join(ROOT, "tests", "csrc", "firtree_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the layout driver does not build:\n" + r.stderr[-3000:]
    return exe


def run(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


def test_fir_trunks_branches_feeds_rows_and_lists(driver):
    """chains: 0 trunk of word 100 (2 sections, 31 taps), 1 ordinary (1 section, 63 taps), 2 branch (1 section, 63 taps), 3 branch (63
    taps alone, SAT0DB), 4 branch (3 sections, no FIR), 5 trunk of word 104 (7 taps alone), 6 branch of it (255 taps alone, delay A),
    7 branch (17 sections, 700 taps, dressed), 8 branch of word 200, which nobody writes (1500 taps alone), 9 branch of it (delay B, no
    FIR), 10 ordinary (2 sections, 63 taps, delay B), 11 trunk of word 106 (2 sections, no FIR), 12 branch of it (SAT0DB)"""
    t = run(driver, "tree")
    assert t["has_mem"] == 1 and t["counts"] == [3, 8, 2] and t["bad_indices"] == 0 and t["max_taps"] == 1500
    # [word, src, trunk, row, col0, ncol, first_own, n_own]: a trunk with a FIR is read from its row like one with a cascade alone
    assert t["trees"] == [[100, ROW, 0, 0, 0, 2, 0, 0], [104, ROW, 5, 1, 2, 1, 0, 0], [106, ROW, 11, 2, 3, 0, 0, 1], [200, WORD, -1, 3, 3, 0, 1, 0]]
    assert t["col_tree"] == [0, 0, 1] and t["cols"] == 3 and t["tiles"] == [[0, 4, 0, 3]]
    # the branches that are a FIR alone: no column, no record of the stage's own, no row of the tree's -- a ring feed
    assert t["feeds"] == [[0, 3], [1, 6], [3, 8]] and t["feed_start"] == [0, 1, 2, 2, 3]
    assert t["own"] == [12] and t["stored"] == [0] * 12 + [1]
    assert t["kind"] == [1, 0, 2, 2, 2, 1, 2, 2, 2, 2, 0, 1, 2]
    assert t["load_mode"] == [GAIN, PLAIN, RAW, FED, RAW, PLAIN, FED, RAW, FED, RAW, PLAIN, GAIN, RAW]
    assert t["in_io"] == [64, 65, 0, 0, 1, 69, 0, 2, 0, 0, 74, 75, 0]
    # every chain with a FIR has a ring; the trunks' launch, the plain one and the handed one each take their list
    assert t["fir"] == [0, 1, 2, 3, 5, 6, 7, 8, 10]
    assert t["fir_trunk"] == [0, 5] and t["fir_plain"] == [1, 2, 3, 8] and t["fir_hand"] == [6, 7, 10]
    # rows: the three trunks', the one the stage fills for branch 9, then a row of its own for every handed FIR chain
    assert t["rows"] == 7 and t["hand_row"] == [0, -1, -1, -1, -1, 1, 4, 5, -1, 3, 6, 2, -1]
    assert t["tail"] == [6, 7, 9, 10] and t["pass"] == [] and t["pass_dressed"] == []
    assert t["io_in"] == [64, 75] and t["io_out"] == [1, 12]
    assert t["overlap_ok"] == 0 and t["all_rows"] == 0 and t["shared"] == 0


def test_cascades_in_front_of_a_fir_feed_the_ring(driver):
    g = run(driver, "tree")["groups"]
    assert [(x["nsec"], x["phase"], x["wide"], x["hand"], x["all_fir"], x["ids"]) for x in g] == [
        (2, 0, 0, 0, 1, [0, 10]),     # the FIR trunk beside an ordinary handed FIR chain: neither WIDE nor HAND, the FIRs stand behind
        (1, 0, 0, 0, 1, [1]),
        (1, 1, 0, 0, 1, [2]),         # a branch's cascade on the branch block, into the ring
        (3, 1, 0, 0, 0, [4]),
        (17, 1, 0, 0, 1, [7]),        # dressed behind its FIR: the cascade is an ordinary one
        (2, 0, 1, 1, 0, [11])]        # a trunk without a FIR hands over as ever
    assert [x["to_ring"] for x in g] == [[1, 1], [1], [1], [0], [1], []] and g[4]["pieces"] == 2


def test_feed_lists_across_tiles(driver):
    """17 trees (one more than a tile holds); tree 3 has 5 branches that are a FIR alone, tree 5 has 70 columns and closes its tile, tree
    16 -- in the second tile -- has 17 feeds"""
    t = run(driver, "feeds")
    assert t["bad_indices"] == 0 and t["counts"] == [17, 92, 0] and t["rows"] == 17 and t["cols"] == 70
    assert t["tiles"] == [[0, 6, 0, 70], [6, 11, 70, 0]]
    assert t["feed_start"] == [0] * 4 + [5] * 13 + [22]
    assert t["feeds"] == [[3, c] for c in range(17, 22)] + [[16, c] for c in range(92, 109)]
    assert t["fir"] == t["fir_plain"] == list(range(17, 22)) + list(range(92, 109)) and t["fir_trunk"] == [] and t["fir_hand"] == []
    assert [t["load_mode"][c] for c in (17, 21, 22, 91, 92, 108)] == [FED, FED, RAW, RAW, FED, FED]
    assert [(x["nsec"], x["phase"], x["hand"], len(x["ids"])) for x in t["groups"]] == [(1, 0, 1, 17), (1, 1, 0, 70)]


@pytest.mark.parametrize("scenario", ["plain", "memtree"])
def test_plans_without_a_tree_fir_are_as_before(driver, scenario):
    """a plan without memory words, and a "chain_mem" plan without FIRs: the same tables with the flag on and off"""
    on, off = run(driver, scenario), run(driver, scenario + "_off")
    assert on == off and "error" not in on and on["feeds"] == [] and on["feed_start"] == [] and on["fir_trunk"] == []
    assert on["has_mem"] == (scenario == "memtree")


@pytest.mark.parametrize("scenario, text", [
    ("tree_off", "chain 0: a FIR beside memory words has no kernel"),              # without the flag every text stays
    ("trunk_fir_off", "chain 0: a FIR beside memory words has no kernel"),
    ("branch_fir_off", "chain 0: a FIR beside memory words has no kernel"),
    ("beside_off", "chain 1: a FIR beside memory words has no kernel"),
    ("format2", "chain 0: a FIR beside memory words has no kernel"),              # (the flag means formats 4 and 6)
    ("no_fir_tail", "chain 1: a delay line has no kernel here"),
    ("no_fir_tail_dressed", "chain 1: a dressed finish has no kernel here"),
    ("trunk_taps_high", "chain 0: FIR addresses words outside the loaded buffer"),
    ("trunk_history_high", "chain 0: FIR addresses words outside the loaded buffer"),
    ("branch_taps_high", "chain 1: FIR addresses words outside the loaded buffer"),
    ("branch_history_negative", "chain 1: FIR addresses words outside the loaded buffer"),
    ("trunk_stored", "chain 0: not a trunk"),
    ("trunk_delayed", "chain 0: not a trunk"),
    ("groups", "FIR groups beside memory words have no kernel"),
])
def test_refusals(driver, scenario, text):
    assert run(driver, scenario) == {"error": text}


@pytest.mark.parametrize("scenario, lists", [
    ("trunk_fir", ([0], [0], [], [])),
    ("branch_fir", ([0], [], [0], [])),
    ("beside", ([1], [], [1], [])),
    ("trunk_history_last", ([0], [0], [], [])),                                   # the history's last word is the buffer's last
])
def test_the_smallest_plans(driver, scenario, lists):
    t = run(driver, scenario)
    assert (t["fir"], t["fir_trunk"], t["fir_plain"], t["fir_hand"]) == lists and t["bad_indices"] == 0

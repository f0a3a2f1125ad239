"""The "chain_mem" stage of a chain plan's host-side tables (avdsp_amd/csrc/avdsp_plan_layout.h, mem_trees), without a
GPU: the trees, their hand-over rows, the columns of the branch block, mem_stage's tiles, the two phases of cascade launches, who
finishes what, and every word index outside the buffer refused.  tests/csrc/memtree_layout_driver.cpp is built against that header
alone with AddressSanitizer and UBSan and run as a program of its own (the way tests/test_plan_layout.py builds its driver); it holds
the scenarios, what it prints is compared with literal values that follow from the rules."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN, RAW = 1, 2                              # AVDSP_LOAD_GAIN; kLoadRaw, device-side only
ROW, SAMPLE, WORD = 0, 1, 2                   # MemTree::src


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("memtreelayout") / "memtree_layout_driver")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "memtree_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    return exe


def run(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


def test_trees_rows_columns_and_who_finishes_what(driver):
    """chains: 0 trunk of word 100 (2 sections), 1 ordinary, 2 branch (3 sections), 3 branch (none, SAT0DB), 4 branch (none, delay), 5 trunk
    of word 104 (no sections), 6 branch of it (none, delay), 7 and 8 branches of word 200, which nobody writes (17 sections; none, dressed),
    9 branch of word 100 again (1 section, delay), 10 ordinary, 11 a passthrough"""
    t = run(driver, "tree")
    assert t["has_mem"] == 1 and t["counts"] == [2, 7, 2]
    # [word, src, trunk, row, col0, ncol, first_own, n_own]: trees with a trunk first, in program order, then the words nobody writes
    assert t["trees"] == [[100, ROW, 0, 0, 0, 2, 0, 1], [104, SAMPLE, 5, 1, 2, 0, 1, 0], [200, WORD, -1, -1, 2, 1, 1, 1]]
    assert t["col_tree"] == [0, 0, 2] and t["cols"] == 3          # the columns of a tree are consecutive, also for branches that are not adjacent
    assert t["own"] == [3, 8] and t["stored"] == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert t["kind"] == [1, 0, 2, 2, 2, 1, 2, 2, 2, 2, 0, 0]
    # branches with sections read their column as it is; trunks and ordinary chains keep their head and their IO
    assert [t["load_mode"][i] for i in (2, 7, 9)] == [RAW] * 3 and [t["in_io"][i] for i in (2, 7, 9)] == [0, 2, 1]
    assert t["load_mode"][0] == GAIN and t["in_io"][0] == 64 and t["in_io"][5] == 69
    # rows: the trunk with sections (read by the stage and by branch 4), one the stage fills for branch 6, one of branch 9's own cascade
    assert t["rows"] == 3 and t["hand_row"] == [0, -1, -1, -1, 0, -1, 1, -1, -1, 2, -1, -1]
    assert t["tail"] == [4, 6, 9] and t["pass"] == [11] and t["pass_dressed"] == []
    assert t["tiles"] == [[0, 3, 0, 3]]
    # the input window: trunks and ordinary chains only; the output window: every STORE
    assert t["io_in"] == [64, 75] and t["io_out"] == [1, 11]
    assert t["overlap_ok"] == 0 and t["all_rows"] == 0


def test_two_phases_of_launch_groups(driver):
    g = run(driver, "tree")["groups"]
    assert [(x["nsec"], x["phase"], x["wide"], x["hand"], x["ids"]) for x in g] == [
        (2, 0, 1, 1, [0]),            # the trunk: WIDE + HAND
        (1, 0, 0, 0, [1, 10]),        # ordinary chains stay on the caller's block
        (3, 1, 0, 0, [2]),
        (17, 1, 0, 0, [7]),
        (1, 1, 1, 1, [9])]            # a delayed branch hands over to chain_tail like any delayed chain -- not in the ordinary group of its length
    assert g[3]["pieces"] == 2 and all(x["pieces_in_phase"] for x in g)


def test_tiles_close_at_16_trees_or_64_columns(driver):
    t = run(driver, "tiles")
    assert t["cols"] == 111 and t["rows"] == 41 and t["counts"] == [42, 111, 0]
    assert t["tiles"] == [[0, 16, 0, 16], [16, 16, 16, 16], [32, 9, 32, 78], [41, 1, 110, 1]]
    assert t["trees"][40] == [400, ROW, 80, 40, 40, 70, 0, 0] and t["trees"][41] == [402, SAMPLE, 151, -1, 110, 1, 0, 0]
    assert t["col_tree"] == list(range(40)) + [40] * 70 + [41]
    assert [(x["nsec"], x["phase"], len(x["ids"])) for x in t["groups"]] == [(1, 0, 41), (1, 1, 110), (2, 1, 1)]


def test_a_plan_without_memory_words_is_as_before(driver):
    on, off = run(driver, "plain"), run(driver, "plain_off")
    assert on == off and on["has_mem"] == 0 and on["trees"] == [] and on["tiles"] == []
    assert all(x["phase"] == 0 for x in on["groups"])
    assert on["all_rows"] == 16                                     # two 16-lane groups: the table of all rows is still made
    assert on["hand_row"] == [-1, -1, 0, -1, -1, -1] and on["tail"] == [2] and on["pass"] == [3]


@pytest.mark.parametrize("scenario, text", [
    ("tree_off", "chain 0: a memory word has no kernel here"),
    ("trunk_off", "chain 0: a memory word has no kernel here"),
    ("branch_off", "chain 1: load mode 4"),                                   # check_heads goes on refusing a load mode it does not know
    ("word_high", "chain 0: memory word outside the loaded buffer"),          # its second word is the first behind the buffer
    ("word_zero", "chain 0: memory word outside the loaded buffer"),
    ("branch_high", "chain 0: memory word outside the loaded buffer"),
    ("branch_negative", "chain 0: memory word outside the loaded buffer"),
    ("format3", "memory words have no kernels in format 3"),
    ("instances", "memory words have no chain instances"),
    ("mux", "memory words beside LOAD_MUX chains have no kernels"),
    ("two_trunks", "chain 1: a second trunk of memory word 100"),
    ("overlap", "chain 1: its memory word overlaps another"),
    ("lag", "chain 0: a branch in front of its trunk"),
    ("fir", "chain 1: a FIR beside memory words has no kernel"),
    ("branch_fir", "chain 0: a FIR beside memory words has no kernel"),
    ("stored_trunk", "chain 0: not a trunk"),
    ("trunk_from_mem", "chain 0: not a trunk"),
])
def test_refusals(driver, scenario, text):
    assert run(driver, scenario) == {"error": text}


def test_the_last_two_words_of_the_buffer_are_a_word(driver):
    t = run(driver, "word_last")
    assert t["trees"] == [[4094, ROW, 0, 0, 0, 0, 0, 0]] and t["tiles"] == [[0, 1, 0, 0]] and t["hand_row"] == [0]

"""Way operations in a chain plan's host-side tables (avdsp_amd/csrc/avdsp_plan_layout.h; "chain_ways"), without a GPU:
a chain with a run of GAIN / NEGX is a tail chain exactly as a delayed one is -- its record in `tail`, a hand-over row where a cascade
or the memory-word stage fills one, its cascade group WIDE + HAND, never a passthrough and never one of the stage's own stores -- and a
plan without way operations takes exactly the tables it took, with the flag on and off.  tests/csrc/ways_layout_driver.cpp is built
against that header alone with AddressSanitizer and UBSan and run as a program of its own (the way tests/test_memtree_layout.py builds
its driver); it holds the scenarios, what it prints is compared with literal values that follow from the rules."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW, SAMPLE = 0, 1                            # MemTree::src


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("wayslayout")
    flags = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    # skipped only where the sanitizers' runtimes are missing (an empty program does not link); any other build error is a failure
    empty = tmp / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    r = subprocess.run(flags + ["-o", str(tmp / "empty"), str(empty)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    exe = str(tmp / "ways_layout_driver")
    cmd = flags + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
                   os.path.join(ROOT, "tests", "csrc", "ways_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "ways_layout_driver.cpp does not build:\n" + r.stderr[-3000:]
    return exe


def run(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


@pytest.mark.parametrize("scenario", ["ways", "ways_format2", "ways_format4"])
def test_tail_records_rows_and_who_finishes_what(driver, scenario):
    """chains: 0 ordinary (2 sections), 1 operations behind 2 sections, 2 operations behind the head, 3 delayed (1 section), 4 operations
    and a delay behind 17 sections, 5 a passthrough, 6 operations and a dressed finish behind the head, 7 trunk of word 100 (1 section),
    8 branch of it without sections, with operations, 9 branch without sections or operations, 10 trunk of word 104 (no sections), 11
    and 12 branches of it with operations (none, 2 sections), 13 dressed (2 sections)"""
    t = run(driver, scenario)
    assert t["way_ops"] == 7
    # every chain with operations is chain_tail's, in program order beside the delayed chain; none is a passthrough or dressed passthrough
    assert t["tail"] == [1, 2, 3, 4, 6, 8, 11, 12] and t["pass"] == [5] and t["pass_dressed"] == [] and t["dressed"] == 2
    # rows: mem_trees' first (the trunk with sections; the one the stage fills for branch 11), then one per tail chain with a cascade.
    # Branch 8 reads its trunk's row; chains 2 and 6 have none: chain_tail loads their sample itself
    assert t["rows"] == 6 and t["hand_row"] == [-1, 2, -1, 3, 4, -1, -1, 0, 0, -1, -1, 1, 5, -1]
    assert t["mem_row"] == [-1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, 1, -1, -1]
    # [word, src, trunk, row, col0, ncol, first_own, n_own]: tree 1's trunk has no sections, the row is there for branch 11 alone
    assert t["trees"] == [[100, ROW, 7, 0, 0, 0, 0, 1], [104, SAMPLE, 10, 1, 0, 1, 1, 0]]
    # the stage finishes branch 9 and only it: a branch with operations is not a MemOwn
    assert t["own"] == [9] and t["stored"] == [0] * 9 + [1] + [0] * 4


def test_cascade_groups_are_wide_and_hand(driver):
    g = run(driver, "ways")["groups"]
    assert [(x["nsec"], x["phase"], x["wide"], x["hand"], x["ids"]) for x in g] == [
        (2, 0, 0, 0, [0]),            # the ordinary chain keeps its biquad_row group ...
        (2, 0, 1, 1, [1]),            # ... a chain with operations of the same length is WIDE + HAND, a group of its own
        (1, 0, 1, 1, [3, 7]),         # the delayed chain and the trunk, as before
        (17, 0, 1, 1, [4]),
        (2, 1, 1, 1, [12]),           # a branch with sections and operations: phase 1, handed like a delayed branch
        (2, 0, 1, 0, [13])]           # dressed, no operations: WIDE alone
    assert g[0]["rows"] == 1 and all(x["rows"] == 0 for x in g[1:])           # (no biquad_row records for WIDE groups)
    # of a long cascade only the last piece hands over, and only it keeps the run
    assert g[3]["piece_nsec"] == [9, 8] and g[3]["piece_wide"] == [0, 1] and g[3]["piece_hand"] == [0, 1] and g[3]["piece_ways_n"] == [0, 2]


def test_a_plan_without_way_operations_takes_the_tables_it_took(driver):
    """delayed, dressed, long, passthrough, a trunk with a plain, a delayed and a stage-finished branch: flag on and off, the same JSON"""
    on, off = run(driver, "plain"), run(driver, "plain_off")
    assert on == off and on["way_ops"] == 0
    assert on["tail"] == [2, 8] and on["pass"] == [3] and on["own"] == [9] and on["rows"] == 2 and on["hand_row"] == [-1, -1, 1, -1, -1, -1, 0, -1, 0, -1]
    assert [(x["nsec"], x["phase"], x["wide"], x["hand"]) for x in on["groups"]] == [(1, 0, 0, 0), (2, 0, 1, 0), (1, 0, 1, 1), (17, 0, 0, 0), (3, 0, 0, 0), (2, 0, 1, 1), (1, 1, 0, 0)]


@pytest.mark.parametrize("scenario, text", [
    ("ways_off", "chain 1: way operations have no kernel here"),           # avdsp_plan_desc::chain_ways 0
    ("format3", "chain 0: way operations have no kernel here"),
    ("format5", "chain 0: way operations have no kernel here"),
    ("instances", "chain 0: way operations have no kernel here"),
    ("fir", "chain 0: way operations have no kernel here"),
    ("mux", "chain 0: way operations have no kernel here"),
    ("five", "chain 0: 5 way operations"),
    ("negative", "chain 0: -1 way operations"),
    ("bad_op", "chain 0: way operation 3"),
    ("trunk", "chain 0: not a trunk"),
])
def test_records_the_device_library_refuses(driver, scenario, text):
    assert run(driver, scenario) == {"error": text}

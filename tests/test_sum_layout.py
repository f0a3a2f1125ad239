"""Sum heads in a chain plan's host-side tables (avdsp_amd/csrc/avdsp_plan_layout.h; "chain_sum"), without a GPU: every
sum head is a tree of its own behind all word trees, without word and trunk, its one branch the head's chain -- a column, one of the
stage's own stores, the tree's row for chain_tail or a feed, as any branch --, its terms in a table beside the trees, each from where
a LOAD_MEM of its word takes the accumulator; a plan without sum heads takes exactly the tables it took, with the flag on and off.
tests/csrc/sum_layout_driver.cpp is built against that header alone with AddressSanitizer and UBSan and run as a program of its own
(the way tests/test_ways_layout.py builds its driver); it holds the scenarios, what it prints is compared with literal values that
follow from the rules."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW, SAMPLE, WORD, SUM = 0, 1, 2, 3           # MemTree::src, MemTerm::src
ADD, SUB = 1, 2                               # AVDSP_SUM_*
GAIN, RAW, FED = 1, 2, 5                      # AVDSP_LOAD_GAIN, kLoadRaw, kLoadFed
G0, G1 = 0x3F000000, 0x3F000001               # the driver's trunk gains


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("sumlayout")
    flags = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    # skipped only where the sanitizers' runtimes are missing (an empty program does not link); any other build error is a failure
    empty = tmp / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    r = subprocess.run(flags + ["-o", str(tmp / "empty"), str(empty)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    exe = str(tmp / "sum_layout_driver")
    cmd = flags + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
                   os.path.join(ROOT, "tests", "csrc", "sum_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "sum_layout_driver.cpp does not build:\n" + r.stderr[-3000:]
    return exe


def run(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


@pytest.mark.parametrize("scenario", ["sum", "sum_format2", "sum_format4"])
def test_sum_trees_terms_and_who_finishes_what(driver, scenario):
    """chains: 0 trunk of word 100 (2 sections), 1 trunk of word 104 (none), 2 branch of 100 (1 section), 3 branch of 108, which nobody
    writes, 4 bus 100 + 104 - 108 with 2 sections, 5 bus 108 + 108 without, 6 bus 104 + 112 with a delay line, 7 bus 100 + 104 with way
    operations, 8 ordinary, 9 bus 104 + 100 with a section and a delay line"""
    t = run(driver, scenario)
    # [word, src, trunk, row, col0, ncol, first_own, n_own]: three word trees in program order, then a sum tree per head -- no word, no
    # trunk; the row of trees 5 and 6 is one the stage FILLS for chain_tail
    assert t["trees"] == [[100, ROW, 0, 0, 0, 1, 0, 0], [104, SAMPLE, 1, -1, 1, 0, 0, 0], [108, WORD, -1, -1, 1, 0, 0, 1],
                          [0, SUM, -1, -1, 1, 1, 1, 0], [0, SUM, -1, -1, 2, 0, 1, 1], [0, SUM, -1, 1, 2, 0, 2, 0], [0, SUM, -1, 2, 2, 0, 2, 0], [0, SUM, -1, -1, 2, 1, 2, 0]]
    assert t["sums"] == 5 and t["branches"] == 7 and t["constant"] == 1 and t["cols"] == 3
    # [src, row, word, in_io, load_mode, gain_bits, op]: word 100 from its trunk's row, word 104 as load_stage of its trunk's sample (never
    # a row), words 108 and 112 -- 112 has no tree at all -- from the mirror; the first term of a head has no operation
    t100, t104 = [ROW, 0, 100, 64, GAIN, G0], [SAMPLE, -1, 104, 65, GAIN, G1]
    assert t["sum_start"] == [0, 0, 0, 0, 3, 5, 7, 9, 11]
    assert t["terms"] == [t100 + [0], t104 + [ADD], [WORD, -1, 108, 0, 0, 0, SUB],
                          [WORD, -1, 108, 0, 0, 0, 0], [WORD, -1, 108, 0, 0, 0, ADD],
                          t104 + [0], [WORD, -1, 112, 0, 0, 0, ADD],
                          t100 + [0], t104 + [ADD],
                          t104 + [0], t100 + [ADD]]
    # who finishes what: branch 3 and bus 5 the stage itself; buses 6 and 7 chain_tail, from the rows the stage fills; bus 9 chain_tail
    # from its own cascade's row; buses 4 and 9 are kLoadRaw chains of columns 1 and 2
    assert t["own"] == [3, 5] and t["stored"] == [0, 0, 0, 1, 0, 1, 0, 0, 0, 0] and t["tail"] == [6, 7, 9] and t["pass"] == []
    assert t["rows"] == 4 and t["mem_row"] == [0, -1, -1, -1, -1, -1, 1, 2, -1, -1] and t["hand_row"] == [0, -1, -1, -1, -1, -1, 1, 2, -1, 3]
    assert t["col_tree"] == [0, 3, 7] and t["load"] == [GAIN, GAIN] + [RAW] * 6 + [0, RAW] and t["in_io"] == [64, 65, 0, 0, 1, 0, 0, 0, 72, 2]
    assert t["kind"] == [1, 1, 2, 2, 2, 2, 2, 2, 0, 2] and t["tiles"] == [[0, 8, 0, 3]]
    # a head loads no IO: the input span is the trunks' and the ordinary chain's
    assert t["io_in"] == [64, 72] and t["io_out"] == [2, 9]
    assert [(g["nsec"], g["phase"], g["wide"], g["hand"], g["ids"]) for g in t["groups"]] == [
        (2, 0, 1, 1, [0]), (1, 1, 0, 0, [2]), (2, 1, 0, 0, [4]), (1, 0, 0, 0, [8]), (1, 1, 1, 1, [9])]


def test_a_lone_fir_behind_the_head_is_a_feed_of_the_sum_tree(driver):
    t = run(driver, "feed")
    assert t["trees"] == [[100, ROW, 0, 0, 0, 0, 0, 0], [0, SUM, -1, -1, 0, 0, 0, 0]]
    assert t["feed"] == [1] and t["feed_start"] == [0, 0, 1] and t["sum_start"] == [0, 0, 2] and t["load"] == [GAIN, FED] and t["fir"] == [1]
    assert t["own"] == [] and t["cols"] == 0


@pytest.mark.parametrize("n", [15, 16, 17])
def test_sum_trees_across_the_tile_seam(driver, n):
    """3 word trees, then n sum trees (every third without sections): the tile of 16 trees closes inside the sum trees"""
    t = run(driver, f"seam{n}")
    assert len(t["trees"]) == 3 + n and [x[1] for x in t["trees"]] == [ROW, SAMPLE, WORD] + [SUM] * n and t["sums"] == n
    cols = [0 if k % 3 == 0 else 1 for k in range(n)]
    first = 2 + sum(cols[:13])                               # columns in front of tree 16: the two branches' and 13 sum trees'
    assert t["tiles"] == [[0, 16, 0, first], [16, 3 + n - 16, first, sum(cols[13:])]]
    assert t["sum_start"] == [0, 0, 0] + [3 * k for k in range(n + 1)]
    assert t["col_tree"] == [0, 2] + [3 + k for k in range(n) if cols[k]]
    assert t["own"] == [3] + [5 + k for k in range(n) if not cols[k]]
    assert all(x[4] == sum(cols[:k]) + 2 and x[5] == cols[k] for k, x in enumerate(t["trees"][3:]))


def test_a_plan_without_sum_heads_takes_the_tables_it_took(driver):
    """ordinary chains, a trunk with a plain, a delayed and a stage-finished branch, a trunk without sections and a branch with way
    operations, a constant branch of 17 sections: flag on and off, the same JSON, and no table of the sum trees"""
    on, off = run(driver, "plain"), run(driver, "plain_off")
    assert on == off and on["sums"] == 0 and on["terms"] == [] and on["sum_start"] == []
    assert on["trees"] == [[100, ROW, 2, 0, 0, 1, 0, 1], [104, SAMPLE, 6, 1, 1, 0, 1, 0], [108, WORD, -1, -1, 1, 1, 1, 0]]
    assert on["tail"] == [4, 7] and on["pass"] == [1] and on["own"] == [5] and on["rows"] == 2 and on["tiles"] == [[0, 3, 0, 2]]


@pytest.mark.parametrize("scenario, text", [
    ("sum_off", "chain 4: a sum head has no kernel here"),                 # avdsp_plan_desc::chain_sum 0
    ("eight", "chain 0: 8 sum terms"),
    ("negative", "chain 0: -1 sum terms"),
    ("bad_op", "chain 0: sum operation 3"),
    ("word_outside", "chain 0: memory word of a sum term outside the loaded buffer"),
    ("word_zero", "chain 0: memory word of a sum term outside the loaded buffer"),
    ("head_outside", "chain 0: memory word outside the loaded buffer"),
    ("overlap", "chain 1: the memory word of a sum term overlaps another"),
    ("before_trunk", "chain 1: a sum term in front of its trunk"),
    ("sum_trunk", "chain 0: a sum head that is a trunk"),
    ("sum_trunk_load_mem", "chain 0: a sum head that is a trunk"),
    ("no_branch", "chain 0: a sum head that is no branch"),
    ("format3", "memory words have no kernels in format 3"),
])
def test_records_the_device_library_refuses(driver, scenario, text):
    assert run(driver, scenario) == {"error": text}

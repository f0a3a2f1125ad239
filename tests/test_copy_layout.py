"""The "chain_copy" stage of a chain plan's host-side tables (avdsp_amd/csrc/avdsp_plan_layout.h, copy_list), without a
GPU: the live pairs sorted by destination, the IO spans and stores_whole_window with them, a plan without pairs left as it was, and
every plan copy_pairs could not run refused with a text.  tests/csrc/copy_layout_driver.cpp is built against that header alone with
AddressSanitizer and UBSan and run as a program of its own (the way tests/test_memtree_layout.py builds its driver); it holds the
scenarios, what it prints is compared with literal values that follow from the rules."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("copylayout") / "copy_layout_driver")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "copy_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    return exe


def run(driver, scenario):
    r = subprocess.run([driver, scenario], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


def test_pairs_are_sorted_by_destination_and_join_the_spans(driver):
    """chains 64 -> 0 and 65 -> 1 (2 sections each), 66 -> 2 (none); pairs 70 -> 9, 64 -> 5, 70 -> 3, 71 -> 12, 90 -> 4"""
    t = run(driver, "sort")
    assert t["dst"] == [3, 4, 5, 9, 12] and t["src"] == [70, 90, 64, 70, 71]
    assert t["io_in"] == [64, 90] and t["io_out"] == [0, 12]
    assert t["whole"] == 0                                     # 3 stores + 5 pairs in a span of 13
    assert t["groups"][:2] == [2, 2] and t["pass"] == [2] and t["dev_chains"] == 3          # the chains' tables do not know of the pairs
    assert t["ahead"] == [] and t["overlap_ok"] == 0


def test_a_plan_of_pairs_alone(driver):
    t = run(driver, "alone")
    assert t["dst"] == [1, 2, 3] and t["src"] == [9, 8, 8]
    assert t["io_in"] == [8, 9] and t["io_out"] == [1, 3] and t["whole"] == 1
    assert t["groups"] == [] and t["pass"] == [] and t["dev_chains"] == 0 and t["all_rows"] == 0


def test_stores_whole_window_counts_the_pairs_its_span_includes(driver):
    assert run(driver, "whole_chains")["whole"] == 1 and run(driver, "whole_chains")["io_out"] == [0, 2]
    t = run(driver, "whole")                                   # pairs at 3 and 4 behind the chains' 0, 1, 2
    assert t["whole"] == 1 and t["io_out"] == [0, 4]
    t = run(driver, "hole")                                    # a pair at 5: 3 and 4 are untouched slots of the window
    assert t["whole"] == 0 and t["io_out"] == [0, 5]


def test_a_plan_without_pairs_is_as_before(driver):
    on, off = run(driver, "plain"), run(driver, "plain_off")
    assert on == off and on["src"] == [] and on["dst"] == []
    assert on["io_in"] == [64, 66] and on["io_out"] == [0, 2] and on["whole"] == 1 and on["pass"] == [2] and on["groups"][:2] == [2, 2]


def test_pairs_beside_load_mux_lists(driver):
    t = run(driver, "mux_ok")                                  # a source may be an IO a list names
    assert t["dst"] == [8, 9] and t["src"] == [80, 64] and t["io_in"] == [64, 80] and t["io_out"] == [0, 9]


def test_a_delayed_chain_may_keep_no_store(driver):
    """chain 1 stores nothing (its STOREs are repeated by a later chain): chain_tail runs it for its line; the others as before"""
    t = run(driver, "storeless_delay")
    assert t["tail"] == [1] and t["pass"] == [2] and t["io_out"] == [0, 2] and t["whole"] == 0 and t["dev_chains"] == 3
    assert run(driver, "storeless_off") == {"error": "chain 1: bad IO"}
    assert run(driver, "storeless_plain") == {"error": "chain 1: bad IO"}


@pytest.mark.parametrize("scenario, text", [
    ("flag_off", "LOAD_STORE pairs have no kernel here"),
    ("instances", "LOAD_STORE pairs have no chain instances"),
    ("null_list", "bad LOAD_STORE pair list"),
    ("src_high", "pair 0: IO 65536 -> 9 outside [0,65536)"),
    ("src_negative", "pair 0: IO -1 -> 9 outside [0,65536)"),
    ("dst_high", "pair 0: IO 70 -> 65536 outside [0,65536)"),
    ("dst_negative", "pair 0: IO 70 -> -3 outside [0,65536)"),
    ("dst_twice", "pair 1: IO 9 is the destination of two pairs"),
    ("dst_loaded", "pair 0: its destination IO 65 is loaded or stored by a chain"),
    ("dst_stored", "pair 0: its destination IO 1 is loaded or stored by a chain"),
    ("dst_mux_entry", "pair 0: its destination IO 66 is loaded or stored by a chain"),
    ("src_stored", "pair 0: its source IO 2 is stored by a chain"),
    ("src_is_dst", "pair 1: its source IO 9 is the destination of a pair"),
])
def test_refusals(driver, scenario, text):
    assert run(driver, scenario) == {"error": text}

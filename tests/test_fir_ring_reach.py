"""Which FIR variant the ring cases launch, without a GPU (a device cannot say which variant ran): for every FIR launch of every block
of every case of tests/fir_ring_cases.py -- the cases of tests/test_gpu_fir_ring_routes.py and program DEEP's of
tests/state_scripts.py -- tests/csrc/plan_layout_driver.cpp is asked what fir_choice / fir_hand_choice (avdsp_plan_layout.h) return
for it, the call tests/test_plan_layout.py makes.  fir_tile's window ring runs exactly for fir_tile with four row
tiles after halving, the lean boundary, neither BIG nor SPLIT: blocks meant for the ring must get that, blocks meant as another
kernel between ring launches must not.  A case whose name promises a wrap of the column pointer has a chain long enough for it, and
the options of the blocks-in-flight arrangements take the launch path they are listed with (tests/route_driver.py).

Tried by hand once, both fail here as they should: `fir_lean` 1 taken out of fir_ring_cases.RING_OPTS (every flight, staged and shard
case: "meant for the ring, fir_choice gives (4, 0, 0, 0)") and out of state_scripts.RING_PREFIX (the A / B / D / E DEEP cases likewise);
the 513-frame blocks of FLIGHT_BLOCKS / STAGED_BLOCKS / N_BLOCKS shrunk to 512 (R 2 where the ring was meant) and blocks_to's chunk in
script_A_ring shrunk to 512 (no launch meant for the ring is left: the literal count of RING_LAUNCHES fails)."""
import os
import shutil
import subprocess

import pytest

from tests import fir_ring_cases as rc
from tests import route_driver as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1
RING = (TILE, 4, 0, 0, 1)                    # family, R, BIG, SPLIT, LEAN
CASES = rc.reach_cases()


@pytest.fixture(scope="module")
def choice(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("ringreach") / "plan_layout_driver")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "plan_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    seen = {}

    def ask(L):
        """(family, R, BIG, SPLIT, LEAN), hand"""
        args = ("hand", L["impl"], L["n"], L["frames"], L["rows"], int(L["cascades"]), L["plan_taps"]) if L["hand"] else \
               ("choice", L["impl"], L["n"], L["frames"], L["rows"], 0, L["lean"], int(L["cascades"]), L["plan_taps"])
        if args not in seen:
            p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
            assert p.returncode == 0, p.stderr[-1500:]
            out = p.stdout.split()
            seen[args] = (tuple(map(int, out[:5])), out[5:] == ["HAND"])
        return seen[args]
    return ask


def test_the_driver_answers_for_handed_launches(choice):
    """fir_hand_choice: fir_tile whatever fir_impl says (but 0), lean by rule, never split, halved like any launch"""
    L = dict(impl=1, n=2, frames=1024, rows=4, lean=-1, cascades=True, plan_taps=8192, hand=True)
    assert choice(L) == (RING, True)
    assert choice(dict(L, frames=512)) == ((TILE, 2, 0, 0, 1), True)
    assert choice(dict(L, impl=4)) == (RING, True) and choice(dict(L, impl=0)) == ((0, 1, 0, 0, 0), True)
    assert choice(dict(L, rows=0)) == ((TILE, 1, 1, 0, 1), True)              # two chains by cost: one row tile, long chunks -- not the ring
    assert choice(dict(L, hand=False)) == ((TILE, 4, 0, 0, 0), False)          # the same launch unhanded: the boundary by the plan, the long one


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_block_meant_for_the_ring_reaches_it(choice, name):
    case = CASES[name]
    launches = case["launches"]
    assert launches
    ring = 0
    for k, L in enumerate(launches):
        got, hand = choice(L)
        assert hand == L["hand"]
        what = f"{name}, launch {k} ({L['frames']} frames, fir_impl {L['impl']}, fir_rows {L['rows']}, fir_lean {L['lean']})"
        if L["ring"]:
            assert L["frames"] > 512, f"{what}: meant for the ring, but four row tiles are halved at 512 frames"
            assert got == RING, f"{what}: meant for the ring, fir_choice gives {got[1:]} of family {got[0]}"
            ring += 1
        else:
            assert got != RING, f"{what}: meant as another kernel between ring launches, fir_choice gives the ring"
    assert (ring == 0) == bool(case.get("no_ring"))
    if "ring_launches" in case:
        assert ring == case["ring_launches"], f"{name}: {ring} ring launches, the scripts are written for {case['ring_launches']}"
    if case.get("some_other"):
        marks = [L["ring"] for L in launches]
        if True in marks:
            first, last = marks.index(True), len(marks) - 1 - marks[::-1].index(True)
            assert False in marks[first:last], f"{name}: no other kernel between two ring launches"
    elif not name.startswith("script-") and not case.get("no_ring"):
        assert all(L["ring"] for L in launches)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_that_promise_a_wrap_have_the_taps_for_it(name):
    case = CASES[name]
    need = {0: 1, 1: rc.FIRST_WRAP, 2: rc.SECOND_WRAP}[case["wraps"]]
    assert (rc.FIRST_WRAP, rc.SECOND_WRAP) == (1345, 2753)
    assert max(case["taps"]) >= need, f"{name} promises {case['wraps']} wrap(s) of the column pointer: a chain of {need} taps or more"
    if case["wraps"] == 2:
        assert any(rc.FIRST_WRAP <= t < rc.SECOND_WRAP for t in case["taps"]), f"{name}: no chain that wraps exactly once"


def test_the_programs_are_what_the_cases_say():
    assert rc.BASE == [(2, 4096), (1, 1345), (0, 2753), (1, 380), (3, 4097), (2, 1409), (0, 1900), (2, 65), (1, 3000)]
    assert len(rc.BASE) % 4 == 1 and sum(1 for s, _ in rc.BASE if s == 0) == 2          # a short last workgroup; not all_cascaded, and an overlap mode
    assert rc.FLIGHT_BLOCKS == [1024, 600, 1024, 513, 1024, 333, 1024, 1024, 700, 100, 1024, 1024, 1024] and sum(rc.FLIGHT_BLOCKS) > 8192 + 2048
    assert rc.STAGED_BLOCKS == [1024, 1024, 1024, 600, 513] and rc.TREE_BLOCKS == [1024, 600, 1024, 1024]
    assert [rc.shard_range(len(rc.TEN), 3, r) for r in range(3)] == [(0, 4), (4, 3), (7, 3)]      # two shards start off a multiple of four
    spec, stores, gap = rc.STAGED["two_stores"][1:]
    assert len(spec) * stores == 10 and gap == 1                                         # ten columns: no 16-byte run
    assert rc.STAGED["gapped"][3] == 2
    # every arrangement of tests/dev/gpu_overlap_sweep.ARR but the "fir_lean" 0 one, with the ring's options on top
    from tests.dev.gpu_overlap_sweep import ARR
    mine = [{k: v for k, v in a["opts"].items() if k not in ("fir_rows",)} for a in rc.FLIGHT.values()]
    for a in ARR:
        if a.get("fir_lean") == 0:
            continue
        want = {"fir_impl": 1, **a, "fir_lean": 1}
        assert want in mine, a
    assert all(a["opts"]["fir_rows"] == 4 and a["opts"]["fir_lean"] == 1 for a in rc.FLIGHT.values())
    assert {a["opts"].get("fir_ahead") for a in rc.FLIGHT.values()} >= {0, 1} and {a["opts"].get("fir_launch") for a in rc.FLIGHT.values()} >= {1, 2}
    assert all(rc.FLIGHT[n]["ring"] and rc.FLIGHT[n]["opts"]["fir_impl"] == 1 for n in rc.FLIGHT_STRESS.values()) and set(rc.FLIGHT_STRESS) == set(rc.FMTS)
    assert set(k for a in rc.FLIGHT.values() for k in a["opts"]) <= set(rc.FLIGHT_DEFAULTS)


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    exe, why = rd.build_driver(tmp_path_factory.mktemp("ringroute"))
    if exe is None:
        pytest.skip(why)
    return lambda **facts: rd.ask(exe, **facts)


@pytest.mark.parametrize("name", sorted(rc.FLIGHT))
def test_flight_arrangements_take_the_path_they_are_listed_with(route, name):
    """the base program's plan under each arrangement, a 1024-frame block, the streams apart: staged exactly where the case expects
    "fir_ahead_now" 1; a refused combination is not a candidate; what the others set reaches the route"""
    a = rc.FLIGHT[name]
    o = a["opts"]
    n_fir, _, plan_taps = rc.plan_facts(rc.BASE)
    facts = dict(overlap=o["overlap"], fir_ahead=o.get("fir_ahead", -1), ready_words=o.get("ready_words", -1), fir_launch=o.get("fir_launch", -1),
                 fir_impl=o["fir_impl"], nframes=1024, out_stride=len(rc.BASE), n_fir=n_fir, max_taps=plan_taps // n_fir, n_ahead_cols=len(rc.BASE),
                 n_fir_only=sum(1 for s, _ in rc.BASE if s == 0))
    r = route(ahead_apart=1, side_by_side=1, **facts)
    assert r["under"] == 1
    assert (r["path"] == rd.STAGED) == bool(a["staged"])
    if "refused" in a:
        assert r["ahead_candidate"] == 0 and a["refused"]
        if o.get("fir_launch", -1) >= 0:
            assert r["fir_launch_mode"] == 0
    if o["overlap"] == 2:
        assert r["path"] == rd.OWN_FIR
    # the base program's two FIR-only chains append their input inside the FIR launch: FIRs on two streams in turn follow each other
    assert r["fir_follows_fir"] == int(bool(a["staged"]) or o["overlap"] == 2)
    if r["path"] == rd.DIRECT:
        if o.get("fir_launch", -1) >= 0:
            assert r["fir_launch_mode"] == o["fir_launch"]
        if o.get("ready_words", -1) >= 0:
            assert r["ready_mode"] == o["ready_words"]
        else:
            assert r["ready_mode"] == 0                     # by the plan: 9 x 4097 taps are far below kReadyBehindTaps
    if a["staged"]:
        assert r["ready_mode"] == 0 and r["fir_launch_mode"] == 0      # the event, whatever "ready_words" says; no launch mode

"""tests/lowered_programs.py without a GPU: the generator is deterministic and the oracle loads what it makes; every core
of every seed of the committed slice is lowered to the chain kernels with the seven options on -- the host's report calls give the
counts the description predicts -- and none of them with the options off, so the device sweep cannot hide behind the interpreter; the
slice holds every pair of forms the grammar allows in one core, and every form at the chain counts 16, 17 and 37; and the player's
scripts are played oracle against oracle, where a checkpoint's fresh oracle must repeat the first one's frames and state."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import lowered_programs as lp

RUNS = lp.slice_runs()


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in lp.OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def reports(r, k):
    """what the host says of core k: None where it is refused"""
    try:
        return dict(chains=r.core_info(k)["chains"], copy=r.copy_info(k), finish=r.finish_info(k), delay=r.delay_info(k), fir_tail=r.fir_tail_info(k),
                    mux_tail=r.mux_tail_info(k), mem=r.mem_info(k), mem_fir=r.mem_fir_info(k), fir_group=r.fir_group_info(k))
    except rt.AvdspError as e:
        assert e.code == -8
        return None


@pytest.mark.parametrize("seed, fmt", RUNS)
def test_the_same_seed_gives_the_same_words_and_the_oracle_loads_them(seed, fmt):
    prog, in_stride, out_stride, desc = lp.random_lowered_program(seed, fmt)
    lp._CACHE.clear()                                          # (drawn and encoded again, not remembered)
    again, _, out_again, desc_again = lp.random_lowered_program(seed, fmt)
    assert (prog == again).all() and out_stride == out_again and [c["forms"] for c in desc["cores"]] == [c["forms"] for c in desc_again["cores"]]
    assert 1 <= len(desc["cores"]) <= 4 and in_stride == lp.IN_STRIDE and out_stride <= lp.IN
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    assert o.rc >= 0 and len(o.cores) == len(desc["cores"])
    s = lp.script(seed, fmt)
    assert 3 <= len(s["blocks"]) <= 6 and sum(s["blocks"]) <= lp.MAX_FRAMES and set(s["blocks"]) <= set(lp.BLOCKS) and len(s["events"]) == len(s["blocks"])


@pytest.mark.parametrize("seed, fmt", RUNS)
def test_every_core_of_the_slice_is_lowered_with_the_options_on_and_none_with_them_off(seed, fmt):
    prog, _, _, desc = lp.random_lowered_program(seed, fmt)
    for fs in (48000, 44100):
        r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
        assert r.rc >= 0 and len(r.cores) == len(desc["cores"])
        for key in lp.OPTIONS:
            r.set_option(key, 1)
        want = lp.describe(desc["drawn"], fmt, fs)
        for k, c in enumerate(want):
            got = reports(r, k)
            assert got is not None, f"seed {seed} format {fmt} at {fs} Hz: core {k} ({c['cls']}: {sorted(c['forms'])}) is refused: {r.last_error()}"
            assert got == c["info"], f"seed {seed} format {fmt} at {fs} Hz: core {k} ({c['cls']}): {({a: (got[a], c['info'][a]) for a in got if got[a] != c['info'][a]})}"
        for key in lp.OPTIONS:
            r.set_option(key, 0)
        for k, c in enumerate(want):                           # as before the options existed: not lowered
            got = reports(r, k)
            assert got is None or (got["chains"] == 0 and got["copy"] == (0, 0)), f"seed {seed} format {fmt}: core {k} ({c['cls']}) is lowered with every option off"
            assert "not lowered to the HIP path" in r.last_error() or "stored by more than one chain" in r.last_error(), r.last_error()
        r.release()


def lowered_cores():
    """(forms, chains) of every core of the slice -- test_every_core_of_the_slice_is_lowered... holds each of them to the host"""
    return [(c["forms"], c["chains"]) for seed, fmt in RUNS for c in lp.random_lowered_program(seed, fmt)[3]["cores"]]


def test_the_table_of_forms():
    assert len(lp.FORMS) == 17 and len(set(lp.FORMS)) == 17
    assert len(lp.ALLOWED_PAIRS) == 17 * 16 // 2 - 12          # all but LOAD_MUX heads and fir_shared groups beside the six tree forms
    for c in lowered_cores():
        assert c[0] <= set(lp.FORMS)
        assert not any(frozenset((a, b)) in lp.EXCLUDED for a in c[0] for b in c[0]), c


def test_every_allowed_pair_stands_in_one_core_of_the_slice():
    cores = lowered_cores()
    missing = [p for p in lp.ALLOWED_PAIRS if not any(p[0] in f and p[1] in f for f, _ in cores)]
    assert not missing, missing


@pytest.mark.parametrize("chains", [16, 17, 37])
def test_every_form_stands_in_a_core_of_each_chain_count_edge(chains):
    forms = set().union(*[f for f, n in lowered_cores() if n == chains])
    assert forms == set(lp.FORMS), sorted(set(lp.FORMS) - forms)


def test_a_tree_core_is_followed_by_a_core_that_reads_its_word():
    assert any(c["reads_an_earlier_cores_word"] for seed, fmt in RUNS for c in lp.random_lowered_program(seed, fmt)[3]["cores"])


def test_the_slice_draws_every_event_and_size():
    scripts = [lp.script(seed, fmt) for seed, fmt in RUNS]
    assert {e[0] for s in scripts for e in s["events"]} == set(lp.EVENTS)
    assert {b for s in scripts for b in s["blocks"]} == set(lp.BLOCKS)
    assert {s["fs"] for s in scripts} == {44100, 48000} and {s["input"] for s in scripts} == {"lcg", "stress"}
    assert {s["call"] for s in scripts} == {"run_block", "run_block_all"}
    drawn = [it for seed, fmt in RUNS for c in lp.random_lowered_program(seed, fmt)[3]["drawn"] for it in lp.chains_of(c)]
    assert {it["nsec"] for it in drawn} == set(lp.SECS) and {it["taps"] for it in drawn} >= set(lp.TAPS) | {0}
    param = [it for it in drawn if it["kind"] != "trunk" and it["slot"] and it["form"] == "param"]
    assert any(it["us"] == 0 for it in param) and any(it["us"] > it["max_us"] for it in param)          # a bypass, a clamped one
    assert [len(v) for v in lp.PINNED.values()] == [6, 6, 6] and all(set(lp.PINNED[f]) <= set(lp.SLICE[f]) for f in lp.PINNED)
    assert len(lp.GPU_CASES) == 11 and sorted(x for _, fmt, seeds in lp.GPU_CASES for x in ([(s, fmt) for s in seeds] if fmt else [(s, f) for f, s in seeds])) == sorted(RUNS)


@pytest.mark.parametrize("seed, fmt", RUNS)
def test_the_scripts_play_oracle_against_oracle(seed, fmt):
    """the player's own plumbing, before a device sees it: sentinels, in-place calls, edits into both copies, resets -- and at a
    checkpoint the second oracle is a FRESH one given the saved state and words, which must repeat what the first one (reset, its state
    put back) makes of the frames that follow, outputs and state"""
    trace = []
    assert lp.play(seed, fmt, device=False, trace=trace) == []
    s = lp.script(seed, fmt)
    assert [t[1] for t in trace] == s["blocks"] and [t[0] for t in trace] == s["events"]
    prog, _, out_stride, desc = lp.random_lowered_program(seed, fmt)
    if all(e[0] in ("none", "other_call", "toggle", "impl") for e in s["events"]):
        # nothing breaks the stream: one uninterrupted oracle run gives the same frames and the same end state
        o = po.OracleProgram(fmt, prog, fs=s["fs"], random=s["random"], dither=s["dither"])
        x = lp.script_input(seed, fmt, s)
        pos = 0
        for ev, n, want, state in trace:
            got = o.run_block(x[pos:pos + n], out_stride, lp.IN, out=lp.sentinel(fmt, (n, out_stride)))
            assert (got.view(np.uint32) == want.view(np.uint32)).all() and (o.state == state).all()
            pos += n

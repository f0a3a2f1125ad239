"""Dressed finishes, delay lines and a head TPDF_CALC in cores with LOAD_MUX heads, host side ("mux_tail"): which cores
dspRuntimeSetOption("mux_tail", 1) lowers to the chain kernels and which stay with the interpreter, each with a text of its own; what
avdsp_plan_layout.h makes of such chains (a stand-alone driver of that header, no HIP); and a run of the oracle over every program of
tests/test_gpu_muxtail.py.  Host-only: dspRuntimeCoreInfo / MuxTailInfo / MuxInfo / FinishInfo / DelayInfo / FirTailInfo run nothing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import muxtail_programs as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ("chain_finish", "chain_delay", "fir_tail", "mux_tail")
OLD_DRESSED = "a dressed SAT0DB behind a FIR or a LOAD_MUX head is not lowered to the HIP path"
OLD_DELAYED = "a DSP_DELAY in a chain with a DSP_FIR or a LOAD_MUX head is not lowered to the HIP path"
OLD_DRESSED_BESIDE = "dressed finishes or a head TPDF_CALC beside LOAD_MUX heads are not lowered to the HIP path"
OLD_DELAYED_BESIDE = "chains with a DSP_DELAY beside LOAD_MUX heads are not lowered to the HIP path"
CLASH = "a delay line and a LOAD_MUX result word share words of the state area"
M2 = [(0, 0.3), (1, -0.2)]


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, fs=48000, finish=1, delay=1, fir=1, tail=1, prog=None):
    if prog is None:
        prog, _, _ = mp.program(fmt, cores)
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    r.set_option("chain_finish", finish)
    r.set_option("chain_delay", delay)
    r.set_option("fir_tail", fir)
    if tail is not None:
        r.set_option("mux_tail", tail)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeMuxTailInfo lowers it and reports zeros when it is refused)"""
    assert r.mux_tail_info(core_index) == (0, 0, 0)
    return r.last_error()


def test_option_default_range_and_inheritance():
    cores = [mp.core([mp.chain(M2, slot="A", finish="tpdf")], calc=0)]
    r = loaded(6, cores, tail=None)
    assert r.get_option("mux_tail") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("mux_tail", bad)
    assert r.get_option("mux_tail") == 0 and r.mux_tail_info() == (0, 0, 0)
    rt.lib().dspRuntimeRelease()
    for key in OPTIONS:                                        # set without a program: the default of programs loaded later
        rt.Runtime.set_global_option(key, 1)
    prog, _, _ = mp.program(6, cores)
    r1 = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    assert r1.get_option("mux_tail") == 1 and r1.core_info()["chains"] == 1 and r1.mux_tail_info() == (1, 1, 1)
    r2 = rt.Runtime(6, prog.copy(), fs=48000, random=1, dither=24)     # a second context: the options are copied ...
    assert r2.get_option("mux_tail") == 1 and r2.mux_tail_info() == (1, 1, 1)
    r2.set_option("mux_tail", 0)                               # ... and each context keeps its own
    assert r2.mux_tail_info() == (0, 0, 0) and chains_of(r2) == 0 and r1.get_option("mux_tail") == 1 and r1.mux_tail_info() == (1, 1, 1)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_0_keeps_the_four_old_texts(fmt):
    plain = mp.chain(M2, nsec=1)
    for chains, calc, text in [([mp.chain(M2, nsec=2, finish="tpdf_gain")], None, OLD_DRESSED), ([mp.chain(M2, nsec=2, slot="A")], None, OLD_DELAYED),
                               ([plain, mp.chain(None, nsec=2, finish="gain")], None, OLD_DRESSED_BESIDE), ([plain], 0, OLD_DRESSED_BESIDE),
                               ([plain, mp.chain(None, nsec=2, slot="B")], None, OLD_DELAYED_BESIDE)]:
        r = loaded(fmt, [mp.core(chains, calc=calc)], tail=0)
        assert chains_of(r) == 0 and text in refusal(r), r.last_error()
        r.set_option("mux_tail", 1)
        assert chains_of(r) == len(chains)


KINDS = {"stage_finished": dict(nsec=0, finish="tpdf_gain"), "stage_handed": dict(nsec=0, slot="A", finish="sat"), "stage_handed_dressed": dict(nsec=0, slot="B", form="param", finish="tpdf"),
         "cascade_dressed": dict(nsec=2, finish="gain"), "cascade_handed": dict(nsec=17, slot="B", finish="none"), "fir_handed": dict(nsec=2, taps=33, slot="A", form="param", finish="tpdf_gain"),
         "fir_dressed": dict(nsec=0, taps=7, finish="tpdf")}


@pytest.mark.parametrize("head", ["mux", "load", "load_gain"])
@pytest.mark.parametrize("fmt, kind", [(f, k) for f in (2, 4, 6) for k in sorted(KINDS) if f != 2 or "fir" not in k])      # (format 2 has no FIR)
def test_option_lowers_every_kind_behind_every_head(fmt, head, kind):
    """the chain under test behind a LOAD_MUX, a LOAD or a LOAD_GAIN head, a plain LOAD_MUX chain beside it, a head TPDF_CALC"""
    c = mp.chain(M2 if head == "mux" else None, load_gain=None if head == "load" else 0.5, inp=1, **KINDS[kind])
    chains = [mp.chain(M2, nsec=1), c]
    r = loaded(fmt, [mp.core(chains, calc=0)], tail=0)
    assert chains_of(r) == 0 and "LOAD_MUX head" in refusal(r)
    r.set_option("mux_tail", 1)
    want = mp.counts(chains)
    assert r.core_info() == dict(chains=2, max_sections=max(1, c["nsec"]), max_taps=c["taps"])
    assert r.mux_tail_info() == want["mux_tail"] and want["mux_tail"][2] == (1 if head == "mux" and kind.startswith("stage") else 0)
    assert r.finish_info() == (want["dressed"], 1) and r.delay_info() == want["delay"] and r.fir_tail_info() == want["fir_tail"]
    assert r.mux_info()["mux_chains"] == (2 if head == "mux" else 1)


def test_info_is_zero_without_mux_heads():
    r = loaded(6, [mp.core([mp.chain(None, nsec=2, slot="A", finish="tpdf"), mp.chain(None, finish="gain")], calc=0)])
    assert r.core_info()["chains"] == 2 and r.mux_tail_info() == (0, 0, 0) and r.finish_info() == (2, 1) and r.delay_info() == (1, 47)


@pytest.mark.parametrize("fmt", [4, 6])
def test_the_other_options_are_still_needed(fmt):
    cores = [mp.core([mp.chain(M2, slot="A", finish="tpdf_gain"), mp.chain(M2, nsec=2, finish="tpdf")], calc=0)]
    r = loaded(fmt, cores, finish=0)
    assert chains_of(r) == 0 and "is not lowered to the HIP path" in refusal(r) and "opcode 47" not in r.last_error()      # the TPDF_CALC's refusal
    r = loaded(fmt, cores, delay=0)
    assert chains_of(r) == 0 and "opcode 47" in refusal(r)                                                                  # the DELAY's, through `default:`
    r = loaded(fmt, cores)
    assert r.core_info()["chains"] == 2 and r.mux_tail_info() == (2, 1, 1)
    fir = [mp.core([mp.chain(M2, taps=7, slot="A", finish="sat"), mp.chain(M2, nsec=1)])]
    r = loaded(fmt, fir, fir=0)
    assert chains_of(r) == 0 and OLD_DELAYED in refusal(r)
    r = loaded(fmt, [mp.core([mp.chain(M2, taps=7, finish="gain"), mp.chain(M2, nsec=1)])], fir=0)
    assert chains_of(r) == 0 and OLD_DRESSED in refusal(r)
    r = loaded(fmt, fir)
    assert r.core_info()["chains"] == 2 and r.fir_tail_info() == (1, 1) and r.mux_tail_info() == (0, 1, 0)
    # a plain SAT0DB or none around the DELAY needs no chain_finish
    r = loaded(fmt, [mp.core([mp.chain(M2, slot="A", finish="sat"), mp.chain(M2, slot="A", finish="none"), mp.chain(M2, nsec=1, slot="B", finish="sat")])], finish=0)
    assert r.core_info()["chains"] == 3 and r.mux_tail_info() == (0, 3, 2)


P = mp.chain(M2, nsec=1)
REFUSED = {
    "delay_dp": (6, [mp.core([P, mp.chain(M2, slot="A", odd="dp")])], "DSP_DELAY_DP is not lowered"),
    "delay_1": (2, [mp.core([P, mp.chain(M2, slot="A", odd="d1")])], "DSP_DELAY_1 is not lowered"),
    "two_delays": (4, [mp.core([P, mp.chain(M2, slot="B", odd="two")])], "a second DSP_DELAY in one chain"),
    "delay_in_front_of_the_banks": (2, [mp.core([P, mp.chain(M2, nsec=2, odd="head")])], "a DSP_DELAY in front of the banks"),
    "delay_in_front_of_the_fir": (6, [mp.core([P, mp.chain(M2, taps=7, odd="front")])], "a DSP_DELAY in front of the chain's DSP_FIR"),
    "format_3": (3, [mp.core([P, mp.chain(M2, slot="A")])], "LOAD_MUX is not lowered to the HIP path in format 3"),
    "format_5": (5, [mp.core([mp.chain(None, slot="A"), P])], "a DSP_DELAY is not lowered to the HIP path in format 5"),
    "format_5_dressed": (5, [mp.core([mp.chain(None, finish="tpdf"), P])], "opcode 43"),
    "format_2_has_no_fir": (2, [mp.core([P, mp.chain(M2, taps=7, slot="A")])], "DSP_FIR in int64 mode"),
    "another_dither_width": (6, [mp.core([P, mp.chain(M2, finish="tpdf")], calc=0), mp.core([mp.chain(None, nsec=1)], calc=20)], "the program changes its dither width"),
    "tpdf_calc_behind_the_head": (4, [mp.core([P], calc=0), mp.core([P], calc=0)], None),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_not_lowered_with_every_option_on(case):
    fmt, cores, text = REFUSED[case]
    r = loaded(fmt, cores)
    if text is None:                                           # (two cores with a head TPDF_CALC of the default width each: both lowered)
        assert [chains_of(r, k) for k in range(2)] == [1, 1] and [r.finish_info(k) for k in range(2)] == [(0, 1)] * 2
        return
    assert chains_of(r) == 0
    assert text in refusal(r), r.last_error()


def test_instances_keep_such_cores_on_the_interpreter():
    r = loaded(6, [mp.core([mp.chain(M2, slot="A", finish="sat"), mp.chain(M2, finish="gain")])])
    assert r.core_info()["chains"] == 2 and r.mux_tail_info() == (1, 1, 2)
    r.set_instances(4)
    assert chains_of(r) == 0 and r.mux_tail_info() == (0, 0, 0)
    r.set_instances(0)
    assert r.core_info()["chains"] == 2 and r.mux_tail_info() == (1, 1, 2)


def test_shard_counts_its_own_chains():
    ch = [mp.chain(M2, nsec=i % 2, slot="A" if i % 2 else None, us=100 * (i + 1), finish="tpdf" if i % 3 == 0 else "sat") for i in range(12)]
    r = loaded(4, [mp.core(ch, calc=0)])
    assert r.mux_tail_info() == mp.counts(ch)["mux_tail"] == (4, 6, 2)
    for rank in range(3):
        r.set_shard(rank, 3)
        assert r.mux_tail_info() == mp.counts(ch[4 * rank:4 * rank + 4])["mux_tail"]
    r.set_shard(0, 1)
    assert r.mux_tail_info() == (4, 6, 2)


DAMAGE = ["line_over_a_result_word", "result_word_inside_a_line", "two_lines_share_words", "line_past_the_data", "empty_mux_table", "mux_entry_outside_the_io_range",
          "result_word_past_the_data"]


@pytest.mark.parametrize("fmt, which", [(f, w) for f in (2, 6) for w in DAMAGE] + [(6, "line_inside_a_fir_history")])      # (format 2 has no FIR)
def test_damaged_payloads_are_refused_not_followed(fmt, which):
    fir = which == "line_inside_a_fir_history"
    chains = [mp.chain(M2, slot="A", us=2100, finish="sat"), mp.chain(M2, nsec=1, slot="B", form="param", us=1000, finish="sat"), mp.chain(M2, nsec=1, taps=300 if fir else 0)]
    prog, _, _ = mp.program(fmt, [mp.core(chains)])
    prog = prog.copy()
    line0, line1 = mp.words_of(prog, mp.OP_DELAY)              # [op, size or us, line, parameter]
    mux0, mux1, mux2 = mp.words_of(prog, mp.OP_LOAD_MUX)       # [op, table, result word]
    data = int(prog[2])
    text, damaged = "outside the state area", False
    if which == "line_over_a_result_word":
        prog[line0 + 2] = int(prog[mux1 + 2]) - 50             # index word + 100 samples: chain 1's result word among them
        text = CLASH
    elif which == "result_word_inside_a_line":
        prog[mux2 + 2] = int(prog[line1 + 2])                  # ... the line's index word itself
        text = CLASH
    elif which == "two_lines_share_words":
        prog[line1 + 2] = int(prog[line0 + 2]) + 2                # (inside line 0, and over no result word)
        text = "two delay lines of the core share words of the state area"
    elif which == "line_past_the_data":
        prog[line0 + 2] = data - mp.samples(2100)              # index word + 100 samples: one word too many
    elif which == "line_inside_a_fir_history":
        f = mp.words_of(prog, 51)[0]                           # DSP_FIR: [op, offset at 44.1 kHz, offset at 48 kHz, history]
        prog[line0 + 2] = int(prog[f + 3]) + 5
        text = "a delay line and a FIR's history share words of the state area"
    elif which == "empty_mux_table":
        prog[mux1 + int(np.int32(prog[mux1 + 1]))] = mp.OP_LOAD_MUX << 16
        text, damaged = "LOAD_MUX table with 0 entries", True
    elif which == "mux_entry_outside_the_io_range":
        prog[mux1 + int(np.int32(prog[mux1 + 1])) + 3] = 70000
        text, damaged = "IO number 70000 outside", True
    elif which == "result_word_past_the_data":
        prog[mux0 + 2] = data - 1
        damaged = True
    mp.resealed(prog)
    r = loaded(fmt, None, prog=prog)
    assert r.mux_tail_info() == (0, 0, 0)
    assert text in r.last_error(), r.last_error()
    assert chains_of(r) == 0
    if damaged:                                                # (dspRuntimeMuxInfo tells a damaged table from a core that is merely not lowered)
        with pytest.raises(rt.AvdspError) as e:
            r.mux_info()
        assert e.value.code == -8
    else:
        assert r.mux_info()["mux_chains"] == 0


def test_the_gpu_tests_mix_reaches_every_kind_of_chain():
    """tests/test_gpu_muxtail.py's 123-chain core: the five kinds and plain chains in mux_tile's groups and among mux_plain's chains, every
    section count, slot, form, line length, finish and store count -- and the lowering takes it as that"""
    ch, group = mp.five_kinds_chains()
    tile = [c for c, g in zip(ch, group) if g in ("g16", "g17", "g65")]
    plain = [c for c, g in zip(ch, group) if g in ("p15", "private")]
    assert [group.count(g) for g in ("g16", "g17", "g65", "p15", "private", "load")] == [16, 17, 65, 15, 4, 6]
    assert {mp.kind(c) for c in tile} == {"plain", "cascade_dressed", "cascade_handed", "stage_finished", "stage_handed"}
    assert {mp.kind(c) for c in plain} >= {"plain", "cascade_handed", "stage_finished", "stage_handed"}
    staged = [c for c in ch if mp.kind(c).startswith("stage")]
    assert {c["finish"] for c in staged} == set(mp.FIN) and {c["stores"] for c in staged} == {1, 2}
    d = [c for c in ch if c["slot"]]
    assert {c["nsec"] for c in ch} == set(mp.SECS) == {c["nsec"] for c in d} and {(c["slot"], c["form"]) for c in d} == {(s, f) for s in "AB" for f in ("fixed", "param")}
    assert {mp.samples(c["us"]) for c in d if not c["nsec"] and c["mux"]} == {0, 1, 3, 47, 1199} and {c["finish"] for c in d} == set(mp.FIN)
    assert any(c["slot"] for c, g in zip(ch, group) if g == "load") and any(mp.dressed(c) and not c["slot"] and not c["nsec"] for c, g in zip(ch, group) if g == "load")
    for fmt in (2, 4, 6):
        r = loaded(fmt, [mp.core(ch, calc=0)])
        assert r.core_info()["chains"] == 123 and r.mux_tail_info() == mp.counts(ch)["mux_tail"] and r.delay_info() == mp.counts(ch)["delay"]
        assert r.mux_info() == dict(mux_chains=117, groups=3, grouped_chains=98, longest_list=33)


@pytest.mark.parametrize("name", sorted(mp.gpu_programs()))
def test_the_oracle_runs_every_program_of_the_gpu_tests(name):
    """... and the lowering takes every core of them with the counts the GPU tests assert"""
    formats, cores = mp.gpu_programs()[name]
    for fmt in formats:
        prog, nin, nout = mp.program(fmt, cores)
        r = loaded(fmt, None, prog=prog)
        for k, c in enumerate(cores):
            want = mp.counts(c["chains"])
            assert r.core_info(k)["chains"] == len(c["chains"]), r.last_error()
            assert r.mux_tail_info(k) == want["mux_tail"] and r.finish_info(k)[0] == want["dressed"] and r.delay_info(k) == want["delay"] and r.fir_tail_info(k) == want["fir_tail"]
        x = pb.lcg_input(70, nin, fmt == 6, seed=2)
        o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
        y = o.run_block(x, nout, mp.IN)
        assert y.shape == (70, nout) and np.ascontiguousarray(y).view(np.uint32).any(axis=0).sum() > nout // 2 and o.state.any()


# ---------------------------------------------------------------- the plan's tables (avdsp_plan_layout.h), a driver of its own
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("muxtail") / "muxtail_layout_driver")
    base = ["g++", "-std=c++17", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "csrc", "muxtail_layout_driver.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:                                      # (no sanitizer runtime here: the plain build checks the tables all the same)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    return exe


A, B = 1, 2                                                    # AVDSP_DELAY_A / _B
TPDF, GAIN = 1, 2                                              # AVDSP_FINISH_TPDF / _GAIN
LOAD, LOAD_GAIN, MUX, MUX_PRIVATE = 0, 1, 2, 3
RAW = 2                                                        # kLoadRaw


def layout(driver, fmt, chains, mux_tail=1, fir_tail=1, calc=0):
    """chains: (head, nsec, taps, finish, delay_slot, sat)"""
    args = [driver, fmt, mux_tail, fir_tail, calc] + [v for c in chains for v in c]
    r = subprocess.run(list(map(str, args)), capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


#       0 cascade dressed        1 cascade handed       2 FIR handed               3 stage finished       4 stage handed           5 stage handed, dressed
MIX = [(MUX, 2, 0, TPDF, 0, 1), (MUX, 2, 0, 0, A, 1), (MUX, 0, 7, GAIN, B, 1), (MUX_PRIVATE, 0, 0, GAIN, 0, 1), (MUX, 0, 0, 0, A, 0), (MUX_PRIVATE, 0, 0, TPDF, B, 1),
       #  6 stage stored (plain)  7 plain cascade        8 LOAD, dressed            9 LOAD_GAIN, delayed    10 LOAD, delayed cascade
       (MUX, 0, 0, 0, 0, 1), (MUX, 1, 0, 0, 0, 1), (LOAD, 0, 0, TPDF, 0, 1), (LOAD_GAIN, 0, 0, 0, A, 1), (LOAD, 3, 0, 0, B, 1)]


@pytest.mark.parametrize("fmt", [4, 6])
def test_layout_of_the_five_kinds(driver, fmt):
    L = layout(driver, fmt, MIX, calc=1)
    assert L["col"] == [0, 1, 2, -1, -1, -1, -1, 7, 8, 9, 10] and L["count"] == [3, 3, 3, 2, 3, 2, 3, 3, 0, 0, 0]
    assert L["mux_stored"] == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0] and L["n_mux_stored"] == 2 and L["n_mux_finished"] == 1
    assert L["mux_handed"] == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0] and L["n_mux_handed"] == 2 and L["tail_forms"] == 1
    assert L["tail"] == [1, 2, 4, 5, 9, 10] and L["hand_row"] == [-1, 0, 1, -1, 2, 3, -1, -1, -1, -1, 4] and L["n_hand_rows"] == 5
    assert L["pass"] == [] and L["pass_dressed"] == [8] and L["fir_hand"] == [2] and L["n_dressed"] == 5 and L["overlap_ok"] == 0
    assert L["load_mode"] == [RAW] * 8 + [LOAD, LOAD_GAIN, LOAD] and L["in_io"] == list(range(11))          # every chain reads its own column
    g = {(x["nsec"], x["wide"], x["hand"]): x["ids"] for x in L["groups"]}
    assert g == {(2, 1, 0): [0], (2, 1, 1): [1], (1, 0, 0): [7], (3, 1, 1): [10]}
    assert L["plain"] == list(range(11)) and L["ntiles"] == 0


def test_layout_format_2(driver):
    L = layout(driver, 2, [c for c in MIX if not c[2]], fir_tail=0)
    assert L["mux_handed"] == [0, 0, 0, 1, 1, 0, 0, 0, 0, 0] and L["hand_row"] == [-1, 0, -1, 1, 2, -1, -1, -1, -1, 3] and L["tail_forms"] == 1
    assert layout(driver, 2, MIX) == {"error": "chain 2: FIR has no int64 definition"}


def test_layout_takes_the_tail_forms_only_when_a_plan_needs_them(driver):
    """neither a stage-finished nor a stage-handed chain: the stage as it was, whatever stands behind the columns"""
    for chains, forms, stored in [(MIX[:3] + MIX[6:], 0, 1), (MIX[6:8], 0, 1), (MIX[:3] + MIX[3:4], 1, 1), (MIX[7:8] + MIX[4:5], 1, 0), (MIX[7:], 0, 0)]:
        L = layout(driver, 6, chains)
        assert (L["tail_forms"], L["n_mux_stored"]) == (forms, stored), chains


def test_layout_of_a_mix_group(driver):
    """20 chains of one list, every fourth handed by the stage, every fourth finished by it: one tile, the stage-stored chains counted"""
    chains = [(MUX, 0, 0, 0, A, 1) if i % 4 == 0 else (MUX, 0, 0, TPDF | GAIN, 0, 1) if i % 4 == 1 else (MUX, 2, 0, 0, 0, 1) if i % 4 == 2 else (MUX, 0, 0, 0, 0, 0) for i in range(20)]
    L = layout(driver, 6, chains)
    assert L["ntiles"] == 1 and L["tile_ids"] == list(range(20)) and L["plain"] == []
    assert L["n_mux_handed"] == 5 and L["n_mux_finished"] == 5 and L["n_mux_stored"] == 10 and L["n_hand_rows"] == 5
    assert L["tail"] == list(range(0, 20, 4)) and [L["hand_row"][i] for i in L["tail"]] == list(range(5))
    assert layout(driver, 2, chains)["ntiles"] == 0            # format 2: no mux_tile


def test_layout_without_the_flag_keeps_the_texts(driver):
    assert layout(driver, 6, MIX, mux_tail=0) == {"error": "chain 0: a dressed finish has no kernel here"}
    assert layout(driver, 6, MIX[1:], mux_tail=0) == {"error": "chain 0: a delay line has no kernel here"}
    assert layout(driver, 6, MIX[6:8], mux_tail=0, calc=1) == {"error": "a head TPDF_CALC has no kernel here"}
    assert layout(driver, 6, MIX[6:8], mux_tail=0)["tail_forms"] == 0
    assert layout(driver, 6, MIX, fir_tail=0) == {"error": "chain 2: a dressed finish has no kernel here"}
    assert layout(driver, 5, MIX) == {"error": "LOAD_MUX chains have no kernels in format 5"}
    assert layout(driver, 6, MIX[8:], mux_tail=0, calc=1)["pass_dressed"] == [0]      # (no LOAD_MUX chain: the flag is not asked for)

"""Handed FIR chains, host side ("fir_tail"): which cores dspRuntimeSetOption("fir_tail", 1) lowers to the chain kernels
-- a DSP_DELAY and / or a dressed finish behind a chain's DSP_FIR, formats 4 and 6 -- and which stay with the interpreter, each with a
text of its own; and what avdsp_plan_layout.h makes of such chains (a stand-alone driver of that header, no HIP).  Host-only:
dspRuntimeCoreInfo / FirTailInfo / FinishInfo / DelayInfo / FirGroupInfo run nothing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import firtail_programs as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_DRESSED = "a dressed SAT0DB behind a FIR or a LOAD_MUX head is not lowered to the HIP path"
OLD_DELAYED = "a DSP_DELAY in a chain with a DSP_FIR or a LOAD_MUX head is not lowered to the HIP path"


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in ("fir_tail", "chain_delay", "chain_finish"):
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, fs=48000, finish=1, delay=1, tail=1):
    prog, _, _ = fp.program(fmt, cores)
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    r.set_option("chain_finish", finish)
    r.set_option("chain_delay", delay)
    if tail is not None:
        r.set_option("fir_tail", tail)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeFirTailInfo lowers it and reports zeros when it is refused)"""
    assert r.fir_tail_info(core_index) == (0, 0)
    return r.last_error()


def test_option_default_range_and_inheritance():
    core = [fp.core([fp.chain(2, 64, "A")], calc=0)]
    r = loaded(6, core, tail=None)
    assert r.get_option("fir_tail") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("fir_tail", bad)
    assert r.get_option("fir_tail") == 0 and r.fir_tail_info() == (0, 0)
    rt.lib().dspRuntimeRelease()
    for key in ("fir_tail", "chain_delay", "chain_finish"):    # set without a program: the default of programs loaded later
        rt.Runtime.set_global_option(key, 1)
    prog, _, _ = fp.program(6, core)
    r1 = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    assert r1.get_option("fir_tail") == 1 and r1.core_info()["chains"] == 1 and r1.fir_tail_info() == (1, 1)
    r2 = rt.Runtime(6, prog.copy(), fs=48000, random=1, dither=24)     # a second context: the options are copied ...
    assert r2.get_option("fir_tail") == 1 and r2.fir_tail_info() == (1, 1)
    r2.set_option("fir_tail", 0)                               # ... and each context keeps its own
    assert r2.fir_tail_info() == (0, 0) and r1.get_option("fir_tail") == 1 and r1.fir_tail_info() == (1, 1) and r2.get_option("fir_tail") == 0


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_0_keeps_the_old_refusal_texts(fmt):
    r = loaded(fmt, [fp.core([fp.chain(2, 64, None, finish="tpdf_gain")], calc=0)], tail=0)
    assert chains_of(r) == 0 and OLD_DRESSED in refusal(r)
    r = loaded(fmt, [fp.core([fp.chain(2, 64, "A", finish="sat")])], tail=0)
    assert chains_of(r) == 0 and OLD_DELAYED in refusal(r)
    r = loaded(fmt, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="front")])], tail=0)
    assert chains_of(r) == 0 and "a DSP_DELAY in a chain with a DSP_FIR is not lowered to the HIP path" in refusal(r)


@pytest.mark.parametrize("fmt", [4, 6])
@pytest.mark.parametrize("finish", ["none", "sat", "tpdf", "gain", "tpdf_gain"])
@pytest.mark.parametrize("slot, form", [("A", "fixed"), ("A", "param"), ("B", "fixed"), ("B", "param"), (None, "fixed")])
def test_option_lowers_the_handed_core(fmt, slot, form, finish):
    dressed = finish in fp.FINISHES
    ch = [fp.chain(2, 64, slot, form, us=1000, finish=finish), fp.chain(0, 300, slot, form, us=2100, finish=finish, stores=2),
          fp.chain(17, 7, slot, form, us=63, finish=finish), fp.chain(1, 33, None, finish="sat"), fp.chain(3, 0, None, finish="sat")]
    r = loaded(fmt, [fp.core(ch, calc=0)], tail=0)
    if slot or dressed:
        assert chains_of(r) == 0 and (OLD_DELAYED if slot == "A" or (slot and not dressed) else OLD_DRESSED) in refusal(r)
    r.set_option("fir_tail", 1)
    handed = 3 if slot or dressed else 0
    assert r.core_info() == dict(chains=5, max_sections=17, max_taps=300)
    assert r.fir_tail_info() == (handed, 3 if slot else 0) == fp.handed(ch)
    assert r.finish_info() == (3 if dressed else 0, 1)
    assert r.delay_info() == ((3, fp.samples(2100)) if slot else (0, 0))
    r.set_option("fir_tail", 0)
    assert r.fir_tail_info() == (0, 0) and chains_of(r) == (0 if slot or dressed else 5)


@pytest.mark.parametrize("fmt", [4, 6])
def test_chain_finish_and_chain_delay_are_still_needed(fmt):
    cores = [fp.core([fp.chain(2, 64, "A", finish="tpdf_gain"), fp.chain(0, 7, "B", finish="tpdf")], calc=0)]
    r = loaded(fmt, cores, finish=0, delay=1)
    assert chains_of(r) == 0 and "is not lowered to the HIP path" in refusal(r) and "opcode 47" not in r.last_error()      # the TPDF_CALC's / dressed opcode's refusal
    r = loaded(fmt, cores, finish=1, delay=0)
    assert chains_of(r) == 0 and "opcode 47" in refusal(r)                                                                  # the DELAY's, through `default:`
    r = loaded(fmt, cores, finish=1, delay=1)
    assert r.core_info()["chains"] == 2 and r.fir_tail_info() == (2, 2) and r.finish_info() == (2, 1) and r.delay_info() == (2, 47)
    # a plain SAT0DB or none behind FIR and DELAY needs no chain_finish
    r = loaded(fmt, [fp.core([fp.chain(2, 64, "A", finish="sat"), fp.chain(0, 7, "A", finish="none"), fp.chain(1, 9, "B", finish="sat")])], finish=0)
    assert r.core_info()["chains"] == 3 and r.fir_tail_info() == (3, 3)


REFUSED = {
    "pure_delay_variant": (6, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="pure_delay")])], "FIR pure-delay variant is not lowered yet"),
    "format_3": (3, [fp.core([fp.chain(2, 64, "A", finish="sat")])], "a DSP_DELAY is not lowered to the HIP path in format 3"),
    "format_5": (5, [fp.core([fp.chain(0, 64, "B", finish="sat")])], "a DSP_DELAY is not lowered to the HIP path in format 5"),
    "format_5_dressed": (5, [fp.core([fp.chain(0, 64, None, finish="tpdf")])], "opcode 43"),
    "format_2_has_no_fir": (2, [fp.core([fp.chain(2, 64, "A", finish="sat")])], "DSP_FIR in int64 mode"),
    "mux_head_delayed": (6, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="mux"), fp.chain(1, 0, None, finish="sat")])], "a DSP_FIR or a LOAD_MUX head"),
    "mux_head_dressed": (4, [fp.core([fp.chain(2, 64, None, finish="gain", odd="mux"), fp.chain(1, 0, None, finish="sat")])], "a dressed SAT0DB behind a FIR or a LOAD_MUX head"),
    "beside_mux_chains": (6, [fp.core([fp.chain(2, 0, None, finish="sat", odd="mux"), fp.chain(1, 64, "A", finish="sat")])], "beside LOAD_MUX heads"),
    "delay_dp": (6, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="dp")])], "DSP_DELAY_DP is not lowered"),
    "delay_1": (4, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="d1")])], "DSP_DELAY_1 is not lowered"),
    "delay_in_front_of_the_fir": (6, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="front")])], "a DSP_DELAY in front of the chain's DSP_FIR"),
    "two_firs": (4, [fp.core([fp.chain(2, 64, "A", finish="sat", odd="two_firs")])], "more than one FIR per chain"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_not_lowered_with_the_option_on(case):
    fmt, cores, text = REFUSED[case]
    r = loaded(fmt, cores)
    assert chains_of(r) == 0
    assert text in refusal(r), r.last_error()


def test_instances_keep_handed_cores_on_the_interpreter():
    r = loaded(6, [fp.core([fp.chain(2, 64, "A", finish="sat"), fp.chain(0, 7, None, finish="gain")])])
    assert r.core_info()["chains"] == 2 and r.fir_tail_info() == (2, 1)
    r.set_instances(4)
    assert chains_of(r) == 0 and "while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.core_info()["chains"] == 2 and r.fir_tail_info() == (2, 1)


@pytest.mark.parametrize("fmt", [4, 6])
def test_a_bypassed_fir_makes_an_ordinary_cascade_chain(fmt):
    """length 0 at the current rate: fir_op is set, fir_taps is 0 -- with "fir_tail" 1 the chain is a dressed / delayed cascade chain
    (the WIDE / HAND cascade forms), not a handed FIR chain; with 0 it is refused as before"""
    cores = [fp.core([fp.chain(2, 0, "A", finish="tpdf_gain", odd="bypass"), fp.chain(0, 0, None, finish="tpdf", odd="bypass"), fp.chain(3, 0, "B", finish="sat", odd="bypass")], calc=0)]
    r = loaded(fmt, cores, tail=0)
    assert chains_of(r) == 0 and OLD_DELAYED in refusal(r)
    r.set_option("fir_tail", 1)
    assert r.core_info() == dict(chains=3, max_sections=3, max_taps=0)
    assert r.fir_tail_info() == (0, 0) and r.finish_info() == (2, 1) and r.delay_info() == (2, 47)


@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_groups_leave_handed_chains_out(fmt):
    """17 chains on one bank, two of them handed: 15 are fewer than a group; 20 with two handed: a group of 18"""
    def bank(n):
        ch = [fp.chain(2 if i % 2 else 0, 100, None, finish="sat", bank=1) for i in range(n)]
        ch[3] = fp.chain(2, 100, "A", "fixed", 1000, finish="tpdf_gain", bank=1)
        ch[11] = fp.chain(0, 100, None, finish="tpdf", bank=1)
        return [fp.core(ch, calc=0)]
    r = loaded(fmt, bank(17))
    assert r.core_info()["chains"] == 17 and r.fir_tail_info() == (2, 1)
    assert r.fir_group_info() == dict(groups=0, grouped_chains=0, largest_group=0)
    r = loaded(fmt, bank(20))
    assert r.fir_tail_info() == (2, 1) and r.fir_group_info() == dict(groups=1, grouped_chains=18, largest_group=18)
    plain = [fp.core([fp.chain(0, 100, None, finish="sat", bank=1) for _ in range(17)])]
    assert loaded(fmt, plain).fir_group_info() == dict(groups=1, grouped_chains=17, largest_group=17)      # (all plain: grouped as ever)


def test_shard_counts_its_own_chains():
    ch = [fp.chain(1, 16 + i, "A" if i % 2 else None, us=100 * (i + 1), finish="tpdf" if i % 3 == 0 else "sat") for i in range(12)]
    r = loaded(4, [fp.core(ch, calc=0)])
    assert r.fir_tail_info() == fp.handed(ch) == (8, 6)
    r.set_shard(1, 3)                                          # chains 4 .. 7: 5 and 7 are delayed, 6 is dressed
    assert r.fir_tail_info() == fp.handed(ch[4:8]) == (3, 2)
    r.set_shard(2, 3)
    assert r.fir_tail_info() == fp.handed(ch[8:12]) == (2, 2)
    r.set_shard(0, 1)
    assert r.fir_tail_info() == (8, 6)


@pytest.mark.parametrize("fmt", [4, 6])
@pytest.mark.parametrize("which", ["fir_state_past_the_data", "fir_taps_past_the_program", "line_inside_a_fir_history", "fir_history_inside_a_line",
                                   "line_past_the_data"])
def test_damaged_payloads_are_refused_not_followed(fmt, which):
    prog, _, _ = fp.program(fmt, [fp.core([fp.chain(2, 64, "A", "fixed", us=2100, finish="sat"), fp.chain(1, 40, "B", "param", us=1000, finish="sat")])])
    prog = prog.copy()
    fir0, fir1 = fp.fir_words(prog)                            # [op, offset at 44.1 kHz, offset at 48 kHz, history]
    line0, line1 = fp.words_of(prog, fp.OP_DELAY)              # [op, size or us, line, parameter]
    data = int(prog[2])
    text = "outside the state area"
    if which == "fir_state_past_the_data":
        prog[fir0 + 3] = data - 63                             # 64 words from there: one too many
    elif which == "fir_taps_past_the_program":
        imp = fir1 + int(np.int32(prog[fir1 + 2]))             # the impulse's length word at 48 kHz: taps far beyond the program
        assert int(prog[imp]) == 40
        prog[imp] = 1 << 15
        text = "outside the program"
    elif which == "line_inside_a_fir_history":
        prog[line0 + 2] = int(prog[fir0 + 3]) + 5              # over its own chain's history, and no other line
        text = "a delay line and a FIR's history share words of the state area"
    elif which == "fir_history_inside_a_line":
        prog[fir1 + 3] = int(prog[line0 + 2]) + 50
        text = "a delay line and a FIR's history share words of the state area"
    elif which == "line_past_the_data":
        prog[line0 + 2] = data - fp.samples(2100)              # index word + 100 samples: one word too many
    fp.resealed(prog)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    assert r.rc >= 0
    for key in ("chain_finish", "chain_delay", "fir_tail"):
        r.set_option(key, 1)
    assert r.fir_tail_info() == (0, 0)
    assert text in r.last_error(), r.last_error()
    assert chains_of(r) == 0


def test_the_gpu_tests_mix_reaches_every_kind_of_chain():
    """tests/test_gpu_firtail.py's 37-chain core: every tap count, section count, slot, form, finish, store count and line length among
    its handed chains, plain FIR chains and cascade chains beside them -- and the lowering takes it as that"""
    from tests.test_gpu_firtail import FIN, SECS, TAPS, US, mixed_chains
    ch = mixed_chains(37)
    h = [c for c in ch if c["taps"] and (c["slot"] or c["finish"] in fp.FINISHES)]
    assert {c["taps"] for c in h} == set(TAPS) and {c["nsec"] for c in h} == set(SECS)
    assert {(c["slot"], c["form"]) for c in h} >= {("A", "fixed"), ("A", "param"), ("B", "fixed"), ("B", "param"), (None, "fixed")}
    assert {c["finish"] for c in h} == set(FIN) and {c["stores"] for c in h} == {1, 2} and {c["us"] for c in h if c["slot"]} == set(US)
    assert any(c["taps"] and not c["slot"] and c["finish"] in ("sat", "none") for c in ch)        # plain FIR chains beside them
    assert any(not c["taps"] for c in ch)                                                            # ... and cascade chains
    assert fp.handed(mixed_chains(1)) == (1, 1) and fp.handed(mixed_chains(5))[0] >= 3
    for fmt in (4, 6):
        r = loaded(fmt, [fp.core(ch, calc=0)])
        assert r.core_info()["chains"] == 37 and r.fir_tail_info() == fp.handed(ch) == (len(h), sum(1 for c in h if c["slot"]))


# ---------------------------------------------------------------- the plan's tables (avdsp_plan_layout.h), a driver of its own
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("firtail") / "firtail_layout_driver")
    base = ["g++", "-std=c++17", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "csrc", "firtail_layout_driver.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:                                      # (no sanitizer runtime here: the plain build checks the tables all the same)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    return exe


A, B = 1, 2                                                    # AVDSP_DELAY_A / _B
TPDF_GAIN = 3                                                  # AVDSP_FINISH_TPDF_GAIN


def layout(driver, fmt, fir_tail, chains, grouped=0):
    """chains: (nsec, taps, finish, delay_slot, sat[, bank])"""
    args = [driver, "layout", fmt, fir_tail, grouped]
    for c in chains:
        args += list(c) + ([-1] if len(c) == 5 else [])
    r = subprocess.run(list(map(str, args)), capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)


MIX = [(2, 64, TPDF_GAIN, A, 1), (2, 64, 0, 0, 1), (2, 0, TPDF_GAIN, A, 1), (0, 7, 1, 0, 1), (17, 300, 0, B, 1), (5, 0, 0, 0, 1), (2, 9, 0, 0, 0), (0, 0, 0, A, 0)]


@pytest.mark.parametrize("fmt", [4, 6])
def test_layout_lists_and_groups(driver, fmt):
    L = layout(driver, fmt, 1, MIX)
    assert L["fir"] == [0, 1, 3, 4, 6] and L["fir_hand"] == [0, 3, 4] and L["fir_plain"] == [1, 6]
    assert L["tail"] == [0, 2, 3, 4, 7] and L["pass"] == [] and L["pass_dressed"] == []
    assert L["n_dressed"] == 3 and L["max_taps"] == 300 and L["overlap_ok"] == 0
    g = {(x["nsec"], x["wide"], x["hand"]): x for x in L["groups"]}
    # the handed FIR chains 0 and 4 sit in ring-feeding groups, neither wide nor hand: chain 0 with the plain FIR chains of its length
    assert g[(2, 0, 0)]["ids"] == [0, 1, 6] and g[(2, 0, 0)]["all_fir"] == 1 and g[(2, 0, 0)]["nrows"] == 3
    assert g[(2, 1, 1)]["ids"] == [2]                         # the delayed cascade chain without a FIR: the HAND cascade, as before
    assert g[(17, 0, 0)]["ids"] == [4] and [(p["nsec"], p["wide"], p["hand"], p["all_fir"], p["nrows"]) for p in g[(17, 0, 0)]["pieces"]] == [(9, 0, 0, 0, 1), (8, 0, 0, 1, 1)]
    assert g[(5, 0, 0)]["ids"] == [5] and len(L["groups"]) == 4 and L["dev_chains"] == len(MIX) + 1
    assert [c for c in L["merged_rows"] if c >= 0] == [0, 1, 6, 5]                          # the merged row launch: as plain FIR chains


def test_layout_without_the_flag_keeps_the_texts(driver):
    assert layout(driver, 6, 0, MIX) == {"error": "chain 0: a dressed finish has no kernel here"}
    assert layout(driver, 6, 0, MIX[4:]) == {"error": "chain 0: a delay line has no kernel here"}
    assert layout(driver, 5, 1, MIX[4:]) == {"error": "chain 0: a delay line has no kernel here"}      # formats 4 and 6 only
    assert layout(driver, 3, 1, MIX[3:4]) == {"error": "chain 0: a dressed finish has no kernel here"}
    assert layout(driver, 2, 1, MIX[:1]) == {"error": "chain 0: FIR has no int64 definition"}


def test_layout_overlap_only_without_handed_chains(driver):
    plain = [(2, 64, 0, 0, 1), (3, 9, 0, 0, 0)]
    assert layout(driver, 6, 1, plain)["overlap_ok"] == 1
    assert layout(driver, 6, 1, plain + [(2, 64, 0, A, 1)])["overlap_ok"] == 0
    assert layout(driver, 6, 1, plain + [(2, 64, TPDF_GAIN, 0, 1)])["overlap_ok"] == 0


def test_layout_shared_groups_hold_plain_chains_only(driver):
    bank = [(0, 100, 0, 0, 1)] + [(2 if i % 2 else 0, 100, 0, 0, 1, 0) for i in range(1, 20)]
    bank[3] = (2, 100, TPDF_GAIN, A, 1, 0)
    bank[11] = (0, 100, 1, 0, 1, 0)
    L = layout(driver, 6, 1, bank, grouped=1)
    assert L["fir_hand"] == [3, 11] and L["shared_ids"] == [i for i in range(20) if i not in (3, 11)] and L["shared_rest"] == []
    L = layout(driver, 6, 1, bank + [(1, 30, 0, 0, 1)], grouped=0)
    assert L["shared_ids"] == [] and L["fir_plain"] == [i for i in range(21) if i not in (3, 11)]


@pytest.mark.parametrize("impl, n, frames, rows, want", [
    (1, 37, 100, 0, dict(family=1, R=1, BIG=1)), (1, 37, 1024, 1, dict(family=1, R=1, BIG=0)), (1, 5, 300, 2, dict(family=1, R=2, BIG=0)),
    (1, 5, 600, 4, dict(family=1, R=4, BIG=0)), (1, 5, 256, 2, dict(family=1, R=1, BIG=1)), (1, 5, 512, 4, dict(family=1, R=2, BIG=0)),
    (0, 5, 600, 4, dict(family=0, R=1, BIG=0)), (2, 5, 600, 0, dict(family=1, R=1, BIG=1)), (4, 4096, 1024, 0, dict(family=1, R=4, BIG=0))])
def test_hand_choice(driver, impl, n, frames, rows, want):
    """fir_tile with fir_impl 1 .. 4, fir_plain with 0; never split, always lean (fir_tile), always HAND"""
    r = subprocess.run([driver, "choice", str(impl), str(n), str(frames), str(rows)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    c = json.loads(r.stdout)
    assert c["HAND"] == 1 and c["SPLIT"] == 0 and c["LEAN"] == (1 if want["family"] == 1 else 0)
    assert {k: c[k] for k in want} == want

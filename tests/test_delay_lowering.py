"""Delay lines, host side ("chain_delay"): which cores dspRuntimeSetOption("chain_delay", 1) lowers to the chain kernels
-- one DSP_DELAY per chain behind the banks, on either side of the SAT0DB slot, fixed or parameter form -- and which stay with the
interpreter, each with a text of its own.  Host-only: dspRuntimeCoreInfo / dspRuntimeDelayInfo run nothing."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import delay_programs as dp


@pytest.fixture(autouse=True)
def _options_back():
    yield
    rt.Runtime.set_global_option("chain_delay", 0)
    rt.Runtime.set_global_option("chain_finish", 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, fs=48000):
    prog, _, _ = dp.program(fmt, cores)
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeDelayInfo lowers it and reports zeros when it is refused)"""
    assert r.delay_info(core_index) == (0, 0)
    return r.last_error()


def test_option_default_and_range():
    r = loaded(6, [dp.core([dp.chain(2, "A")])])
    assert r.get_option("chain_delay") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("chain_delay", bad)
    assert r.get_option("chain_delay") == 0
    rt.Runtime.set_global_option("chain_delay", 1)             # the default of programs loaded later
    r2 = loaded(6, [dp.core([dp.chain(2, "A")])])
    assert r2.get_option("chain_delay") == 1 and r2.core_info()["chains"] == 1 and r2.delay_info() == (1, dp.samples(1000))


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("form", ["fixed", "param"])
@pytest.mark.parametrize("slot", ["A", "B"])
def test_option_lowers_the_delayed_core(fmt, slot, form):
    ch = [dp.chain(2, slot, form, us=1000), dp.chain(0, slot, form, us=2100, finish="sat" if slot == "B" else "none"),
          dp.chain(17, slot, form, us=63, stores=2), dp.chain(1, None)]
    r = loaded(fmt, [dp.core(ch)])
    assert r.core_info()["chains"] == 0 and r.delay_info() == (0, 0)
    assert "opcode 47" in r.last_error() and "is not lowered to the HIP path" in r.last_error()      # today's text, through `default:`
    r.set_option("chain_delay", 1)
    assert r.core_info() == dict(chains=4, max_sections=17, max_taps=0)
    assert r.delay_info() == (3, dp.samples(2100)) and dp.samples(2100) == 100
    r.set_option("chain_delay", 0)
    assert r.core_info()["chains"] == 0 and r.delay_info() == (0, 0)


def test_line_lengths_follow_the_rate_and_the_parameter():
    ch = [dp.chain(1, "A", "param", us=1000, max_us=1500), dp.chain(1, "A", "fixed", us=20), dp.chain(0, "B", "param", us=25000, max_us=25000)]
    prog, _, _ = dp.program(6, [dp.core(ch)])
    r = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_delay", 1)
    assert dp.samples(20) == 0 and dp.samples(21) == 1 and dp.samples(63) == 3 and dp.samples(1000) == 47 and dp.samples(25000) == 1199
    assert r.delay_info() == (3, 1199)
    w = dp.us_words(prog)
    assert len(w) == 2
    r.buf[w[1]] = 0                                            # the long line bypassed: the 1000 us line is the longest
    assert r.delay_info() == (3, 47)
    r.buf[w[0]] = 60000                                        # ... asked for more than its size: clamped to 1500 us at 48 kHz
    assert r.delay_info() == (3, dp.samples(60000, max_us=1500)) and dp.samples(60000, max_us=1500) == 72
    r44 = rt.Runtime(6, prog, fs=44100, random=1, dither=24)
    r44.set_option("chain_delay", 1)
    assert r44.delay_info() == (3, dp.samples(25000, 44100)) and dp.samples(25000, 44100) == 1102


def test_shard_counts_its_own_chains():
    ch = [dp.chain(1, "A" if i % 2 else None, us=100 * (i + 1)) for i in range(12)]
    r = loaded(4, [dp.core(ch)])
    r.set_option("chain_delay", 1)
    r.set_shard(1, 3)                                          # chains 4 .. 7: the delayed ones are 5 and 7
    assert r.delay_info() == (2, dp.samples(800))
    r.set_shard(0, 1)
    assert r.delay_info() == (6, dp.samples(1200))


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("finish", ["tpdf", "gain", "tpdf_gain"])
def test_a_dressed_finish_needs_chain_finish_too(fmt, finish):
    r = loaded(fmt, [dp.core([dp.chain(2, "A", finish=finish), dp.chain(0, "B", finish=finish)], calc=0)])
    r.set_option("chain_delay", 1)
    assert chains_of(r) == 0
    assert "is not lowered to the HIP path" in refusal(r) and "opcode 47" not in r.last_error()      # the dressed opcode's (or TPDF_CALC's) refusal, as before
    r.set_option("chain_finish", 1)
    assert r.core_info()["chains"] == 2 and r.delay_info() == (2, 47) and r.finish_info() == (2, 1)
    r.set_option("chain_delay", 0)
    assert chains_of(r) == 0 and "opcode 47" in refusal(r)


def test_plain_and_no_finish_do_not_need_chain_finish():
    r = loaded(6, [dp.core([dp.chain(2, "A", finish="sat"), dp.chain(2, "A", finish="none"), dp.chain(0, "B", finish="sat"), dp.chain(0, "A", finish="none")])])
    r.set_option("chain_delay", 1)
    assert r.get_option("chain_finish") == 0 and r.core_info()["chains"] == 4 and r.delay_info() == (4, 47)


REFUSED = {
    "delay_dp": (6, [dp.core([dp.chain(2, "A", odd="dp")])], "DSP_DELAY_DP is not lowered"),
    "delay_1": (4, [dp.core([dp.chain(2, "A", odd="d1")])], "DSP_DELAY_1 is not lowered"),
    "delay_dp_int64": (2, [dp.core([dp.chain(0, "B", odd="dp")])], "DSP_DELAY_DP is not lowered"),
    "in_front_of_the_banks": (6, [dp.core([dp.chain(2, None, odd="head")])], "a DSP_DELAY in front of the banks"),
    "behind_a_store": (6, [dp.core([dp.chain(2, None, stores=2, odd="stored")])], "a DSP_DELAY behind a STORE"),
    "two_delays": (2, [dp.core([dp.chain(2, "B", odd="two")])], "a second DSP_DELAY in one chain"),
    "two_delays_no_sat": (6, [dp.core([dp.chain(2, "B", finish="none", odd="two")])], "a second DSP_DELAY in one chain"),
    "with_a_fir": (6, [dp.core([dp.chain(2, "A", odd="fir")])], "a DSP_DELAY in a chain with a DSP_FIR"),
    "mux_head": (6, [dp.core([dp.chain(2, "A", odd="mux"), dp.chain(1, None)])], "a DSP_FIR or a LOAD_MUX head"),
    "beside_mux_chains": (4, [dp.core([dp.chain(2, None, odd="mux"), dp.chain(1, "A")])], "beside LOAD_MUX heads"),
    "format_3": (3, [dp.core([dp.chain(2, "A")])], "in format 3"),
    "format_5": (5, [dp.core([dp.chain(0, "B")])], "in format 5"),
    "sat0db_on_both_sides": (6, [dp.core([dp.chain(2, "B", odd="sat_twice")])], "SAT0DB outside the supported chain order"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_not_lowered_with_the_option_on(case):
    fmt, cores, text = REFUSED[case]
    r = loaded(fmt, cores)
    r.set_option("chain_delay", 1)
    assert chains_of(r) == 0
    assert text in refusal(r), r.last_error()


def test_instances_keep_delayed_cores_on_the_interpreter():
    r = loaded(6, [dp.core([dp.chain(2, "A"), dp.chain(0, "B")])])
    r.set_option("chain_delay", 1)
    assert r.core_info()["chains"] == 2
    r.set_instances(4)
    assert r.core_info()["chains"] == 0 and "while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.core_info()["chains"] == 2 and r.delay_info() == (2, 47)


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("which", ["payload_too_short", "data_offset_past_the_data", "data_offset_negative", "line_past_the_data",
                                   "parameter_past_the_program", "parameter_in_front_of_the_program", "negative_size", "shared_line"])
def test_damaged_payloads_are_refused_not_followed(fmt, which):
    prog, _, _ = dp.program(fmt, [dp.core([dp.chain(2, "A", "param", us=1000), dp.chain(1, "B", "fixed", us=2100)])])
    prog = prog.copy()
    par, fix = dp.words_of(prog, dp.OP_DELAY)
    data = int(prog[2])
    text = "outside the state area"
    if which == "payload_too_short":
        # the opcode shortened to two payload words, the word it gives up made a NOP of one word
        prog[fix] = (dp.OP_DELAY << 16) | 3
        prog[fix + 3] = 1
        text = "opcode payload shorter than 3 words"
    elif which == "data_offset_past_the_data":
        prog[par + 2] = 1 << 24
    elif which == "data_offset_negative":
        prog[fix + 2] = 0xFFFFFFFE
    elif which == "line_past_the_data":
        prog[fix + 2] = data - dp.samples(2100)                # index word + 100 samples: one word too many
    elif which == "parameter_past_the_program":
        prog[par + 3] = 1 << 24
        text = "outside the program"
    elif which == "parameter_in_front_of_the_program":
        prog[par + 3] = np.uint32(-(par + 5) & 0xFFFFFFFF)
        text = "outside the program"
    elif which == "negative_size":
        prog[par + 1] = 0x80000010
        text = "negative size"
    elif which == "shared_line":
        prog[fix + 2] = int(prog[par + 2]) + 3                 # inside the first chain's line
        text = "share words of the state area"
    dp.resealed(prog)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    assert r.rc >= 0
    r.set_option("chain_delay", 1)
    assert r.delay_info() == (0, 0)
    assert text in r.last_error(), r.last_error()
    assert chains_of(r) == 0


def test_line_that_just_fits_is_lowered():
    prog, _, _ = dp.program(6, [dp.core([dp.chain(1, "B", "fixed", us=2100)])])
    prog = prog.copy()
    (fix,) = dp.words_of(prog, dp.OP_DELAY)
    prog[fix + 2] = int(prog[2]) - dp.samples(2100) - 1
    dp.resealed(prog)
    r = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_delay", 1)
    assert r.delay_info() == (1, 100)

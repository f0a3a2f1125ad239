"""Dressed finishes, host side ("chain_finish"): which cores dspRuntimeSetOption("chain_finish", 1) lowers to the chain
kernels -- SAT0DB_TPDF / SAT0DB_GAIN / SAT0DB_TPDF_GAIN in the SAT0DB slot, one TPDF_CALC at the head -- and which stay with the
interpreter.  Host-only: dspRuntimeCoreInfo / dspRuntimeFinishInfo run nothing."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import finish_programs as fp


@pytest.fixture(autouse=True)
def _option_back():
    yield
    rt.Runtime.set_global_option("chain_finish", 0)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, dither=24):
    prog, _, _ = fp.program(fmt, cores)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=dither)
    assert r.rc >= 0
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("finish", fp.FINISHES)
def test_option_lowers_the_dressed_core(fmt, finish):
    N = 5
    r = loaded(fmt, [fp.core([fp.chain(2, finish) for _ in range(N)], calc=0)])
    assert r.get_option("chain_finish") == 0
    assert r.core_info()["chains"] == 0 and r.finish_info() == (0, 0)
    r.set_option("chain_finish", 1)
    assert r.get_option("chain_finish") == 1
    assert r.core_info()["chains"] == N and r.finish_info() == (N, 1)
    r.set_option("chain_finish", 0)
    assert r.core_info()["chains"] == 0 and r.finish_info() == (0, 0)


def test_option_is_the_default_of_later_programs_and_takes_0_or_1():
    rt.Runtime.set_global_option("chain_finish", 1)
    r = loaded(6, [fp.core([fp.chain(1, "gain"), fp.chain(0, "tpdf"), fp.chain(3, "sat")])])
    assert r.get_option("chain_finish") == 1
    assert r.core_info()["chains"] == 3 and r.finish_info() == (2, 0)
    with pytest.raises(rt.AvdspError):
        r.set_option("chain_finish", 2)


def test_calc_width_equal_to_the_default_is_taken():
    r = loaded(4, [fp.core([fp.chain(2, "tpdf")], calc=24)])
    r.set_option("chain_finish", 1)
    assert r.core_info()["chains"] == 1 and r.finish_info() == (1, 1)


REFUSED = {
    "calc_behind_a_load": (6, [fp.core([fp.chain(2, "tpdf", head="calc"), fp.chain(2, "tpdf")])]),
    "calc_16_under_24": (6, [fp.core([fp.chain(2, "tpdf")], calc=16)]),
    "tpdf_opcode": (6, [fp.core([fp.chain(2, "tpdf", head="tpdf_op"), fp.chain(2, "tpdf")], calc=0)]),
    "fir_and_sat0db_tpdf": (6, [fp.core([fp.chain(2, "tpdf", head="fir")], calc=0)]),
    "fir_and_sat0db_tpdf_f4": (4, [fp.core([fp.chain(0, "tpdf_gain", head="fir")])]),
    "load_mux_head": (6, [fp.core([fp.chain(2, "tpdf", head="mux"), fp.chain(2, "tpdf")], calc=0)]),
    "load_mux_head_beside": (4, [fp.core([fp.chain(2, "sat", head="mux"), fp.chain(2, "gain")])]),
    "format_3": (3, [fp.core([fp.chain(2, "tpdf")], calc=0)]),
    "format_5": (5, [fp.core([fp.chain(2, "gain")])]),
    "two_calcs": (6, [fp.core([fp.chain(2, "tpdf", head="calc")], calc=0)]),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_not_lowered_with_the_option_on(case):
    fmt, cores = REFUSED[case]
    r = loaded(fmt, cores)
    r.set_option("chain_finish", 1)
    assert chains_of(r) == 0
    assert r.finish_info() == (0, 0)


@pytest.mark.parametrize("fmt", [2, 6])
def test_another_cores_calc_of_another_width_keeps_every_core_on_the_interpreter(fmt):
    dressed = fp.core([fp.chain(2, "tpdf"), fp.chain(1, "tpdf_gain")], calc=0)
    r = loaded(fmt, [dressed, fp.core([fp.chain(1, "sat")], calc=16)])
    r.set_option("chain_finish", 1)
    assert chains_of(r, 0) == 0 and r.finish_info(0) == (0, 0)
    assert chains_of(r, 1) == 0
    # the same first core beside a plain second one is lowered
    r2 = loaded(fmt, [dressed, fp.core([fp.chain(1, "sat")])])
    r2.set_option("chain_finish", 1)
    assert r2.core_info(0)["chains"] == 2 and r2.finish_info(0) == (2, 1)
    assert r2.core_info(1)["chains"] == 1 and r2.finish_info(1) == (0, 0)


def test_instances_keep_dressed_cores_on_the_interpreter():
    r = loaded(6, [fp.core([fp.chain(2, "tpdf")], calc=0)])
    r.set_option("chain_finish", 1)
    assert r.core_info()["chains"] == 1
    r.set_instances(4)
    assert r.core_info()["chains"] == 0 and r.finish_info() == (0, 0)
    r.set_instances(0)
    assert r.core_info()["chains"] == 1 and r.finish_info() == (1, 1)


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("which", ["gain_past_the_program", "gain_in_front_of_the_program", "result_past_the_data", "result_negative",
                                   "result_on_the_last_word"])
def test_damaged_offsets_are_refused_not_followed(fmt, which):
    prog, _, _ = fp.program(fmt, [fp.core([fp.chain(2, "tpdf_gain"), fp.chain(1, "gain")], calc=0)])
    prog = prog.copy()
    if which.startswith("gain"):
        op = fp.words_of(prog, fp.OP_SAT0DB_TPDF_GAIN)[0]
        prog[op + 1] = (1 << 24) if which == "gain_past_the_program" else np.uint32(-(op + 5) & 0xFFFFFFFF)
    else:
        op = fp.words_of(prog, fp.OP_TPDF_CALC)[0]
        prog[op + 2] = {"result_past_the_data": 1 << 24, "result_negative": 0xFFFFFFFE, "result_on_the_last_word": int(prog[2]) - 1}[which]
    fp.resealed(prog)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    assert r.rc >= 0
    r.set_option("chain_finish", 1)
    with pytest.raises(rt.AvdspError) as e:                    # refused by the chain lowering, and by the interpreter's scan behind it
        r.core_info()
    assert e.value.code == -8
    assert r.finish_info() == (0, 0)

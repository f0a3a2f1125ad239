"""Host-only checks of the LOAD_MUX chain heads: lower_core takes a weighted sum of inputs as the head of a chain in
formats 2, 4 and 6, dspRuntimeMuxInfo reports the mix groups (lists of one IO sequence, 16 chains or more, formed on the rank's
slice), damaged tables are refused without a crash, and progbuilder's words are the repo encoder's.  No GPU: nothing runs a block."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from avdsp_amd import encoder as enc
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests.mux_recipes import (EDGE_PROGRAMS, ROW_TAIL_GROUPS, SEAM_LENGTHS, check_seam_lengths, expected_mux_info, live_edit, mixer_program, mux_tables,
                               several_groups)


@pytest.fixture(autouse=True)
def _release():
    yield
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def words_of(prog, op):
    """word indices of the opcodes `op` in the opcode stream"""
    pos, at = 0, []
    while True:
        skip, code = int(prog[pos]) & 0xFFFF, int(prog[pos]) >> 16
        if skip == 0:
            return at
        if code == op:
            at.append(pos)
        pos += skip


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_shared_lists_are_one_group(fmt):
    r = rt.Runtime(fmt, pb.synth_mixer_program(fmt, 40, 9, 2))
    assert r.core_info() == dict(chains=40, max_sections=2, max_taps=0)
    assert r.mux_info() == dict(mux_chains=40, groups=1, grouped_chains=40, longest_list=9)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_private_lists_are_no_group(fmt):
    r = rt.Runtime(fmt, pb.synth_mixer_program(fmt, 40, 24, 0, lists="private", entries=5))
    assert r.core_info()["chains"] == 40
    assert r.mux_info() == dict(mux_chains=40, groups=0, grouped_chains=0, longest_list=5)


def test_fifteen_chains_are_no_group():
    r = rt.Runtime(6, pb.synth_mixer_program(6, 15, 4, 1))
    assert r.core_info()["chains"] == 15
    assert r.mux_info() == dict(mux_chains=15, groups=0, grouped_chains=0, longest_list=4)
    r = rt.Runtime(6, pb.synth_mixer_program(6, 16, 4, 1))
    assert r.mux_info() == dict(mux_chains=16, groups=1, grouped_chains=16, longest_list=4)


def test_same_ios_in_another_order_are_another_group():
    """20 lists on inputs (0, 1, 2), 18 on (2, 1, 0), 3 on (0, 1): two groups, the short ones in none"""
    O = 41
    pw = pb.ProgramWriter(6, capacity=4096)
    pw.core()
    for o in range(O):
        pw.param()
        ios = (0, 1, 2) if o % 2 == 0 and o < 40 else (2, 1, 0) if o < 36 else (0, 1)
        t = pw.mux_inputs([(O + io, 0.1 * (o + 1) / O) for io in ios])
        pw.load_mux(t)
        pw.store(o)
    r = rt.Runtime(6, pw.end_of_code())
    assert r.core_info()["chains"] == O
    assert r.mux_info() == dict(mux_chains=O, groups=2, grouped_chains=38, longest_list=3)


def test_fir_behind_the_head():
    r = rt.Runtime(6, pb.synth_mixer_program(6, 20, 8, 3, ntaps=31))
    assert r.core_info() == dict(chains=20, max_sections=3, max_taps=31)
    with pytest.raises(rt.AvdspError):                                    # (the int64 FIR stays refused)
        rt.Runtime(2, pb.synth_mixer_program(6, 20, 8, 3, ntaps=31)).core_info()


def test_groups_follow_the_shard():
    prog = pb.synth_mixer_program(6, 40, 6, 1)
    rt.lib().dspRuntimeSetShard(1, 3)                                     # chains 14 .. 26: 13 of them
    r = rt.Runtime(6, prog)
    assert r.shard_info()["nchains"] == 13
    assert r.mux_info() == dict(mux_chains=13, groups=0, grouped_chains=0, longest_list=6)
    rt.lib().dspRuntimeSetShard(0, 2)
    r.release()
    r = rt.Runtime(6, prog)
    assert r.mux_info() == dict(mux_chains=20, groups=1, grouped_chains=20, longest_list=6)


@pytest.mark.parametrize("fmt", [3, 5])
def test_float_accumulator_formats_keep_the_interpreter(fmt):
    r = rt.Runtime(fmt, pb.synth_mixer_program(6, 20, 4, 2))
    assert r.core_info()["chains"] == 0
    assert r.mux_info() == dict(mux_chains=0, groups=0, grouped_chains=0, longest_list=0)


def test_generic_option_keeps_the_interpreter():
    r = rt.Runtime(6, pb.synth_mixer_program(6, 20, 4, 2))
    r.set_option("generic", 1)
    try:
        assert r.core_info()["chains"] == 0 and r.mux_info()["mux_chains"] == 0
    finally:
        r.set_option("generic", 0)


def test_list_io_stored_by_the_core_is_not_lowered():
    O = 4
    pw = pb.ProgramWriter(6, capacity=1024)
    pw.core()
    for o in range(O):
        pw.param()
        t = pw.mux_inputs([(O + 0, 0.5), (1 if o == 3 else O + 1, 0.25)])   # chain 3 mixes IO 1, which chain 1 stores
        pw.load_mux(t)
        pw.store(o)
    r = rt.Runtime(6, pw.end_of_code())
    assert r.core_info()["chains"] == 0
    assert r.mux_info()["mux_chains"] == 0


def damaged(which):
    prog = pb.synth_mixer_program(6, 3, 4, 1).copy()
    op = words_of(prog, pb.OP_LOAD_MUX)[1]
    table = op + int(np.int32(prog[op + 1]))
    assert int(prog[table]) == (pb.OP_LOAD_MUX << 16) | 4
    if which == "count0":
        prog[table] = pb.OP_LOAD_MUX << 16
    elif which == "count_negative":
        prog[table] = (pb.OP_LOAD_MUX << 16) | 0x8000
    elif which == "count_past_the_program":
        prog[table] = (pb.OP_LOAD_MUX << 16) | 0x7FFF
    elif which == "io_high":
        prog[table + 3] = 1 << 20
    elif which == "io_negative":
        prog[table + 1] = 0xFFFFFFFF
    elif which == "result_outside":
        prog[op + 2] = int(prog[2]) - 1                                  # 8 bytes from the last state word on
    elif which == "result_negative":
        prog[op + 2] = 0xFFFFFFFE
    elif which == "table_outside":
        prog[op + 1] = 1 << 24
    prog[3] = pb.checksum(prog)[0]
    return prog


@pytest.mark.parametrize("which", ["count0", "count_negative", "count_past_the_program", "io_high", "io_negative", "result_outside",
                                   "result_negative", "table_outside"])
def test_damaged_table_is_refused(which):
    r = rt.Runtime(6, damaged(which))
    assert r.rc >= 0
    with pytest.raises(rt.AvdspError) as e:
        r.mux_info()
    assert e.value.code == -8
    try:                                                                  # the core is no chain core; the interpreter's scan decides the rest
        assert r.core_info()["chains"] == 0
    except rt.AvdspError as e2:
        assert e2.code == -8


def test_shard_info_spans_the_list_ios():
    O = 30
    pw = pb.ProgramWriter(6, capacity=4096)
    pw.core()
    for o in range(O):
        pw.param()
        t = pw.mux_inputs([(100 + 2 * o + 1, 0.5), (100 + 2 * o, 0.25), (40 + o, 0.1)])
        pw.load_mux(t)
        pw.sat0db()
        pw.store(o)
    prog = pw.end_of_code()
    r = rt.Runtime(6, prog)
    s = r.shard_info()
    assert (s["total_chains"], s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (30, 40, 159, 0, 29)
    rt.lib().dspRuntimeSetShard(2, 3)                                     # chains 20 .. 29
    r.release()
    r = rt.Runtime(6, prog)
    s = r.shard_info()
    assert (s["first_chain"], s["nchains"], s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (20, 10, 60, 159, 20, 29)


@pytest.mark.parametrize("fmt", [2, 6])
def test_mux_words_are_the_encoders(fmt):
    """ProgramWriter.mux_inputs / load_mux against libavdsp_encoder.so's dspLoadMux_Inputs / dspLoadMux_Data / dsp_LOAD_MUX"""
    lists = [[(8, 0.5), (9, -0.25), (40, 1.9990234)], [(9, 0.125)], [(10, -2.0), (10, 0.3), (8, 0.0), (33, 0.7)]]
    lists = [[(io, float(np.float32(g))) for io, g in pairs] for pairs in lists]      # (dspGainParam_t is a float)

    def build(L):
        L.dspLoadMux_Inputs.argtypes = [C.c_int]
        L.dspLoadMux_Data.argtypes = [C.c_int, C.c_float]
        L.dsp_LOAD_MUX.argtypes = [C.c_int]; L.dsp_LOAD_MUX.restype = C.c_int
        L.dsp_PARAM.restype = C.c_int
        L.dsp_CORE()
        for o, pairs in enumerate(lists):
            L.dsp_PARAM()
            t = L.dspLoadMux_Inputs(len(pairs))
            for io, g in pairs:
                L.dspLoadMux_Data(io, g)
            L.dsp_LOAD_MUX(t)
            L.dsp_SAT0DB()
            L.dsp_STORE(o)

    want = enc.encode(build, fmt, pb.F48000, pb.F48000)
    pw = pb.ProgramWriter(fmt, capacity=1024)
    pw.core()
    for o, pairs in enumerate(lists):
        pw.param()
        t = pw.mux_inputs(pairs)
        pw.load_mux(t)
        pw.sat0db()
        pw.store(o)
    got = pw.end_of_code()
    assert len(got) == len(want) and (got == want).all()


# sha-256 (first 16 hex digits) of synth_program's words as the commit before the mixer helpers made them
SYNTH_SHA = {
    (6, 8, 4, 300): "6f95e3e9ffbdece0", (6, 40, 16, 64): "15cb653e879df915", (4, 17, 0, 65): "3d6e88c272770fb8",
    (2, 64, 16, 0): "c6237d4ecc797949", (3, 5, 3, 7): "0ec1286eeb2940d7", (5, 6, 2, 0): "e4d40e26e1a71936",
    (6, 12, 2, 33, pb.F44100, pb.F96000): "bd9953118c186236",
}


@pytest.mark.parametrize("args", list(SYNTH_SHA), ids=str)
def test_synth_program_is_unchanged(args):
    w = pb.synth_program(*args)
    assert hashlib.sha256(np.ascontiguousarray(w).tobytes()).hexdigest()[:16] == SYNTH_SHA[args]


def test_synth_program_with_banks_is_unchanged():
    w = pb.synth_program(6, 40, 1, 16, fir_banks=2)
    assert hashlib.sha256(np.ascontiguousarray(w).tobytes()).hexdigest()[:16] == "07d3da7d45d8c6ba"


def test_mixer_recipe_is_a_chain_core():
    prog = mixer_program(dict(fmt=4, outputs=20, inputs=17, entries=17, lists="twice", sections=2, taps=9, sat=1, seed=5))
    r = rt.Runtime(4, prog)
    assert r.core_info() == dict(chains=20, max_sections=2, max_taps=9)
    assert r.mux_info() == dict(mux_chains=20, groups=1, grouped_chains=20, longest_list=17)


# ---- the programs of tests/test_gpu_mux_edges.py: what dspRuntimeMuxInfo says of them, and a run of the oracle over each ----------------

EDGE_INFO = dict(
    several_groups=dict(mux_chains=121, groups=3, grouped_chains=103, longest_list=64),
    list_seams=dict(mux_chains=16 * len(SEAM_LENGTHS), groups=29, grouped_chains=16 * len(SEAM_LENGTHS), longest_list=129),
    row_tails=dict(mux_chains=sum(ROW_TAIL_GROUPS), groups=12, grouped_chains=sum(ROW_TAIL_GROUPS), longest_list=6),
    shard_40=dict(mux_chains=40, groups=1, grouped_chains=40, longest_list=12),
    shard_47=dict(mux_chains=47, groups=1, grouped_chains=47, longest_list=12),
    live_edit=dict(mux_chains=36, groups=2, grouped_chains=33, longest_list=7),
    small_mixer=dict(mux_chains=20, groups=1, grouped_chains=20, longest_list=5),
    small_mixer_fir=dict(mux_chains=20, groups=1, grouped_chains=20, longest_list=5),
    windows=dict(mux_chains=21, groups=1, grouped_chains=16, longest_list=4),
    stored=dict(mux_chains=143, groups=1, grouped_chains=136, longest_list=6),
)


def test_the_list_lengths_sit_on_the_seams():
    check_seam_lengths()


def test_every_edge_program_is_listed():
    assert set(EDGE_INFO) == set(EDGE_PROGRAMS)
    assert sum(ROW_TAIL_GROUPS) == 627 and len(SEAM_LENGTHS) == 29


@pytest.mark.parametrize("fmt", [6, 4, 2])
@pytest.mark.parametrize("name", sorted(EDGE_PROGRAMS))
def test_edge_program_groups_and_oracle_run(name, fmt):
    """every chain of the program is lowered, the groups are the ones its lists spell, and the oracle runs it: every stored IO
    carries a signal, no other does"""
    prog, meta = EDGE_PROGRAMS[name](fmt)
    r = rt.Runtime(fmt, prog)
    assert r.rc > 0
    assert r.core_info()["chains"] == meta["nchains"]
    assert r.mux_info() == EDGE_INFO[name] == expected_mux_info(meta)
    assert len(mux_tables(prog)) == EDGE_INFO[name]["mux_chains"]
    o = po.OracleProgram(fmt, prog)
    assert o.rc == r.rc
    W, I = meta["width"], meta["inputs"]
    out = o.run_block(pb.lcg_input(24, I, fmt == 6, seed=7), W, W)
    stored = sorted(io for ch in meta["chains"] for io in ch["out"])
    assert len(set(stored)) == len(stored)
    live = np.nonzero((out != 0).any(axis=0))[0].tolist()
    assert live == stored, f"{name}: IOs {sorted(set(stored) ^ set(live))[:8]} are stored without a signal, or carry one unstored"
    assert o.state.any()


def test_the_interleaved_groups_scatter_a_tiles_chains():
    _, meta = several_groups(6)
    ids = [c for c, ch in enumerate(meta["chains"]) if ch["group"] == 2]
    assert len(ids) == 70 and ids[:3] == [2, 8, 14] and ids[-1] == meta["nchains"] - 1 == 122
    assert min(np.diff(ids[:16])) > 1                                                   # no two chains of its first row tile are neighbours
    gains = {(v, j) for ch in meta["chains"] if ch["group"] == 2 for j, v in enumerate(ch["gains"])}
    assert len(gains) > 70 * 64 - 3 * 70 * 2                                            # the gains differ by chain and position


def test_live_edit_groups_after_the_edits():
    """the host-only twin of test_gpu_mux_edges.test_live_edits: a list that names another IO leaves its group; a group of 15 is none"""
    prog, meta = live_edit(6)
    tabs, W = mux_tables(prog), meta["width"]
    r = rt.Runtime(6, prog)
    assert r.mux_info() == dict(mux_chains=36, groups=2, grouped_chains=33, longest_list=7)
    assert int(r.buf[tabs[5] + 1 + 2 * 3]) == W + 3 and int(r.buf[tabs[20] + 1 + 2 * 1]) == W + 4
    r.buf[tabs[5] + 1 + 2 * 3] = W + 5
    assert r.mux_info() == dict(mux_chains=36, groups=2, grouped_chains=32, longest_list=7)
    r.buf[tabs[20] + 1 + 2 * 1] = W + 3
    assert r.mux_info() == dict(mux_chains=36, groups=1, grouped_chains=16, longest_list=7)

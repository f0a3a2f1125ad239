"""Dressed finishes, delay lines and a head TPDF_CALC in cores with LOAD_MUX chain heads ("mux_tail" 1): the WIDE / HAND
cascade groups and the handed FIR launch behind a column of the mux stage, and the stage's own TAIL forms -- mux_tile<., true> and
mux_plain<., true> finish a sectionless dressed chain from the full accumulator and hand a sectionless delayed one to chain_tail.  The
interpreter gives the same bits, so every case first asserts through dspRuntimeMuxTailInfo / CoreInfo / FinishInfo / DelayInfo /
FirTailInfo that its core is on the chain kernels, with the kinds it expects ("mux_tail" 0 is the control), then is held to the oracle
word for word: the outputs of every block and the whole state area after it (lines, index words, LOAD_MUX result words, the TPDF_CALC
result, the generator)."""
import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import muxtail_programs as mp

pytestmark = pytest.mark.gpu
IN = mp.IN
BLOCKS = [1, 7, 64, 65, 100, 333, 1029]              # in sequence at 48 kHz; 65: a second frame tile of mux_tile; 1029: two launches (block_f0 in the addend table)
OPTIONS = ("chain_finish", "chain_delay", "fir_tail", "mux_tail")


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key, v in [(k, 0) for k in OPTIONS] + [("biquad_impl", 1)]:
        rt.Runtime.set_global_option(key, v)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    g, w = words(got), words(want)
    bad = np.nonzero((g != w).any(axis=0))[0]
    assert bad.size == 0, (f"{what}: outputs {bad[:8].tolist()} differ, first frame "
                           f"{np.nonzero(g[:, bad[0]] != w[:, bad[0]])[0][:3].tolist()}: "
                           f"{g[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()} for {w[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()}")


def same_state(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} state words differ, first {bad[:6].tolist()}"


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def tailed_runtime(fmt, prog, cores=None, dither=24, fs=48000, stage=True):
    """the four options on; every core must be on the chain kernels with the kinds `cores` (a list of chain lists) says.  On the code
    before "mux_tail" the option and dspRuntimeMuxTailInfo do not exist: every test here fails there."""
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=dither)
    for key in OPTIONS:
        r.set_option(key, 1)
    for k, chains in enumerate(cores or []):
        want = mp.counts(chains, fs)
        assert r.core_info(k)["chains"] == len(chains), r.last_error()
        assert r.mux_info(k)["mux_chains"] == sum(1 for c in chains if c["mux"]) > 0
        assert r.mux_tail_info(k) == want["mux_tail"] and (want["mux_tail"][2] > 0) == stage
        assert r.finish_info(k)[0] == want["dressed"] and r.delay_info(k) == want["delay"] and r.fir_tail_info(k) == want["fir_tail"]
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def run_and_compare(r, o, x, nout, what, blocks, run="run_block"):
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN)
        same(getattr(r, run)(x[a:a + b], nout, IN), want, f"{what}, block {k} of {b} frames")
        same_state(r.sync_state(), o.state, f"{what}, after block {k}")


# ---- 1. the five kinds of chain in one core -----------------------------------------------------------------------------------------------
_REF = {}


def five_kinds(fmt, dither=24):
    """program, input, and the oracle's outputs and state after each block -- computed once, shared, never written"""
    key = (fmt, dither)
    if key not in _REF:
        chains, group = mp.five_kinds_chains()
        prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
        x = pb.lcg_input(sum(BLOCKS), nin, fmt == 6, seed=31)
        o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
        outs, states = [], []
        for a, b in cut(BLOCKS):
            outs.append(o.run_block(x[a:a + b], nout, IN))
            states.append(o.state.copy())
        for v in outs + states + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, nout, outs, states, chains, group)
    return _REF[key]


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_five_kinds_in_one_core(fmt, dither):
    prog, x, nout, outs, states, chains, group = five_kinds(fmt, dither)
    r = tailed_runtime(fmt, prog, [chains], dither)
    assert r.finish_info()[1] == 1
    assert r.mux_info() == dict(mux_chains=117, groups=3, grouped_chains=98, longest_list=33)
    for k, (a, b) in enumerate(cut(BLOCKS)):
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, dither {dither}, block {k} of {b} frames")
        same_state(r.sync_state(), states[k], f"format {fmt}, dither {dither}, after block {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with "mux_tail" 0 -- no chain, the same bits"""
    prog, x, nout, outs, states, chains, _ = five_kinds(fmt)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    for key in OPTIONS[:3]:
        r.set_option(key, 1)
    assert r.get_option("mux_tail") == 0 and r.mux_tail_info() == (0, 0, 0) and chains_of(r) == 0
    for k, (a, b) in enumerate(cut(BLOCKS[:5])):
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, mux_tail 0, block {k}")
        same_state(r.sync_state(), states[k], f"format {fmt}, mux_tail 0, after block {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_switched_off_and_on_inside_one_stream(fmt):
    """the chain kernels run the first blocks, the interpreter the next, the chain kernels the last: lines, counters, result words and
    generator go over through the mirror both ways"""
    prog, x, nout, outs, states, chains, _ = five_kinds(fmt)
    r = tailed_runtime(fmt, prog, [chains])
    for k, (a, b) in enumerate(cut(BLOCKS)):
        if k == 2:
            r.set_option("mux_tail", 0)
            assert r.mux_tail_info() == (0, 0, 0) and chains_of(r) == 0
        if k == 4:
            r.set_option("mux_tail", 1)
            assert r.core_info()["chains"] == len(chains) and r.mux_tail_info() == mp.counts(chains)["mux_tail"]
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, option switched, block {k}")
        same_state(r.sync_state(), states[k], f"format {fmt}, option switched, block {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_biquad_impl_0(fmt):
    """the cross-check cascade (biquad_simple's WIDE and HAND forms) behind the stage's columns"""
    prog, x, nout, outs, states, chains, _ = five_kinds(fmt)
    r = tailed_runtime(fmt, prog, [chains])
    r.set_option("biquad_impl", 0)
    for k, (a, b) in enumerate(cut(BLOCKS[:5])):
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, biquad_impl 0, block {k}")
        same_state(r.sync_state(), states[k], f"format {fmt}, biquad_impl 0, after block {k}")


# ---- 2. the reference's own program shape -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["run_block_all", "run_block"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_reference_dac_program_shape(fmt, run):
    """four cores of LOAD_MUX(2) -> BIQUADS(12) -> SAT0DB -> DELAY(param, max 5000 us, default 0) -> STORE, STORE: as authored (every
    line bypassed), then with the microsecond words edited to 2100 us through dspRuntimeUploadParams"""
    cores = mp.reference_shape_cores()
    prog, nin, nout = mp.program(fmt, cores)
    w = mp.us_words(prog)
    assert len(w) == 4 and nout == 8
    x = pb.lcg_input(64 + 300 + 300 + 1100, nin, fmt == 6, seed=9)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [c["chains"] for c in cores], stage=False)
    assert [r.delay_info(k) for k in range(4)] == [(1, 0)] * 4 and [r.mux_tail_info(k) for k in range(4)] == [(0, 1, 0)] * 4
    run_and_compare(r, o, x[:364], nout, f"format {fmt}, {run}, as authored", [64, 300], run)
    for word in w:
        o.buf[word] = 2100
        r.buf[word] = 2100
    r.upload_params()
    assert [r.delay_info(k) for k in range(4)] == [(1, mp.samples(2100))] * 4
    run_and_compare(r, o, x[364:], nout, f"format {fmt}, {run}, 2100 us", [300, 1100], run)


# ---- 3. in-place calls ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [6, 2])
def test_one_frame_and_100_frames_in_place(fmt):
    """143 dressed chains that the stage finishes itself (format 6: three workgroups of mux_tile<6, true>; format 2: mux_plain<2, true>),
    input IO IN + j in the column where output j goes: the stage reads a copy of the block, for one-frame calls too"""
    import torch
    O, I = 143, 6
    chains = mp.in_place_chains(O, I)
    prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
    assert (nin, nout) == (I, O)
    x = pb.lcg_input(104, I, fmt == 6, seed=77)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [chains])
    assert r.mux_tail_info() == (O, 0, O)
    for a, b in cut([1, 1, 100, 1, 1]):
        want = o.run_block(x[a:a + b], O, IN)
        frame = np.zeros((b, O), dtype=rt.sample_dtype(fmt))
        frame[:, :I] = x[a:a + b]
        d = dm.to_device(frame)
        r.run_block_device(d.data_ptr(), O, IN, d.data_ptr(), O, 0, b, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same(dm.to_host(d), want, f"format {fmt}, {b} frames in place at {a}")
    same_state(r.sync_state(), o.state, f"format {fmt}, in place")


# ---- 4. special samples ---------------------------------------------------------------------------------------------------------------------
def test_inf_nan_and_subnormal_samples_in_the_last_frame():
    """format 6: the last frame of an 81-frame block writes the LOAD_MUX result words -- Inf, NaN and subnormals among its sums -- and
    the cascades behind the columns replay their blocks"""
    fmt = 6
    chains = mp.small_core()
    prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
    x = pb.lcg_input(81 + 40, nin, True, seed=21).copy()
    x[80] = [np.inf, np.nan, np.float32(1e-41), -np.inf, np.float32(-3e-39)]
    x[37, 0] = np.inf; x[50, 1] = np.nan; x[60:64, :] = np.float32(1e-41)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [chains])
    run_and_compare(r, o, x, nout, "Inf / NaN / subnormals", [81, 40])


@pytest.mark.parametrize("fmt", [2, 6])
def test_full_scale_inputs_under_a_finish_gain_of_1_1(fmt):
    chains = mp.small_core(gain=1.1)
    prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
    rng = np.random.default_rng(5)
    if fmt == 6:
        x = np.ascontiguousarray(rng.choice(np.array([1.0, -1.0, 0.999999, -0.999, 0.0, 0.5], dtype=np.float32), (300, nin)))
    else:
        x = rng.choice(np.array([0x7FFFFFFF, -0x80000000, 0x7FFFFF00, -0x7FFFFFFF, 0x7FFFFFFE, 0, 0x40000000], dtype=np.int64), (300, nin))
        x = np.ascontiguousarray(x.astype(np.int32))
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [chains])
    run_and_compare(r, o, x, nout, f"format {fmt}, full scale", [100, 200])


# ---- 5. shards: one group through mux_tile<., true> and through mux_plain<., true> ------------------------------------------------------------
@pytest.mark.parametrize("fmt", [4, 6])
def test_shard_1_of_3(fmt):
    """a core of a 47-chain group and a core of a 40-chain group: whole, both are mix groups of mux_tile; rank 1 of 3 runs 16 chains of
    the first (16 / 16 / 15: still a mix group) and 13 of the second (14 / 13 / 13: under the minimum, mux_plain).  Both are held to the
    same oracle, so the same group gives the same bits either way, and the rank touches no other chain's line or result word"""
    cores = mp.shard_cores()
    prog, nin, nout = mp.program(fmt, cores)
    blocks = [7, 65, 100]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=4)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [c["chains"] for c in cores])
    assert [r.mux_info(k)["grouped_chains"] for k in range(2)] == [47, 40]
    r.set_shard(1, 3)
    cols = []
    for k, (n, grouped) in enumerate([(16, 16), (13, 0)]):
        s = r.shard_info(k)
        mine = cores[k]["chains"][s["first_chain"]:s["first_chain"] + s["nchains"]]
        assert s["nchains"] == n and r.mux_info(k)["grouped_chains"] == grouped
        assert r.mux_tail_info(k) == mp.counts(mine)["mux_tail"] and mp.counts(mine)["mux_tail"][2] >= 6
        assert {"stage_finished", "stage_handed"} <= {mp.kind(c) for c in mine}
        cols += list(range(s["out_io_min"], s["out_io_max"] + 1))
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN)
        got = r.run_block(x[a:a + b], nout, IN)
        same(got[:, cols], want[:, cols], f"format {fmt}, shard 1 of 3, block {k}")
        st = r.sync_state()
        diff = st != o.state
        assert not st[diff].any(), "a state word that is neither the oracle's nor untouched (another rank's chain)"
        assert (st == o.state)[o.state != 0].sum() > 100
    r.set_shard(0, 1)


# ---- 6. live edits, reset -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_mux_gains_and_a_delay_word_edited_between_blocks(fmt):
    chains = mp.small_core()
    prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
    us = mp.us_words(prog)
    tables = [op + int(np.int32(prog[op + 1])) for op in mp.words_of(prog, mp.OP_LOAD_MUX)]
    assert len(us) == 5 and len(tables) == 22
    x = pb.lcg_input(5 * 70, nin, fmt == 6, seed=3)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [chains])
    rng = np.random.default_rng(6)
    for k, (a, b) in enumerate(cut([70] * 5)):
        if k:
            for t in (tables[0], tables[3], tables[8], tables[18]):               # a gain of a grouped list and of a private one
                g = np.float32(rng.uniform(-0.5, 0.5))
                word = (int(g.view(np.int32)) if fmt != 2 else round(float(g) * (1 << 28))) & 0xFFFFFFFF      # a float, or Q4.28
                o.buf[t + 2 + 2 * (k % 2)] = word
                r.buf[t + 2 + 2 * (k % 2)] = word
            for word, v in zip(us, [(300, 21, 0, 2100, 63), (60000, 0, 63, 21, 2100), (0, 0, 0, 0, 0), (2100, 63, 1000, 63, 21)][k - 1]):
                o.buf[word] = v
                r.buf[word] = v
            r.upload_params()
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, edit {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, edit {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_reset_to_44100_with_another_seed(fmt):
    chains = mp.small_core()
    prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
    x = pb.lcg_input(400, nin, fmt == 6, seed=8)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [chains])
    same(r.run_block(x[:100], nout, IN), o.run_block(x[:100], nout, IN), f"format {fmt}, 48000 Hz")
    assert o.reset(44100, 77, 24) == 0 and r.reset(44100, 77, 24) == 0
    assert r.mux_tail_info() == mp.counts(chains, 44100)["mux_tail"] and r.delay_info() == mp.counts(chains, 44100)["delay"]
    run_and_compare(r, o, x[100:], nout, f"format {fmt}, 44100 Hz", [100, 200])


# ---- 7. "fir_tail" beside it ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [4, 6])
def test_handed_fir_chains_behind_mux_heads(fmt):
    """LOAD_MUX -> [0 / 2 sections] -> FIR(7 / 255 taps) -> [DELAY] -> SAT0DB_TPDF_GAIN -> STORE, plain MUX+FIR chains beside them, and the
    stage's own kinds in the same core"""
    chains = mp.fir_tail_chains()
    prog, nin, nout = mp.program(fmt, [mp.core(chains, calc=0)])
    blocks = [1, 64, 333, 1029]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=41)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tailed_runtime(fmt, prog, [chains])
    assert r.fir_tail_info() == (6, 3) and r.core_info()["max_taps"] == 255 and r.mux_tail_info() == (8, 4, 2)
    run_and_compare(r, o, x, nout, f"format {fmt}, fir_tail beside mux_tail", blocks)

"""Delay lines on the chain kernels ("chain_delay" 1): one DSP_DELAY behind a chain's banks, on either side of the SAT0DB
slot -- the cascades' HAND forms and chain_tail.  Every case is held to the oracle bit for bit, outputs and the whole state area (the
lines and their index words among it) after each block, with the option on; the option off (the interpreter, as before) is the control
on the same inputs."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import delay_programs as dp

pytestmark = pytest.mark.gpu
IN = dp.IN
BLOCKS = [1, 7, 64, 100, 333, 1029]                  # in sequence: one frame, under a batch, a wave of frames, ragged, more than one launch
SECS = [17, 0, 1, 2, 16, 40]                         # two pieces, no cascade, short rows, a full row, three pieces
US = [63, 20, 1000, 21, 2100, 25000]                 # lines of 3 (many visits per launch), 0 (bypass), 47, 1, 100 and 1199 (longer than a launch) samples
SLOTS = ["A", "B", None, "B", "A"]
FIN = ["tpdf_gain", "tpdf", "gain", "sat", "none"]


@pytest.fixture(autouse=True)
def _options_back():
    yield
    rt.Runtime.set_global_option("chain_delay", 0)
    rt.Runtime.set_global_option("chain_finish", 0)
    rt.Runtime.set_global_option("biquad_impl", 1)
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


def mixed_chains(n, dressed=True):
    """sections, slots, forms, line lengths, finishes and store counts mixed in one core; every fifth chain has no delay, every third
    stores twice, every fourth loads without gain.  dressed False: plain SAT0DB or no finish only."""
    out = []
    for i in range(n):
        fin = FIN[(i + i // 5) % 5] if dressed else ("sat", "none")[(i + i // 5) % 2]
        us = US[(5 * i + i // 6) % 6]
        out.append(dp.chain(SECS[i % 6], SLOTS[i % 5], ("param", "fixed")[(i + i // 5) % 2], us=us, max_us=max(us, 50), finish=fin,
                            gain=0.9 + 0.01 * (i % 7), stores=2 if i % 3 == 1 else 1, load_gain=None if i % 4 == 3 else 0.4 + 0.01 * i))
    return out


def lines_of(chains, fs=48000):
    """(delayed chains, longest line) by the formula"""
    d = [dp.samples(c["us"], fs, c["max_us"] if c["form"] == "param" else None) for c in chains if c["slot"]]
    return (len(d), max(d, default=0))


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


_REF = {}


def reference(fmt, n, dither, dressed=True):
    """program, input, and the oracle's outputs and state after each block -- computed once, shared, never written"""
    key = (fmt, n, dither, dressed)
    if key not in _REF:
        chains = mixed_chains(n, dressed)
        prog, nin, nout = dp.program(fmt, [dp.core(chains, calc=0 if dressed else None)])
        x = pb.lcg_input(sum(BLOCKS), nin, fmt == 6, seed=11 + n)
        o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
        outs, states = [], []
        for a, b in cut(BLOCKS):
            outs.append(o.run_block(x[a:a + b], nout, IN))
            states.append(o.state.copy())
        for v in outs + states + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, nout, outs, states, chains)
    return _REF[key]


def delayed_runtime(fmt, prog, dither=24, finish=1, fs=48000):
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=dither)
    r.set_option("chain_finish", finish)
    r.set_option("chain_delay", 1)                            # (unknown to the code before this option existed: every test here fails there)
    return r


def run_and_compare(r, x, nout, outs, states, what, run="run_block"):
    for k, (a, b) in enumerate(cut(BLOCKS)):
        got = getattr(r, run)(x[a:a + b], nout, IN)
        same(got, outs[k], f"{what}, block {k} of {b} frames")
        same_state(r.sync_state(), states[k], f"{what}, after block {k}")


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("n", [1, 17, 37])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_delayed_core_matches_the_oracle(fmt, n, dither):
    prog, x, nout, outs, states, chains = reference(fmt, n, dither)
    r = delayed_runtime(fmt, prog, dither)
    assert r.core_info()["chains"] == n and r.delay_info() == lines_of(chains)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, {n} chains, dither {dither}, chain_delay 1")
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_plain_finishes_need_no_chain_finish(fmt):
    prog, x, nout, outs, states, chains = reference(fmt, 17, 24, dressed=False)
    r = delayed_runtime(fmt, prog, finish=0)
    assert r.get_option("chain_finish") == 0 and r.core_info()["chains"] == 17 and r.delay_info() == lines_of(chains)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, chain_finish 0, chain_delay 1")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with the option off -- no chain, the same bits"""
    prog, x, nout, outs, states, _ = reference(fmt, 17, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    assert r.get_option("chain_delay") == 0 and r.core_info()["chains"] == 0 and r.delay_info() == (0, 0)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, chain_delay 0")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_biquad_impl_0(fmt):
    """the cross-check path: biquad_simple_hand hands over what chain_tail takes"""
    prog, x, nout, outs, states, _ = reference(fmt, 17, 24)
    r = delayed_runtime(fmt, prog)
    r.set_option("biquad_impl", 0)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, biquad_impl 0")


def three_cores(fmt):
    """the crossover shape in several cores, the TPDF_CALC in the first only"""
    cores = [dp.core([dp.chain(5, "A", "fixed", 1000, finish="tpdf_gain", load_gain=0.7), dp.chain(3, "B", "param", 63, finish="tpdf", load_gain=0.7)], calc=0),
             dp.core([dp.chain(4, "A", "param", 2100, finish="tpdf"), dp.chain(0, "B", "fixed", 21, finish="tpdf_gain"), dp.chain(2, None, finish="tpdf_gain"),
                      dp.chain(0, "A", "fixed", 1000, finish="none", load_gain=None)]),
             dp.core([dp.chain(17, "B", "fixed", 2100, finish="sat", stores=2), dp.chain(1, "A", "param", 1000, finish="gain")])]
    return dp.program(fmt, cores)


@pytest.mark.parametrize("run", ["run_block_all", "run_block"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_three_cores(fmt, run):
    prog, nin, nout = three_cores(fmt)
    x = pb.lcg_input(64 + 300 + 1100, nin, fmt == 6, seed=33)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(fmt, prog)
    assert [r.delay_info(k) for k in range(3)] == [(2, 47), (3, 100), (2, 100)]
    assert [r.core_info(k)["chains"] for k in range(3)] == [2, 4, 2]
    for k, (a, b) in enumerate(cut([64, 300, 1100])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(getattr(r, run)(x[a:a + b], nout, IN), want, f"format {fmt}, {run}, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, {run}, block {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_shard_1_of_3(fmt):
    """this process runs chains 13 .. 24 of 37 and touches no other chain's line"""
    prog, x, nout, outs, states, chains = reference(fmt, 37, 24)
    r = delayed_runtime(fmt, prog)
    r.set_shard(1, 3)
    s = r.shard_info()
    assert (s["total_chains"], s["first_chain"], s["nchains"]) == (37, 13, 12)
    assert r.delay_info() == lines_of(chains[13:25])
    lo, hi = s["out_io_min"], s["out_io_max"] + 1
    for k, (a, b) in enumerate(cut(BLOCKS)):
        got = r.run_block(x[a:a + b], hi - lo, IN, lo)
        same(got, outs[k][:, lo:hi], f"format {fmt}, shard 1 of 3, block {k}")
        st = r.sync_state()
        diff = st != states[k]
        assert not st[diff].any(), "a state word that is neither the oracle's nor untouched (another rank's chain)"
        assert (st == states[k])[states[k] != 0].sum() > 100
    r.set_shard(0, 1)


def test_inf_and_nan_samples_take_the_replay():
    """a format-6 block with Inf and NaN samples: biquad_pipe's replay (cascade_in_reference_order) hands over too, and the line keeps
    the non-finite words"""
    fmt = 6
    chains = [dp.chain(s, sl, fo, us, finish=f, load_gain=lg) for s, sl, fo, us, f, lg in
              [(2, "A", "fixed", 63, "tpdf", None), (1, "B", "param", 1000, "tpdf_gain", 0.5), (16, "A", "param", 2100, "gain", None),
               (17, "B", "fixed", 63, "tpdf", 0.5), (0, "A", "fixed", 1000, "tpdf_gain", None), (3, "A", "fixed", 21, "sat", None), (2, None, "fixed", 0, "tpdf", None)]]
    prog, nin, nout = dp.program(fmt, [dp.core(chains, calc=0)])
    x = pb.lcg_input(400, nin, True, seed=21).copy()
    x[37, 0] = np.inf; x[150, 1] = -np.inf; x[151, 2] = np.nan; x[20, 3] = np.inf; x[399, 4] = np.nan; x[250, 5] = np.inf
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(fmt, prog)
    assert r.delay_info() == (6, 100)
    for k, (a, b) in enumerate(cut([100, 100, 200])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"Inf / NaN, block {k}")
        same_state(r.sync_state(), o.state, f"Inf / NaN, block {k}")


def test_full_scale_inputs_wrap_like_the_oracle_in_format_2():
    """the line holds the LOW 32 bits of the 64-bit accumulator: in slot A, in front of any saturation, full-scale sums wrap"""
    fmt = 2
    chains = [dp.chain(s, sl, fo, us, finish=f, gain=1.1, load_gain=lg) for s, sl, fo, us, f, lg in
              [(0, "A", "fixed", 63, "gain", None), (0, "A", "param", 1000, "tpdf_gain", 1.0), (1, "A", "fixed", 21, "sat", None), (2, "B", "fixed", 63, "tpdf_gain", 1.0),
               (0, "B", "param", 63, "sat", None), (17, "A", "fixed", 1000, "none", 1.0), (1, "A", "param", 2100, "tpdf", None)]]
    prog, nin, nout = dp.program(fmt, [dp.core(chains, calc=0)])
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([0x7FFFFFFF, -0x80000000, 0x7FFFFF00, -0x7FFFFFFF, 0x7FFFFFFE, 0, 0x40000000], dtype=np.int64), (300, nin))
    x = np.ascontiguousarray(x.astype(np.int32))
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(fmt, prog)
    assert r.delay_info() == (7, 100)
    for k, (a, b) in enumerate(cut([100, 200])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format 2, full scale, block {k}")
        same_state(r.sync_state(), o.state, f"format 2, full scale, block {k}")
    assert (want == 0x7FFFFFFF & (-1 << 8)).any() or (want == np.int32(-0x80000000)).any()      # (the clamps were reached)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_parameter_edits_between_blocks(fmt):
    """the microsecond word edited between blocks: shorter (the counter may stand beyond the new line: the `odd` start), longer than
    the line's size (clamped), zero (bypass: line and counter untouched), and back"""
    chains = [dp.chain(2, "A", "param", 2100, max_us=3000, finish="tpdf_gain"), dp.chain(0, "B", "param", 1000, max_us=1000, finish="sat"),
              dp.chain(17, "B", "param", 63, max_us=2100, finish="tpdf"), dp.chain(1, "A", "fixed", 1000, finish="none")]
    prog, nin, nout = dp.program(fmt, [dp.core(chains, calc=0)])
    w = dp.us_words(prog)
    assert len(w) == 3
    x = pb.lcg_input(7 * 90, nin, fmt == 6, seed=3)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(fmt, prog)
    edits = [None, (300, 21, 2100), (60000, 60000, 60000), (0, 0, 0), (2100, 1000, 63), (21, 300, 0), (1000, 0, 1000)]
    now = (2100, 1000, 63)
    for k, (a, b) in enumerate(cut([90] * 7)):
        if edits[k]:
            now = edits[k]
            for word, us in zip(w, now):
                o.buf[word] = us
                r.buf[word] = us
            r.upload_params()
        assert r.delay_info() == (4, max([dp.samples(1000)] + [dp.samples(us, max_us=m) for us, m in zip(now, (3000, 1000, 2100))]))
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, edit {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, edit {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_index_word_outside_the_line_reads_as_0(fmt):
    chains = [dp.chain(2, "A", "param", 1000, max_us=2100, finish="sat"), dp.chain(0, "B", "fixed", 2100, finish="sat"), dp.chain(1, "A", "fixed", 63, finish="none")]
    prog, nin, nout = dp.program(fmt, [dp.core(chains)])
    lw = dp.line_words(prog)
    x = pb.lcg_input(3 * 120, nin, fmt == 6, seed=9)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(fmt, prog, finish=0)
    pokes = [None, (5000, 100, 0x7FFFFFFF), (60, 99, 3)]     # outside each line's allocation; then: beyond the 47 asked for but inside the 100 laid out (`odd`), the last slot, one past the end
    for k, (a, b) in enumerate(cut([120] * 3)):
        if pokes[k]:
            r.sync_state()
            for word, v in zip(lw, pokes[k]):
                o.state[word] = v
                r.state[word] = v
            r.upload_state()
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, poke {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, poke {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_reset_to_44100(fmt):
    """another rate: other line lengths (the fixed forms and the parameter forms alike), coefficients of the other rate"""
    chains = mixed_chains(9)
    prog, nin, nout = dp.program(fmt, [dp.core(chains, calc=0)])
    x = pb.lcg_input(500, nin, fmt == 6, seed=8)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(fmt, prog)
    same(r.run_block(x[:200], nout, IN), o.run_block(x[:200], nout, IN), f"format {fmt}, 48000 Hz")
    assert o.reset(44100, 77, 24) == 0 and r.reset(44100, 77, 24) == 0
    assert r.delay_info() == lines_of(chains, 44100) and lines_of(chains, 44100) != lines_of(chains)
    for k, (a, b) in enumerate(cut([200, 300])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, 44100 Hz, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, 44100 Hz, block {k}")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_switched_between_blocks_of_one_stream(fmt):
    """the interpreter runs the first blocks, the chain kernels the next, the interpreter the last: lines, counters, generator and filter
    state go over through the mirror"""
    prog, x, nout, outs, states, _ = reference(fmt, 17, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    for k, (a, b) in enumerate(cut(BLOCKS)):
        if k == 2:
            r.set_option("chain_delay", 1)
            assert r.core_info()["chains"] == 17
        if k == 5:
            r.set_option("chain_delay", 0)
            assert r.core_info()["chains"] == 0
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, option switched, block {k}")
        same_state(r.sync_state(), states[k], f"format {fmt}, option switched, block {k}")


@pytest.mark.parametrize("impl", [1, 0])
def test_subnormal_samples_behind_a_plain_load_leave_signed_zeros_in_the_state(impl):
    """Format 6, found by tests/dev/gpu_lowered_sweep.py (seeds 2, 10 and 12): a sample loaded WITHOUT a gain reaches section 0 of
    biquad_pipe's WIDE and HAND forms (a dressed chain, a delayed chain) as its own bits -- the compiler folds (float)(double)sample --
    and a subnormal one went into the section's x words as it was, where the reference's cvtss2sd has read it as a signed zero.  The
    outputs never differed (the arithmetic widens and flushes); the state area did.  Blocks of 1, 2 and 3 frames end on subnormal
    samples of both signs, so x1 and x2 of section 0 hold them; biquad_impl 0 (the reference-order cascade, which has the same
    expression but kept the conversions) is the control."""
    chains = [dp.chain(1, "A", "fixed", 1000, finish="gain", load_gain=None), dp.chain(2, None, finish="tpdf", load_gain=None),
              dp.chain(16, "B", "param", 63, max_us=100, finish="sat", load_gain=None), dp.chain(1, "A", "fixed", 63, finish="none", load_gain=0.5)]
    prog, nin, nout = dp.program(6, [dp.core(chains, calc=0)])
    blocks = [1, 2, 3, 64, 1]
    x = pb.lcg_input(sum(blocks), nin, True, seed=4).copy()
    sub = np.array([0x00477B3C, 0x80000001, 0x007FFFFF, 0x80400000], dtype=np.uint32)
    for end in np.cumsum(blocks):
        x.view(np.uint32)[end - 1, :] = sub
        if end >= 2:
            x.view(np.uint32)[end - 2, :] = sub[::-1]
    o = po.OracleProgram(6, prog, fs=48000, random=1, dither=24)
    r = delayed_runtime(6, prog)
    r.set_option("biquad_impl", impl)
    assert r.core_info()["chains"] == 4 and r.delay_info()[0] == 3 and r.finish_info() == (2, 1)
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"biquad_impl {impl}, block {k}")
        same_state(r.sync_state(), o.state, f"biquad_impl {impl}, block {k}")

"""Dressed finishes on the chain kernels ("chain_finish" 1): SAT0DB_TPDF / SAT0DB_GAIN / SAT0DB_TPDF_GAIN in a chain's
SAT0DB slot and the TPDF_CALC at the head of the core -- dither_block, biquad_pipe's WIDE form, finish_stage.  Every case is held to
the oracle bit for bit, outputs and the state area after each block, with the option on; the option off (the interpreter, as before)
is the control on the same inputs."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import finish_programs as fp

pytestmark = pytest.mark.gpu
IN = fp.IN
BLOCKS = [1, 7, 64, 100, 333, 1029]                  # in sequence: one frame, under a batch, a wave of frames, ragged, more than one launch
SECS = [17, 0, 1, 2, 16, 40]                         # no cascade, short rows, a full row, two pieces, three pieces
FIN = ["tpdf_gain", "tpdf", "gain", "sat"]


@pytest.fixture(autouse=True)
def _option_back():
    yield
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


def mixed_chains(n, gain=0.9):
    """sections, finishes and store counts mixed in one core; every third chain stores twice, every fourth loads without gain"""
    return [fp.chain(SECS[i % len(SECS)], FIN[i % len(FIN)], gain=gain + 0.01 * (i % 7), stores=2 if i % 3 == 1 else 1,
                     load_gain=None if i % 4 == 3 else 0.4 + 0.01 * i) for i in range(n)]


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


_REF = {}


def reference(fmt, n, dither):
    """program, input, and the oracle's outputs and state after each block -- computed once, shared, never written"""
    key = (fmt, n, dither)
    if key not in _REF:
        prog, nin, nout = fp.program(fmt, [fp.core(mixed_chains(n), calc=0)])
        x = pb.lcg_input(sum(BLOCKS), nin, fmt == 6, seed=11 + n)
        o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
        outs, states = [], []
        for a, b in cut(BLOCKS):
            outs.append(o.run_block(x[a:a + b], nout, IN))
            states.append(o.state.copy())
        for v in outs + states + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, nout, outs, states)
    return _REF[key]


def run_and_compare(r, x, nout, outs, states, what, run="run_block"):
    for k, (a, b) in enumerate(cut(BLOCKS)):
        got = getattr(r, run)(x[a:a + b], nout, IN)
        same(got, outs[k], f"{what}, block {k} of {b} frames")
        same_state(r.sync_state(), states[k], f"{what}, after block {k}")


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("n", [1, 17, 37])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_dressed_core_matches_the_oracle(fmt, n, dither):
    prog, x, nout, outs, states = reference(fmt, n, dither)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=dither)
    r.set_option("chain_finish", 1)
    assert r.core_info()["chains"] == n and r.finish_info() == (sum(FIN[i % 4] != "sat" for i in range(n)), 1)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, {n} chains, dither {dither}, chain_finish 1")
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with the option off -- no chain, the same bits"""
    prog, x, nout, outs, states = reference(fmt, 17, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    assert r.get_option("chain_finish") == 0 and r.core_info()["chains"] == 0
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, chain_finish 0")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_biquad_impl_0(fmt):
    """the cross-check path: biquad_simple's WIDE form calls the same finish_stage"""
    prog, x, nout, outs, states = reference(fmt, 17, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    r.set_option("biquad_impl", 0)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, biquad_impl 0")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_block_all_entry_point(fmt):
    prog, x, nout, outs, states = reference(fmt, 17, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, dspRuntimeBlockAll", run="run_block_all")
    assert r.get_option("pieces") == 1 and r.get_option("strands") == 0


def full_scale(nframes, nch, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == 6:
        x = rng.choice(np.array([1.0, -1.0, 0.999999, -0.999999, 1.5, -2.0, 0.0, -0.0], dtype=np.float32), (nframes, nch))
        return np.ascontiguousarray(x, dtype=np.float32)
    x = rng.choice(np.array([0x7FFFFFFF, -0x80000000, 0x7FFFFF00, -0x7FFFFFFF, 0x7FFFFFFE, 0, 0x40000000], dtype=np.int64), (nframes, nch))
    return np.ascontiguousarray(x.astype(np.int32))


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_full_scale_inputs_saturate(fmt):
    chains = [fp.chain(s, f, gain=1.1, load_gain=lg) for s, f, lg in
              [(0, "gain", None), (0, "tpdf_gain", 1.0), (1, "gain", None), (2, "tpdf_gain", None), (0, "tpdf", None), (17, "tpdf_gain", 1.0), (1, "tpdf", None)]]
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    x = full_scale(300, nin, fmt, 5)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    assert r.finish_info() == (len(chains), 1)
    for k, (a, b) in enumerate(cut([100, 200])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, full scale, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, full scale, block {k}")
    if fmt != 6:                                              # the clamps were reached (format 6 stores +-1.0)
        assert (want == 0x7FFFFFFF & (-1 << 8)).any() or (want == np.int32(-0x80000000)).any()
    else:
        assert (want == 1.0).any() and (want == -1.0).any()


def test_inf_and_nan_samples_take_the_replay():
    """a format-6 block with Inf and NaN samples: biquad_pipe's replay (cascade_in_reference_order) finishes through finish_stage too"""
    fmt = 6
    chains = [fp.chain(s, f, load_gain=lg) for s, f, lg in
              [(2, "tpdf", None), (1, "tpdf_gain", 0.5), (16, "gain", None), (17, "tpdf", 0.5), (0, "tpdf_gain", None), (3, "sat", None), (2, "tpdf", None)]]
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    x = pb.lcg_input(400, nin, True, seed=21).copy()
    x[37, 0] = np.inf; x[150, 1] = -np.inf; x[151, 2] = np.nan; x[20, 3] = np.inf; x[399, 4] = np.nan; x[250, 5] = np.inf
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    for k, (a, b) in enumerate(cut([100, 100, 200])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"Inf / NaN, block {k}")
        same_state(r.sync_state(), o.state, f"Inf / NaN, block {k}")


def rew_program(fmt):
    """the reference's REWgenericEQ shape: pure per-channel chains in several cores, the TPDF_CALC in the first only -- the later cores
    dither with the value the first one's last frame left"""
    cores = [fp.core([fp.chain(5, "tpdf", load_gain=0.7), fp.chain(3, "tpdf", load_gain=0.7)], calc=0),
             fp.core([fp.chain(4, "tpdf", load_gain=0.6), fp.chain(0, "tpdf", load_gain=0.6), fp.chain(2, "tpdf_gain", load_gain=0.6)]),
             fp.core([fp.chain(17, "tpdf", load_gain=0.5), fp.chain(1, "gain", load_gain=0.5)])]
    return fp.program(fmt, cores)


@pytest.mark.parametrize("run", ["run_block_all", "run_block"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_rew_shape_three_cores(fmt, run):
    prog, nin, nout = rew_program(fmt)
    x = pb.lcg_input(64 + 300 + 1100, nin, fmt == 6, seed=33)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    assert [r.finish_info(k) for k in range(3)] == [(2, 1), (3, 0), (2, 0)]
    for k, (a, b) in enumerate(cut([64, 300, 1100])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(getattr(r, run)(x[a:a + b], nout, IN), want, f"format {fmt}, {run}, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, {run}, block {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_shard_1_of_3(fmt):
    """this process runs chains 13 .. 24 of 37; the TPDF_CALC runs on every rank (each has the whole generator)"""
    prog, x, nout, outs, states = reference(fmt, 37, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    r.set_shard(1, 3)
    s = r.shard_info()
    assert (s["total_chains"], s["first_chain"], s["nchains"]) == (37, 13, 12)
    assert r.finish_info() == (sum(FIN[i % 4] != "sat" for i in range(13, 25)), 1)
    lo, hi = s["out_io_min"], s["out_io_max"] + 1
    for k, (a, b) in enumerate(cut(BLOCKS)):
        got = r.run_block(x[a:a + b], hi - lo, IN, lo)
        same(got, outs[k][:, lo:hi], f"format {fmt}, shard 1 of 3, block {k}")
        st = r.sync_state()
        diff = st != states[k]
        assert not st[diff].any(), "a state word that is neither the oracle's nor untouched (another rank's chain)"
        assert (st == states[k])[states[k] != 0].sum() > 100
    r.set_shard(0, 1)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_switched_on_between_two_blocks(fmt):
    """one stream: the interpreter runs the first blocks, the chain kernels the rest -- generator, result word and filter state go over
    through the mirror"""
    prog, x, nout, outs, states = reference(fmt, 17, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    for k, (a, b) in enumerate(cut(BLOCKS)):
        if k == 3:
            r.set_option("chain_finish", 1)
            assert r.core_info()["chains"] == 17
        if k == 5:
            r.set_option("chain_finish", 0)
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, option switched, block {k}")
        same_state(r.sync_state(), states[k], f"format {fmt}, option switched, block {k}")


@pytest.mark.parametrize("fmt", [2, 6])
def test_reset_with_another_seed(fmt):
    prog, nin, nout = fp.program(fmt, [fp.core(mixed_chains(9), calc=0)])
    x = pb.lcg_input(500, nin, fmt == 6, seed=8)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    first = o.run_block(x[:200], nout, IN)
    same(r.run_block(x[:200], nout, IN), first, f"format {fmt}, seed 1")
    assert o.reset(48000, 77, 20) == 0 and r.reset(48000, 77, 20) == 0
    wants = []
    for k, (a, b) in enumerate(cut([200, 300])):
        wants.append(o.run_block(x[a:a + b], nout, IN))
        same(r.run_block(x[a:a + b], nout, IN), wants[k], f"format {fmt}, seed 77, dither 20, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, seed 77, block {k}")
    assert not (words(wants[0]) == words(first)).all()        # (the same 200 frames under the other seed and width)

"""Handed FIR chains ("fir_tail" 1): a DSP_DELAY and / or a dressed finish BEHIND a chain's DSP_FIR -- fir_tile's and
fir_plain's HAND forms fill the hand-over block, chain_tail goes on from it.  Every case first asserts through dspRuntimeFirTailInfo
that its chains are handed (the interpreter would give the same bits: parity alone proves nothing), then is held to the oracle bit for
bit, outputs and the whole state area (FIR histories, lines and their index words among it) after each block."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import firtail_programs as fp

pytestmark = pytest.mark.gpu
IN = fp.IN
BLOCKS = [1, 7, 64, 100, 333, 1029]                  # in sequence at 48 kHz; the last one is two launches
FORM_BLOCKS = [300, 600, 64]                         # two row tiles per wave need more than 256 frames, four more than 512
SECS = [2, 0, 16, 17]                                # a short row, no cascade, a full row, two pieces
TAPS = [255, 7, 700, 1500]                           # ..., under one group of k-steps, across a chunk of the ordinary forms, across a BIG chunk
US = [1000, 20, 21, 25000]                           # lines of 47, 0 (bypass), 1 and 1199 (longer than a launch) samples
SLOTS = ["A", "B", None, "B", "A"]
FIN = ["tpdf_gain", "tpdf", "gain", "sat", "none"]


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key, v in (("fir_tail", 0), ("chain_delay", 0), ("chain_finish", 0), ("fir_impl", 1), ("fir_rows", 0), ("fir_lean", -1), ("fir_split", 0), ("overlap", 0)):
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


def mixed_chains(n):
    """sections, taps, slots, forms, line lengths, finishes and store counts mixed in one core.  Chains without a delay and with a plain
    finish or none are plain FIR chains beside the handed ones; every ninth chain has no FIR (a dressed or delayed cascade chain);
    every third stores twice, every fourth loads without gain."""
    out = []
    for i in range(n):
        us = US[(i + i // 4) % 4]
        out.append(fp.chain(SECS[i % 4], 0 if i % 9 == 8 else TAPS[(i + i // 4) % 4], SLOTS[i % 5], ("fixed", "param")[(i // 3) % 2], us=us, max_us=max(us, 50),
                            finish=FIN[(i + i // 5) % 5], gain=0.9 + 0.01 * (i % 7), stores=2 if i % 3 == 1 else 1, load_gain=None if i % 4 == 3 else 0.4 + 0.01 * i))
    return out


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


_REF = {}


def reference(fmt, n, dither=24, blocks=BLOCKS):
    """program, input, and the oracle's outputs and state after each block -- computed once, shared, never written"""
    key = (fmt, n, dither, tuple(blocks))
    if key not in _REF:
        chains = mixed_chains(n)
        prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
        x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=11 + n)
        o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
        outs, states = [], []
        for a, b in cut(blocks):
            outs.append(o.run_block(x[a:a + b], nout, IN))
            states.append(o.state.copy())
        for v in outs + states + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, nout, outs, states, chains)
    return _REF[key]


def handed_runtime(fmt, prog, chains=None, dither=24, fs=48000, core_index=0):
    """the three options on; the core's chains must be handed as `chains` says (on the code before "fir_tail" the option and
    dspRuntimeFirTailInfo do not exist: every test here fails there)"""
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=dither)
    r.set_option("chain_finish", 1)
    r.set_option("chain_delay", 1)
    r.set_option("fir_tail", 1)
    if chains is not None:
        assert r.core_info(core_index)["chains"] == len(chains), r.last_error()
        assert r.fir_tail_info(core_index) == fp.handed(chains) and fp.handed(chains)[0] > 0
    return r


def run_and_compare(r, x, nout, outs, states, what, blocks=BLOCKS, run="run_block"):
    for k, (a, b) in enumerate(cut(blocks)):
        got = getattr(r, run)(x[a:a + b], nout, IN)
        same(got, outs[k], f"{what}, block {k} of {b} frames")
        same_state(r.sync_state(), states[k], f"{what}, after block {k}")


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("n", [1, 5, 37])
@pytest.mark.parametrize("fmt", [4, 6])
def test_handed_core_matches_the_oracle(fmt, n, dither):
    prog, x, nout, outs, states, chains = reference(fmt, n, dither)
    r = handed_runtime(fmt, prog, chains, dither)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, {n} chains, dither {dither}, fir_tail 1")
    r.release()


FORMS = {"rows_1": [("fir_rows", 1)], "rows_2": [("fir_rows", 2)], "rows_4": [("fir_rows", 4)], "lean_0": [("fir_lean", 0)], "lean_1": [("fir_lean", 1)],
         "fir_impl_0": [("fir_impl", 0)], "fir_split_1": [("fir_split", 1)], "overlap_1": [("overlap", 1)]}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("fmt", [4, 6])
def test_kernel_forms(fmt, form):
    """one, two and four row tiles per wave (blocks of 300 and 600 frames keep two and four), the cross-check FIR, and the options a
    handed launch does not follow -- the lean boundary is fixed, "fir_split" and "overlap" give the unsplit, back-to-back path"""
    prog, x, nout, outs, states, chains = reference(fmt, 5, 24, FORM_BLOCKS)
    r = handed_runtime(fmt, prog, chains)
    for key, v in FORMS[form]:
        r.set_option(key, v)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, {form}", FORM_BLOCKS)


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with "fir_tail" 0 -- no chain, the same bits"""
    prog, x, nout, outs, states, _ = reference(fmt, 5, 24, FORM_BLOCKS)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    r.set_option("chain_delay", 1)
    assert r.get_option("fir_tail") == 0 and r.core_info()["chains"] == 0 and r.fir_tail_info() == (0, 0)
    run_and_compare(r, x, nout, outs, states, f"format {fmt}, fir_tail 0", FORM_BLOCKS)


def test_inf_nan_and_subnormal_samples():
    """format 6: Inf and NaN reach the FIR's sums (the lean form sums such a tile again the reference's way) and the lines; subnormal
    samples are flushed on the way into the ring"""
    fmt = 6
    chains = [fp.chain(s, t, sl, fo, us, finish=f, load_gain=lg) for s, t, sl, fo, us, f, lg in
              [(2, 255, "A", "fixed", 1000, "tpdf", None), (0, 7, "B", "param", 1000, "tpdf_gain", 0.5), (16, 700, "A", "param", 21, "gain", None),
               (17, 64, "B", "fixed", 63, "tpdf", 0.5), (0, 300, None, "fixed", 0, "tpdf_gain", None), (1, 40, "A", "fixed", 21, "sat", None), (2, 33, None, "fixed", 0, "sat", None)]]
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    x = pb.lcg_input(400, nin, True, seed=21).copy()
    x[37, 0] = np.inf; x[150, 1] = -np.inf; x[151, 2] = np.nan; x[20, 3] = np.inf; x[399, 4] = np.nan; x[250, 5] = np.inf; x[30, 6] = np.nan
    x[60:70, :] = np.float32(1e-41)
    x[71, :] = np.float32(-1e-40)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = handed_runtime(fmt, prog, chains)
    assert r.fir_tail_info() == (6, 5)
    for k, (a, b) in enumerate(cut([100, 100, 200])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"Inf / NaN / subnormals, block {k}")
        same_state(r.sync_state(), o.state, f"Inf / NaN / subnormals, block {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_full_scale_inputs_under_a_gain_of_1_1(fmt):
    chains = [fp.chain(s, t, sl, fo, us, finish=f, gain=1.1, load_gain=lg) for s, t, sl, fo, us, f, lg in
              [(0, 7, "A", "fixed", 63, "gain", None), (0, 255, "A", "param", 1000, "tpdf_gain", 1.0), (1, 64, "A", "fixed", 21, "sat", None), (2, 33, "B", "fixed", 63, "tpdf_gain", 1.0),
               (0, 16, "B", "param", 63, "sat", None), (17, 100, None, "fixed", 0, "gain", 1.0), (1, 700, "A", "param", 2100, "tpdf", None)]]
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    rng = np.random.default_rng(5)
    if fmt == 6:
        x = np.ascontiguousarray(rng.choice(np.array([1.0, -1.0, 0.999999, -0.999, 0.0, 0.5], dtype=np.float32), (300, nin)))
    else:
        x = rng.choice(np.array([0x7FFFFFFF, -0x80000000, 0x7FFFFF00, -0x7FFFFFFF, 0x7FFFFFFE, 0, 0x40000000], dtype=np.int64), (300, nin))
        x = np.ascontiguousarray(x.astype(np.int32))
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = handed_runtime(fmt, prog, chains)
    for k, (a, b) in enumerate(cut([100, 200])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, full scale, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, full scale, block {k}")


def three_cores(fmt):
    """handed chains in several cores, the TPDF_CALC in the first only"""
    cores = [fp.core([fp.chain(5, 255, "A", "fixed", 1000, finish="tpdf_gain", load_gain=0.7), fp.chain(3, 7, "B", "param", 63, finish="tpdf", load_gain=0.7)], calc=0),
             fp.core([fp.chain(4, 700, "A", "param", 2100, finish="tpdf"), fp.chain(0, 64, "B", "fixed", 21, finish="tpdf_gain"), fp.chain(2, 33, None, finish="tpdf_gain"),
                      fp.chain(0, 16, None, finish="none", load_gain=None), fp.chain(2, 0, "A", "fixed", 1000, finish="tpdf")]),
             fp.core([fp.chain(17, 100, "B", "fixed", 2100, finish="sat", stores=2), fp.chain(1, 1500, "A", "param", 1000, finish="gain")])]
    return fp.program(fmt, cores), cores


@pytest.mark.parametrize("run", ["run_block_all", "run_block"])
@pytest.mark.parametrize("fmt", [4, 6])
def test_three_cores(fmt, run):
    (prog, nin, nout), cores = three_cores(fmt)
    x = pb.lcg_input(64 + 300 + 1100, nin, fmt == 6, seed=33)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = handed_runtime(fmt, prog)
    assert [r.fir_tail_info(k) for k in range(3)] == [(2, 2), (3, 2), (2, 2)] == [fp.handed(c["chains"]) for c in cores]
    assert [r.core_info(k)["chains"] for k in range(3)] == [2, 5, 2]
    for k, (a, b) in enumerate(cut([64, 300, 1100])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(getattr(r, run)(x[a:a + b], nout, IN), want, f"format {fmt}, {run}, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, {run}, block {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_shard_1_of_3(fmt):
    """this process runs chains 13 .. 24 of 37 and touches no other chain's history or line"""
    prog, x, nout, outs, states, chains = reference(fmt, 37, 24)
    r = handed_runtime(fmt, prog)
    r.set_shard(1, 3)
    s = r.shard_info()
    assert (s["total_chains"], s["first_chain"], s["nchains"]) == (37, 13, 12)
    assert r.fir_tail_info() == fp.handed(chains[13:25]) and fp.handed(chains[13:25])[0] >= 6
    lo, hi = s["out_io_min"], s["out_io_max"] + 1
    for k, (a, b) in enumerate(cut(BLOCKS)):
        got = r.run_block(x[a:a + b], hi - lo, IN, lo)
        same(got, outs[k][:, lo:hi], f"format {fmt}, shard 1 of 3, block {k}")
        st = r.sync_state()
        diff = st != states[k]
        assert not st[diff].any(), "a state word that is neither the oracle's nor untouched (another rank's chain)"
        assert (st == states[k])[states[k] != 0].sum() > 100
    r.set_shard(0, 1)


@pytest.mark.parametrize("fmt", [4, 6])
def test_reset_to_44100_with_another_seed(fmt):
    """another rate: the other impulse of every FIR (another length), other line lengths, other coefficients"""
    chains = mixed_chains(9)
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    x = pb.lcg_input(500, nin, fmt == 6, seed=8)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = handed_runtime(fmt, prog, chains)
    same(r.run_block(x[:200], nout, IN), o.run_block(x[:200], nout, IN), f"format {fmt}, 48000 Hz")
    assert o.reset(44100, 77, 24) == 0 and r.reset(44100, 77, 24) == 0
    assert r.fir_tail_info() == fp.handed(chains) and r.core_info()["max_taps"] == 1000
    for k, (a, b) in enumerate(cut([200, 300])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, 44100 Hz, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, 44100 Hz, block {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_parameter_edits_between_blocks(fmt):
    """the microsecond word edited between blocks through dspRuntimeUploadParams: shorter, longer than the line's size (clamped), zero
    (bypass), and back -- no new plan, the FIR histories stay in their rings"""
    chains = [fp.chain(2, 255, "A", "param", 2100, max_us=3000, finish="tpdf_gain"), fp.chain(0, 7, "B", "param", 1000, max_us=1000, finish="sat"),
              fp.chain(17, 700, "B", "param", 63, max_us=2100, finish="tpdf"), fp.chain(1, 64, "A", "fixed", 1000, finish="none")]
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    w = fp.us_words(prog)
    assert len(w) == 3
    x = pb.lcg_input(7 * 90, nin, fmt == 6, seed=3)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = handed_runtime(fmt, prog, chains)
    edits = [None, (300, 21, 2100), (60000, 60000, 60000), (0, 0, 0), (2100, 1000, 63), (21, 300, 0), (1000, 0, 1000)]
    for k, (a, b) in enumerate(cut([90] * 7)):
        if edits[k]:
            for word, us in zip(w, edits[k]):
                o.buf[word] = us
                r.buf[word] = us
            r.upload_params()
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, edit {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, edit {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_switched_off_and_on_inside_one_stream(fmt):
    """the interpreter runs the first blocks, the chain kernels the next, the interpreter again, the chain kernels the last: FIR
    histories (ring <-> the reference's delay-line layout), lines, counters and generator go over through the mirror both ways"""
    prog, x, nout, outs, states, chains = reference(fmt, 5, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    r.set_option("chain_delay", 1)
    for k, (a, b) in enumerate(cut(BLOCKS)):
        if k in (1, 4):
            r.set_option("fir_tail", 1)
            assert r.core_info()["chains"] == 5 and r.fir_tail_info() == fp.handed(chains)
        if k == 3:
            r.set_option("fir_tail", 0)
            assert r.core_info()["chains"] == 0 and r.fir_tail_info() == (0, 0)
        same(r.run_block(x[a:a + b], nout, IN), outs[k], f"format {fmt}, option switched, block {k}")
        same_state(r.sync_state(), states[k], f"format {fmt}, option switched, block {k}")


@pytest.mark.parametrize("n, grouped", [(17, 0), (20, 18)])
@pytest.mark.parametrize("fmt", [4, 6])
def test_a_bank_with_two_handed_chains(fmt, n, grouped):
    """n chains on one impulse bank, two of them handed: the host's grouping skips those two -- 15 are fewer than a group needs and all
    go to fir_tile, 18 are a group of fir_shared beside the two on the HAND form"""
    chains = [fp.chain(2 if i % 2 else 0, 100, None, finish="sat", bank=1, load_gain=0.3 + 0.01 * i) for i in range(n)]
    chains[3] = fp.chain(2, 100, "A", "fixed", 1000, finish="tpdf_gain", bank=1)
    chains[11] = fp.chain(0, 100, None, finish="tpdf", bank=1)
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    x = pb.lcg_input(64 + 300, nin, fmt == 6, seed=14)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = handed_runtime(fmt, prog, chains)
    assert r.fir_tail_info() == (2, 1)
    assert r.fir_group_info() == dict(groups=1 if grouped else 0, grouped_chains=grouped, largest_group=grouped)
    for k, (a, b) in enumerate(cut([64, 300])):
        want = o.run_block(x[a:a + b], nout, IN)
        same(r.run_block(x[a:a + b], nout, IN), want, f"format {fmt}, bank of {n}, block {k}")
        same_state(r.sync_state(), o.state, f"format {fmt}, bank of {n}, block {k}")
        assert r.get_option("fir_shared_chains") == grouped

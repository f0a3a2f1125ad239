"""LOAD_STORE lists beside the chain kernels ("chain_copy" 1): copy_pairs once per block call, the chains as ever.
Every case first proves through core_info / copy_info that the core is on the chain kernels, and is then held to the oracle bit for bit
after each block -- the whole output block (its untouched columns keep a sentinel), the whole state area and the program words behind
the header -- with the option on; the option off (the interpreter, as before) is the control on the same inputs."""
import os

import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import copy_programs as cp

pytestmark = pytest.mark.gpu
IN = cp.IN
BLOCKS = [1, 7, 64, 333, 1029]                       # in sequence: one frame, under a wave, a wave, ragged, more than one cascade launch
HEAD = 12                                            # program words of the header (its checksum covers them alone)
OPTIONS = ("chain_copy", "chain_mem", "chain_finish", "chain_delay")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    g, w = words(got), words(want)
    bad = np.nonzero((g != w).any(axis=0))[0]
    assert bad.size == 0, (f"{what}: columns {bad[:8].tolist()} differ, first frame "
                           f"{np.nonzero(g[:, bad[0]] != w[:, bad[0]])[0][:3].tolist()}: "
                           f"{g[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()} for {w[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()}")


def same_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:6].tolist()}"


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def pair_list(n):
    """n pairs: a run of consecutive sources to consecutive destinations (from IO IN + 40 to IO 100), then scattered ones (sources may
    repeat); from 5 pairs on the last three are a forwarded pair (it reads the first pair's destination) and two writers of one IO"""
    run = (n + 1) // 2
    pairs = [(IN + 40 + k, 100 + k) for k in range(run)]
    pairs += [(IN + 40 + (k * 37) % 401, 100 + run + (k * 29) % 257) for k in range(n - run)]
    if n >= 5:
        pairs[-3:] = [(100, 98), (IN + 41, 99), (IN + 42, 99)]
    return pairs


def sentinel(fmt, shape):
    out = np.empty(shape, dtype=rt.sample_dtype(fmt))
    out.view(np.uint32)[...] = 0x7FC0BEEF if fmt in (5, 6) else 0x5A5A1234
    return out


def beside(n, tree=True):
    """a head list of n pairs in front of the TPDF_CALC; a plain, a dressed and a delayed chain, a tree, a long cascade with two
    stores; a list between chains, one behind the trunk, one at the end"""
    items = [cp.plain(nsec=2, finish="sat"), cp.copies([(IN + 30, 90), (IN, 93)]), cp.plain(nsec=0, finish="tpdf_gain", load_gain=None),
             cp.plain(nsec=1, slot="A", us=1000, finish="sat")]
    if tree:
        items += [cp.trunk("a", 2), cp.copies([(IN + 31, 91)]), cp.branch("a", nsec=1, finish="tpdf"), cp.branch("a", nsec=0, finish="none")]
    items += [cp.plain(nsec=17, finish="gain", stores=2), cp.copies([(IN + 32, 92), (92, 94)])]
    return cp.core(items, calc=0, head=[cp.copies(pair_list(n))])


_REF = {}


def reference(fmt, cores, tag, blocks=BLOCKS, dither=24, seed=11):
    """program, input, windows, and the oracle's output blocks (from a block of sentinels), state and program words after each block --
    computed once, shared, never written"""
    key = (fmt, tag)
    if key not in _REF:
        prog, nin, nout = cp.program(fmt, cores)
        in_stride, out_stride = cp.windows(cores, nin, nout)
        x = pb.lcg_input(sum(blocks), in_stride, fmt in (5, 6), seed=seed)
        o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
        total = int(prog[1])
        outs, states, progs = [], [], []
        for a, b in cut(blocks):
            outs.append(o.run_block(x[a:a + b], out_stride, IN, out=sentinel(fmt, (b, out_stride))))
            states.append(o.state.copy())
            progs.append(o.buf[HEAD:total].copy())
        for v in outs + states + progs + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, out_stride, outs, states, progs)
    return _REF[key]


def runtime(fmt, prog, on=OPTIONS, dither=24):
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=dither)
    for key in on:
        r.set_option(key, 1)                                  # ("chain_copy" is unknown to the code before the option existed: every test here fails there)
    return r


def run_and_compare(r, fmt, x, out_stride, outs, states, progs, what, run="run_block", blocks=BLOCKS):
    for k, (a, b) in enumerate(cut(blocks)):
        got = getattr(r, run)(x[a:a + b], out_stride, IN, out=sentinel(fmt, (b, out_stride)))
        w = f"{what}, block {k} of {b} frames"
        same(got, outs[k], w)
        same_words(r.sync_state(), states[k], w + ", state area")
        same_words(r.buf[HEAD:HEAD + len(progs[k])], progs[k], w + ", program words")


@pytest.mark.parametrize("n", [1, 5, 64, 65, 300])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_lists_beside_chains_match_the_oracle(fmt, n):
    core = beside(n)
    prog, x, out_stride, outs, states, progs = reference(fmt, [core], ("beside", n))
    r = runtime(fmt, prog)
    live = len(cp.resolve(cp.all_pairs(core)))
    assert live == (n if n < 5 else n - 1) + 5
    assert r.core_info()["chains"] == 7 and r.copy_info() == (n + 5, live) and r.mem_info() == (1, 2, 0), r.last_error()
    assert (outs[-1].view(np.uint32) == sentinel(fmt, (1, 1)).view(np.uint32)[0, 0]).all(axis=0).sum() > 0      # some columns are nobody's
    run_and_compare(r, fmt, x, out_stride, outs, states, progs, f"format {fmt}, {n} pairs")
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with the option off -- no chain, the same bits"""
    prog, x, out_stride, outs, states, progs = reference(fmt, [beside(65)], ("beside", 65))
    r = runtime(fmt, prog, on=OPTIONS[1:])
    assert r.get_option("chain_copy") == 0 and r.core_info()["chains"] == 0 and r.copy_info() == (0, 0)
    run_and_compare(r, fmt, x, out_stride, outs, states, progs, f"format {fmt}, chain_copy 0")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_list_needs_no_other_option(fmt):
    core = cp.core([cp.copies(pair_list(5)), cp.plain(nsec=2, finish="sat"), cp.plain(nsec=0, finish="none", load_gain=None), cp.copies([(IN + 9, 95)])])
    prog, x, out_stride, outs, states, progs = reference(fmt, [core], "alone_option")
    r = runtime(fmt, prog, on=("chain_copy",))
    assert r.core_info()["chains"] == 2 and r.copy_info() == (6, 5), r.last_error()
    run_and_compare(r, fmt, x, out_stride, outs, states, progs, f"format {fmt}, chain_copy alone")


@pytest.mark.parametrize("run", ["run_block", "run_block_all"])
@pytest.mark.parametrize("fmt", [2, 3, 4, 5, 6])
def test_a_core_of_pairs_alone(fmt, run):
    """no chain in the core: copy_pairs is the plan's one launch; a second core of chains beside it"""
    cores = [cp.core([cp.copies(pair_list(65))]), cp.core([cp.plain(nsec=2, finish="sat"), cp.plain(nsec=0, finish="sat")])]
    prog, x, out_stride, outs, states, progs = reference(fmt, cores, "pairs_alone")
    r = runtime(fmt, prog, on=("chain_copy",))
    assert [r.core_info(k)["chains"] for k in range(2)] == [0, 2] and [r.copy_info(k) for k in range(2)] == [(65, 64), (0, 0)], r.last_error()
    assert r.shard_info(0)["total_chains"] == 0 and r.shard_info(0)["out_io_max"] == 100 + 33 + max((k * 29) % 257 for k in range(29))
    run_and_compare(r, fmt, x, out_stride, outs, states, progs, f"format {fmt}, pairs alone, {run}", run=run)


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("geometry", ["same", "shifted"])
@pytest.mark.parametrize("fmt", [2, 6])
def test_in_place_calls(fmt, geometry, tree):
    """one [frames][io] block in device memory as both windows.  "same": both windows are the whole block, IO = column.  "shifted":
    the input window starts at IO IN, the output window at IO 0, over the same words -- input IO IN + j lies where output j goes, and a
    pair's destination column may be another pair's source column: copy_pairs reads the copy the call sets aside"""
    import torch
    core = beside(65, tree)
    prog, nin, nout = cp.program(fmt, [core])
    in_stride, out_stride = cp.windows([core], nin, nout)
    W = IN + in_stride if geometry == "same" else max(in_stride, out_stride)
    in_base = 0 if geometry == "same" else IN
    col = IN if geometry == "same" else 0
    blocks = [1, 7, 333, 1029]
    x = pb.lcg_input(sum(blocks), in_stride, fmt == 6, seed=23)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = runtime(fmt, prog)
    assert r.core_info()["chains"] == (7 if tree else 4) and r.copy_info()[1] == 64 + (5 if tree else 4), r.last_error()
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        frame = sentinel(fmt, (b, W))
        frame[:, col:col + in_stride] = x[a:a + b]
        want = frame.copy()
        o.run_block(want, W, in_base, 0, out=want)
        d = dm.to_device(frame)
        r.run_block_device(d.data_ptr(), W, in_base, d.data_ptr(), W, 0, b, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        w = f"format {fmt}, {geometry} windows in place, block {k} of {b} frames"
        same(dm.to_host(d), want, w)
        same_words(r.sync_state(), o.state, w + ", state area")
        same_words(r.buf[HEAD:total], o.buf[HEAD:total], w + ", program words")


@pytest.mark.parametrize("fmt", [4, 6])
def test_a_fir_core_with_a_head_list_under_default_options(fmt):
    """4 chains x 64 taps behind two sections each, a head list: every option at its default but "chain_copy" -- the cascades run
    under the previous block's FIR ("overlap"), the copy goes with the caller's stream -- over three consecutive blocks"""
    core = cp.core([cp.copies(pair_list(5))] + [cp.plain(nsec=2, finish="sat", fir=64) for _ in range(4)])
    blocks = [1024, 1024, 300]
    prog, x, out_stride, outs, states, progs = reference(fmt, [core], "fir", blocks=blocks)
    r = runtime(fmt, prog, on=("chain_copy",))
    assert r.core_info() == dict(chains=4, max_sections=2, max_taps=64) and r.copy_info() == (5, 4), r.last_error()
    for k, (a, b) in enumerate(cut(blocks)):
        got = r.run_block(x[a:a + b], out_stride, IN, out=sentinel(fmt, (b, out_stride)))
        same(got, outs[k], f"format {fmt}, FIR core, block {k}")
    same_words(r.sync_state(), states[-1], f"format {fmt}, FIR core, state area")


def test_dacdiy1_through_run_block_all(fmt=2):
    """tests/golden/dacdiy1.bin (dspProg_3ways_LR4 of oktodac_diy.c) in its own format, 2, with the goldens' own windows -- input stride 16 from IO 8, output
    stride 32 from IO 0, which share IO numbers -- in blocks of 64, the four options on: core 1 (list, TPDF_CALC, two trunks) on the chain
    kernels, all 32 columns against the oracle"""
    prog = np.fromfile(os.path.join(GOLDEN, "dacdiy1.bin"), dtype=np.uint32)
    x = pb.lcg_input(4 * 64, 16, fmt == 6, seed=3)
    o = po.OracleProgram(fmt, prog.copy(), fs=48000, random=1, dither=24)
    r = runtime(fmt, prog.copy())
    assert r.core_info(0)["chains"] == 2 and r.copy_info(0) == (5, 4) and r.mem_info(0) == (2, 0, 0), r.last_error()
    assert [r.core_info(k)["chains"] for k in (1, 2, 3)] == [2, 2, 2], r.last_error()      # (the fourth core: both chains store IOs 30 and 6)
    total = int(prog[1])
    for k in range(4):
        xb = x[64 * k:64 * (k + 1)]
        want = o.run_block(xb, 32, 8, 0, out=sentinel(fmt, (64, 32)))
        got = r.run_block_all(xb, 32, 8, 0, out=sentinel(fmt, (64, 32)))
        same(got, want, f"dacdiy1.bin, format {fmt}, block {k}")
        same_words(r.sync_state(), o.state, f"dacdiy1.bin, format {fmt}, block {k}, state area")
        same_words(r.buf[HEAD:total], o.buf[HEAD:total], f"dacdiy1.bin, format {fmt}, block {k}, program words")


@pytest.mark.parametrize("fmt", [3, 6])
def test_one_launch_per_block_call(fmt):
    """the copy kernel, not the interpreter: copy_pairs' timer (the pass kernels' kind) counts one span for a call of 1029 frames --
    more than one cascade launch -- of a core of 65 pairs alone, and nothing else runs; with the option off it counts none"""
    cores = [cp.core([cp.copies(pair_list(65))])]
    prog, x, out_stride, outs, _, _ = reference(fmt, cores, "one_launch", blocks=[1029])
    r = runtime(fmt, prog, on=("chain_copy",))
    assert r.copy_info() == (65, 64)
    r.set_option("profile", 1)
    try:
        kinds = range(8)
        for k in kinds:
            r.kernel_time(k)
        same(r.run_block(x, out_stride, IN, out=sentinel(fmt, (1029, out_stride))), outs[0], f"format {fmt}, one call")
        assert [r.kernel_time(k)[1] for k in kinds] == [0, 0, 1, 0, 0, 0, 0, 0]
        r.set_option("chain_copy", 0)
        for k in kinds:
            r.kernel_time(k)
        same(r.run_block(x, out_stride, IN, out=sentinel(fmt, (1029, out_stride))), outs[0], f"format {fmt}, one call, chain_copy 0")
        assert r.kernel_time(2)[1] == 0
    finally:
        r.set_option("profile", 0)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_last_chain_to_store_an_io_wins(fmt):
    """chains of one core that store the same IOs (oktodac_diy's fourth core): the later chain's words arrive, the earlier chain -- left
    without a STORE, or with the one nobody repeats -- still runs its banks and its line; ordinary, delayed and tree chains"""
    def d(nsec, slot, us, finish, ios, **kw):
        return cp.stores_to(cp.plain(nsec=nsec, slot=slot, us=us, finish=finish, **kw), ios)
    a = cp.stores_to(cp.branch("a", nsec=0, slot="B", us=63, finish="sat"), [9])
    b = cp.stores_to(cp.branch("a", nsec=1, slot="A", us=1000, finish="tpdf"), [9, 10])
    items = [d(2, "A", 1000, "tpdf_gain", [7, 8]), d(1, "B", 63, "sat", [7, 8]), d(1, None, 0, "sat", [3, 4]), d(17, None, 0, "gain", [4, 5]),
             cp.trunk("a", 2), a, d(0, "A", 2100, "none", [6, 6], load_gain=None), b, d(0, None, 0, "sat", [2, 1, 2])]
    prog, nin, _ = cp.program(fmt, [cp.core(items, calc=0, head=[cp.copies([(IN + 20, 0)])])])
    in_stride, out_stride = 21, 12
    x = pb.lcg_input(sum(BLOCKS), in_stride, fmt == 6, seed=29)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = runtime(fmt, prog)
    assert r.core_info()["chains"] == 9 and r.copy_info() == (1, 1) and r.delay_info()[0] == 5, r.last_error()
    total = int(prog[1])
    for k, (lo, n) in enumerate(cut(BLOCKS)):
        want = o.run_block(x[lo:lo + n], out_stride, IN, out=sentinel(fmt, (n, out_stride)))
        got = r.run_block(x[lo:lo + n], out_stride, IN, out=sentinel(fmt, (n, out_stride)))
        w = f"format {fmt}, repeated stores, block {k} of {n} frames"
        same(got, want, w)
        same_words(r.sync_state(), o.state, w + ", state area")
        same_words(r.buf[HEAD:total], o.buf[HEAD:total], w + ", program words")
    assert (words(got)[:, 11] == words(sentinel(fmt, (1, 1)))[0, 0]).all()

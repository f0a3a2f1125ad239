"""Memory words on the chain kernels ("chain_mem" 1): trunks that end in STORE_MEM, branches that start with LOAD_MEM,
mem_stage between their cascades.  Every case is held to the oracle bit for bit after each block -- the outputs, the whole state area
and the program words behind the header (the memory words among them) -- with the option on; the option off (the interpreter, as
before) is the control on the same inputs."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import memtree_programs as mp

pytestmark = pytest.mark.gpu
IN = mp.IN
BLOCKS = [1, 7, 64, 100, 333, 1029]                  # in sequence: one frame, under a tile, a tile of frames, ragged, more than one launch
TSEC = [2, 0, 1, 16, 17, 40]                         # trunks: a short row, no cascade (the stage loads the sample), a full row, two and three pieces
FAN = [3, 1, 2, 0, 17]                               # branches per tree; 0: a word nobody reads
BSEC = [0, 1, 3, 16, 17]
US = [63, 20, 1000, 21, 2100, 25000]                 # lines of 3, 0 (bypass), 47, 1, 100 and 1199 (longer than a launch) samples
SLOTS = ["A", "B", None, "B", "A"]
FIN = ["tpdf_gain", "tpdf", "gain", "sat", "none"]
HEAD = 12                                            # program words of the header (its checksum covers them alone)


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in ("chain_mem", "chain_delay", "chain_finish"):
        rt.Runtime.set_global_option(key, 0)
    rt.Runtime.set_global_option("biquad_impl", 1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    g, w = words(got), words(want)
    bad = np.nonzero((g != w).any(axis=0))[0]
    assert bad.size == 0, (f"{what}: outputs {bad[:8].tolist()} differ, first frame "
                           f"{np.nonzero(g[:, bad[0]] != w[:, bad[0]])[0][:3].tolist()}: "
                           f"{g[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()} for {w[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()}")


def same_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:6].tolist()}"


def a_branch(key, i, j, dressed=True, delayed=True):
    fin = FIN[(i + j + j // 5) % 5] if dressed else ("sat", "none")[(i + j) % 2]
    us = US[(i + j) % 6]
    return mp.branch(key, nsec=BSEC[(i + j) % 5], slot=SLOTS[(i + 2 * j) % 5] if delayed else None, form=("param", "fixed")[(i + j) % 2], us=us,
                     max_us=max(us, 50), finish=fin, gain=0.9 + 0.01 * ((i + j) % 7), stores=2 if (i + j) % 3 == 1 else 1)


def mixed_items(n, dressed=True, delayed=True):
    """n trees: trunk sections, fan-outs, branch sections, slots, forms, line lengths, finishes and store counts mixed; every fourth
    trunk loads without gain; an ordinary chain (plain, dressed or delayed) behind every second trunk; the last branch of every third
    tree stands behind the next tree's trunk; every sixth tree is followed by two branches of a word the core does not write"""
    items, late = [], None
    for i in range(n):
        key = f"t{i}"
        items.append(mp.trunk(key, TSEC[i % 6], None if i % 4 == 3 else 0.4 + 0.01 * i))
        if late is not None:
            items.append(late)
            late = None
        if i % 2 == 0:
            us = US[(i // 2) % 6]
            items.append(mp.plain(nsec=BSEC[(i // 2) % 5], slot=SLOTS[(i // 2) % 5] if delayed else None, us=us, max_us=max(us, 50),
                                  finish=FIN[(i // 2) % 5] if dressed else "sat", load_gain=None if i % 4 else 0.6))
        mine = [a_branch(key, i, j, dressed, delayed) for j in range(FAN[i % 5])]
        if i % 3 == 1 and mine:
            late = mine.pop()
        items += mine
        if i % 6 == 0:
            items += [a_branch(f"w{i}", i, 0, dressed, delayed), a_branch(f"w{i}", i, 3, dressed, delayed)]
    if late is not None:
        items.append(late)
    return items


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def given_words(prog, wd, fmt):
    """non-zero values for the words nobody writes"""
    for k, (key, w) in enumerate(sorted(wd.items())):
        if key.startswith("w"):
            mp.set_word(prog, w, (0.31 - 0.07 * k) * (-1) ** k, fmt)


def oracle_run(fmt, prog, x, nout, dither, blocks, fs=48000, run=None):
    """the oracle's outputs, state and program words after each block"""
    o = po.OracleProgram(fmt, prog, fs=fs, random=1, dither=dither)
    total = int(prog[1])
    outs, states, progs = [], [], []
    for a, b in cut(blocks):
        outs.append(o.run_block(x[a:a + b], nout, IN))
        states.append(o.state.copy())
        progs.append(o.buf[HEAD:total].copy())
    return outs, states, progs


_REF = {}


def reference(fmt, n, dither=24, dressed=True, delayed=True, items=None, tag=None, seed=5):
    """program, input, and the oracle's outputs, state and program words after each block -- computed once, shared, never written"""
    key = (fmt, n, dither, dressed, delayed, tag)
    if key not in _REF:
        items = items if items is not None else mixed_items(n, dressed, delayed)
        c = mp.core(items, calc=0 if dressed else None)
        prog, nin, nout, wd = mp.program(fmt, [c])
        given_words(prog, wd, fmt)
        nout = max(nout, 1)                                       # (a core of trunks stores nothing: a window of one column)
        x = pb.lcg_input(sum(BLOCKS), nin, fmt == 6, seed=seed + n)
        outs, states, progs = oracle_run(fmt, prog, x, nout, dither, BLOCKS)
        for v in outs + states + progs + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, nout, outs, states, progs, c)
    return _REF[key]


def tree_runtime(fmt, prog, dither=24, finish=1, delay=1, fs=48000):
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=dither)
    r.set_option("chain_mem", 1)                              # (unknown to the code before this option existed: every test here fails there)
    r.set_option("chain_finish", finish)
    r.set_option("chain_delay", delay)
    return r


def compare_block(r, got, out, state, progw, what):
    same(got, out, what)
    same_words(r.sync_state(), state, what + ", state area")
    same_words(r.buf[HEAD:HEAD + len(progw)], progw, what + ", program words")


def run_and_compare(r, x, nout, outs, states, progs, what, run="run_block", blocks=BLOCKS):
    for k, (a, b) in enumerate(cut(blocks)):
        got = getattr(r, run)(x[a:a + b], nout, IN)
        compare_block(r, got, outs[k], states[k], progs[k], f"{what}, block {k} of {b} frames")


def nchains(c):
    return len(c["items"])


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("n", [1, 7, 37])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_trees_match_the_oracle(fmt, n, dither):
    prog, x, nout, outs, states, progs, c = reference(fmt, n, dither)
    r = tree_runtime(fmt, prog, dither)
    assert r.core_info()["chains"] == nchains(c) and r.mem_info() == mp.counts(c), r.last_error()
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, {n} trees, dither {dither}, chain_mem 1")
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_plain_trees_need_no_other_option(fmt):
    """plain finishes and no delay line: chain_finish 0 and chain_delay 0"""
    prog, x, nout, outs, states, progs, c = reference(fmt, 7, 24, dressed=False, delayed=False)
    r = tree_runtime(fmt, prog, finish=0, delay=0)
    assert r.get_option("chain_finish") == 0 and r.get_option("chain_delay") == 0
    assert r.core_info()["chains"] == nchains(c) and r.mem_info() == mp.counts(c), r.last_error()
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, chain_mem alone")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with the option off -- no chain, the same bits"""
    prog, x, nout, outs, states, progs, _ = reference(fmt, 7, 24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    r.set_option("chain_finish", 1)
    r.set_option("chain_delay", 1)
    assert r.get_option("chain_mem") == 0 and r.core_info()["chains"] == 0 and r.mem_info() == (0, 0, 0)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, chain_mem 0")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_biquad_impl_0(fmt):
    """the cross-check path: biquad_simple_hand hands the trunks over, biquad_simple reads the raw columns"""
    prog, x, nout, outs, states, progs, c = reference(fmt, 7, 24)
    r = tree_runtime(fmt, prog)
    r.set_option("biquad_impl", 0)
    assert r.core_info()["chains"] == nchains(c) and r.mem_info() == mp.counts(c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, biquad_impl 0")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_trunks_alone(fmt):
    """a core of trunks only: nothing is stored, the words hold every block's last frame"""
    items = [mp.trunk(f"t{i}", TSEC[i], None if i % 2 else 0.7) for i in range(6)]
    prog, x, nout, outs, states, progs, c = reference(fmt, 6, 24, items=items, tag="trunks")
    r = tree_runtime(fmt, prog)
    assert r.core_info()["chains"] == 6 and r.mem_info() == (6, 0, 0), r.last_error()
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, trunks only")
    w = mp.mem_ops(prog)[0][1]
    assert nout == 1 and progs[-1][w - HEAD:w - HEAD + 2].any()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_tree_wider_than_a_tile(fmt):
    """70 branches of one word (more columns than a tile of the stage closes at), beside a tree of 17 and one nobody reads"""
    items = [mp.trunk("a", 3), mp.trunk("b", 0, None), mp.trunk("c", 2)]
    items += [a_branch("a", 1, j) for j in range(70)] + [a_branch("b", 2, j) for j in range(17)]
    prog, x, nout, outs, states, progs, c = reference(fmt, 3, 24, items=items, tag="wide")
    r = tree_runtime(fmt, prog)
    assert r.core_info()["chains"] == 90 and r.mem_info() == (3, 87, 0), r.last_error()
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, 70 branches")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_words_nobody_writes_follow_upload_params(fmt):
    """branches of words the core only reads: constant through a block, edited between blocks through upload_params()"""
    items = [mp.branch("w0", nsec=2, finish="tpdf_gain"), mp.branch("w0", nsec=0, finish="sat", stores=2), mp.trunk("t", 1),
             mp.branch("w1", nsec=0, slot="A", us=63, finish="tpdf"), mp.branch("t", nsec=1, finish="sat"), mp.branch("w1", nsec=17, slot="B", us=1000, finish="gain")]
    c = mp.core(items, calc=0)
    prog, nin, nout, wd = mp.program(fmt, [c])
    given_words(prog, wd, fmt)
    blocks = [64, 5, 1029, 100]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=8)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tree_runtime(fmt, prog)
    assert r.core_info()["chains"] == 6 and r.mem_info() == (1, 5, 4), r.last_error()
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        if k:
            for buf in (o.buf, r.buf):
                mp.set_word(buf, wd["w0"], 0.2 * k - 0.5, fmt)
                mp.set_word(buf, wd["w1"], -0.11 * k, fmt)
            r.upload_params()
        want = o.run_block(x[a:a + b], nout, IN)
        compare_block(r, r.run_block(x[a:a + b], nout, IN), want, o.state, o.buf[HEAD:total], f"format {fmt}, block {k}")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_word_at_an_odd_index(fmt):
    """a hand-made program: both opcodes' offsets moved by one word inside a dspMem_LocationMultiple(2) -- two 32-bit accesses"""
    items = [mp.trunk("a", 2), mp.branch("a", nsec=1, finish="sat"), mp.branch("a", nsec=0, finish="tpdf_gain"),
             mp.branch("a", nsec=0, slot="B", us=63, finish="sat"), mp.trunk("b", 0), mp.branch("b", nsec=0, finish="none")]
    c = mp.core(items, calc=0)
    prog, nin, nout, wd = mp.program(fmt, [c], pairs=("a", "b"))
    for op, target in mp.mem_ops(prog):
        prog[op + 1] += 1
    assert all(t % 2 == 1 for _, t in mp.mem_ops(prog))
    x = pb.lcg_input(sum(BLOCKS), nin, fmt == 6, seed=9)
    outs, states, progs = oracle_run(fmt, prog, x, nout, 24, BLOCKS)
    r = tree_runtime(fmt, prog)
    assert r.core_info()["chains"] == 6 and r.mem_info() == (2, 4, 0), r.last_error()
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, odd word index")


def three_cores(fmt):
    """the oktodac_diy arrangement: trunks in core 1, their branches in cores 2 and 3 (which see the trunks' last frame of the block),
    and trees local to core 3"""
    c1 = mp.core([mp.trunk("l", 5, 0.7), mp.trunk("r", 0, None), mp.trunk("s", 17, 0.6)], calc=0)
    c2 = mp.core([mp.branch("l", nsec=4, slot="A", form="param", us=2100, finish="tpdf"), mp.branch("r", nsec=0, slot="B", us=21, finish="tpdf_gain"),
                  mp.plain(nsec=2, finish="tpdf_gain"), mp.branch("l", nsec=0, finish="none")])
    c3 = mp.core([mp.branch("s", nsec=1, finish="gain"), mp.trunk("m", 2), mp.branch("r", nsec=16, slot="A", us=1000, finish="sat", stores=2),
                  mp.branch("m", nsec=3, finish="tpdf"), mp.branch("m", nsec=0, slot="A", form="param", us=63, finish="sat")])
    return mp.program(fmt, [c1, c2, c3]), [c1, c2, c3]


@pytest.mark.parametrize("run", ["run_block_all", "run_block"])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_three_cores(fmt, run):
    (prog, nin, nout, wd), cores = three_cores(fmt)
    blocks = [64, 300, 1100]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=33)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tree_runtime(fmt, prog)
    assert [r.mem_info(k) for k in range(3)] == [mp.counts(c) for c in cores] == [(3, 0, 0), (0, 3, 3), (1, 4, 2)], r.last_error()
    assert [r.core_info(k)["chains"] for k in range(3)] == [3, 4, 5]
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN)
        got = getattr(r, run)(x[a:a + b], nout, IN)                  # (run_block: core by core)
        compare_block(r, got, want, o.state, o.buf[HEAD:total], f"format {fmt}, {run}, block {k}")


def test_inf_and_nan_samples_take_the_replay():
    """a format-6 block with Inf and NaN samples: the replay (cascade_in_reference_order) hands the trunks over too, and the words keep
    the non-finite accumulators"""
    fmt = 6
    items = [mp.trunk("a", 2, None), mp.branch("a", nsec=1, slot="A", us=63, finish="tpdf"), mp.branch("a", nsec=0, finish="tpdf_gain"),
             mp.trunk("b", 0, 0.5), mp.branch("b", nsec=3, finish="sat"), mp.branch("b", nsec=0, slot="B", us=1000, finish="gain"),
             mp.trunk("c", 17, None), mp.branch("c", nsec=16, finish="none"), mp.plain(nsec=2, finish="tpdf", load_gain=None)]
    prog, nin, nout, wd = mp.program(fmt, [mp.core(items, calc=0)])
    blocks = [400, 37]
    x = pb.lcg_input(sum(blocks), nin, True, seed=21).copy()
    x[37, 0] = np.inf; x[150, 1] = -np.inf; x[151, 2] = np.nan; x[20, 3] = np.inf; x[399, 1] = np.nan; x[436, 0] = np.nan
    outs, states, progs = oracle_run(fmt, prog, x, nout, 24, blocks)
    r = tree_runtime(fmt, prog)
    assert r.core_info()["chains"] == 9 and r.mem_info() == (3, 5, 0), r.last_error()
    run_and_compare(r, x, nout, outs, states, progs, "format 6, Inf and NaN", blocks=blocks)


def test_full_scale_samples_in_format_2():
    fmt = 2
    prog, _, nout, _, _, _, c = reference(fmt, 7, 24)
    nin = sum(it["kind"] != "branch" for it in c["items"])
    blocks = [100, 333]
    x = pb.lcg_input(sum(blocks), nin, False, seed=4).copy()
    x[::3] = np.int32(0x7FFFFFFF); x[1::3] = np.int32(-0x80000000)
    outs, states, progs = oracle_run(fmt, np.array(prog), x, nout, 24, blocks)
    r = tree_runtime(fmt, np.array(prog))
    assert r.core_info()["chains"] == nchains(c) and r.mem_info() == mp.counts(c)
    run_and_compare(r, x, nout, outs, states, progs, "format 2, full scale", blocks=blocks)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_reset_to_44100_mid_stream(fmt):
    """another rate: other coefficients, other line lengths, the data area zeroed -- the memory words survive, as in the reference"""
    prog, x, nout, _, _, _, c = reference(fmt, 7, 24)
    o = po.OracleProgram(fmt, np.array(prog), fs=48000, random=1, dither=24)
    r = tree_runtime(fmt, np.array(prog))
    assert r.mem_info() == mp.counts(c)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut([100, 333, 64])):
        if k == 1:
            assert o.reset(44100, 1, 24) >= 0 and r.reset(44100, 1, 24) >= 0
            assert r.core_info()["chains"] == nchains(c) and r.mem_info() == mp.counts(c), r.last_error()
        want = o.run_block(x[a:a + b], nout, IN)
        compare_block(r, r.run_block(x[a:a + b], nout, IN), want, o.state, o.buf[HEAD:total], f"format {fmt}, block {k}")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_switched_inside_a_stream(fmt):
    """on, off and on again between blocks: a replan each time, the same stream"""
    prog, x, nout, outs, states, progs, c = reference(fmt, 7, 24)
    r = tree_runtime(fmt, prog)
    for k, (a, b) in enumerate(cut(BLOCKS)):
        r.set_option("chain_mem", 0 if k in (2, 3) else 1)
        assert r.core_info()["chains"] == (0 if k in (2, 3) else nchains(c))
        assert r.mem_info() == ((0, 0, 0) if k in (2, 3) else mp.counts(c))
        compare_block(r, r.run_block(x[a:a + b], nout, IN), outs[k], states[k], progs[k], f"format {fmt}, block {k}")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_stage_runs_once_per_launch(fmt):
    """the chain kernels, not the interpreter: mem_stage's timer (the stage's kind, as the mux stage's) counts a span per launch of
    1024 frames, the interpreter's none; with the option off it is the other way round"""
    prog, x, nout, _, _, _, c = reference(fmt, 7, 24)
    r = tree_runtime(fmt, prog)
    r.set_option("profile", 1)
    try:
        r.kernel_time(7), r.kernel_time(3)
        r.run_block(x[:1029], nout, IN)
        assert r.kernel_time(7)[1] == 2
        r.set_option("chain_mem", 0)
        r.kernel_time(7), r.kernel_time(3)
        r.run_block(x[:1029], nout, IN)
        assert r.kernel_time(7)[1] == 0 and r.kernel_time(3)[1] + r.kernel_time(5)[1] + r.kernel_time(6)[1] >= 1
    finally:
        r.set_option("profile", 0)

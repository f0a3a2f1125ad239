"""A DSP_FIR in a trunk or a branch of a memory-word tree on the chain kernels ("mem_fir" 1 beside "chain_mem" 1): the
trunks' FIR launch in front of mem_stage, the stage's FEED form for branches that are a FIR alone, the branches' cascades into the
rings, the plain and the handed FIR launch behind them.  Every case is held to the oracle bit for bit after each block -- the outputs,
the whole state area (FIR histories and delay lines among it) and the program words behind the header (the memory words among them);
each first asserts through mem_fir_info() that its chains are lowered.  "mem_fir" 0 (the interpreter, as before) is the control."""
import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import firtree_programs as tp

pytestmark = pytest.mark.gpu
IN = tp.IN
BLOCKS = [1, 7, 64, 100, 333, 1029]                  # in sequence: a lane, under a tile of the stage, a tile, ragged, more than one launch
TSEC = [2, 0, 17]                                    # trunks: a row, no cascade, two pieces ...
TTAPS = [31, 0, 255, 0, 7, 700]                      # ... with and without a FIR
BSEC = [0, 1, 17]
BTAPS = [63, 0, 255, 7, 700]                         # (1500, past one 896-position chunk: two branches and an ordinary chain below)
US = [63, 20, 1000, 21, 25000]                       # lines of 3, 0 (bypass), 47, 1 and 1199 (longer than a launch) samples
SLOTS = ["A", "B", None, "B", "A"]
FIN = ["tpdf_gain", "tpdf", "gain", "sat", "none"]
HEAD = 12                                            # program words of the header (its checksum covers them alone)
OPTIONS = ("mem_fir", "chain_mem", "fir_tail", "chain_delay", "chain_finish")


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS + ("fir_lean",):
        rt.Runtime.set_global_option(key, 0 if key != "fir_lean" else -1)
    for key, v in (("biquad_impl", 1), ("fir_impl", 1), ("fir_rows", 0)):
        rt.Runtime.set_global_option(key, v)
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


def a_branch(key, i, j, taps=None, nsec=None):
    """branch j of tree i: sections, taps, plain or handed (both slots, both delay forms, the line lengths, the four finishes and none), one
    or two STOREs -- mixed by index"""
    taps = BTAPS[(i + 2 * j) % 5] if taps is None else taps
    nsec = BSEC[(i + j) % 3] if nsec is None else nsec
    stores = 2 if (i + j) % 3 == 1 else 1
    if (i + j) % 2:
        return tp.branch(key, nsec=nsec, taps=taps, finish=("sat", "none")[(i + j) // 2 % 2], stores=stores)
    us = US[(i + j) % 5]
    return tp.branch(key, nsec=nsec, taps=taps, slot=SLOTS[(i + 2 * j) % 5], form=("param", "fixed")[(i + j) // 2 % 2], us=us, max_us=max(us, 50),
                     finish=FIN[(i + j + j // 5) % 5], gain=0.9 + 0.01 * ((i + j) % 7), stores=stores)


def mixed_items(n=18):
    """n trees: trunk sections and taps, fan-outs, branch sections and taps mixed.  The stage's tiles (stage_tiles below): trees 0 .. 15
    fill one (16 trees); tree 16, the 17th, has 66 branches with a section each and no FIR -- more columns than a tile closes at --
    and is a tile alone; tree 17 and the words nobody writes follow in a third, whose feed lists so begin behind a tile closed by its
    columns.  Tree 3 has 5 branches that are a FIR alone, trees 11 and 17 have 17 each (more feeds than a tile has trees); trees 7 and
    14 have no FIR anywhere (tree 14's trunk has 17 sections); an ordinary chain -- a FIR alone, a handed FIR chain, a delayed cascade
    chain, a dressed passthrough -- behind every second trunk; two branches of a word nobody writes behind every sixth tree; the last
    branch of every third tree stands behind the next tree's trunk"""
    items, late = [], None
    for i in range(n):
        key = f"t{i}"
        firless = i in (7, 14)
        items.append(tp.trunk(key, TSEC[i % 3], 0 if firless else TTAPS[i % 6], None if i % 4 == 3 else 0.4 + 0.01 * i))
        if late is not None:
            items.append(late)
            late = None
        if i % 2 == 0:
            k = i // 2
            us = US[k % 5]
            items.append([tp.plain(nsec=0, taps=1500 if k == 0 else 63, load_gain=None),
                          tp.plain(nsec=2, taps=255, slot=SLOTS[k % 5], us=us, finish=FIN[k % 5]),
                          tp.plain(nsec=1, taps=0, slot="A", form="param", us=us, max_us=max(us, 50), finish="tpdf"),
                          tp.plain(nsec=0, taps=0, finish="tpdf_gain", load_gain=None)][k % 4])
        if i == 3:
            mine = [a_branch(key, i, j, taps=63, nsec=0) for j in range(5)] + [a_branch(key, i, 5, taps=0, nsec=1)]
        elif i in (11, 17):
            mine = [a_branch(key, i, j, taps=63 if j % 4 else 7, nsec=0) for j in range(17)]
        elif i == 16:
            mine = [a_branch(key, i, j, taps=0, nsec=1) for j in range(66)]
        else:
            mine = [a_branch(key, i, j, taps=0 if firless else 1500 if (i, j) == (5, 1) else None) for j in range([3, 1, 2, 4][i % 4])]
        if i % 3 == 1 and len(mine) > 1:
            late = mine.pop()
        items += mine
        if i % 6 == 0:
            items += [a_branch(f"w{i}", i, 0, taps=1500 if i == 6 else 255, nsec=0), a_branch(f"w{i}", i, 3, taps=63, nsec=1)]
    if late is not None:
        items.append(late)
    return items


def stage_tiles(items):
    """mem_trees' rule (avdsp_plan_layout.h) on a core's items: the trees with a trunk in program order, then the words nobody writes; a
    tile is closed at 16 trees, or once it holds 64 columns (a column per branch with sections).  -> per tile (first tree, trees, columns,
    ring feeds), and per tree its key"""
    keys = [it["key"] for it in items if it["kind"] == "trunk"]
    keys += [k for k in dict.fromkeys(it["key"] for it in items if it["kind"] == "branch") if k not in keys]
    cols = {k: sum(it["kind"] == "branch" and it["key"] == k and it["nsec"] > 0 for it in items) for k in keys}
    feeds = {k: sum(it["kind"] == "branch" and it["key"] == k and not it["nsec"] and tp.has_fir(it) for it in items) for k in keys}
    tiles = []
    for n, k in enumerate(keys):
        if not tiles or tiles[-1][1] == 16 or tiles[-1][2] >= 64:
            tiles.append([n, 0, 0, 0])
        tiles[-1][1] += 1
        tiles[-1][2] += cols[k]
        tiles[-1][3] += feeds[k]
    return [tuple(t) for t in tiles], keys


def small_items():
    """what the interpreter gets through in a moment: a FIR trunk, a branch with a cascade and a FIR, two that are a FIR alone (one
    handed), a FIR-less branch, an ordinary FIR-only chain, a branch of a word nobody writes"""
    return [tp.trunk("a", 2, 31, 0.7), tp.branch("a", nsec=1, taps=63), tp.branch("a", nsec=0, taps=63, finish="none", stores=2),
            tp.branch("a", nsec=0, taps=7, slot="A", us=1000, finish="tpdf_gain"), tp.branch("a", nsec=0, taps=0, slot="B", us=63, finish="sat"),
            tp.plain(nsec=0, taps=40, load_gain=None), tp.trunk("b", 0, 15, None), tp.branch("b", nsec=0, taps=0, finish="tpdf"),
            tp.branch("w", nsec=0, taps=9)]


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def given_words(prog, wd, fmt):
    """non-zero values for the words nobody writes"""
    for k, (key, w) in enumerate(sorted(wd.items())):
        if key.startswith("w"):
            tp.set_word(prog, w, (0.31 - 0.07 * k) * (-1) ** k, fmt)


def oracle_run(fmt, prog, x, nout, dither, blocks, fs=48000):
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


def reference(fmt, tag, dither=24, blocks=BLOCKS, seed=5):
    """program, input, and the oracle's outputs, state and program words after each block -- computed once, shared, never written"""
    key = (fmt, tag, dither, tuple(blocks))
    if key not in _REF:
        c = tp.core(mixed_items() if tag == "mixed" else small_items(), calc=0)
        prog, nin, nout, wd = tp.program(fmt, [c])
        given_words(prog, wd, fmt)
        x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=seed)
        outs, states, progs = oracle_run(fmt, prog, x, nout, dither, blocks)
        for v in outs + states + progs + [x, prog]:
            v.flags.writeable = False
        _REF[key] = (prog, x, nout, outs, states, progs, c)
    return _REF[key]


def tree_runtime(fmt, prog, dither=24, fs=48000, mem_fir=1):
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=dither)
    for key in OPTIONS[1:]:
        r.set_option(key, 1)
    r.set_option("mem_fir", mem_fir)                          # (unknown to the code before this option existed: every test here fails there)
    return r


def lowered(r, c, core_index=0):
    """the core's chains are on the chain kernels: every trunk, branch and FIR of it counted"""
    assert r.core_info(core_index)["chains"] == len(c["items"]), r.last_error()
    assert r.mem_fir_info(core_index) == tp.fir_counts(c) and r.mem_info(core_index) == tp.mem_counts(c) and r.fir_tail_info(core_index) == tp.tail_counts(c)


def compare_block(r, got, out, state, progw, what):
    same(got, out, what)
    same_words(r.sync_state(), state, what + ", state area")
    same_words(r.buf[HEAD:HEAD + len(progw)], progw, what + ", program words")


def run_and_compare(r, x, nout, outs, states, progs, what, run="run_block", blocks=BLOCKS):
    for k, (a, b) in enumerate(cut(blocks)):
        got = getattr(r, run)(x[a:a + b], nout, IN)
        compare_block(r, got, outs[k], states[k], progs[k], f"{what}, block {k} of {b} frames")


def test_the_mix_reaches_every_seam():
    """host-only bookkeeping on the 18-tree core: what the cases below rely on"""
    items = mixed_items()
    c = tp.core(items, calc=0)
    trunks = [it for it in items if it["kind"] == "trunk"]
    br = [it for it in items if it["kind"] == "branch"]
    assert len(trunks) == 18 and {(it["nsec"], bool(it["taps"])) for it in trunks} == {(s, f) for s in TSEC for f in (False, True)}
    assert {(it["nsec"], bool(it["taps"])) for it in br} == {(s, f) for s in BSEC for f in (False, True)}
    assert {it["taps"] for it in items} >= {0, 7, 255, 700, 1500}
    assert {it["slot"] for it in br if tp.is_handed(it)} == {"A", "B", None} and {it["form"] for it in br if tp.is_handed(it) and it["slot"]} == {"param", "fixed"}
    assert {it["finish"] for it in br if tp.has_fir(it)} == set(FIN) and {it["stores"] for it in br if tp.has_fir(it)} == {1, 2}
    assert {it["us"] for it in br if tp.is_handed(it) and it["slot"]} == set(US)
    feeds = {}
    for it in br:
        if tp.has_fir(it) and not it["nsec"]:
            feeds[it["key"]] = feeds.get(it["key"], 0) + 1
    assert feeds["t3"] == 5 and feeds["t11"] == 17 and feeds["t17"] == 17
    # the stage's tiles: a full one (16 trees), one closed by its columns (tree 16 alone, 66 >= 64), and behind it the tile of tree 17
    # and the three words nobody writes, with 17 + 3 feeds
    tiles, keys = stage_tiles(items)
    assert keys[16:] == ["t16", "t17", "w0", "w6", "w12"]
    assert [(t[0], t[1]) for t in tiles] == [(0, 16), (16, 1), (17, 4)] and tiles[1][2:] == (66, 0) and tiles[2][3] == 20 and tiles[0][3] >= 22
    assert tp.fir_counts(c)[0] >= 8 and tp.fir_counts(c)[2] >= 10 and tp.mem_counts(c)[2] == 6
    assert sum(it["taps"] for it in items) * sum(BLOCKS) <= 5e7          # the oracle's work per case, in tap-frames
    lowered(tree_runtime(6, tp.program(6, [c])[0]), c)


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_trees_match_the_oracle(fmt, dither):
    prog, x, nout, outs, states, progs, c = reference(fmt, "mixed", dither)
    r = tree_runtime(fmt, prog, dither)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, 18 trees, dither {dither}, mem_fir 1")
    r.release()


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_off_is_the_interpreter_as_before(fmt):
    """the control: the same program and inputs with "mem_fir" 0 -- no chain, the same bits -- and with 1"""
    blocks = [7, 64, 100]
    prog, x, nout, outs, states, progs, c = reference(fmt, "small", blocks=blocks)
    r = tree_runtime(fmt, prog, mem_fir=0)
    assert r.get_option("mem_fir") == 0 and r.get_option("chain_mem") == 1 and r.core_info()["chains"] == 0 and r.mem_fir_info() == (0, 0, 0)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, mem_fir 0", blocks=blocks)
    r.release()
    r = tree_runtime(fmt, prog)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, mem_fir 1", blocks=blocks)


@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_impl_0_appends_every_input_once(fmt):
    """fir_plain, the reference's loop, over four blocks: branches that are a FIR alone (fed by the stage) beside an ordinary FIR-only
    chain and a FIR-only trunk (which append their own input) -- an input appended twice shows as a history shifted by a block"""
    blocks = [64, 100, 7, 333]
    prog, x, nout, outs, states, progs, c = reference(fmt, "small", blocks=blocks)
    r = tree_runtime(fmt, prog)
    r.set_option("fir_impl", 0)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, fir_impl 0", blocks=blocks)


@pytest.mark.parametrize("rows, frames", [(1, 100), (2, 300), (4, 600)])
@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_rows(fmt, rows, frames):
    blocks = [frames, 64]
    prog, x, nout, outs, states, progs, c = reference(fmt, "mixed", blocks=blocks)
    r = tree_runtime(fmt, prog)
    r.set_option("fir_rows", rows)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, fir_rows {rows}", blocks=blocks)


@pytest.mark.parametrize("lean", [0, 1])
@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_lean(fmt, lean):
    blocks = [333, 64]
    prog, x, nout, outs, states, progs, c = reference(fmt, "mixed", blocks=blocks)
    r = tree_runtime(fmt, prog)
    r.set_option("fir_lean", lean)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, fir_lean {lean}", blocks=blocks)


@pytest.mark.parametrize("fmt", [4, 6])
def test_biquad_impl_0(fmt):
    blocks = [333, 64]
    prog, x, nout, outs, states, progs, c = reference(fmt, "mixed", blocks=blocks)
    r = tree_runtime(fmt, prog)
    r.set_option("biquad_impl", 0)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, f"format {fmt}, biquad_impl 0", blocks=blocks)


def test_inf_nan_and_subnormal_samples():
    """format 6: non-finite samples go through the trunks' cascades and FIRs into the words and the branches' rings; subnormal ones are
    flushed where the reference flushes them"""
    fmt = 6
    c = tp.core(small_items(), calc=0)
    prog, nin, nout, wd = tp.program(fmt, [c])
    given_words(prog, wd, fmt)
    blocks = [400, 37, 64]
    x = pb.lcg_input(sum(blocks), nin, True, seed=21).copy()
    x[37, 0] = np.inf; x[150, 1] = -np.inf; x[151, 2] = np.nan; x[20, 2] = np.inf; x[399, 1] = np.nan; x[436, 0] = np.nan
    x.view(np.uint32)[200:230, :] = np.array([0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32)[np.arange(30) % 3][:, None]
    outs, states, progs = oracle_run(fmt, prog, x, nout, 24, blocks)
    r = tree_runtime(fmt, prog)
    lowered(r, c)
    run_and_compare(r, x, nout, outs, states, progs, "format 6, Inf, NaN and subnormals", blocks=blocks)


def three_cores(fmt):
    """trunks in core 1, their branches in cores 2 and 3 (which see the trunks' last frame of the block), and a tree local to core 3"""
    c1 = tp.core([tp.trunk("l", 2, 255, 0.7), tp.trunk("r", 0, 31, None), tp.trunk("s", 17, 0, 0.6)], calc=0)
    c2 = tp.core([tp.branch("l", nsec=0, taps=700, slot="A", form="param", us=2100, finish="tpdf"), tp.branch("r", nsec=1, taps=63, finish="none"),
                  tp.plain(nsec=2, taps=63, finish="tpdf_gain"), tp.branch("l", nsec=0, taps=63, stores=2)])
    c3 = tp.core([tp.branch("s", nsec=0, taps=255), tp.trunk("m", 2, 7), tp.branch("r", nsec=17, taps=0, slot="A", us=1000, finish="sat", stores=2),
                  tp.branch("m", nsec=0, taps=63, slot="B", us=63, finish="sat"), tp.branch("m", nsec=1, taps=0, finish="tpdf")])
    return tp.program(fmt, [c1, c2, c3]), [c1, c2, c3]


@pytest.mark.parametrize("run", ["run_block_all", "run_block"])
@pytest.mark.parametrize("fmt", [4, 6])
def test_three_cores(fmt, run):
    (prog, nin, nout, wd), cores = three_cores(fmt)
    blocks = [64, 300, 1100]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=33)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tree_runtime(fmt, prog)
    for k, c in enumerate(cores):
        lowered(r, c, k)
    assert [r.mem_fir_info(k) for k in range(3)] == [(2, 0, 0), (0, 3, 1), (1, 2, 1)] and r.mem_info(1) == (0, 3, 3)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN)
        got = getattr(r, run)(x[a:a + b], nout, IN)                  # (run_block: core by core)
        compare_block(r, got, want, o.state, o.buf[HEAD:total], f"format {fmt}, {run}, block {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_reset_to_44100_mid_stream(fmt):
    """another rate: the other impulses (of other lengths), other coefficients and line lengths, the data area zeroed -- the memory words
    survive, as in the reference"""
    prog, x, nout, _, _, _, c = reference(fmt, "mixed")
    o = po.OracleProgram(fmt, np.array(prog), fs=48000, random=1, dither=24)
    r = tree_runtime(fmt, np.array(prog))
    lowered(r, c)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut([100, 333, 64])):
        if k == 1:
            assert o.reset(44100, 1, 24) >= 0 and r.reset(44100, 1, 24) >= 0
            lowered(r, c)
            assert r.core_info()["max_taps"] == 1000
        want = o.run_block(x[a:a + b], nout, IN)
        compare_block(r, r.run_block(x[a:a + b], nout, IN), want, o.state, o.buf[HEAD:total], f"format {fmt}, block {k}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_switched_inside_a_stream(fmt):
    """on, off and on again between blocks: a replan each time -- the FIR histories go ring -> mirror -> ring -- the same stream"""
    blocks = [64, 7, 100, 33, 333]
    prog, x, nout, outs, states, progs, c = reference(fmt, "small", blocks=blocks)
    r = tree_runtime(fmt, prog)
    for k, (a, b) in enumerate(cut(blocks)):
        on = k not in (1, 2)
        r.set_option("mem_fir", 1 if on else 0)
        assert r.core_info()["chains"] == (len(c["items"]) if on else 0) and r.mem_fir_info() == (tp.fir_counts(c) if on else (0, 0, 0))
        compare_block(r, r.run_block(x[a:a + b], nout, IN), outs[k], states[k], progs[k], f"format {fmt}, block {k}, mem_fir {int(on)}")


@pytest.mark.parametrize("fmt", [4, 6])
def test_an_in_place_call(fmt):
    """one [frames][io] block in device memory as both windows: the trunks and the ordinary FIR-only chain read their samples behind
    the stage's and the first FIR launch's stores -- from the copy the call sets aside"""
    import torch
    c = tp.core(small_items(), calc=0)
    prog, nin, nout, wd = tp.program(fmt, [c])
    given_words(prog, wd, fmt)
    W = IN + nin
    blocks = [1, 100, 1029]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=23)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = tree_runtime(fmt, prog)
    lowered(r, c)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        frame = np.empty((b, W), dtype=rt.sample_dtype(fmt))
        frame.view(np.uint32)[...] = 0x7FC0BEEF if fmt == 6 else 0x5A5A1234
        frame[:, IN:IN + nin] = x[a:a + b]
        want = frame.copy()
        o.run_block(want, W, 0, 0, out=want)
        d = dm.to_device(frame)
        r.run_block_device(d.data_ptr(), W, 0, d.data_ptr(), W, 0, b, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        w = f"format {fmt}, in place, block {k} of {b} frames"
        same(dm.to_host(d), want, w)
        same_words(r.sync_state(), o.state, w + ", state area")
        same_words(r.buf[HEAD:total], o.buf[HEAD:total], w + ", program words")


@pytest.mark.parametrize("fmt", [4, 6])
def test_the_launches_of_a_block(fmt):
    """the chain kernels, not the interpreter: per launch of 1024 frames one span of the stage's timer and three of the FIR's (the
    trunks' launch, the plain one, the handed one); with "mem_fir" 0 the interpreter's and none of these"""
    prog, x, nout, _, _, _, c = reference(fmt, "small", blocks=[7, 64, 100])
    r = tree_runtime(fmt, np.array(prog))
    lowered(r, c)
    r.set_option("profile", 1)
    try:
        r.kernel_time(7), r.kernel_time(1)
        r.run_block(x[:100], nout, IN)
        assert r.kernel_time(7)[1] == 1 and r.kernel_time(1)[1] == 3
        r.set_option("mem_fir", 0)
        r.kernel_time(7), r.kernel_time(1)
        r.run_block(x[100:171], nout, IN)
        assert r.kernel_time(7)[1] == 0 and r.kernel_time(1)[1] == 0
    finally:
        r.set_option("profile", 0)

"""Memory-word trees under a set shard ("shard_trees" 1) on the device: every rank of a world gets a Runtime of its own,
one after the other in this process, and is held to the oracle bit for bit after each block -- its chains' output columns (every other
column keeps the sentinel), the state words of its chains (the rest as uploaded), its trunks' memory words (every other program word
as loaded); then the ranks' columns together are the oracle's whole block.  Blocks of 64, 100 and 1029 frames: the last crosses the
launch seam of 1024."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from tests import firtree_programs as tp
from tests import lowered_programs as lp
from tests import shard_tree_programs as stp

pytestmark = pytest.mark.gpu
IN, HEAD = tp.IN, lp.HEAD
BLOCKS = [64, 100, 1029]
RANDOM_WORLD = 3


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in lp.OPTIONS + ("shard_trees",):
        try:
            rt.Runtime.set_global_option(key, 0)
        except rt.AvdspError:                                  # (a library without "shard_trees")
            pass
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- runs and their references (computed once on the CPU, shared, never written) ----
def hand_made(name, fmt, items, calc=None):
    core, nout = stp.core_of_items(items)
    prog, nin, nout2, wd = tp.program(fmt, [tp.core(items, calc=calc)])
    assert nout == nout2
    for k, (key, w) in enumerate(sorted(wd.items())):
        if key.startswith("w"):
            tp.set_word(prog, w, (0.31 - 0.07 * k) * (-1) ** k, 2 if fmt == 2 else 6)
    return dict(name=f"{name}, format {fmt}", fmt=fmt, prog=prog, in_stride=nin, out_stride=nout + 2, cores=[core], words=wd, seed=len(items))


def random_run(seed, fmt):
    prog, in_stride, out_stride, desc = lp.random_lowered_program(seed, fmt)
    return dict(name=f"random seed {seed}, format {fmt}", fmt=fmt, prog=prog, in_stride=in_stride, out_stride=out_stride,
                cores=stp.random_run_cores(desc["drawn"]), words=desc["words"], seed=seed)


_REF = {}


def reference(run, blocks=BLOCKS):
    """input, and the oracle's outputs (over the sentinel), state and program words after each block"""
    from oracle import pyoracle as po
    key = (run["name"], tuple(blocks))
    if key not in _REF:
        fmt, total = run["fmt"], int(run["prog"][1])
        x = pb.lcg_input(sum(blocks), run["in_stride"], fmt in (5, 6), seed=300 + run["seed"])
        o = po.OracleProgram(fmt, run["prog"].copy(), fs=48000, random=1, dither=24)
        assert o.rc >= 0
        outs, states, progs = [], [], []
        for a, b in cut(blocks):
            outs.append(o.run_block(x[a:a + b], run["out_stride"], IN, out=lp.sentinel(fmt, (b, run["out_stride"]))))
            states.append(o.state.copy())
            progs.append(o.buf[:total].copy())
        for v in outs + states + progs + [x]:
            v.flags.writeable = False
        _REF[key] = (x, outs, states, progs)
    return _REF[key]


def a_runtime(run):
    r = rt.Runtime(run["fmt"], run["prog"].copy(), fs=48000, random=1, dither=24)
    assert r.rc >= 0
    for key in lp.OPTIONS + ("shard_trees",):                # (unknown to the library before this option existed: every test here fails there)
        r.set_option(key, run.get("shard_trees", 1) if key == "shard_trees" else 1)
    return r


def owned(run, rank, world):
    """what `rank` of `world` owns: its output columns, a mask over the state area, the first words of its trunks' memory words, and
    per core the cut the library must report"""
    owners = lp.state_owners(run["prog"])
    cols, mine, trunk_words, cuts = set(), set(), [], []
    for ci, c in enumerate(run["cores"]):
        cu = stp.cut_of(c, rank, world)
        cuts.append(cu)
        lo, m = (0, len(c["chains"])) if cu is None else cu
        if cu is None:
            cols.update(c["extra_cols"])
        for ch in range(lo, lo + m):
            cols.update(c["stores"][ch])
            mine.add((ci, ch))
            if c["chains"][ch]["kind"] == "trunk":
                trunk_words.append(run["words"][c["chains"][ch]["key"]])
    return cols, mine, owners, trunk_words, cuts


def state_mask(owners, mine, n):
    own = np.zeros(n, dtype=bool)
    edges = [a for a, *_ in owners] + [n]
    for (a, ci, ch, _), b in zip(owners, edges[1:]):
        if ch < 0 or (ci, ch) in mine:                         # (a core's head TPDF_CALC runs on every rank)
            own[a:b] = True
    return own


def first_bad(got, want):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} words differ, first at {bad[:6].tolist()}: {got[bad[:3]].tolist()} for {want[bad[:3]].tolist()}"


def play_rank(run, rank, world, blocks=BLOCKS):
    """-> per block, the rank's output block"""
    fmt, total = run["fmt"], int(run["prog"][1])
    x, outs, states, progs = reference(run, blocks)
    cols, mine, owners, trunk_words, cuts = owned(run, rank, world)
    r = a_runtime(run)
    r.set_shard(rank, world)
    for ci, cu in enumerate(cuts):                            # the library cuts where the rule says
        s = r.shard_info(ci)
        if cu is None:
            assert s["total_chains"] == 0 or run["cores"][ci]["chains"] == [], f"{run['name']}: core {ci} should run whole on every rank"
        else:
            assert (s["total_chains"], s["first_chain"], s["nchains"]) == (len(run["cores"][ci]["chains"]),) + tuple(cu), f"{run['name']}, core {ci}: {r.last_error()}"
    state0, prog0 = r.state.copy(), run["prog"][:total].copy()
    own = state_mask(owners, mine, len(state0))
    other_cols = [c for c in range(run["out_stride"]) if c not in cols]
    got_all = []
    for k, (a, b) in enumerate(cut(blocks)):
        what = f"{run['name']}, rank {rank} of {world}, block {k} of {b} frames"
        got = r.run_block(x[a:a + b], run["out_stride"], IN, out=lp.sentinel(fmt, (b, run["out_stride"])))
        want = outs[k].copy()
        want[:, other_cols] = lp.sentinel(fmt, (b, len(other_cols)))
        g, w = words(got), words(want)
        bad = np.nonzero((g != w).any(axis=0))[0]
        assert bad.size == 0, f"{what}: output columns {bad[:8].tolist()} differ (the rank's own: {sorted(cols)[:8]} ...)"
        st = r.sync_state()
        assert (st[own] == states[k][own]).all(), f"{what}: its chains' state: {first_bad(st[own], states[k][own])}"
        assert (st[~own] == state0[~own]).all(), f"{what}: the other chains' state moved: {first_bad(st[~own], state0[~own])}"
        wantp = prog0.copy()
        for wd in trunk_words:
            wantp[wd:wd + 2] = progs[k][wd:wd + 2]
        assert (r.buf[HEAD:total] == wantp[HEAD:]).all(), f"{what}: program words: {first_bad(r.buf[HEAD:total], wantp[HEAD:])}"
        got_all.append(got)
    r.release()
    return got_all, cols


def play_world(run, world, blocks=BLOCKS):
    _, outs, _, _ = reference(run, blocks)
    together = [lp.sentinel(run["fmt"], o.shape) for o in outs]
    for rank in range(world):
        got, cols = play_rank(run, rank, world, blocks)
        for k, g in enumerate(got):
            together[k][:, sorted(cols)] = g[:, sorted(cols)]
    for k, (t, o) in enumerate(zip(together, outs)):
        assert (words(t) == words(o)).all(), f"{run['name']}, world {world}, block {k}: the ranks' columns together are not the oracle's block"


# ---- 1. the crossover ----
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_crossover(fmt, world):
    """TPDF_CALC, 5 trees of a trunk (LOAD_GAIN, 2 sections, STORE_MEM) and 3 ways (LOAD_MEM, 2 sections, DELAY, SAT0DB_TPDF_GAIN, STORE),
    2 ordinary chains between the trees"""
    play_world(hand_made("crossover", fmt, stp.crossover(), calc=0), world)


# ---- 2. mem_fir: the rings and hand-over rows of a slice that does not start at chain 0 ----
@pytest.mark.parametrize("fmt", [4, 6])
def test_mem_fir_trees(fmt):
    run = hand_made("mem_fir", fmt, stp.mem_fir_trees())
    assert [stp.cut_of(run["cores"][0], k, 3) for k in range(3)] == [(0, 9), (9, 7), (16, 8)]
    play_world(run, 3)


# ---- 3. a branch behind a later trunk, 17 trees: past one tile of the stage ----
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_late_branch_and_17_trees(fmt):
    """68 chains; rank 1 starts at tree 5, inside what would be the first tile (16 trees) of the whole core, and its cut has moved
    from 24 to 20 because tree 5's last branch stands behind tree 6's trunk"""
    run = hand_made("late17", fmt, stp.late_branch())
    assert [stp.cut_of(run["cores"][0], k, 3) for k in range(3)] == [(0, 20), (20, 24), (44, 24)]
    play_world(run, 3)


@pytest.mark.parametrize("fmt", [2, 6])
def test_ranks_that_come_out_empty(fmt):
    """two interleaved trees behind a TPDF_CALC: one rank holds the core, the others run nothing but the TPDF_CALC"""
    run = hand_made("interleaved", fmt, stp.interleaved(), calc=0)
    assert sorted(stp.cut_of(run["cores"][0], k, 3)[1] for k in range(3)) == [0, 0, 8]
    play_world(run, 3)


@pytest.mark.parametrize("shard_trees", [0, 1])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_an_empty_rank_of_a_treeless_core_runs_its_tpdf_calc(fmt, shard_trees):
    """no memory word anywhere, plain chain shards, whatever "shard_trees" says: core 0 is a TPDF_CALC and two chains, so rank 2 of 3 has
    no chain of it -- and still runs the TPDF_CALC, because the five dithered chains of core 1 (rank 2 runs the fifth) take their
    dither from what it leaves in the program's globals; block after block, the generator's state carried from one to the next"""
    c0 = [stp.ordinary(1), stp.ordinary(3)]
    c1 = [tp.plain(nsec=k % 3, taps=0, finish=("tpdf", "tpdf_gain")[k % 2], gain=0.95, load_gain=0.5 + 0.05 * k) for k in range(5)]
    prog, nin, nout, wd = tp.program(fmt, [tp.core(c0, calc=0), tp.core(c1)])
    k0, n0 = stp.core_of_items(c0)
    k1, n1 = stp.core_of_items(c1, n0)
    k0["mode"] = k1["mode"] = "range"
    assert n1 == nout == 7
    run = dict(name=f"treeless, format {fmt}, shard_trees {shard_trees}", fmt=fmt, prog=prog, in_stride=nin, out_stride=nout + 2, cores=[k0, k1], words=wd,
               seed=7, shard_trees=shard_trees)
    assert stp.cut_of(k0, 2, 3) == (2, 0) and stp.cut_of(k1, 2, 3) == (4, 1)
    play_world(run, 3)


# ---- 4. mid-stream: unsharded, a shard, unsharded again -- FIR histories and delay lines survive both replans ----
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_mid_stream(fmt):
    items = (stp.mem_fir_trees() if fmt != 2 else []) + stp.crossover(3)
    run = hand_made("mid-stream", fmt, items, calc=0)
    total = int(run["prog"][1])
    x, outs, states, progs = reference(run)
    r = a_runtime(run)
    cols, mine, owners, trunk_words, _ = owned(run, 1, 2)
    assert 0 < len(mine) < len(items)
    for k, (a, b) in enumerate(cut(BLOCKS)):
        what = f"{run['name']}, block {k}"
        if k == 1:
            r.set_shard(1, 2)
        got = r.run_block(x[a:a + b], run["out_stride"], IN, out=lp.sentinel(fmt, (b, run["out_stride"])))
        want = outs[k].copy()
        st = r.sync_state()
        if k == 1:
            other = [c for c in range(run["out_stride"]) if c not in cols]
            want[:, other] = lp.sentinel(fmt, (b, len(other)))
            own = state_mask(owners, mine, len(st))
            assert (st[own] == states[k][own]).all() and (st[~own] == states[0][~own]).all(), f"{what}: state"
            wantp = progs[0].copy()
            for wd in trunk_words:
                wantp[wd:wd + 2] = progs[k][wd:wd + 2]
            assert (r.buf[HEAD:total] == wantp[HEAD:]).all(), f"{what}: program words"
        else:
            assert (st == states[k]).all(), f"{what}: state: {first_bad(st, states[k])}"
            assert (r.buf[HEAD:total] == progs[k][HEAD:]).all(), f"{what}: program words"
        assert (words(got) == words(want)).all(), f"{what}: outputs"
        if k == 1:                                            # the whole program again, from the oracle's state and words where the shard left them stale
            r.set_shard(0, 1)
            r.state[:] = states[k]
            r.upload_state()
            r.buf[HEAD:total] = progs[k][HEAD:]
            r.upload_params()
    r.release()


# ---- 5. random tree programs, ranks 0 .. 2 of 3 (tests/test_shard_trees_lowering.py holds the count of runs, without a GPU) ----
@pytest.mark.parametrize("seed, fmt", stp.qualifying_runs(), ids=lambda v: str(v))
def test_random_tree_programs(seed, fmt):
    play_world(random_run(seed, fmt), RANDOM_WORLD)


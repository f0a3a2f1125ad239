"""Sharding memory-word trees, host side ("shard_trees"): the option, where dspRuntimeSetShard cuts a core of trees, what
stays refused under a shard and with which text, and what the report calls say.  Host-only: nothing here runs on a GPU."""
import pytest

from avdsp_amd import runtime as rt
from avdsp_amd import sharding as sh
from tests import copy_programs as cp
from tests import firtree_programs as tp
from tests import lowered_programs as lp
from tests import memtree_programs as mp
from tests import shard_tree_programs as stp

NOT_LOWERED = "is not lowered to the HIP path"
SHARED = "is shared with another core: not lowered to the HIP path while the core is sharded"
ALL = stp.OPTIONS + ("chain_copy",)


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in ALL:
        try:
            rt.Runtime.set_global_option(key, 0)
        except rt.AvdspError:                                  # (a library without "shard_trees")
            pass
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, prog, on=stp.OPTIONS):
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    assert r.rc >= 0
    for key in on:
        r.set_option(key, 1)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    assert r.mem_info(core_index) == (0, 0, 0)
    return r.last_error()


def tree():
    return [mp.trunk("a", 2), mp.branch("a", nsec=1, finish="sat"), mp.branch("a", nsec=0, finish="none")]


# ---- the option ----
def test_option_default_range_and_inheritance():
    r = loaded(6, mp.program(6, [mp.core(tree())])[0], on=())
    assert r.get_option("shard_trees") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("shard_trees", bad)
    assert r.get_option("shard_trees") == 0
    rt.Runtime.set_global_option("shard_trees", 1)             # the default of programs loaded later
    assert loaded(6, mp.program(6, [mp.core(tree())])[0], on=()).get_option("shard_trees") == 1


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_without_chain_mem_nothing_is_lowered(fmt):
    r = loaded(fmt, mp.program(fmt, [mp.core(tree())])[0], on=("shard_trees",))
    for rank, world in ((0, 1), (1, 2)):
        r.set_shard(rank, world)
        assert chains_of(r) == 0 and "opcode 40 (DSP_STORE_MEM) " + NOT_LOWERED in refusal(r)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_sharded_tree_core_is_lowered_and_a_change_replans(fmt):
    r = loaded(fmt, mp.program(fmt, [mp.core(tree() + [mp.plain(nsec=1, finish="sat")])])[0], on=("chain_mem", "shard_trees"))
    r.set_shard(1, 2)
    assert r.core_info()["chains"] == 4 and r.mem_info() == (1, 2, 0), r.last_error()
    assert [r.shard_info()[k] for k in ("total_chains", "first_chain", "nchains")] == [4, 3, 1]
    r.set_option("shard_trees", 0)                             # today's refusal, today's text
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} while the core is sharded" in refusal(r)
    r.set_option("shard_trees", 1)
    assert r.core_info()["chains"] == 4


# ---- the cut rule ----
def test_without_trees_the_rule_is_shard_range():
    for n in range(1, 71):
        for world in range(1, 10):
            b = sh.tree_shard_bounds(list(range(n)), world)
            assert [(b[k], b[k + 1]) for k in range(world)] == [sh.shard_range(n, world, k) for k in range(world)], (n, world)


def test_the_rule_on_hand_made_trees():
    """literal values that follow from the rule: the open positions, then the nearest one to each balanced cut (a tie: the lower)"""
    # 0 | 1 2 3 | 4 | 5 6: open 0, 1, 4, 5, 7
    t = [0, 1, 1, 1, 4, 5, 5]
    assert sh.tree_shard_bounds(t, 2) == [0, 4, 7]             # the cut at 4: open
    assert sh.tree_shard_bounds(t, 3) == [0, 4, 5, 7]          # 3 -> 4 (1 is two away); 5 is open
    assert sh.tree_shard_bounds(t, 7) == [0, 1, 1, 4, 4, 5, 5, 7]      # 2 -> 1, 3 -> 4, 6 -> 5 (a tie of 5 and 7: the lower)
    # a tree that is not adjacent closes everything between its first and its last chain: open 0, 3, 4
    assert sh.tree_shard_bounds([0, 1, 0, 3], 4) == [0, 0, 3, 3, 4]    # 1 -> 0, 2 -> 3
    # two interleaved trees: 0 and n alone are open; a cut goes to the nearer end, a tie to 0 -- one rank holds the core
    assert sh.tree_shard_bounds([0, 1, 0, 1, 0, 1, 0, 1], 2) == [0, 0, 8]
    assert sh.tree_shard_bounds([0, 1, 0, 1, 0, 1, 0], 2) == [0, 7, 7]
    assert sh.tree_shard_bounds([0, 1, 0, 1, 0, 1, 0, 1], 3) == [0, 0, 8, 8]


@pytest.mark.parametrize("name", sorted(stp.SHAPES))
def test_the_library_cuts_where_the_rule_says(name):
    """shard_info() per rank against tree_shard_bounds(); the ranks' ranges are disjoint and cover the core; no tree is split"""
    fmt = 6
    prog, _, _, _, items = stp.shape(name, fmt)
    r = loaded(fmt, prog)
    n, trees = len(items), stp.tree_of(items)
    assert r.core_info()["chains"] == n, r.last_error()
    inner_open = 0
    for world in stp.WORLDS:
        want = stp.ranges(items, world)
        got = []
        for rank in range(world):
            r.set_shard(rank, world)
            s = r.shard_info()
            assert s["total_chains"] == n, r.last_error()
            got.append((s["first_chain"], s["nchains"]))
        assert got == want, (name, world)
        assert got[0][0] == 0 and sum(m for _, m in got) == n and all(a + m == b for (a, m), (b, _) in zip(got, got[1:]))
        owner = {}
        for rank, (a, m) in enumerate(got):
            for i in range(a, a + m):
                assert owner.setdefault(trees[i], rank) == rank, f"{name}, world {world}: tree {trees[i]} is on two ranks"
        inner_open += sum(0 < a < n for a, _ in got)
    if name == "interleaved":                                  # no open position inside: one rank holds the core, the others are empty
        assert inner_open == 0
    elif n > 1:
        assert inner_open > 0


def test_a_late_branch_moves_the_cut():
    """17 trees of 1 + 3, world 3: the balanced cut 23 would go to 24, but tree 5's last branch stands at 24, behind tree 6's trunk"""
    items = stp.late_branch()
    assert len(items) == 68 and stp.ranges(items, 3) == [(0, 20), (20, 24), (44, 24)]


# ---- refusals ----
@pytest.mark.parametrize("fmt", [2, 6])
@pytest.mark.parametrize("other, lowered_alone", [
    ("constant_branch", 1),                                    # a reader core's constant branch: it is refused by the same rule
    ("interpreted_load_mem", 0),                               # a core the interpreter runs (a LOAD_MUX head beside) that reads the word with LOAD_MEM
    ("gain_word", 1),                                          # a LOAD_GAIN that takes its gain from the word
])
def test_a_word_two_cores_share(fmt, other, lowered_alone):
    if other == "constant_branch":
        c1 = mp.core([mp.branch("a", nsec=1, finish="sat")])
    elif other == "interpreted_load_mem":
        c1 = mp.core([mp.branch("a", nsec=1, finish="sat"), mp.plain(nsec=1, finish="sat", odd="mux")])
    else:
        c1 = mp.core([mp.plain(nsec=1, finish="sat", odd="gain_of", key="a")])
    prog, _, _, words = mp.program(fmt, [mp.core(tree()), c1])
    r = loaded(fmt, prog)
    assert r.core_info(0)["chains"] == 3 and chains_of(r, 1) == lowered_alone          # unsharded: as ever
    r.set_shard(0, 2)
    assert chains_of(r, 0) == 0 and f"memory word {words['a']} {SHARED}" in refusal(r, 0)
    if other == "constant_branch":
        assert chains_of(r, 1) == 0 and f"memory word {words['a']} {SHARED}" in refusal(r, 1)
    elif other == "gain_word":
        assert r.core_info(1)["chains"] == 1                   # (it holds no memory word of its own)
    r.set_shard(0, 1)
    assert r.core_info(0)["chains"] == 3


def test_a_word_of_its_own_core_alone_is_not_shared():
    """two cores, each with its own trees and a word nobody writes: nothing is shared, both are cut"""
    c0 = mp.core(tree() + [mp.branch("w0", nsec=1, finish="sat")])
    c1 = mp.core([mp.trunk("b", 1), mp.branch("b", nsec=0, finish="sat"), mp.plain(nsec=1, finish="sat")])
    r = loaded(6, mp.program(6, [c0, c1])[0])
    r.set_shard(1, 2)
    assert r.core_info(0)["chains"] == 4 and r.core_info(1)["chains"] == 3, r.last_error()
    assert (r.shard_info(0)["first_chain"], r.shard_info(0)["nchains"]) == (3, 1)
    assert (r.shard_info(1)["first_chain"], r.shard_info(1)["nchains"]) == (2, 1)


def test_lists_and_instances_keep_their_texts():
    items = [tp.trunk("a", 1, 0), tp.branch("a", nsec=1, taps=0), cp.copies([(tp.IN + 9, 40)])]
    r = loaded(6, tp.program(6, [tp.core(items)])[0], on=ALL)
    assert r.core_info()["chains"] == 2 and r.copy_info() == (1, 1), r.last_error()
    r.set_shard(0, 2)
    assert chains_of(r) == 0 and f"a LOAD_STORE list {NOT_LOWERED} while the core is sharded" in refusal(r)
    r.set_shard(0, 1)
    r2 = loaded(6, mp.program(6, [mp.core(tree())])[0])
    r2.set_shard(0, 2)
    assert r2.core_info()["chains"] == 3
    r2.set_instances(4)
    assert chains_of(r2) == 0 and f"a memory word {NOT_LOWERED} while the program has instances" in refusal(r2)
    r2.set_instances(0)
    assert r2.core_info()["chains"] == 3


# ---- the report calls under a shard (the whole core, or the chains this process runs) ----
def test_report_calls_under_a_shard():
    fmt = 6
    prog, _, _, _, items = stp.shape("crossover", fmt)
    r = loaded(fmt, prog)
    for world in (2, 3):
        for rank, (lo, m) in enumerate(stp.ranges(items, world)):
            r.set_shard(rank, world)
            mine = items[lo:lo + m]
            assert r.core_info() == dict(chains=28, max_sections=3, max_taps=0)          # the whole core
            assert r.mem_info() == tp.mem_counts(dict(items=items)) == (5, 15, 0)         # the whole core
            assert r.finish_info() == (sum(it["finish"] in ("tpdf", "tpdf_gain") for it in mine), 1)      # the rank's chains
            assert r.delay_info()[0] == sum(it["slot"] is not None for it in mine)
            s = r.shard_info()                                 # branches load no IO: the trunks' and the ordinary chains'
            first = sum(it["kind"] != "branch" for it in items[:lo])
            n_in = sum(it["kind"] != "branch" for it in mine)
            assert (s["in_io_min"], s["in_io_max"]) == (tp.IN + first, tp.IN + first + n_in - 1)
    prog, _, _, _, items = stp.shape("mem_fir", fmt)
    r = loaded(fmt, prog)
    r.set_shard(2, 3)
    assert r.mem_fir_info() == tp.fir_counts(dict(items=items)) == (4, 9, 0)              # the whole core
    assert r.core_info() == dict(chains=24, max_sections=2, max_taps=37)
    lo, m = stp.ranges(items, 3)[2]
    assert r.fir_tail_info() == (0, 0) and (r.shard_info()["first_chain"], r.shard_info()["nchains"]) == (lo, m) == (16, 8)


# ---- the random programs tests/test_gpu_shard_trees.py plays ----
def test_enough_random_programs_qualify():
    """(no GPU) the runs of seeds 0 .. 135 whose tree cores hold no LOAD_STORE list and no word another core names -- by the draw, and
    once more by the description and the words of the encoded program"""
    runs = stp.qualifying_runs()
    assert len(runs) >= 6
    for seed, fmt in runs:                                     # (every one: the encoder and describe() take a few seconds for all of them)
        _, _, _, desc = lp.random_lowered_program(seed, fmt)
        at = {}
        for ci, c in enumerate(desc["drawn"]):
            for it in c["items"]:
                if it["kind"] in ("trunk", "branch"):
                    at.setdefault(desc["words"][it["key"]], set()).add(ci)
        for ci, (c, d) in enumerate(zip(desc["drawn"], desc["cores"])):
            if c["cls"] == "tree":
                assert d["info"]["copy"] == (0, 0) and not d["reads_an_earlier_cores_word"]
                assert all(cores == {ci} for w, cores in at.items() if ci in cores)

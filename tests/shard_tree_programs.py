"""Cores for the "shard_trees" tests: memory-word trees that dspRuntimeSetShard cuts at tree boundaries.  Item lists for
tests/firtree_programs.program(); tree_of() is the rule's input as the host derives it from the lowered chains; ranges() the cut per rank
by avdsp_amd/sharding.py tree_shard_bounds().  Test infrastructure, importable without a GPU."""
from avdsp_amd import sharding as sh
from tests import firtree_programs as tp

OPTIONS = ("chain_mem", "mem_fir", "chain_finish", "chain_delay", "fir_tail", "shard_trees")
WORLDS = (2, 3, 8)
US = [63, 21, 1000, 150]                             # lines of 3, 1, 47 and 7 samples at 48 kHz


def tree_of(items):
    """per chain of a core: its tree -- the chain index of the trunk of its word, or the chain's own index"""
    trunk_at = {it["key"]: i for i, it in enumerate(items) if it["kind"] == "trunk"}
    return [trunk_at.get(it["key"], i) if it["kind"] == "branch" else i for i, it in enumerate(items)]


def ranges(items, world):
    """[(first chain, chains)] per rank"""
    b = sh.tree_shard_bounds(tree_of(items), world)
    return [(b[k], b[k + 1] - b[k]) for k in range(world)]


def way(key, k, nsec=2):
    """a crossover way: LOAD_MEM, sections, DELAY, SAT0DB_TPDF_GAIN, STORE"""
    return tp.branch(key, nsec=nsec, taps=0, slot="A", form="param" if k % 2 else "fixed", us=US[k % 4], finish="tpdf_gain", gain=0.9 + 0.01 * (k % 7))


def ordinary(k):
    return tp.plain(nsec=1 + k % 3, taps=0, finish="tpdf" if k % 2 else "sat", load_gain=None if k % 3 == 0 else 0.6)


def crossover(trees=5, ways=3, between=2):
    """the crossover as the reference writes it: per tree a trunk (LOAD_GAIN, 2 sections, STORE_MEM) and `ways` ways; `between`
    ordinary chains between two trees"""
    items = []
    for t in range(trees):
        if t:
            items += [ordinary(2 * t + j) for j in range(between)]
        items.append(tp.trunk(f"t{t}", 2, 0, 0.4 + 0.02 * t))
        items += [way(f"t{t}", t + j) for j in range(ways)]
    return items


def late_branch(trees=17, late=5):
    """trees of 1 + 3 (plain branches of 0, 1 and 2 sections); the last branch of tree `late` stands behind the next tree's trunk"""
    items, held = [], None
    for t in range(trees):
        items.append(tp.trunk(f"t{t}", (2, 0, 1)[t % 3], 0, None if t % 4 == 3 else 0.5))
        if held is not None:
            items.append(held)
            held = None
        mine = [tp.branch(f"t{t}", nsec=j, taps=0, finish=("sat", "none")[(t + j) % 2]) for j in range(3)]
        if t == late:
            held = mine.pop()
        items += mine
    return items


def interleaved(branches=3):
    """two trees whose chains alternate: no open position inside the core"""
    items = [tp.trunk("a", 2, 0), tp.trunk("b", 1, 0, None)]
    for j in range(branches):
        items += [tp.branch("a", nsec=j % 2, taps=0), tp.branch("b", nsec=1 + j % 2, taps=0, finish="none")]
    return items


def constant_alone():
    """one branch of a word nobody writes"""
    return [tp.branch("w0", nsec=1, taps=0)]


def of_length(n):
    """trees of 1 + 3, a branch of a word nobody writes between the second and the third, ordinary chains to fill up: n chains"""
    items = []
    t = 0
    while len(items) + 4 <= n - 1:
        if t == 2:
            items.append(tp.branch("w1", nsec=0, taps=0))
        items.append(tp.trunk(f"t{t}", t % 3, 0))
        items += [tp.branch(f"t{t}", nsec=(t + j) % 3, taps=0, finish=("sat", "none")[j % 2]) for j in range(3)]
        t += 1
    return items + [ordinary(k) for k in range(n - len(items))]


def mem_fir_trees():
    """4 room-correction trees (trunk: 2 sections and a 37-tap FIR; two ways) and 3 FIR-crossover trees (a plain trunk; three ways that
    are a FIR of 20 taps alone) -- formats 4 and 6"""
    items = []
    for t in range(4):
        items.append(tp.trunk(f"r{t}", 2, 37, 0.5 + 0.03 * t))
        items += [tp.branch(f"r{t}", nsec=1 + j, taps=0, finish=("sat", "none")[j]) for j in range(2)]
    for t in range(3):
        items.append(tp.trunk(f"x{t}", 1, 0, None if t == 1 else 0.7))
        items += [tp.branch(f"x{t}", nsec=0, taps=20, finish=("sat", "none", "sat")[j]) for j in range(3)]
    return items


# name -> (item list, whether it holds a FIR, whether its core begins with TPDF_CALC): the shapes the CPU tests and the layout driver share
SHAPES = {
    "crossover": (crossover, False, True),
    "late_branch": (lambda: late_branch(5, 1), False, False),
    "interleaved": (interleaved, False, False),
    "constant_alone": (constant_alone, False, False),
    "chains17": (lambda: of_length(17), False, False),
    "chains37": (lambda: of_length(37), False, False),
    "late17": (late_branch, False, False),
    "mem_fir": (mem_fir_trees, True, False),
}


def shape(name, fmt):
    """-> (program words, inputs, outputs, {key: word}, item list)"""
    make, _, calc = SHAPES[name]
    items = make()
    prog, nin, nout, words = tp.program(fmt, [tp.core(items, calc=0 if calc else None)])
    for k, (key, w) in enumerate(sorted(words.items())):    # the words nobody writes start from values of their own
        if key.startswith("w"):
            tp.set_word(prog, w, (0.31 - 0.07 * k) * (-1) ** k, 2 if fmt == 2 else 6)
    return prog, nin, nout, words, items


# ---- runs: a program, where its chains store, and how a set shard cuts every core (for the device tests) ---------------------------------
def core_of_items(items, first_out=0):
    """a hand-made core as a run's core: firtree_programs.program() gives every STORE the next output"""
    stores, k = [], first_out
    for it in items:
        stores.append(list(range(k, k + it["stores"])))
        k += it["stores"]
    return dict(chains=items, stores=stores, extra_cols=[], mode="tree"), k


def cut_of(core, rank, world):
    """(first chain, chains) of the core that `rank` of `world` runs; None: the core is not cut -- every rank runs it whole"""
    n = len(core["chains"])
    if core["mode"] == "whole":
        return None
    if core["mode"] == "tree":
        return ranges(core["chains"], world)[rank]
    lo, hi = sh.shard_range(n, world, rank)
    return lo, hi - lo


def random_run_cores(drawn):
    """the cores of a tests/lowered_programs.py draw as a run's cores.  Under a shard a core with a LOAD_STORE list or a repeated STORE
    is not lowered and runs whole on every rank, a core of pairs alone too; a tree core is cut at tree boundaries,
    every other core by shard_range"""
    from tests import copy_programs as cp
    out = []
    for c in drawn:
        lists = [it for it in c["head"] + c["items"] if it["kind"] == "copies"]
        chains = [it for it in c["items"] if it["kind"] != "copies"]
        whole = bool(lists) or not chains or any(it.get("dropped") for it in chains)
        live = cp.resolve([p for it in lists for p in it["pairs"]])
        out.append(dict(chains=chains, stores=[list(it.get("store_to") or ()) for it in chains], extra_cols=sorted(live),
                        mode="whole" if whole else "tree" if c["cls"] == "tree" else "range"))
    return out


def qualifies(drawn):
    """a draw with a tree-class core, none of which holds a LOAD_STORE list or a memory word that another core names"""
    trees = [c for c in drawn if c["cls"] == "tree"]
    for c in trees:
        if any(it["kind"] == "copies" for it in c["head"] + c["items"]):
            return False
        keys = {it["key"] for it in c["items"] if it["kind"] in ("trunk", "branch")}
        if any(keys & {it.get("key") for it in o["items"] if it["kind"] in ("trunk", "branch")} for o in drawn if o is not c):
            return False
    return bool(trees)


_RUNS = {}


def qualifying_runs(seeds=range(136), fmts=(2, 4, 6)):
    """[(seed, format)]: the random programs the device test plays as ranks 0 .. 2 of 3 (decided on the draw alone: cheap, no encoder)"""
    from tests import lowered_programs as lp
    key = (tuple(seeds), tuple(fmts))
    if key not in _RUNS:
        _RUNS[key] = [(seed, fmt) for fmt in fmts for seed in seeds if qualifies(lp.draw_cores(seed, fmt)[0])]
    return _RUNS[key]

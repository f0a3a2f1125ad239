"""Two-way COPYXY / SWAPXY forks and runs of GAIN / NEGX, host side ("chain_ways"): which cores
dspRuntimeSetOption("chain_ways", 1) lowers to the chain kernels, what dspRuntimeWaysInfo and dspRuntimeCoreInfo say of them, and which
stay with the interpreter, each with a text of its own -- with "chain_ways" 0 the texts the cores had before the option existed.
Host-only: the report calls lower a core and run nothing."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import ways_programs as wp

NOT_LOWERED = "is not lowered to the HIP path"
OPTIONS = ("chain_ways", "chain_mem", "fir_tail", "chain_delay", "chain_finish", "mux_tail", "shard_trees")


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, prog=None, ways=1, fs=48000, **off):
    """every sibling option on but those named 0 in `off`"""
    if prog is None:
        prog = wp.program(fmt, cores)[0]
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    for key in OPTIONS[1:6]:
        r.set_option(key, off.get(key, 1))
    if ways is not None:
        r.set_option("chain_ways", ways)                       # (unknown to the code before this option existed: every test here fails there)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeWaysInfo lowers it and reports zeros when it is refused)"""
    assert r.ways_info(core_index) == (0, 0)
    return r.last_error()


def a_fork(sec_a=2, sec_b=1, **kw):
    return wp.fork(wp.head(0.5), wp.way(nsec=sec_a, **kw), wp.way(nsec=sec_b))


def crossover(gain=0.7):
    """crossover2x2lfe.c:48-60: LOAD_GAIN, COPYXY, BIQUADS, SAT0DB_TPDF, DELAY, STORE, SWAPXY, BIQUADS, GAIN, SAT0DB_TPDF_GAIN, STORE"""
    return wp.fork(wp.head(0.8), wp.way(nsec=2, finish="tpdf", slot="B", us=1000), wp.way(nsec=2, ops=[("gain", gain)], finish="tpdf_gain", gain=0.9))


def test_option_default_range_and_inheritance():
    c = wp.core([a_fork(), wp.chain(nsec=1, ops=["neg"])])
    r = loaded(6, [c], ways=None)
    assert r.get_option("chain_ways") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("chain_ways", bad)
    assert r.get_option("chain_ways") == 0 and r.ways_info() == (0, 0) and chains_of(r) == 0
    rt.lib().dspRuntimeRelease()
    rt.Runtime.set_global_option("chain_ways", 1)              # set without a program: the default of programs loaded later
    prog = wp.program(6, [c])[0]
    r1 = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    assert r1.get_option("chain_ways") == 1 and r1.core_info()["chains"] == 3 and r1.ways_info() == (1, 1)
    r2 = rt.Runtime(6, prog.copy(), fs=48000, random=1, dither=24)     # a second context: the options are copied ...
    assert r2.get_option("chain_ways") == 1 and r2.ways_info() == (1, 1)
    r2.set_option("chain_ways", 0)                             # ... and each context keeps its own
    assert r2.ways_info() == (0, 0) and chains_of(r2) == 0 and r1.get_option("chain_ways") == 1 and r1.ways_info() == (1, 1)
    r2.set_option("chain_ways", 1)                             # (a change replans: on again)
    assert r2.ways_info() == (1, 1) and r2.core_info()["chains"] == 3


@pytest.mark.parametrize("fmt", [2, 3, 4, 5, 6])
def test_option_0_keeps_the_old_texts(fmt):
    """the generic text for every X/Y opcode, GAIN and NEGX, and the "X/Y tricks" text, as before the option existed"""
    def text_of(items):
        r = loaded(fmt, [wp.core(items)], ways=0)
        assert chains_of(r) == 0
        return refusal(r)
    assert "opcode 12 (DSP_COPYXY) " + NOT_LOWERED in text_of([a_fork()])
    assert "opcode 11 (DSP_SWAPXY) " + NOT_LOWERED in text_of([wp.raw([("load", None), ("sat",), ("store",), ("swapxy",), ("store",)])])
    assert "opcode 41 (DSP_GAIN) " + NOT_LOWERED in text_of([wp.chain(nsec=1, ops=[("gain", 0.5)])])
    assert "opcode 23 (DSP_NEGX) " + NOT_LOWERED in text_of([wp.chain(nsec=1, ops=["neg"])])
    assert "(DSP_SUBYX) " + NOT_LOWERED in text_of([wp.raw([("load", None), ("xy", "SUBYX"), ("store",)])])
    assert "value replaced before any STORE (X/Y tricks are not lowered)" in text_of([wp.raw([("load", None), ("load", None), ("store",)])])


@pytest.mark.parametrize("fmt", [2, 3, 4, 5, 6])
def test_plain_forks_in_every_format(fmt):
    items = [a_fork(2, 1), wp.chain(nsec=1), a_fork(0, 17), wp.fork(wp.head(None), wp.way(nsec=1, finish="none", stores=2), wp.way(nsec=0))]
    c = wp.core(items)
    r = loaded(fmt, [c])
    assert r.core_info() == dict(chains=7, max_sections=17, max_taps=0), r.last_error()
    assert r.ways_info() == (3, 0) == wp.counts(c)[0] and wp.counts(c)[1] == 7
    s = r.shard_info()
    assert (s["total_chains"], s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (7, wp.IN, wp.IN + 3, 0, 7)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_crossover_shape_and_what_a_way_may_be(fmt):
    """dressed finishes, a DELAY in slot A and B (both forms), a FIR in a way (formats 4 and 6), NOPs between head and COPYXY"""
    fir = 33 if fmt != 2 else 0
    items = [crossover(), wp.fork(wp.head(None), wp.way(nsec=1, slot="A", form="param", us=63, finish="gain"), wp.way(nsec=0, taps=fir, finish="sat")),
             wp.raw([("load", 0.5), ("nop",), ("copyxy",), ("nop",), ("biquads", 1), ("store",), ("nop",), ("swapxy",), ("nop",), ("sat",), ("store",)])]
    c = wp.core(items, calc=0)
    r = loaded(fmt, [c])
    assert r.core_info() == dict(chains=6, max_sections=2, max_taps=fir), r.last_error()
    assert r.ways_info() == (3, 1) and r.delay_info() == (2, wp.samples(1000)) and r.finish_info() == (3, 1)
    assert r.fir_tail_info() == (0, 0)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_load_mem_head_makes_two_branches(fmt):
    items = [wp.trunk("a", 2), wp.fork(wp.head(key="a"), wp.way(nsec=1), wp.way(nsec=0, ops=["neg"])), wp.fork(wp.head(key="w"), wp.way(nsec=0), wp.way(nsec=1))]
    c = wp.core(items)
    r = loaded(fmt, [c])
    assert r.core_info() == dict(chains=5, max_sections=2, max_taps=0), r.last_error()
    assert r.ways_info() == (2, 1) and r.mem_info() == (1, 4, 2)
    r.set_option("chain_mem", 0)                               # (the head is "chain_mem"'s)
    assert chains_of(r) == 0 and "(DSP_STORE_MEM) " + NOT_LOWERED in refusal(r)


OPS4 = [("gain", 0.5), "neg", ("gain", -1.25), "neg"]


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_ops_runs(fmt):
    """runs of 1, 2 and 4; with and without sections, delay and dressed finish; in both ways of a fork; on a branch without sections"""
    items = [wp.chain(nsec=2, ops=[("gain", 0.5)]), wp.chain(nsec=0, ops=["neg", ("gain", 0.0)], load_gain=None), wp.chain(nsec=17, ops=OPS4, slot="A", us=1000, finish="tpdf_gain"),
             wp.chain(nsec=0, ops=OPS4, slot="B", us=63, finish="tpdf"), wp.fork(wp.head(0.9), wp.way(nsec=0, ops=["neg"]), wp.way(nsec=1, ops=[("gain", 1.0)])),
             wp.trunk("a", 1), wp.chain(key="a", nsec=0, ops=[("gain", -0.5)]), wp.chain(key="a", nsec=0), wp.chain(nsec=1)]
    c = wp.core(items, calc=0)
    r = loaded(fmt, [c])
    assert r.core_info() == dict(chains=10, max_sections=17, max_taps=0), r.last_error()
    assert r.ways_info() == (1, 7) == wp.counts(c)[0] and r.delay_info() == (2, wp.samples(1000)) and r.mem_info() == (1, 2, 0)


FORK_REFUSALS = {
    "copyxy_not_behind_a_head": ([("load", None), ("biquads", 1), ("copyxy",), ("store",), ("swapxy",), ("store",)], "a COPYXY that is not directly behind a chain head " + NOT_LOWERED),
    "copyxy_in_front_of_any_head": ([("copyxy",), ("load", None), ("store",)], "a COPYXY that is not directly behind a chain head " + NOT_LOWERED),
    "copyxy_without_swapxy_then_a_head": ([("load", None), ("copyxy",), ("store",), ("load", None), ("store",)], "a COPYXY without a SWAPXY in its chain " + NOT_LOWERED),
    "copyxy_without_swapxy_at_the_end": ([("load", None), ("copyxy",), ("store",)], "a COPYXY without a SWAPXY in its chain " + NOT_LOWERED),
    "swapxy_without_copyxy": ([("load", None), ("store",), ("swapxy",), ("store",)], "a SWAPXY without a COPYXY behind its chain's head " + NOT_LOWERED),
    "swapxy_before_a_store": ([("load", None), ("copyxy",), ("biquads", 1), ("swapxy",), ("store",)], "a SWAPXY before way A's first STORE " + NOT_LOWERED),
    "second_swapxy": ([("load", None), ("copyxy",), ("store",), ("swapxy",), ("store",), ("swapxy",), ("store",)], "a second SWAPXY in one chain " + NOT_LOWERED),
    "second_copyxy_in_way_a": ([("load", None), ("copyxy",), ("copyxy",), ("store",), ("swapxy",), ("store",)], "a second COPYXY in one chain " + NOT_LOWERED),
    "second_copyxy_in_way_b": ([("load", None), ("copyxy",), ("store",), ("swapxy",), ("copyxy",), ("store",)], "a second COPYXY in one chain " + NOT_LOWERED),
    "store_mem_in_way_a": ([("load", None), ("copyxy",), ("store_mem", "a"), ("load", None), ("store",)], "a STORE_MEM in a way of a COPYXY / SWAPXY fork " + NOT_LOWERED),
    "store_mem_in_way_b": ([("load", None), ("copyxy",), ("store",), ("swapxy",), ("store_mem", "a")], "a STORE_MEM in a way of a COPYXY / SWAPXY fork " + NOT_LOWERED),
    "load_mux_head": ([("load_mux",), ("copyxy",), ("store",), ("swapxy",), ("store",)], "a COPYXY behind a LOAD_MUX head " + NOT_LOWERED),
    "way_b_never_stored": ([("load", None), ("copyxy",), ("store",), ("swapxy",), ("sat",)], "core ends with a chain that is never stored"),
}


# (memory words and LOAD_MUX have format refusals of their own in formats 3 and 5)
@pytest.mark.parametrize("fmt, case", [(f, c) for c in sorted(FORK_REFUSALS) for f in (3, 6) if f == 6 or not ("store_mem" in c or "load_mux" in c)])
def test_fork_refusals(fmt, case):
    steps, text = FORK_REFUSALS[case]
    r = loaded(fmt, [wp.core([wp.raw(steps)])])
    assert chains_of(r) == 0
    assert text in refusal(r), r.last_error()


@pytest.mark.parametrize("name", wp.XY)
def test_every_other_xy_opcode_is_refused_by_name(name):
    r = loaded(6, [wp.core([wp.raw([("load", None), ("copyxy",), ("store",), ("swapxy",), ("xy", name), ("store",)])])])
    assert chains_of(r) == 0
    t = refusal(r)
    assert f"(DSP_{name}) " + NOT_LOWERED in t and "of the X/Y opcodes only the COPYXY and SWAPXY of a two-way fork are" in t and t.startswith("word ")


OP_REFUSALS = {
    "gain_in_front_of_biquads": (6, [("load", None), ("gain", 0.5), ("biquads", 1), ("store",)], "a GAIN or NEGX in front of a BIQUADS " + NOT_LOWERED),
    "the_crossoverLV6_form": (6, [("load", None), ("copyxy",), ("biquads", 1), ("store",), ("swapxy",), ("gain", 0.5), ("biquads", 1), ("store",)], "a GAIN or NEGX in front of a BIQUADS " + NOT_LOWERED),
    "negx_behind_a_delay": (6, [("load", None), ("biquads", 1), ("delay", 1000), ("neg",), ("store",)], "a NEGX behind a DSP_DELAY, a SAT0DB or a STORE " + NOT_LOWERED),
    "gain_behind_a_sat0db": (4, [("load", None), ("sat",), ("gain", 0.5), ("store",)], "a GAIN behind a DSP_DELAY, a SAT0DB or a STORE " + NOT_LOWERED),
    "gain_behind_a_store": (2, [("load", None), ("store",), ("gain", 0.5), ("store",)], "a GAIN behind a DSP_DELAY, a SAT0DB or a STORE " + NOT_LOWERED),
    "five_in_a_run": (6, [("load", None), ("neg",), ("gain", 0.5), ("neg",), ("neg",), ("gain", 0.5), ("store",)], "more than 4 GAIN / NEGX in a run"),
    "behind_a_fir": (6, [("load", None), ("fir", 8), ("gain", 0.5), ("store",)], "a GAIN in a chain with a DSP_FIR " + NOT_LOWERED),
    "in_front_of_a_fir": (4, [("load", None), ("neg",), ("fir", 8), ("store",)], "a GAIN or NEGX in a chain with a DSP_FIR " + NOT_LOWERED),
    "load_mux_head": (6, [("load_mux",), ("gain", 0.5), ("store",)], "a GAIN in a chain with a LOAD_MUX head " + NOT_LOWERED),
    "beside_a_load_mux_head": (6, [("load_mux",), ("store",), ("load", None), ("neg",), ("store",)], "a GAIN or NEGX in a core with LOAD_MUX heads " + NOT_LOWERED),
    "in_a_trunk": (6, [("load", None), ("biquads", 1), ("gain", 0.5), ("store_mem", "a"), ("load_mem", "a"), ("store",)], "a GAIN or NEGX in a trunk (a chain that ends in STORE_MEM) " + NOT_LOWERED),
    "format_3": (3, [("load", None), ("gain", 0.5), ("store",)], f"a GAIN {NOT_LOWERED} in format 3"),
    "format_5": (5, [("load", None), ("neg",), ("store",)], f"a NEGX {NOT_LOWERED} in format 5"),
    "in_front_of_the_load": (6, [("neg",), ("load", None), ("store",)], "a NEGX in front of the chain's LOAD " + NOT_LOWERED),
}


@pytest.mark.parametrize("case", sorted(OP_REFUSALS))
def test_way_operation_refusals(case):
    fmt, steps, text = OP_REFUSALS[case]
    r = loaded(fmt, [wp.core([wp.raw(steps)])])
    assert chains_of(r) == 0
    assert text in refusal(r), r.last_error()


def test_what_the_refusals_refuse_is_lowered_when_put_right():
    """the same opcodes in the supported order"""
    r = loaded(6, [wp.core([wp.raw([("load", None), ("copyxy",), ("biquads", 1), ("gain", 0.5), ("store",), ("swapxy",), ("biquads", 1), ("neg",), ("delay", 1000), ("sat",), ("store",)])])])
    assert r.core_info()["chains"] == 2 and r.ways_info() == (1, 2) and r.delay_info() == (1, 47)


@pytest.mark.parametrize("which", ["gain_offset_past_the_program", "gain_offset_in_front_of_the_program", "short_gain"])
@pytest.mark.parametrize("fmt", [2, 6])
def test_damaged_payloads_are_refused_not_followed(fmt, which):
    prog = wp.program(fmt, [wp.core([wp.chain(nsec=1, ops=[("gain", 0.5)]), wp.chain(nsec=1)])])[0].copy()
    at = wp.words_of(prog, wp.OP_GAIN)[0]
    if which == "gain_offset_past_the_program":
        prog[at + 1] = int(prog[1]) - at                       # the first word behind the program
        text = "outside the program"
    elif which == "gain_offset_in_front_of_the_program":
        prog[at + 1] = np.uint32(-(at + 1) & 0xFFFFFFFF)
        text = "outside the program"
    else:
        # a GAIN of one word: its payload is the next opcode's.  (The opcode stream stays walkable: the old payload word becomes a NOP)
        skip = int(prog[at]) & 0xFFFF
        prog[at] = (wp.OP_GAIN << 16) | 1
        for k in range(1, skip):
            prog[at + k] = 1                                   # DSP_NOP, one word
        text = "opcode payload shorter than 1 words"
    wp.resealed(prog)
    r = loaded(fmt, None, prog=prog)
    assert r.ways_info() == (0, 0)
    assert text in r.last_error(), r.last_error()
    assert chains_of(r) == 0


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_memory_word_on_a_gain_parameter(fmt):
    """a GAIN that takes its parameter from a word a trunk of the core writes: the launch would read the gain the host recorded"""
    items = [wp.trunk("a", 1), wp.chain(key="a", nsec=1), wp.raw([("load", None), ("biquads", 1), ("gain_of", "a"), ("store",)])]
    r = loaded(fmt, [wp.core(items)])
    assert chains_of(r) == 0 and "is read as a parameter by another opcode of the core" in refusal(r)
    r = loaded(fmt, [wp.core(items[1:])])                      # (nobody writes the word here: an ordinary parameter)
    assert chains_of(r) == 0 and "is read as a parameter by another opcode of the core" in refusal(r)
    r = loaded(fmt, [wp.core(items[2:])])
    assert r.core_info()["chains"] == 1 and r.ways_info() == (0, 1)


def test_instances():
    """forks are ordinary chains to the instances; way operations have no instance form"""
    r = loaded(6, [wp.core([a_fork(), wp.chain(nsec=1)])], chain_delay=0, chain_finish=0, chain_mem=0)
    r.set_instances(4)
    assert r.core_info()["chains"] == 3 and r.ways_info() == (1, 0), r.last_error()
    r.set_instances(0)
    r = loaded(6, [wp.core([wp.chain(nsec=1, ops=[("gain", 0.5)]), a_fork()])])
    assert r.ways_info() == (1, 1)
    r.set_instances(4)
    assert chains_of(r) == 0 and f"a GAIN {NOT_LOWERED} while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.core_info()["chains"] == 3 and r.ways_info() == (1, 1)


def test_shards_cut_between_ways():
    """three forks and an ops chain, 7 chains over 3 ranks: a fork counts where one of its ways runs"""
    c = wp.core([a_fork(), a_fork(1, 1), wp.chain(nsec=1, ops=["neg"]), a_fork(0, 2)])
    r = loaded(6, [c])
    assert r.core_info()["chains"] == 7 and r.ways_info() == (3, 1)
    seen = []
    for rank in range(3):
        r.set_shard(rank, 3)
        s = r.shard_info()
        lo, hi = s["first_chain"], s["first_chain"] + s["nchains"]
        forks = sum(1 for a in (0, 2, 5) if a + 1 >= lo and a < hi)
        assert r.ways_info() == (forks, int(lo <= 4 < hi)), (rank, s)
        seen.append((lo, hi))
    assert seen[0][0] == 0 and seen[-1][1] == 7 and all(seen[k][1] == seen[k + 1][0] for k in range(2))
    assert any(lo % 2 or hi in (1, 3, 6) for lo, hi in seen)      # (a cut inside a fork: its ways on two ranks)
    r.set_shard(0, 1)


def test_shard_trees_keeps_a_load_mem_fork_on_one_rank():
    items = [wp.trunk("a", 1), wp.fork(wp.head(key="a"), wp.way(nsec=1), wp.way(nsec=0)), wp.trunk("b", 0), wp.fork(wp.head(key="b"), wp.way(nsec=0, ops=["neg"]), wp.way(nsec=2))]
    r = loaded(6, [wp.core(items)])
    r.set_option("shard_trees", 1)
    assert r.core_info()["chains"] == 6 and r.ways_info() == (2, 1)
    for rank in range(2):
        r.set_shard(rank, 2)
        s = r.shard_info()
        assert (s["first_chain"], s["nchains"]) == (3 * rank, 3) and r.ways_info() == (1, rank), r.last_error()
    r.set_shard(0, 1)

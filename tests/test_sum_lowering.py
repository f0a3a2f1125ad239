"""Sum heads, host side ("chain_sum"): which cores dspRuntimeSetOption("chain_sum", 1) lowers to the chain kernels, what
dspRuntimeSumInfo, dspRuntimeMemInfo and dspRuntimeCoreInfo say of them, and which stay with the interpreter, each with a text of its
own -- with "chain_sum" 0 the texts the cores had before the option existed.  Host-only: the report calls lower a core and run
nothing."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import sum_programs as sp
from tests import ways_programs as wp

NOT_LOWERED = "is not lowered to the HIP path"
OPTIONS = ("chain_sum", "chain_mem", "fir_tail", "chain_delay", "chain_finish", "mem_fir", "chain_ways", "shard_trees")
OP_LOAD_MEM = 39                                     # include/avdsp_format.h


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, prog=None, sum_=1, fs=48000, **off):
    """every sibling option on but those named 0 in `off`"""
    if prog is None:
        prog = sp.program(fmt, cores)[0]
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    for key in OPTIONS[1:7]:
        r.set_option(key, off.get(key, 1))
    if sum_ is not None:
        r.set_option("chain_sum", sum_)                        # (unknown to the code before this option existed: every test here fails there)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeSumInfo lowers it and reports zeros when it is refused)"""
    assert r.sum_info(core_index) == (0, 0)
    return r.last_error()


def lfe_items():
    return [sp.trunk("a", 2), sp.trunk("b", 0), sp.bus(["a", "b"], ["ADDXY"], nsec=1, finish="sat", slot="B", us=1000)]


def test_option_default_range_inheritance_copy_and_toggle():
    c = sp.core(lfe_items())
    r = loaded(6, [c], sum_=None)
    assert r.get_option("chain_sum") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("chain_sum", bad)
    assert r.get_option("chain_sum") == 0 and r.sum_info() == (0, 0) and chains_of(r) == 0
    rt.lib().dspRuntimeRelease()
    for key in ("chain_mem", "chain_delay", "chain_sum"):      # set without a program: the default of programs loaded later
        rt.Runtime.set_global_option(key, 1)
    prog = sp.program(6, [c])[0]
    r1 = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    assert r1.get_option("chain_sum") == 1 and r1.core_info()["chains"] == 3 and r1.sum_info() == (1, 2)
    r2 = rt.Runtime(6, prog.copy(), fs=48000, random=1, dither=24)     # a second context: the options are copied ...
    assert r2.get_option("chain_sum") == 1 and r2.sum_info() == (1, 2)
    r2.set_option("chain_sum", 0)                              # ... and each context keeps its own
    assert r2.sum_info() == (0, 0) and chains_of(r2) == 0 and r1.get_option("chain_sum") == 1 and r1.sum_info() == (1, 2)
    r2.set_option("chain_sum", 1)                              # (a change replans: on again)
    assert r2.sum_info() == (1, 2) and r2.core_info()["chains"] == 3


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_option_without_chain_mem_does_nothing(fmt):
    r = loaded(fmt, [sp.core(lfe_items())], chain_mem=0)
    assert r.get_option("chain_sum") == 1 and chains_of(r) == 0
    assert "(DSP_STORE_MEM) " + NOT_LOWERED in refusal(r)
    r.set_option("chain_mem", 1)
    assert r.sum_info() == (1, 2)


@pytest.mark.parametrize("fmt", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("ways", [0, 1])
def test_option_0_keeps_the_old_texts(fmt, ways):
    def text_of(items):
        r = loaded(fmt, [sp.core(items)], sum_=0, chain_ways=ways)
        assert chains_of(r) == 0
        return refusal(r)
    xy = "of the X/Y opcodes only the COPYXY and SWAPXY of a two-way fork are" if ways else "opcode"
    for name in ("ADDXY", "SUBXY"):
        t = text_of([sp.raw([("load", None), ("xy", name), ("store",)])])
        assert f"(DSP_{name}) " + NOT_LOWERED in t and xy in t
    if fmt in (3, 5):
        assert f"a memory word {NOT_LOWERED} in format {fmt}" in text_of(lfe_items())
    else:
        assert "value replaced before any STORE (X/Y tricks are not lowered)" in text_of(lfe_items())


@pytest.mark.parametrize("fmt", [3, 5])
def test_formats_3_and_5_keep_their_texts_with_the_option_on(fmt):
    r = loaded(fmt, [sp.core(lfe_items())])
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} in format {fmt}" in refusal(r)
    r = loaded(fmt, [sp.core([sp.raw([("load", None), ("xy", "ADDXY"), ("store",)])])])
    assert chains_of(r) == 0 and "(DSP_ADDXY) " + NOT_LOWERED in refusal(r)


SHAPES = {
    # items -> sum_info, mem_info, chains
    "lfe": (lfe_items, (1, 2), (2, 1, 0), 3),
    "three_terms_one_sub": (lambda: [sp.trunk("a", 1), sp.trunk("b", 17), sp.bus(["a", "b", "w"], ["SUBXY", "ADDXY"], nsec=0, finish="none")], (1, 3), (2, 1, 0), 3),
    "eight_terms": (lambda: [sp.trunk("a", 1), sp.bus(["a", "w1", "w2", "a", "w3", "w4", "w5", "a"], ["ADDXY", "SUBXY"] * 3 + ["ADDXY"], nsec=2)], (1, 8), (1, 1, 0), 2),
    "constants_alone": (lambda: [sp.bus(["u", "v"], ["SUBXY"], nsec=0, finish="tpdf"), sp.chain(nsec=1)], (1, 2), (0, 1, 0), 2),
    "beside_branches": (lambda: [sp.trunk("a", 2), sp.chain(key="a", nsec=1), sp.chain(key="w", nsec=0), sp.bus(["a", "w"], ["ADDXY"], nsec=0, way_ops=[("gain", 0.7), "neg"]),
                                 sp.bus(["w", "a"], ["SUBXY"], nsec=0, slot="A", us=63)], (2, 4), (1, 4, 1), 5),
    "nops_between": (lambda: [sp.trunk("a", 0), sp.raw([("load_mem", "a"), ("nop",), ("load_mem", "w"), ("nop",), ("xy", "ADDXY"), ("nop",), ("load_mem", "a"), ("xy", "SUBXY"),
                                                         ("nop",), ("biquads", 1), ("store",)])], (1, 3), (1, 1, 0), 2),
}


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_what_the_reports_say(fmt, shape):
    items, sums, mem, chains = SHAPES[shape]
    c = sp.core(items(), calc=0)
    r = loaded(fmt, [c])
    assert r.sum_info() == sums, r.last_error()
    assert r.mem_info() == mem and r.core_info()["chains"] == chains
    if shape != "nops_between":
        got = sp.counts(c)
        assert (got[0], got[2], got[3]) == (sums, mem[:2], chains) and r.ways_info() == got[1]


@pytest.mark.parametrize("fmt", [4, 6])
def test_a_lone_fir_behind_the_head(fmt):
    r = loaded(fmt, [sp.core([sp.trunk("a", 1), sp.bus(["a", "w"], ["ADDXY"], nsec=0, taps=33)])])
    assert r.sum_info() == (1, 2) and r.core_info() == dict(chains=2, max_sections=1, max_taps=33) and r.mem_fir_info() == (0, 1, 0), r.last_error()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_lfe_program_is_lowered_whole(fmt):
    prog, nin, nout, words, c = sp.lfe_program(fmt)
    r = loaded(fmt, None, prog=prog)
    assert r.sum_info() == (1, 2) and r.ways_info() == (2, 2) and r.mem_info() == (2, 1, 0), r.last_error()
    assert r.core_info() == dict(chains=7, max_sections=6, max_taps=0) and (nin, nout) == (4, 5)
    assert r.delay_info()[0] == 3 and r.finish_info()[0] == 4
    r.set_option("chain_sum", 0)
    assert chains_of(r) == 0 and "value replaced before any STORE (X/Y tricks are not lowered)" in refusal(r)


A, B = ("load_mem", "a"), ("load_mem", "b")
TRUNKS = [("load", 0.5), ("biquads", 1), ("store_mem", "a"), ("load", None), ("store_mem", "b")]
REFUSALS = {
    "no_addxy_then_store": (TRUNKS + [A, B, ("store",)], "behind a LOAD_MEM head without its ADDXY or SUBXY " + NOT_LOWERED),
    "no_addxy_then_biquads": (TRUNKS + [A, B, ("biquads", 1), ("xy", "ADDXY"), ("store",)], "behind a LOAD_MEM head without its ADDXY or SUBXY " + NOT_LOWERED),
    "no_addxy_then_a_third_load": (TRUNKS + [A, B, A, ("xy", "ADDXY"), ("store",)], "behind a LOAD_MEM head without its ADDXY or SUBXY " + NOT_LOWERED),
    "no_addxy_at_the_end": (TRUNKS + [A, ("store",), A, B], "behind a LOAD_MEM head without its ADDXY or SUBXY " + NOT_LOWERED),
    "no_addxy_behind_a_term": (TRUNKS + [A, B, ("xy", "ADDXY"), A, ("store",)], "behind a LOAD_MEM head without its ADDXY or SUBXY " + NOT_LOWERED),
    "addxy_behind_a_load": ([("load", None), ("xy", "ADDXY"), ("store",)], "an ADDXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "subxy_behind_a_load_gain": ([("load", 0.5), ("xy", "SUBXY"), ("store",)], "an SUBXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "addxy_behind_the_head_alone": (TRUNKS + [A, ("xy", "ADDXY"), ("store",)], "an ADDXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "addxy_twice": (TRUNKS + [A, B, ("xy", "ADDXY"), ("xy", "ADDXY"), ("store",)], "an ADDXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "addxy_behind_banks": (TRUNKS + [A, ("biquads", 1), B, ("xy", "ADDXY"), ("store",)], "value replaced before any STORE (X/Y tricks are not lowered)"),
    "subxy_behind_banks_of_a_load": ([("load", None), ("biquads", 1), ("xy", "SUBXY"), ("store",)], "an SUBXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "addxy_in_way_a": ([("load", None), ("copyxy",), ("xy", "ADDXY"), ("store",), ("swapxy",), ("store",)], "an ADDXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "a_term_in_way_b": (TRUNKS + [A, ("copyxy",), ("store",), ("swapxy",), B, ("xy", "ADDXY"), ("store",)], "value replaced before any STORE (X/Y tricks are not lowered)"),
    "addxy_in_way_b": (TRUNKS + [A, ("copyxy",), ("store",), ("swapxy",), ("xy", "ADDXY"), ("store",)], "an ADDXY that does not stand directly behind a LOAD_MEM behind a LOAD_MEM head (a sum head) " + NOT_LOWERED),
    "a_ninth_word": ([A] + [B, ("xy", "ADDXY")] * 8 + [("store",)], "a sum head of more than 8 memory words"),
    "copyxy_behind_a_sum_head": (TRUNKS + [A, B, ("xy", "ADDXY"), ("copyxy",), ("store",), ("swapxy",), ("store",)], "a COPYXY behind a sum head"),
    "copyxy_behind_its_banks": (TRUNKS + [A, B, ("xy", "SUBXY"), ("biquads", 1), ("copyxy",), ("store",), ("swapxy",), ("store",)], "a COPYXY behind a sum head"),
    "swapxy_behind_a_sum_head": (TRUNKS + [A, B, ("xy", "ADDXY"), ("store",), ("swapxy",), ("store",)], "a SWAPXY without a COPYXY behind its chain's head " + NOT_LOWERED),
    "store_mem_in_the_chain": (TRUNKS + [A, B, ("xy", "ADDXY"), ("biquads", 1), ("store_mem", "c"), ("load_mem", "c"), ("store",)],
                               "a STORE_MEM in a chain that starts with LOAD_MEM " + NOT_LOWERED),
    "a_term_in_front_of_its_trunk": ([("load", None), ("store_mem", "a"), A, B, ("xy", "ADDXY"), ("store",), ("load", None), ("store_mem", "b")],
                                     "a term of a sum head in front of the STORE_MEM of its word (the one-frame-lag form) " + NOT_LOWERED),
    "the_head_in_front_of_its_trunk": ([("load", None), ("store_mem", "b"), A, B, ("xy", "ADDXY"), ("store",), ("load", None), ("store_mem", "a")],
                                       "a LOAD_MEM in front of the STORE_MEM of its word (the one-frame-lag form) " + NOT_LOWERED),
    "never_stored": (TRUNKS + [A, B, ("xy", "ADDXY"), ("sat",)], "core ends with a chain that is never stored"),
}
OTHER_XY = [n for n in wp.XY if n not in ("ADDXY", "SUBXY")]


@pytest.mark.parametrize("fmt", [2, 6])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(fmt, case):
    steps, text = REFUSALS[case]
    r = loaded(fmt, [sp.core([sp.raw(steps)])])
    assert chains_of(r) == 0
    t = refusal(r)
    assert text in t, t
    assert "word " in t or t.startswith("core ends")           # (each names the word it stands at)


@pytest.mark.parametrize("ways", [0, 1])
@pytest.mark.parametrize("name", OTHER_XY)
def test_every_other_xy_opcode_keeps_its_text(name, ways):
    r = loaded(6, [sp.core([sp.raw(TRUNKS + [A, B, ("xy", name), ("store",)])])], chain_ways=ways)
    assert chains_of(r) == 0
    t = refusal(r)
    assert "behind a LOAD_MEM head without its ADDXY or SUBXY " + NOT_LOWERED in t       # (the term's LOAD_MEM is what is refused)
    r =loaded(6, [sp.core([sp.raw(TRUNKS + [A, B, ("xy", "ADDXY"), ("xy", name), ("store",)])])], chain_ways=ways)
    t = refusal(r)
    assert f"(DSP_{name}) " + NOT_LOWERED in t
    assert ("of the X/Y opcodes only the COPYXY and SWAPXY of a two-way fork are" in t) == bool(ways)


@pytest.mark.parametrize("fmt", [2, 6])
def test_term_words_are_held_to_the_rules_of_memory_words(fmt):
    """overlap, the parameter-read rule (a GAIN parameter), and what the refusals refuse put right"""
    prog, _, _, wd = sp.program(fmt, [sp.core([sp.trunk("a", 1), sp.trunk("b", 0), sp.bus(["a", "b"], ["ADDXY"], nsec=1)])])
    r = loaded(fmt, None, prog=prog)
    assert r.sum_info() == (1, 2)
    # the term's offset one word on: it overlaps word b (and the word behind it)
    prog = prog.copy()
    at = wp.words_of(prog, OP_LOAD_MEM)[1]
    assert at + int(np.int32(prog[at + 1])) == wd["b"]
    prog[at + 1] += 1
    wp.resealed(prog)
    r = loaded(fmt, None, prog=prog)
    assert chains_of(r) == 0
    t = refusal(r)
    assert "overlap without being the same word" in t or "is not a free word of a PARAM section" in t, t
    items = [sp.trunk("a", 1), sp.bus(["a", "g"], ["ADDXY"], nsec=0), sp.raw([("load", None), ("biquads", 1), ("gain_of", "g"), ("store",)])]
    r = loaded(fmt, [sp.core(items)])
    assert chains_of(r) == 0 and "memory word" in refusal(r) and "is read as a parameter by another opcode of the core" in refusal(r)
    r = loaded(fmt, [sp.core(items[:2])])
    assert r.sum_info() == (1, 2)


@pytest.mark.parametrize("which", ["term_offset_past_the_program", "term_offset_in_front_of_the_program", "term_on_the_opcode_stream", "short_term"])
@pytest.mark.parametrize("fmt", [2, 6])
def test_damaged_payloads_are_refused_not_followed(fmt, which):
    prog = sp.program(fmt, [sp.core([sp.trunk("a", 1), sp.bus(["a", "w"], ["ADDXY"], nsec=1), sp.chain(nsec=1)])])[0].copy()
    at = wp.words_of(prog, OP_LOAD_MEM)[1]
    if which == "term_offset_past_the_program":
        prog[at + 1] = int(prog[1]) - at - 1                   # its second word is the first behind the program
        text = "outside the program"
    elif which == "term_offset_in_front_of_the_program":
        prog[at + 1] = np.uint32(-(at + 1) & 0xFFFFFFFF)
        text = "outside the program"
    elif which == "term_on_the_opcode_stream":
        prog[at + 1] = 2                                       # the ADDXY behind it
        text = "is not a free word of a PARAM section"
    else:
        # a LOAD_MEM of one word: its payload is the next opcode's.  (The opcode stream stays walkable: the old payload word becomes a NOP)
        skip = int(prog[at]) & 0xFFFF
        prog[at] = (OP_LOAD_MEM << 16) | 1
        for k in range(1, skip):
            prog[at + k] = 1                                   # DSP_NOP, one word
        text = "opcode payload shorter than 1 words"
    wp.resealed(prog)
    r = loaded(fmt, None, prog=prog)
    assert r.sum_info() == (0, 0)
    assert text in r.last_error(), r.last_error()
    assert chains_of(r) == 0


def test_instances():
    r = loaded(6, [sp.core(lfe_items())])
    assert r.sum_info() == (1, 2)
    r.set_instances(4)
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.sum_info() == (1, 2) and r.core_info()["chains"] == 3


@pytest.mark.parametrize("trees", [0, 1])
def test_shards(trees):
    """a sharded core keeps no sum head, under "shard_trees" too; the same core without its bus is cut at tree boundaries as ever"""
    items = lfe_items() + [sp.chain(key="a", nsec=1), sp.chain(nsec=1)]
    r = loaded(6, [sp.core(items)])
    r.set_option("shard_trees", trees)
    assert r.sum_info() == (1, 2) and r.core_info()["chains"] == 5
    r.set_shard(1, 2)
    assert chains_of(r) == 0
    t = refusal(r)
    assert (f"a sum head (LOAD_MEM, LOAD_MEM of word" in t and "while the core is sharded" in t) if trees else f"a memory word {NOT_LOWERED} while the core is sharded" in t
    r.set_shard(0, 1)
    assert r.sum_info() == (1, 2)
    r = loaded(6, [sp.core(items[:2] + items[3:])])
    r.set_option("shard_trees", 1)
    r.set_shard(1, 2)
    assert r.core_info()["chains"] == 4 and r.sum_info() == (0, 0), r.last_error()
    r.set_shard(0, 1)

"""A DSP_FIR in a trunk or a branch of a memory-word tree, host side ("mem_fir"): which cores
dspRuntimeSetOption("mem_fir", 1) lowers to the chain kernels beside "chain_mem" 1, what the report calls say of them, and which stay
with the interpreter, each with a text of its own -- with "mem_fir" 0 the texts the cores had before the option existed.
Host-only: the report calls lower a core and run nothing."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import firtree_programs as tp
from tests import memtree_programs as mp
from tests.delay_programs import OP_DELAY, samples
from tests.finish_programs import resealed

NOT_LOWERED = "is not lowered to the HIP path"
OLD_BRANCH = "a DSP_FIR in a chain that starts with LOAD_MEM " + NOT_LOWERED
OLD_TRUNK = "a DSP_FIR in a trunk (a chain that ends in STORE_MEM) " + NOT_LOWERED
OLD_BESIDE = "memory words beside a chain with a DSP_FIR are not lowered to the HIP path"
OPTIONS = ("mem_fir", "chain_mem", "fir_tail", "chain_delay", "chain_finish")


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, prog=None, mem_fir=1, tail=1, finish=1, delay=1, fs=48000):
    if prog is None:
        prog = tp.program(fmt, cores)[0]
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    r.set_option("chain_mem", 1)
    r.set_option("chain_finish", finish)
    r.set_option("chain_delay", delay)
    r.set_option("fir_tail", tail)
    if mem_fir is not None:
        r.set_option("mem_fir", mem_fir)                       # (unknown to the code before this option existed: every test here fails there)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeMemFirInfo lowers it and reports zeros when it is refused)"""
    assert r.mem_fir_info(core_index) == (0, 0, 0)
    return r.last_error()


def tree(tsec=2, ttaps=31, branches=((1, 63), (0, 63), (1, 0))):
    return [tp.trunk("a", tsec, ttaps)] + [tp.branch("a", nsec=s, taps=t) for s, t in branches]


def test_option_default_range_and_inheritance():
    r = loaded(6, [tp.core(tree())], mem_fir=None)
    assert r.get_option("mem_fir") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("mem_fir", bad)
    assert r.get_option("mem_fir") == 0 and r.mem_fir_info() == (0, 0, 0)
    rt.lib().dspRuntimeRelease()
    for key in ("mem_fir", "chain_mem"):                       # set without a program: the default of programs loaded later
        rt.Runtime.set_global_option(key, 1)
    prog = tp.program(6, [tp.core(tree())])[0]
    r1 = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    assert r1.get_option("mem_fir") == 1 and r1.core_info()["chains"] == 4 and r1.mem_fir_info() == (1, 2, 0)
    r2 = rt.Runtime(6, prog.copy(), fs=48000, random=1, dither=24)     # a second context: the options are copied ...
    assert r2.get_option("mem_fir") == 1 and r2.mem_fir_info() == (1, 2, 0)
    r2.set_option("mem_fir", 0)                                # ... and each context keeps its own
    assert r2.mem_fir_info() == (0, 0, 0) and r1.get_option("mem_fir") == 1 and r1.mem_fir_info() == (1, 2, 0)


@pytest.mark.parametrize("fmt", [4, 6])
def test_the_option_alone_does_nothing(fmt):
    """without "chain_mem" the memory opcodes are not lowered at all, whatever "mem_fir" says"""
    r = loaded(fmt, [tp.core(tree())])
    r.set_option("chain_mem", 0)
    assert r.get_option("mem_fir") == 1 and chains_of(r) == 0 and r.mem_fir_info() == (0, 0, 0)
    assert "(DSP_STORE_MEM) " + NOT_LOWERED in r.last_error() or "(DSP_LOAD_MEM) " + NOT_LOWERED in r.last_error()


@pytest.mark.parametrize("fmt", [4, 6])
def test_option_0_keeps_the_three_old_texts(fmt):
    t = tp.trunk("a", 1)
    r = loaded(fmt, [tp.core([t, tp.branch("a", nsec=1, taps=8)])], mem_fir=0)
    assert chains_of(r) == 0 and OLD_BRANCH in refusal(r)
    r = loaded(fmt, [tp.core([tp.trunk("a", 2, 8), tp.branch("a", nsec=1, taps=0)])], mem_fir=0)
    assert chains_of(r) == 0 and OLD_TRUNK in refusal(r)
    r = loaded(fmt, [tp.core([t, tp.branch("a", nsec=1, taps=0), tp.plain(nsec=1, taps=8)])], mem_fir=0)
    assert chains_of(r) == 0 and OLD_BESIDE in refusal(r)
    r.set_option("mem_fir", 1)
    assert r.core_info() == dict(chains=3, max_sections=1, max_taps=8) and r.mem_fir_info() == (0, 0, 0) and r.mem_info() == (1, 1, 0)
    r.set_option("mem_fir", 0)
    assert chains_of(r) == 0 and OLD_BESIDE in refusal(r)


@pytest.mark.parametrize("tsec", [0, 2, 17])
@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_trunks(fmt, tsec):
    items = [tp.trunk("a", tsec, 31), tp.branch("a", nsec=1, taps=0), tp.branch("a", nsec=0, taps=0, finish="none"),
             tp.trunk("b", tsec, 0, None), tp.branch("b", nsec=0, taps=0)]
    r = loaded(fmt, [tp.core(items)], tail=0, finish=0, delay=0)
    assert r.core_info() == dict(chains=5, max_sections=max(tsec, 1), max_taps=31), r.last_error()
    assert r.mem_fir_info() == (1, 0, 0) == tp.fir_counts(tp.core(items)) and r.mem_info() == (2, 3, 0) and r.fir_tail_info() == (0, 0)


@pytest.mark.parametrize("bsec", [0, 1, 17])
@pytest.mark.parametrize("fmt", [4, 6])
def test_plain_fir_branches(fmt, bsec):
    """plain SAT0DB or nothing behind the FIR, one and two STOREs; an ordinary FIR chain and a FIR-less tree beside"""
    items = [tp.trunk("a", 2, 0), tp.branch("a", nsec=bsec, taps=63), tp.branch("a", nsec=bsec, taps=7, finish="none", stores=2),
             tp.plain(nsec=1, taps=40), tp.plain(nsec=0, taps=9, finish="none"), tp.trunk("b", 1), tp.branch("b", nsec=2, taps=0)]
    c = tp.core(items)
    r = loaded(fmt, [c], tail=0, finish=0, delay=0)
    assert r.core_info() == dict(chains=7, max_sections=max(bsec, 2), max_taps=63), r.last_error()
    assert r.mem_fir_info() == (0, 2, 0) == tp.fir_counts(c) and r.mem_info() == (2, 3, 0) and r.fir_tail_info() == (0, 0)


@pytest.mark.parametrize("slot, form", [("A", "fixed"), ("A", "param"), ("B", "fixed"), ("B", "param"), (None, "fixed")])
@pytest.mark.parametrize("finish", ["none", "sat", "tpdf", "gain", "tpdf_gain"])
def test_handed_fir_branches(slot, form, finish):
    dressed = finish in ("tpdf", "gain", "tpdf_gain")
    items = [tp.trunk("a", 2, 31), tp.branch("a", nsec=1, taps=64, slot=slot, form=form, us=1000, finish=finish),
             tp.branch("a", nsec=0, taps=300, slot=slot, form=form, us=2100, finish=finish, stores=2),
             tp.branch("w", nsec=17, taps=7, slot=slot, form=form, us=63, finish=finish), tp.branch("a", nsec=0, taps=33),
             tp.plain(nsec=2, taps=16, slot=slot, form=form, us=63, finish=finish)]
    c = tp.core(items, calc=0)
    r = loaded(6, [c])
    handed = 3 if slot or dressed else 0
    assert r.core_info() == dict(chains=6, max_sections=17, max_taps=300), r.last_error()
    assert r.mem_fir_info() == (1, 4, handed) == tp.fir_counts(c) and r.mem_info() == (1, 4, 1)
    assert r.fir_tail_info() == (handed + (1 if handed else 0), 4 if slot else 0) == tp.tail_counts(c)
    assert r.delay_info() == ((4, samples(2100)) if slot else (0, 0)) and r.finish_info() == (4 if dressed else 0, 1)


@pytest.mark.parametrize("fmt", [4, 6])
def test_handed_branches_need_fir_tail_chain_finish_and_chain_delay(fmt):
    """with "fir_tail" 0 such a branch keeps fir_tail's refusal texts"""
    delayed = [tp.core([tp.trunk("a", 1), tp.branch("a", nsec=0, taps=64, slot="A", us=1000, finish="sat")])]
    dressed = [tp.core([tp.trunk("a", 1), tp.branch("a", nsec=1, taps=64, finish="tpdf_gain")], calc=0)]
    r = loaded(fmt, delayed, tail=0)
    assert chains_of(r) == 0 and "a DSP_DELAY in a chain with a DSP_FIR or a LOAD_MUX head " + NOT_LOWERED in refusal(r)
    r = loaded(fmt, dressed, tail=0)
    assert chains_of(r) == 0 and "a dressed SAT0DB behind a FIR or a LOAD_MUX head " + NOT_LOWERED in refusal(r)
    r = loaded(fmt, delayed, delay=0)
    assert chains_of(r) == 0 and "opcode 47 (DSP_DELAY)" in refusal(r)
    r = loaded(fmt, dressed, finish=0)
    assert chains_of(r) == 0 and NOT_LOWERED in refusal(r) and "opcode 47" not in r.last_error()
    assert loaded(fmt, delayed).mem_fir_info() == (0, 1, 1) and loaded(fmt, dressed).mem_fir_info() == (0, 1, 1)


@pytest.mark.parametrize("fmt", [4, 6])
def test_constant_word_branches_and_cores(fmt):
    """a writer core and a reader core: the reader's branches of words nobody there writes may have a FIR like any other"""
    c1 = tp.core([tp.trunk("l", 2, 31), tp.trunk("r", 0, 0, None)])
    c2 = tp.core([tp.branch("l", nsec=0, taps=63), tp.branch("r", nsec=1, taps=15, finish="none"), tp.branch("l", nsec=0, taps=0)])
    r = loaded(fmt, [c1, c2], tail=0, finish=0, delay=0)
    assert [r.core_info(k)["chains"] for k in (0, 1)] == [2, 3], r.last_error()
    assert [r.mem_fir_info(k) for k in (0, 1)] == [(1, 0, 0), (0, 2, 0)] and [r.mem_info(k) for k in (0, 1)] == [(2, 0, 0), (0, 3, 3)]


@pytest.mark.parametrize("fmt", [4, 6])
def test_a_bypassed_fir_leaves_an_ordinary_trunk_or_branch(fmt):
    items = [tp.trunk("a", 2, 0, odd="bypass"), tp.branch("a", nsec=1, taps=0, odd="bypass"), tp.branch("a", nsec=0, taps=0, odd="bypass", slot="A", us=1000)]
    r = loaded(fmt, [tp.core(items)], mem_fir=0)
    assert chains_of(r) == 0 and OLD_TRUNK in refusal(r)
    r.set_option("mem_fir", 1)
    assert r.core_info() == dict(chains=3, max_sections=2, max_taps=0), r.last_error()
    assert r.mem_fir_info() == (0, 0, 0) and r.mem_info() == (1, 2, 0) and r.fir_tail_info() == (0, 0) and r.delay_info() == (1, 47)


def test_a_rate_without_taps_and_a_rate_with_other_taps():
    """the impulse at 44.1 kHz is another one of another length: the counts follow the current rate"""
    r = loaded(6, [tp.core(tree())], fs=44100)
    assert r.core_info() == dict(chains=4, max_sections=2, max_taps=42) and r.mem_fir_info() == (1, 2, 0)


REFUSED = {
    "pure_delay_in_a_branch": (6, [tp.trunk("a", 1), tp.branch("a", nsec=1, taps=0, odd="pure_delay")], "FIR pure-delay variant is not lowered yet"),
    "pure_delay_in_a_trunk": (4, [tp.trunk("a", 1, 0, odd="pure_delay"), tp.branch("a", nsec=1, taps=0)], "FIR pure-delay variant is not lowered yet"),
    "two_firs_in_a_branch": (6, [tp.trunk("a", 1), tp.branch("a", nsec=0, taps=16, odd="two_firs")], "more than one FIR per chain"),
    "two_firs_in_a_trunk": (4, [tp.trunk("a", 1, 16, odd="two_firs"), tp.branch("a", nsec=0, taps=0)], "more than one FIR per chain"),
    "delay_in_front_of_a_branch_fir": (6, [tp.trunk("a", 1), tp.branch("a", nsec=1, taps=16, odd="front")], "a DSP_DELAY in front of the chain's DSP_FIR " + NOT_LOWERED),
    "delay_in_front_of_a_trunk_fir": (6, [tp.trunk("a", 1, 16, odd="front"), tp.branch("a", nsec=1, taps=0)], "a DSP_DELAY in front of the chain's DSP_FIR " + NOT_LOWERED),
    "format_2_branch": (2, [tp.trunk("a", 1), tp.branch("a", nsec=1, taps=16)], "DSP_FIR in int64 mode"),
    "format_2_trunk": (2, [tp.trunk("a", 1, 16), tp.branch("a", nsec=1, taps=0)], "DSP_FIR in int64 mode"),
    "format_3": (3, [tp.trunk("a", 1, 16), tp.branch("a", nsec=1, taps=0)], f"a memory word {NOT_LOWERED} in format 3"),
    "format_5": (5, [tp.trunk("a", 1), tp.branch("a", nsec=1, taps=16)], f"a memory word {NOT_LOWERED} in format 5"),
    "a_stored_fir_trunk": (6, [tp.trunk("a", 1, 16, odd="store"), tp.branch("a", nsec=1, taps=0)], "a STORE_MEM that is not the last opcode of its chain " + NOT_LOWERED),
    "a_branch_in_front_of_its_fir_trunk": (6, [tp.branch("a", nsec=0, taps=16), tp.trunk("a", 1, 16)], "a LOAD_MEM in front of the STORE_MEM of its word"),
    "two_fir_trunks_of_one_word": (6, [tp.trunk("a", 1, 16), tp.trunk("a", 0, 8), tp.branch("a", nsec=0, taps=16)], "is written by two STORE_MEM of the core"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_still_refused_with_the_option_on(case):
    fmt, items, text = REFUSED[case]
    r = loaded(fmt, [tp.core(items)])
    assert chains_of(r) == 0
    assert text in refusal(r), r.last_error()


@pytest.mark.parametrize("fmt", [4, 6])
def test_mux_heads_beside_fir_trees_stay_refused(fmt):
    items = [mp.trunk("a", 1), mp.branch("a", nsec=1, finish="sat", odd="fir"), mp.plain(nsec=1, finish="sat", odd="mux")]
    prog = mp.program(fmt, [mp.core(items)])[0]
    r = loaded(fmt, None, prog=prog)
    assert chains_of(r) == 0 and "memory words beside LOAD_MUX heads are not lowered to the HIP path" in refusal(r)


@pytest.mark.parametrize("fmt", [4, 6])
@pytest.mark.parametrize("moved", ["trunk", "branch"])
def test_overlapping_words_stay_refused(fmt, moved):
    """words one apart in a core with a FIR trunk and FIR branches: one opcode's offset moved by one inside a dspMem_LocationMultiple(2),
    the others left where they were"""
    prog = tp.program(fmt, [tp.core(tree())], pairs=("a",))[0].copy()
    code = mp.OP_STORE_MEM if moved == "trunk" else mp.OP_LOAD_MEM
    at = [op for op, _ in tp.mem_ops(prog) if int(prog[op]) >> 16 == code][0]
    prog[at + 1] += 1
    r = loaded(fmt, None, prog=prog)
    assert chains_of(r) == 0 and "of the core overlap without being the same word" in refusal(r)
    prog[at + 1] -= 1                                          # (the program as the encoder made it is lowered)
    assert loaded(fmt, None, prog=prog).mem_fir_info() == (1, 2, 0)


def test_a_set_shard_and_set_instances_refuse():
    r = loaded(6, [tp.core(tree())])
    assert r.core_info()["chains"] == 4 and r.mem_fir_info() == (1, 2, 0)
    r.set_shard(0, 2)
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} while the core is sharded" in refusal(r)
    r.set_shard(0, 1)
    assert r.mem_fir_info() == (1, 2, 0)
    r.set_instances(4)
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.core_info()["chains"] == 4 and r.mem_fir_info() == (1, 2, 0)


@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_groups_skip_the_chains_of_a_tree_core(fmt):
    """a bank of 20 plain FIR chains: a group of 20 alone in its core, no group beside a tree -- fir_shared stores from the caller's block
    in one launch, the chains of a tree core follow the stage"""
    bank = [tp.plain(nsec=2 if i % 2 else 0, taps=100, bank=1) for i in range(20)]
    r = loaded(fmt, [tp.core(bank)])
    assert r.core_info()["chains"] == 20 and r.fir_group_info() == dict(groups=1, grouped_chains=20, largest_group=20)
    r = loaded(fmt, [tp.core([tp.trunk("a", 2, 31), tp.branch("a", nsec=0, taps=100, bank=1)] + bank)])
    assert r.core_info()["chains"] == 22 and r.mem_fir_info() == (1, 1, 0), r.last_error()
    assert r.fir_group_info() == dict(groups=0, grouped_chains=0, largest_group=0)
    r = loaded(fmt, [tp.core(bank), tp.core([tp.trunk("a", 1), tp.branch("a", nsec=1, taps=0)])])      # (a tree in ANOTHER core changes nothing)
    assert r.fir_group_info(0) == dict(groups=1, grouped_chains=20, largest_group=20)


@pytest.mark.parametrize("fmt", [4, 6])
@pytest.mark.parametrize("which", ["trunk_history_past_the_data", "branch_history_past_the_data", "trunk_taps_past_the_program", "branch_taps_past_the_program",
                                   "line_inside_the_trunk_history", "branch_history_inside_a_line", "line_inside_a_fir_history_without_fir_tail"])
def test_damaged_payloads_are_refused_not_followed(fmt, which):
    """chains: the trunk (2 sections, 64 taps), a branch (40 taps alone), a FIR-less branch with a line of 100 samples, an ordinary chain
    with a line of 47 -- a delay line of ANY chain of the core against ANY FIR history of it"""
    items = [tp.trunk("a", 2, 64), tp.branch("a", nsec=0, taps=40), tp.branch("a", nsec=1, taps=0, slot="A", us=2100), tp.plain(nsec=1, taps=0, slot="B", us=1000)]
    prog = tp.program(fmt, [tp.core(items)])[0].copy()
    fir0, fir1 = tp.fir_words(prog)                            # [op, offset at 44.1 kHz, offset at 48 kHz, history]
    line0, line1 = tp.words_of(prog, OP_DELAY)                 # [op, size or us, line, parameter]
    data = int(prog[2])
    text, tail = "outside the state area", 1
    if which == "trunk_history_past_the_data":
        prog[fir0 + 3] = data - 63                             # 64 words from there: one too many
    elif which == "branch_history_past_the_data":
        prog[fir1 + 3] = data - 39
    elif which.endswith("taps_past_the_program"):
        fir = fir0 if which.startswith("trunk") else fir1
        imp = fir + int(np.int32(prog[fir + 2]))               # the impulse's length word at 48 kHz: taps far beyond the program
        assert int(prog[imp]) in (64, 40)
        prog[imp] = 1 << 15
        text = "outside the program"
    elif which == "line_inside_the_trunk_history":
        prog[line1 + 2] = int(prog[fir0 + 3]) + 5              # the ordinary chain's line over the trunk's history
        text = "a delay line and a FIR's history share words of the state area"
    elif which == "branch_history_inside_a_line":
        prog[fir1 + 3] = int(prog[line0 + 2]) + 50             # the branch's history inside its sibling's line
        text = "a delay line and a FIR's history share words of the state area"
    else:
        prog[line0 + 2] = int(prog[fir1 + 3]) + 5              # no handed chain here: the check holds without "fir_tail" too
        text, tail = "a delay line and a FIR's history share words of the state area", 0
    resealed(prog)
    r = loaded(fmt, None, prog=prog, tail=tail)
    assert r.mem_fir_info() == (0, 0, 0)
    assert text in r.last_error(), r.last_error()
    assert chains_of(r) == 0


def test_the_undamaged_program_of_the_payload_test_is_lowered():
    items = [tp.trunk("a", 2, 64), tp.branch("a", nsec=0, taps=40), tp.branch("a", nsec=1, taps=0, slot="A", us=2100), tp.plain(nsec=1, taps=0, slot="B", us=1000)]
    r = loaded(6, [tp.core(items)], tail=0)
    assert r.core_info() == dict(chains=4, max_sections=2, max_taps=64) and r.mem_fir_info() == (1, 1, 0) and r.delay_info() == (2, 100)

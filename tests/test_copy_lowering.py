"""LOAD_STORE lists, host side ("chain_copy"): which cores dspRuntimeSetOption("chain_copy", 1) lowers to the chain
kernels -- a list in front of the TPDF_CALC, between chains, behind a trunk, at the end, alone -- what the host makes of a list's
sequential meaning, and which cores stay with the interpreter, each with a text of its own.  Host-only: dspRuntimeCoreInfo /
dspRuntimeCopyInfo run nothing."""
import os

import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import copy_programs as cp

NOT_LOWERED = "not lowered to the HIP path"
IN = cp.IN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in ("chain_copy", "chain_mem", "chain_delay", "chain_finish"):
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores=None, prog=None, fs=48000, copy=1):
    if prog is None:
        prog = cp.program(fmt, cores)[0]
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    if copy:
        r.set_option("chain_copy", 1)
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeCopyInfo lowers it and reports zeros when it is refused)"""
    assert r.copy_info(core_index) == (0, 0)
    return r.last_error()


def emptied(prog, at):
    """the list at word `at` without its pairs: the words it gives up made NOPs of one word"""
    n = (int(prog[at]) & 0xFFFF) - 1
    prog[at] = (cp.OP_LOAD_STORE << 16) | 1
    prog[at + 1:at + 1 + n] = (2 << 16) | 1


def sat(nsec=1, **kw):
    return cp.plain(nsec=nsec, finish="sat", **kw)


def test_option_default_round_trip_and_unknown_key():
    core = cp.core([cp.copies([(IN + 5, 40)]), sat()])
    r = loaded(6, [core], copy=0)
    assert r.get_option("chain_copy") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("chain_copy", bad)
    assert r.get_option("chain_copy") == 0
    with pytest.raises(rt.AvdspError):
        r.set_option("chain_copies", 1)
    r.set_option("chain_copy", 1)
    assert r.get_option("chain_copy") == 1 and r.copy_info() == (1, 1)
    r.set_option("chain_copy", 0)
    assert r.get_option("chain_copy") == 0 and r.copy_info() == (0, 0)


def test_option_is_the_default_of_later_loads_and_copied_between_contexts():
    core = cp.core([cp.copies([(IN + 5, 40)]), sat()])
    rt.Runtime.set_global_option("chain_copy", 1)              # without a program: the default of programs loaded later
    r = loaded(6, [core], copy=0)
    assert r.get_option("chain_copy") == 1 and r.copy_info() == (1, 1) and r.core_info()["chains"] == 1
    r.set_option("chain_copy", 0)                              # on a program: that program's, and the default from now on
    r2 = loaded(6, [core], copy=0)                             # a second context starts from it ...
    assert r2.get_option("chain_copy") == 0 and r2.copy_info() == (0, 0)
    r2.set_option("chain_copy", 1)                             # ... and has a value of its own
    assert r2.get_option("chain_copy") == 1 and r2.copy_info() == (1, 1)
    assert r.get_option("chain_copy") == 0 and r.copy_info() == (0, 0)
    r3 = loaded(6, [core], copy=0)
    assert r3.get_option("chain_copy") == 1 and r2.get_option("chain_copy") == 1 and r.get_option("chain_copy") == 0


@pytest.mark.parametrize("fmt", [2, 3, 4, 5, 6])
def test_option_off_gives_todays_text(fmt):
    r = loaded(fmt, [cp.core([cp.copies([(IN + 5, 40)]), sat()])], copy=0)
    assert chains_of(r) == 0 and r.copy_info() == (0, 0)
    assert "opcode 38 (DSP_LOAD_STORE) is " + NOT_LOWERED in r.last_error()          # through `default:`, as ever
    r.set_option("chain_copy", 1)
    assert r.core_info() == dict(chains=1, max_sections=1, max_taps=0) and r.copy_info() == (1, 1)


def test_option_off_behind_a_trunk_gives_todays_text():
    r = loaded(6, [cp.core([cp.trunk("a", 1), cp.copies([(IN + 5, 40)]), cp.branch("a", nsec=1, finish="sat")])], copy=0)
    r.set_option("chain_mem", 1)
    assert chains_of(r) == 0 and "a STORE_MEM that is not the last opcode of its chain is " + NOT_LOWERED in refusal(r)
    r.set_option("chain_copy", 1)
    assert r.core_info()["chains"] == 2 and r.copy_info() == (1, 1) and r.mem_info() == (1, 1, 0)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_every_position(fmt):
    """a list in front of the TPDF_CALC, at the head, between chains, behind a trunk, at the end, and alone in a core"""
    src = lambda k: IN + 20 + k                                # noqa: E731
    c0 = cp.core([cp.copies([(src(2), 102), (src(3), 103)]), sat(), cp.copies([(src(4), 104)]), cp.trunk("a", 2),
                  cp.copies([(src(5), 105), (src(6), 106), (src(7), 107)]), cp.branch("a", nsec=1, finish="tpdf"), sat(0),
                  cp.copies([(src(8), 108)])], calc=0, head=[cp.copies([(src(0), 100), (src(1), 101)])])
    c1 = cp.core([cp.copies([(src(k), 120 + k) for k in range(6)])])
    c2 = cp.core([sat(2)])
    c3 = cp.core([cp.copies([(src(0), 130)]), sat(0), cp.copies([(src(1), 131)])])
    prog = cp.program(fmt, [c0, c1, c2, c3])[0]
    for at, _ in cp.lists_of(prog)[-2:]:                       # the last core's lists made empty ones (the encoder writes none)
        emptied(prog, at)
    r = loaded(fmt, prog=cp.resealed(prog))
    r.set_option("chain_mem", 1)
    r.set_option("chain_finish", 1)
    assert r.core_info(0)["chains"] == 4, r.last_error()
    assert [r.copy_info(k) for k in range(4)] == [(9, 9), (6, 6), (0, 0), (0, 0)], r.last_error()
    assert [r.core_info(k)["chains"] for k in range(4)] == [4, 0, 1, 1]          # core_info counts chains only
    assert r.mem_info(0) == (1, 1, 0) and r.finish_info(0) == (1, 1)
    s = r.shard_info(0)                                        # the spans include the pairs
    assert (s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (IN, src(8), 0, 108)
    s = r.shard_info(1)
    assert (s["total_chains"], s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (0, src(0), src(5), 120, 125)


@pytest.mark.parametrize("fmt", [3, 5])
def test_formats_3_and_5(fmt):
    r = loaded(fmt, [cp.core([cp.copies([(IN + 9, 50)]), sat(), cp.copies([(IN + 8, 51)])]), cp.core([cp.copies([(IN + 1, 60), (IN + 2, 61)])])])
    assert r.core_info(0)["chains"] == 1 and [r.copy_info(k) for k in range(2)] == [(2, 2), (2, 2)], r.last_error()


def test_an_empty_list_alone_is_no_chain_core():
    prog = cp.program(6, [cp.core([cp.copies([(IN + 3, 40)])])])[0]
    emptied(prog, cp.lists_of(prog)[0][0])
    r = loaded(6, prog=cp.resealed(prog))
    assert chains_of(r) == 0 and "core contains no LOAD..STORE chain" in refusal(r)
    r = loaded(6, [cp.core([cp.copies([(IN + 3, IN + 3)])])])      # a self-copy alone: no live pair either
    assert chains_of(r) == 0 and "core contains no LOAD..STORE chain" in refusal(r)


def test_forwarding_last_writer_and_self_copies():
    a, b, c, d = IN + 1, IN + 2, IN + 3, IN + 4
    cases = [
        ([(a, 40), (40, 41), (41, 42)], 3),                    # forwarding: 40, 41 and 42 all take input a
        ([(a, 40), (b, 40)], 1),                               # the last writer wins
        ([(a, b), (b, a)], 1),                                 # b takes a; a gets its own word back
        ([(a, a)], 0),                                         # a self-copy
        ([(a, 40), (40, 40), (b, 41), (41, 41)], 2),
        ([(c, 45), (a, c), (45, c)], 1),                       # c written and restored: 45 takes c
    ]
    for pairs, live in cases:
        r = loaded(6, [cp.core([cp.copies(pairs), sat()])])
        assert r.copy_info() == (len(pairs), live) and len(cp.resolve(pairs)) == live, (pairs, r.last_error())
    # across two lists of one core, a chain between them
    r = loaded(6, [cp.core([cp.copies([(a, 40)]), sat(), cp.copies([(40, 41), (d, 40)])])])
    assert r.copy_info() == (3, 2) and r.core_info()["chains"] == 1, r.last_error()
    s = r.shard_info()
    assert (s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (IN, d, 0, 41)


def test_oktodac_diys_own_five_pairs():
    """oktodac_diy.c:126-131 writes USBIN(1) twice: five pairs, four live"""
    pairs = cp.lists_of(np.fromfile(os.path.join(GOLDEN, "dacdiy1.bin"), dtype=np.uint32))[0][1]
    assert len(pairs) == 5 and len({b for _, b in pairs}) == 4
    prog = cp.program(6, [cp.core([cp.copies([(IN + a, 100 + b) for a, b in pairs]), sat()])])[0]
    r = loaded(6, prog=prog)
    assert r.copy_info() == (5, 4), r.last_error()
    last = {100 + b: IN + a for a, b in pairs}
    assert cp.resolve([(IN + a, 100 + b) for a, b in pairs]) == last


@pytest.mark.parametrize("fmt", [2, 6])
def test_refusals_each_with_its_text(fmt):
    def text_of(items, **kw):
        r = loaded(fmt, [cp.core(items, **kw)])
        assert chains_of(r) == 0
        return refusal(r)
    x = IN + 30
    # chain 0 loads IO IN and stores IO 0
    assert f"IO 0 is stored by a chain of the core and read by a LOAD_STORE pair: a copy of a chain's output is {NOT_LOWERED}" in text_of([sat(), cp.copies([(0, 50)])])
    assert "a copy of a chain's output" in text_of([cp.copies([(0, 50)]), sat()])
    assert f"IO 0 is written by a LOAD_STORE pair and stored by a chain of the core: {NOT_LOWERED}" in text_of([cp.copies([(x, 0)]), sat()])
    assert "IO 0 is written by a LOAD_STORE pair and stored by a chain of the core" in text_of([sat(), cp.copies([(x, 0)])])
    assert f"IO {IN} is written by a LOAD_STORE pair and loaded by a chain of the core: forwarding a pair into a chain is {NOT_LOWERED}" in text_of([cp.copies([(x, IN)]), sat()])
    assert "forwarding a pair into a chain" in text_of([sat(), cp.copies([(x, IN)])])
    assert "forwarding a pair into a chain" in text_of([cp.copies([(IN, 60), (x, IN)]), sat(), cp.copies([(60, IN)])])      # written and restored around the chain
    assert f"IO {x} is both read and written by the LOAD_STORE pairs of the core: {NOT_LOWERED}" in text_of([cp.copies([(x, 50), (x + 1, x)]), sat()])
    assert f"a LOAD_STORE list between a chain's LOAD and its first STORE is {NOT_LOWERED}" in text_of([sat(), cp.copies([(x, 50)], inside=True)])


def test_a_source_may_be_a_chains_input():
    r = loaded(6, [cp.core([cp.copies([(IN, 50), (IN, 51), (IN + 1, 52)]), sat(), sat(0)])])
    assert r.core_info()["chains"] == 2 and r.copy_info() == (3, 3), r.last_error()


def test_damaged_lists_are_refused_not_followed():
    prog = cp.program(6, [cp.core([cp.copies([(IN + 5, 40), (IN + 6, 41)]), sat()])])[0]
    at = cp.lists_of(prog)[0][0]
    odd = prog.copy()
    odd[at] = (cp.OP_LOAD_STORE << 16) | 4                     # three payload words, the fourth made a NOP of one word
    odd[at + 4] = (2 << 16) | 1
    r = loaded(6, prog=cp.resealed(odd))
    assert chains_of(r) == 0 and "a LOAD_STORE list of 3 words is no list of pairs (damaged)" in refusal(r)
    for k, bad in ((1, 65536), (2, -1), (4, 1 << 20)):
        p = prog.copy()
        p[at + k] = np.uint32(np.int32(bad))
        r = loaded(6, prog=p)
        assert chains_of(r) == 0 and f"IO number {bad} outside [0,65536)" in refusal(r)


def test_a_set_shard_and_set_instances_refuse():
    r = loaded(6, [cp.core([cp.copies([(IN + 5, 40)]), sat(), sat(2)])])
    assert r.core_info()["chains"] == 2 and r.copy_info() == (1, 1)
    r.set_shard(0, 2)
    assert chains_of(r) == 0 and f"a LOAD_STORE list is {NOT_LOWERED} while the core is sharded" in refusal(r)
    r.set_shard(0, 1)
    assert r.core_info()["chains"] == 2 and r.copy_info() == (1, 1)
    r.set_instances(4)
    assert chains_of(r) == 0 and f"a LOAD_STORE list is {NOT_LOWERED} while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.core_info()["chains"] == 2 and r.copy_info() == (1, 1)


def dacdiy1():
    prog = np.fromfile(os.path.join(GOLDEN, "dacdiy1.bin"), dtype=np.uint32)
    r = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    assert r.rc >= 0 and len(r.cores) == 4
    for key in ("chain_mem", "chain_finish", "chain_delay"):
        r.set_option(key, 1)
    return r


def test_dacdiy1_the_list_was_what_kept_core_1_off_the_chain_kernels():
    """tests/golden/dacdiy1.bin is dspProg_3ways_LR4 of oktodac_diy.c: LOAD_STORE (5 pairs), TPDF_CALC and two trunks in core 1"""
    r = dacdiy1()
    assert chains_of(r, 0) == 0 and "opcode 38 (DSP_LOAD_STORE)" in refusal(r, 0)
    r.set_option("chain_copy", 1)
    assert r.copy_info(0) == (5, 4), r.last_error()
    assert r.core_info(0)["chains"] == 2 and r.mem_info(0) == (2, 0, 0) and r.finish_info(0) == (0, 1)
    assert [r.core_info(k)["chains"] for k in (1, 2)] == [2, 2] and [r.mem_info(k) for k in (1, 2)] == [(0, 2, 2)] * 2
    assert [r.copy_info(k) for k in range(1, 4)] == [(0, 0)] * 3
    s = r.shard_info(0)
    assert (s["in_io_min"], s["in_io_max"], s["out_io_min"], s["out_io_max"]) == (8, 17, 0, 25)


def test_dacdiy1_no_core_is_refused():
    """With "chain_copy", "chain_mem", "chain_finish" and "chain_delay" on, dither 24: no core is refused, and copy_info(0) == (5, 4).
    The fourth core stores both chains of its high way to USBIN(lefthigh) and DACOUT(lefthigh) (oktodac_diy.c:194-204, IOs 30 and 6):
    the later chain's STOREs win, the earlier chain keeps its banks and its line and stores nothing"""
    r = dacdiy1()
    assert chains_of(r, 3) == 0 and "IO 6 is stored by more than one chain of the core" in refusal(r, 3)
    r.set_option("chain_copy", 1)
    assert r.copy_info(0) == (5, 4), r.last_error()
    info = [chains_of(r, k) for k in range(4)]
    assert all(n > 0 for n in info), (info, r.last_error())
    assert info == [2, 2, 2, 2] and r.mem_info(3) == (0, 2, 2) and r.delay_info(3)[0] == 2
    s = r.shard_info(3)
    assert (s["out_io_min"], s["out_io_max"]) == (6, 30)


def delayed(nsec=1, **kw):
    return cp.plain(nsec=nsec, slot="A", us=1000, finish="sat", **kw)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_last_chain_to_store_an_io_wins(fmt):
    """two chains that store one IO: with 0 the text of old; with 1 the earlier STORE is dead -- taken out of a chain that stores
    elsewhere too, and a chain left without a STORE is kept where it has a delay line (chain_tail runs it for the line)"""
    both = [cp.stores_to(sat(), [3, 4]), cp.stores_to(sat(2), [4, 5])]                     # IO 4 twice: the first chain keeps IO 3
    r = loaded(fmt, [cp.core(both)], copy=0)
    assert chains_of(r) == 0 and r.last_error().endswith("IO 4 is stored by more than one chain of the core")
    r.set_option("chain_copy", 1)
    assert r.core_info()["chains"] == 2, r.last_error()
    s = r.shard_info()
    assert (s["out_io_min"], s["out_io_max"]) == (3, 5)
    r = loaded(fmt, [cp.core([cp.stores_to(delayed(), [7, 8]), cp.stores_to(delayed(2), [7, 8])])])
    r.set_option("chain_delay", 1)
    assert r.core_info()["chains"] == 2 and r.delay_info()[0] == 2, r.last_error()
    r = loaded(fmt, [cp.core([cp.stores_to(sat(), [7, 7])])])                              # one chain, one IO twice
    assert r.core_info()["chains"] == 1, r.last_error()


@pytest.mark.parametrize("fmt", [2, 6])
def test_a_chain_left_without_a_store_needs_a_delay_line(fmt):
    r = loaded(fmt, [cp.core([cp.stores_to(sat(), [7]), cp.stores_to(sat(2), [7])])])
    assert chains_of(r) == 0
    assert f"IO 7 is stored by more than one chain of the core, and the earlier chain stores nothing else and has no DSP_DELAY: {NOT_LOWERED}" in refusal(r)
    r.set_shard(0, 2)                                          # (under a shard nothing is resolved: the text of old)
    assert chains_of(r) == 0 and r.last_error().endswith("IO 7 is stored by more than one chain of the core")

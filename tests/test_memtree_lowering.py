"""Memory words, host side ("chain_mem"): which cores dspRuntimeSetOption("chain_mem", 1) lowers to the chain kernels --
trunks that end in STORE_MEM, branches that start with LOAD_MEM -- and which stay with the interpreter, each with a text of its own.
Host-only: dspRuntimeCoreInfo / dspRuntimeMemInfo run nothing."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from tests import memtree_programs as mp
from tests.finish_programs import resealed

OP_BIQUADS = 50
NOT_LOWERED = "is not lowered to the HIP path"


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in ("chain_mem", "chain_delay", "chain_finish"):
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def loaded(fmt, cores, fs=48000, prog=None, **kw):
    if prog is None:
        prog = mp.program(fmt, cores, **kw)[0]
    r = rt.Runtime(fmt, prog, fs=fs, random=1, dither=24)
    assert r.rc >= 0
    return r


def chains_of(r, core_index=0):
    try:
        return r.core_info(core_index)["chains"]
    except rt.AvdspError as e:                                 # (a core neither path takes counts as not lowered)
        assert e.code == -8
        return 0


def refusal(r, core_index=0):
    """the chain lowering's text for the core (dspRuntimeMemInfo lowers it and reports zeros when it is refused)"""
    assert r.mem_info(core_index) == (0, 0, 0)
    return r.last_error()


def tree(nsec=2, branches=((1, "sat"), (0, "none"))):
    return [mp.trunk("a", nsec)] + [mp.branch("a", nsec=s, finish=f) for s, f in branches]


def test_option_default_and_range():
    r = loaded(6, [mp.core(tree())])
    assert r.get_option("chain_mem") == 0
    for bad in (2, -1):
        with pytest.raises(rt.AvdspError):
            r.set_option("chain_mem", bad)
    assert r.get_option("chain_mem") == 0
    rt.Runtime.set_global_option("chain_mem", 1)               # the default of programs loaded later
    r2 = loaded(6, [mp.core(tree())])
    assert r2.get_option("chain_mem") == 1 and r2.core_info()["chains"] == 3 and r2.mem_info() == (1, 2, 0)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_gives_todays_text_for_both_opcodes(fmt):
    r = loaded(fmt, [mp.core(tree()), mp.core([mp.branch("a", nsec=1, finish="sat")])])
    assert r.core_info(0)["chains"] == 0 and r.mem_info(0) == (0, 0, 0)
    assert "opcode 40 (DSP_STORE_MEM) " + NOT_LOWERED in r.last_error()          # through `default:`, as ever
    assert r.core_info(1)["chains"] == 0 and r.mem_info(1) == (0, 0, 0)
    assert "opcode 39 (DSP_LOAD_MEM) " + NOT_LOWERED in r.last_error()
    r.set_option("chain_mem", 1)
    assert r.core_info(0) == dict(chains=3, max_sections=2, max_taps=0) and r.mem_info(0) == (1, 2, 0)
    assert r.core_info(1) == dict(chains=1, max_sections=1, max_taps=0) and r.mem_info(1) == (0, 1, 1)
    r.set_option("chain_mem", 0)
    assert r.core_info(0)["chains"] == 0 and r.mem_info(0) == (0, 0, 0)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_shapes(fmt):
    """mem_info() and core_info() per shape: trunk sections 0 .. 40, trunks alone, branches alone, ordinary chains between, branches
    that are not adjacent, delayed and dressed branches under their own options"""
    items = [mp.trunk("a", 0, None), mp.plain(nsec=2, finish="sat"), mp.trunk("b", 40), mp.branch("a", nsec=0, finish="none", stores=2),
             mp.branch("b", nsec=17, finish="sat"), mp.trunk("c", 16), mp.branch("a", nsec=3, finish="sat"), mp.branch("z", nsec=1, finish="sat"),
             mp.plain(nsec=0, finish="none", load_gain=None)]
    r = loaded(fmt, [mp.core(items), mp.core([mp.trunk("z", 1), mp.trunk("y", 17)]), mp.core([mp.branch("y", nsec=0, finish="sat")])])
    r.set_option("chain_mem", 1)
    assert [r.core_info(k) for k in range(3)] == [dict(chains=9, max_sections=40, max_taps=0), dict(chains=2, max_sections=17, max_taps=0),
                                                  dict(chains=1, max_sections=0, max_taps=0)], r.last_error()
    assert [r.mem_info(k) for k in range(3)] == [(3, 4, 1), (2, 0, 0), (0, 1, 1)]
    s = r.shard_info(0)                                        # branches load no IO: trunks and ordinary chains span the input window
    assert (s["in_io_min"], s["in_io_max"]) == (mp.IN, mp.IN + 4)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_delayed_and_dressed_branches_need_their_options(fmt):
    items = [mp.trunk("a", 2), mp.branch("a", nsec=1, slot="A", us=1000, finish="tpdf_gain"), mp.branch("a", nsec=0, slot="B", us=63, finish="sat")]
    r = loaded(fmt, [mp.core(items, calc=0)])
    r.set_option("chain_mem", 1)
    assert chains_of(r) == 0 and "opcode 7 (DSP_TPDF_CALC)" in refusal(r)
    r.set_option("chain_finish", 1)
    assert chains_of(r) == 0 and "opcode 47 (DSP_DELAY)" in refusal(r)
    r.set_option("chain_delay", 1)
    assert r.core_info()["chains"] == 3 and r.mem_info() == (1, 2, 0) and r.delay_info() == (2, 47) and r.finish_info() == (1, 1)


@pytest.mark.parametrize("odd, text", [
    ("store", "a STORE_MEM that is not the last opcode of its chain"),
    ("sat", "a STORE_MEM that is not the last opcode of its chain"),
    ("delay", "a STORE_MEM that is not the last opcode of its chain"),
    ("front", "a STORE_MEM in front of the banks or between two banks"),
    ("between", "a STORE_MEM in front of the banks or between two banks"),
    ("fir", "a DSP_FIR in a trunk (a chain that ends in STORE_MEM)"),
    ("mux", "a memory word in a chain with a LOAD_MUX head"),
    ("from_mem", "a STORE_MEM in a chain that starts with LOAD_MEM"),
])
@pytest.mark.parametrize("fmt", [4, 6])
def test_trunks_that_are_refused(fmt, odd, text):
    r = loaded(fmt, [mp.core([mp.trunk("b", 1), mp.trunk("a", 2, odd=odd), mp.branch("a", nsec=1, finish="sat"), mp.branch("b", nsec=0, finish="sat")])])
    r.set_option("chain_mem", 1)
    r.set_option("chain_delay", 1)
    assert chains_of(r) == 0
    assert text + " " + NOT_LOWERED in refusal(r)


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_words_that_are_refused(fmt):
    def text_of(items, **kw):
        r = loaded(fmt, [mp.core(items)], **kw)
        r.set_option("chain_mem", 1)
        assert chains_of(r) == 0
        return refusal(r)
    a, b = mp.branch("a", nsec=1, finish="sat"), mp.branch("a", nsec=0, finish="sat")
    assert "is written by two STORE_MEM of the core" in text_of([mp.trunk("a", 1), a, mp.trunk("a", 0), b])
    assert "a LOAD_MEM in front of the STORE_MEM of its word (the one-frame-lag form) " + NOT_LOWERED in text_of([a, mp.trunk("a", 1), b])
    assert "is read as a parameter by another opcode of the core" in text_of([mp.trunk("a", 1), a, mp.plain(nsec=1, finish="sat", odd="gain_of", key="a")])
    assert "a STORE_MEM that is not the last opcode" not in text_of([mp.trunk("a", 1), a, mp.plain(nsec=1, finish="sat", odd="gain_of", key="a")])


@pytest.mark.parametrize("fmt", [4, 6])
def test_fir_and_mux_in_and_beside_trees(fmt):
    def text_of(items):
        r = loaded(fmt, [mp.core(items)])
        r.set_option("chain_mem", 1)
        assert chains_of(r) == 0
        return refusal(r)
    t = mp.trunk("a", 1)
    assert "a DSP_FIR in a chain that starts with LOAD_MEM " + NOT_LOWERED in text_of([t, mp.branch("a", nsec=1, finish="sat", odd="fir")])
    assert "memory words beside a chain with a DSP_FIR are not lowered to the HIP path" in text_of([t, mp.branch("a", nsec=1, finish="sat"), mp.plain(nsec=1, finish="sat", odd="fir")])
    assert "a memory word in a chain with a LOAD_MUX head " + NOT_LOWERED in text_of([mp.trunk("b", 0, odd="mux")])
    assert "memory words beside LOAD_MUX heads are not lowered to the HIP path" in text_of([t, mp.branch("a", nsec=1, finish="sat"), mp.plain(nsec=1, finish="sat", odd="mux")])


@pytest.mark.parametrize("fmt", [3, 5])
def test_formats_3_and_5(fmt):
    r = loaded(fmt, [mp.core(tree())])
    r.set_option("chain_mem", 1)
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} in format {fmt}" in refusal(r)


def test_overlapping_words():
    """words one apart: the trunk's offset moved by one inside a dspMem_LocationMultiple(2), the branch's left where it was"""
    prog = mp.program(6, [mp.core(tree())], pairs=("a",))[0]
    store = [op for op, _ in mp.mem_ops(prog) if int(prog[op]) >> 16 == mp.OP_STORE_MEM][0]
    prog[store + 1] += 1
    r = loaded(6, None, prog=prog)
    r.set_option("chain_mem", 1)
    assert chains_of(r) == 0 and "of the core overlap without being the same word" in refusal(r)


def test_a_set_shard_and_set_instances_refuse():
    r = loaded(6, [mp.core(tree())])
    r.set_option("chain_mem", 1)
    assert r.core_info()["chains"] == 3
    r.set_shard(0, 2)
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} while the core is sharded" in refusal(r)
    r.set_shard(0, 1)
    assert r.core_info()["chains"] == 3 and r.mem_info() == (1, 2, 0)
    r.set_instances(4)
    assert chains_of(r) == 0 and f"a memory word {NOT_LOWERED} while the program has instances" in refusal(r)
    r.set_instances(0)
    assert r.core_info()["chains"] == 3 and r.mem_info() == (1, 2, 0)


@pytest.mark.parametrize("opcode", ["STORE_MEM", "LOAD_MEM"])
@pytest.mark.parametrize("which", ["payload_too_short", "offset_past_the_program", "offset_in_front_of_the_program", "target_in_the_opcode_stream",
                                   "target_on_a_bank_header", "second_word_on_a_bank_header"])
def test_damaged_payloads_are_refused_not_followed(which, opcode):
    prog = mp.program(6, [mp.core(tree())])[0]
    code = mp.OP_STORE_MEM if opcode == "STORE_MEM" else mp.OP_LOAD_MEM
    at = [op for op, _ in mp.mem_ops(prog) if int(prog[op]) >> 16 == code][0]
    banks = [op + int(np.int32(prog[op + 2])) for op in mp.words_of(prog, OP_BIQUADS)]
    if which == "payload_too_short":
        prog[at] = (code << 16) | 1                            # the opcode shortened to no payload, the word it gives up made a NOP of one word
        prog[at + 1] = (2 << 16) | 1
        prog = resealed(prog)                                  # (the header's checksum sums the opcode words)
        want = "opcode payload shorter than 1 words"
    elif which == "offset_past_the_program":
        prog[at + 1] = int(prog[1]) - at - 1                   # its second word is the first behind the program
        want = "outside the program"
    elif which == "offset_in_front_of_the_program":
        prog[at + 1] = np.uint32(np.int32(-at - 1))
        want = "outside the program"
    elif which == "target_in_the_opcode_stream":
        prog[at + 1] = 0
        want = f"{opcode} target (word {at}) is not a free word of a PARAM section: it would rewrite the opcode stream"
    elif which == "target_on_a_bank_header":
        prog[at + 1] = np.uint32(np.int32(banks[1] - at))
        want = f"{opcode} target (word {banks[1]}) is not a free word of a PARAM section: it would rewrite a count, IO number or length"
    else:
        prog[at + 1] = np.uint32(np.int32(banks[1] - 1 - at))  # the first word is the last coefficient of the bank in front: free
        want = f"{opcode} target (word {banks[1]}) is not a free word of a PARAM section: it would rewrite a count, IO number or length"
    r = loaded(6, None, prog=prog)
    r.set_option("chain_mem", 1)
    assert chains_of(r) == 0
    assert want in refusal(r)


@pytest.mark.parametrize("fmt", [2, 6])
def test_load_mem_data_is_refused(fmt):
    """a hand-made program (the encoder has no call for it): a branch's LOAD_MEM, behind an ordinary chain, made a LOAD_MEM_DATA, opcode 60"""
    prog = mp.program(fmt, [mp.core([mp.trunk("a", 1), mp.plain(nsec=1, finish="sat"), mp.branch("a", nsec=1, finish="sat")])])[0]
    at = [op for op, _ in mp.mem_ops(prog) if int(prog[op]) >> 16 == mp.OP_LOAD_MEM][0]
    prog[at] = (60 << 16) | (int(prog[at]) & 0xFFFF)
    r = loaded(fmt, None, prog=resealed(prog))
    assert chains_of(r) == 0 and "opcode 40 (DSP_STORE_MEM) " + NOT_LOWERED in refusal(r)          # the option off: the trunk's opcode comes first
    r.set_option("chain_mem", 1)
    assert chains_of(r) == 0 and "LOAD_MEM_DATA " + NOT_LOWERED in refusal(r)

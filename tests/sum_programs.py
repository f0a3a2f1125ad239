"""Programs for the "chain_sum" tests, on top of tests/ways_programs.py: its cores, items and ways, and one more item,

    bus(keys, ops, **way)      LOAD_MEM(keys[0]), (LOAD_MEM(keys[k]), ops[k - 1]) ..., then a way      ops: "ADDXY" | "SUBXY"
                               (the way's own run of GAIN / NEGX, way()'s `ops`, is `way_ops` here)

a sum head in front of whatever a way() may be.  A key may occur twice; a key no trunk() of the program stores is a constant word
(set_word).  lfe_program() is the opcode sequence of the reference's dspprogs/crossover2x2lfe.c core."""
import numpy as np

from tests import ways_programs as wp
from tests.ways_programs import IN, chain, core, fork, head, program, raw, set_word, trunk, way          # noqa: F401

MAX_TERMS = 8                                        # AVDSP_MAX_SUM_TERMS


def bus_steps(keys, ops):
    assert len(keys) == len(ops) + 1 and all(op in ("ADDXY", "SUBXY") for op in ops)
    s = [("load_mem", keys[0])]
    for k, op in zip(keys[1:], ops):
        s += [("load_mem", k), ("xy", op)]
    return s


def bus(keys, ops, **kw):
    """an item of a core: a raw() item for ways_programs (which counts no chain for it), its keys and operations kept for counts()"""
    w = way(ops=kw.pop("way_ops", ()), **kw)
    it = raw(bus_steps(list(keys), list(ops)) + wp._way_steps(w))
    it["bus"] = (list(keys), list(ops))
    it["way"] = w
    return it


def counts(c):
    """what sum_info(), ways_info(), mem_info()[:2] and core_info()["chains"] say of a core of chains, forks, trunks and buses:
    (heads, words loaded by them), (forks, chains with a run of GAIN / NEGX), (trunks, branches), chains"""
    buses = [it for it in c["items"] if "bus" in it]
    (forks, ops), chains = wp.counts(c)
    ops += sum(bool(it["way"]["ops"]) for it in buses)
    trunks = sum(it["kind"] == "trunk" for it in c["items"])
    branches = len(buses) + sum(len(it["ways"]) for it in c["items"] if it["kind"] in ("chain", "fork") and it["head"]["key"] is not None)
    return (len(buses), sum(len(it["bus"][0]) for it in buses)), (forks, ops), (trunks, branches), chains + len(buses)


def lfe_core(lfe=True):
    """crossover2x2lfe.c:104-110: TPDF_CALC(24), two prefilter trunks (LOAD_GAIN, BIQUADS of 6, STORE_MEM), two crossOver2ways forks
    (LOAD_GAIN, COPYXY, BIQUADS of 4, SAT0DB_TPDF, DELAY, STORE, SWAPXY, BIQUADS of 4, GAIN, SAT0DB_TPDF_GAIN, STORE) and the LFE channel
    (LOAD_MEM, LOAD_MEM, ADDXY, BIQUADS of 4, SAT0DB, DELAY, STORE).  (Every LOAD of these builders takes an input of its own.)"""
    items = [trunk("mem1", 6, 1.0), trunk("mem2", 6, 1.0)]
    for _ in range(2):
        items.append(fork(head(1.0), way(nsec=4, finish="tpdf", slot="B", form="param", us=294, max_us=1470),
                          way(nsec=4, ops=[("gain", 0.8)], finish="tpdf_gain", gain=0.8)))
    if lfe:
        items.append(bus(["mem1", "mem2"], ["ADDXY"], nsec=4, finish="sat", slot="B", form="param", us=0, max_us=2941))
    return core(items, calc=24)


def lfe_program(fmt):
    """-> (program words, inputs, outputs, {key: word}, the core)"""
    c = lfe_core()
    return program(fmt, [c]) + (c,)


def set_word_bits(prog, word, bits, fmt):
    """the two program words of a memory word from the 64 bits of an accumulator -- an int64 (format 2) or the bits of a double"""
    v = np.array([bits], dtype=np.uint64).view(np.uint32)
    prog[word], prog[word + 1] = v[0], v[1]

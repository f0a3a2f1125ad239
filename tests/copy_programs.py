"""Programs for the LOAD_STORE tests ("chain_copy"), built with the encoder like tests/memtree_programs.py's: cores of
[items in front of the TPDF_CALC] + [TPDF_CALC] + items in program order, an item being

    copies([(in, out), ...])    one DSP_LOAD_STORE list of those pairs, IO numbers as given
    trunk(key, ...)             LOAD | LOAD_GAIN, [BIQUADS], STORE_MEM(word of `key`)            (memtree_programs.trunk)
    branch(key, ...)            LOAD_MEM(word of `key`), then what delay_programs.chain() describes behind its load
    plain(...)                  an ordinary chain, delay_programs.chain(); fir=N: a DSP_FIR of N taps behind the bank
    stores_to(item, [io, ...])  that chain with STOREs to the IOs named

Every trunk and every ordinary chain takes the next input from IO IN, every STORE the next output from IO 0; the pairs name their IOs
themselves (sources anywhere in the input window, destinations wherever no chain stores).  Encoded for 44.1 and 48 kHz."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from tests import delay_programs as dp
from tests.delay_programs import F44100, F48000, FPEAK, resealed, words_of          # noqa: F401
from tests.fuzz_programs import _prototypes
from tests.memtree_programs import branch, trunk                                      # noqa: F401

OP_LOAD_STORE = 38
IN = 512                                                       # first input IO
MAX_IO = 1024


def copies(pairs, inside=False):
    """inside: the list stands between the LOAD of the chain in front of it and that chain's first STORE (the lowering refuses it)"""
    return dict(kind="copies", pairs=[(int(a), int(b)) for a, b in pairs], inside=inside, nsec=0, key=None)


def plain(**kw):
    fir = kw.pop("fir", 0)
    kw.setdefault("slot", None)
    c = dp.chain(**kw)
    c.update(kind="plain", key=None, fir=fir)
    return c


def stores_to(item, ios):
    """the chain stores to these IOs instead of the next free outputs (two chains of a core may then store one IO)"""
    item["store_to"] = [int(v) for v in ios]
    return item


def core(items, calc=None, head=()):
    """head: items (lists) in front of the core's TPDF_CALC"""
    return dict(items=list(items), calc=calc, head=list(head))


def program(fmt, cores):
    """-> (program words, number of chain inputs, number of chain outputs)"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.dsp_LOAD_MEM.argtypes = [C.c_int]
    L.dsp_STORE_MEM.argtypes = [C.c_int]
    L.dspLoadStore_Data.argtypes = [C.c_int, C.c_int]
    nin, nout, words = [0], [0], {}
    chains = [it for c in cores for it in c["items"] if it["kind"] != "copies"]

    def build(L):
        L.dsp_PARAM()
        banks, lines, firs = {}, {}, {}
        for n, it in enumerate(chains):
            if it["nsec"]:
                banks[n] = L.dspBiquad_Sections(it["nsec"])
                for k in range(it["nsec"]):
                    L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * (n % 150) + 190.0 * (k % 30), 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
        for n, it in enumerate(chains):
            if it["kind"] != "trunk" and it["slot"] and it["form"] == "param":
                lines[n] = L.dspDelay_MicroSec_Max_Default(it["max_us"], it["us"])
        for n, it in enumerate(chains):
            if it.get("fir"):
                taps = (np.cos(np.arange(it["fir"]) * (0.37 + 0.05 * n)) / (4.0 + np.arange(it["fir"]))).astype(np.float32)
                firs[n] = L.dspFir_Impulses()
                for _ in (F44100, F48000):
                    L.dspFir_ImpulseData(taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps))
        for it in chains:
            if it["key"] is not None and it["key"] not in words:
                words[it["key"]] = L.dspMem_Location()

        def a_list(it):
            L.dsp_LOAD_STORE()
            for a, b in it["pairs"]:
                L.dspLoadStore_Data(a, b)

        def load(it):
            if it["load_gain"] is None:
                L.dsp_LOAD(IN + nin[0])
            else:
                L.dsp_LOAD_GAIN_Fixed(IN + nin[0], it["load_gain"])
            nin[0] += 1

        def store():
            L.dsp_STORE(nout[0])
            nout[0] += 1

        n = 0
        for c in cores:
            L.dsp_CORE()
            for it in c["head"]:
                a_list(it)
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            items = c["items"]
            for i, it in enumerate(items):
                if it["kind"] == "copies":
                    if not it["inside"]:
                        a_list(it)
                    continue
                inside = items[i + 1] if i + 1 < len(items) and items[i + 1]["kind"] == "copies" and items[i + 1]["inside"] else None
                if it["kind"] == "trunk":
                    load(it)
                    if it["nsec"]:
                        L.dsp_BIQUADS(banks[n])
                    L.dsp_STORE_MEM(words[it["key"]])
                    n += 1
                    continue
                if it["kind"] == "branch":
                    L.dsp_LOAD_MEM(words[it["key"]])
                else:
                    load(it)
                if inside is not None:
                    a_list(inside)
                if it["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if it.get("fir"):
                    L.dsp_FIR(firs[n])
                if it["slot"] == "A":
                    (L.dsp_DELAY(lines[n]) if it["form"] == "param" else L.dsp_DELAY_FixedMicroSec(it["us"]))
                f = it["finish"]
                if f == "sat":
                    L.dsp_SAT0DB()
                elif f == "tpdf":
                    L.dsp_SAT0DB_TPDF()
                elif f == "gain":
                    L.dsp_SAT0DB_GAIN_Fixed(it["gain"])
                elif f == "tpdf_gain":
                    L.dsp_SAT0DB_TPDF_GAIN_Fixed(it["gain"])
                if it["slot"] == "B":
                    (L.dsp_DELAY(lines[n]) if it["form"] == "param" else L.dsp_DELAY_FixedMicroSec(it["us"]))
                if it.get("store_to") is not None:
                    for io in it["store_to"]:
                        L.dsp_STORE(io)
                else:
                    for _ in range(it["stores"]):
                        store()
                n += 1

    prog = enc.encode(build, 2 if fmt == 2 else 6, F44100, F48000, max_io=MAX_IO, capacity=1 << 20)
    return prog, nin[0], nout[0]


def lists_of(prog):
    """the DSP_LOAD_STORE opcodes in program order: (opcode word, [(in, out), ...])"""
    out = []
    for at in words_of(prog, OP_LOAD_STORE):
        n = (int(prog[at]) & 0xFFFF) - 1
        out.append((at, [(int(prog[at + 1 + k]), int(prog[at + 2 + k])) for k in range(0, n - 1, 2)]))
    return out


def resolve(pairs):
    """the live pairs of lists in program order -- {destination: source}, every source an input of the frame: a pair reads what an
    earlier pair left in its source, the last writer of a slot wins, a slot that gets its own word back is untouched"""
    sym = {}
    for a, b in pairs:
        s = sym.get(a, a)
        if s == b:
            sym.pop(b, None)
        else:
            sym[b] = s
    return sym


def all_pairs(c):
    return [p for it in c["head"] + c["items"] if it["kind"] == "copies" for p in it["pairs"]]


def windows(cores, nin, nout):
    """(input stride from IO IN, output stride from IO 0) that cover the chains and every live pair"""
    live = {}
    for c in cores:
        live.update(resolve(all_pairs(c)))
    hi_in = max([IN + max(nin, 1) - 1] + list(live.values()))
    lo_in = min([IN] + list(live.values()))
    assert lo_in >= IN, "pair sources lie in the input window"
    return hi_in - IN + 1, max([max(nout, 1) - 1] + list(live.keys())) + 1

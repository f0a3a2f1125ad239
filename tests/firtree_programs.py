"""Programs for the "mem_fir" tests: memory-word trees with a DSP_FIR in a trunk or a branch, built with the encoder
like tests/memtree_programs.py's -- cores of [TPDF_CALC] + items in program order, an item being

    trunk(key, ...)     LOAD | LOAD_GAIN, [BIQUADS], [FIR], STORE_MEM(word of `key`)
    branch(key, ...)    LOAD_MEM(word of `key`), [BIQUADS], [FIR], then what firtail_programs.chain() describes behind its FIR
    plain(...)          an ordinary chain, firtail_programs.chain()

    copies([...])       one DSP_LOAD_STORE list (copy_programs.copies(); a core's `head`: lists in front of its TPDF_CALC)

An item with a "mux" entry, [(input, gain), ...], starts with a LOAD_MUX of that table instead of its LOAD; one with a "store_to" entry
stores to the IOs named (copy_programs.stores_to()).  A key without a trunk in its core is a word that core only reads.  Every trunk and every ordinary chain takes the next input from IO
IN, every STORE the next output from IO 0; encoded for 44.1 and 48 kHz with an impulse per rate (another one, of another length, at
44.1 kHz).  program() returns the words' indices by key."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from tests import firtail_programs as fp
from tests import memtree_programs as mp
from tests.delay_programs import F44100, F48000
from tests.firtail_programs import fir_words, impulse, words_of          # noqa: F401  (the tests take them from here)
from tests.fuzz_programs import _prototypes
from tests.memtree_programs import IN, mem_ops, set_word                  # noqa: F401

FPEAK = fp.FPEAK


def trunk(key, nsec=2, taps=0, load_gain=0.5, bank=None, odd=None):
    """taps: the FIR's length at 48 kHz (0: none); odd: "bypass" (a DSP_FIR whose impulses have length 0), "pure_delay", "two_firs",
    "front" (a DSP_DELAY in front of the FIR), "store" (a STORE behind the STORE_MEM)"""
    return dict(kind="trunk", key=key, nsec=nsec, taps=taps, load_gain=load_gain, bank=bank, odd=odd, slot=None, form="fixed", us=0, max_us=0,
                finish="none", gain=0.0, stores=0)


def branch(key, **kw):
    """firtail_programs.chain()'s arguments (load_gain is unused), plain unless asked otherwise: no delay, SAT0DB"""
    kw.setdefault("slot", None)
    kw.setdefault("finish", "sat")
    c = fp.chain(**kw)
    c.update(kind="branch", key=key)
    return c


def plain(**kw):
    kw.setdefault("slot", None)
    kw.setdefault("finish", "sat")
    c = fp.chain(**kw)
    c.update(kind="plain", key=None)
    return c


def core(items, calc=None, head=()):
    """head: items (lists) in front of the core's TPDF_CALC"""
    return dict(items=items, calc=calc, head=list(head))


def program(fmt, cores, capacity=1 << 21, pairs=(), lines_last=False):
    """-> (program words, number of inputs, number of outputs, {key: word index}).  pairs: keys laid out as one dspMem_LocationMultiple(2)
    each (the second word pair is unused): room to move an opcode's offset by one word.  lines_last: the delay parameters in a PARAM
    region of their own behind every other parameter, as tests/muxtail_programs.py lays them out (the header's maxOpcode takes a
    [samples : us] word in front of another parameter's head for an opcode, and a line of more samples than there are opcodes makes a
    program the runtimes refuse)"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.dsp_LOAD_MEM.argtypes = [C.c_int]
    L.dsp_STORE_MEM.argtypes = [C.c_int]
    L.dspLoadStore_Data.argtypes = [C.c_int, C.c_int]
    nin, nout, words = [0], [0], {}
    items = [it for c in cores for it in c["items"] if it["kind"] != "copies"]

    def build(L):
        L.dsp_PARAM()
        banks, lines, firs = {}, {}, {}
        for n, it in enumerate(items):
            if it["nsec"]:
                banks[n] = L.dspBiquad_Sections(it["nsec"])
                for k in range(it["nsec"]):
                    L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * (n % 150) + 190.0 * (k % 30), 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
        def the_lines():
            for n, it in enumerate(items):
                if it["slot"] and it["form"] == "param":
                    lines[n] = L.dspDelay_MicroSec_Max_Default(it["max_us"], it["us"])

        if not lines_last:
            the_lines()
        for n, it in enumerate(items):
            key = ("bank", it["bank"]) if it["bank"] is not None else ("chain", n)
            if (it["taps"] or it["odd"] in ("bypass", "pure_delay")) and key not in firs:
                firs[key] = L.dspFir_Impulses()
                for fs in (44100, 48000):
                    if it["odd"] == "pure_delay":
                        L.dspFir_Delay(5)
                    else:
                        t = np.zeros(0, np.float32) if it["odd"] == "bypass" else impulse(it["taps"], n if it["bank"] is None else 500 + it["bank"], fs)
                        L.dspFir_ImpulseData(t.ctypes.data_as(C.POINTER(C.c_float)), len(t))
            it["_fir"] = firs.get(key)
        for it in items:
            if it["key"] is not None and it["key"] not in words:
                words[it["key"]] = L.dspMem_LocationMultiple(2) if it["key"] in pairs else L.dspMem_Location()
        tables = {}
        if any(it.get("mux") for it in items):                 # (the tables in a PARAM region of their own, as muxtail_programs lays them out)
            L.dsp_PARAM()
            for n, it in enumerate(items):
                if it.get("mux"):
                    tables[n] = L.dspLoadMux_Inputs(len(it["mux"]))
                    for io, g in it["mux"]:
                        L.dspLoadMux_Data(IN + io, g)
        if lines_last and any(it["slot"] and it["form"] == "param" for it in items):
            L.dsp_PARAM()
            the_lines()

        def a_list(it):
            L.dsp_LOAD_STORE()
            for a, b in it["pairs"]:
                L.dspLoadStore_Data(a, b)

        def delay(it, n):
            if it["form"] == "param":
                L.dsp_DELAY(lines[n])
            else:
                L.dsp_DELAY_FixedMicroSec(it["us"])

        def store():
            L.dsp_STORE(nout[0])
            nout[0] += 1

        n = 0
        for c in cores:
            L.dsp_CORE()
            for it in c.get("head", ()):
                a_list(it)
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            for it in c["items"]:
                if it["kind"] == "copies":
                    a_list(it)
                    continue
                odd = it["odd"]
                if it["kind"] == "branch":
                    L.dsp_LOAD_MEM(words[it["key"]])
                elif it.get("mux"):
                    L.dsp_LOAD_MUX(tables[n])
                else:
                    if it["load_gain"] is None:
                        L.dsp_LOAD(IN + nin[0])
                    else:
                        L.dsp_LOAD_GAIN_Fixed(IN + nin[0], it["load_gain"])
                    nin[0] += 1
                if it["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if odd == "front":
                    L.dsp_DELAY_FixedMicroSec(1000)
                if it["_fir"] is not None:
                    L.dsp_FIR(it["_fir"])
                    if odd == "two_firs":
                        L.dsp_FIR(it["_fir"])
                if it["kind"] == "trunk":
                    L.dsp_STORE_MEM(words[it["key"]])
                    if odd == "store":
                        store()
                    n += 1
                    continue
                if it["slot"] == "A":
                    delay(it, n)
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
                    delay(it, n)
                if it.get("store_to") is not None:
                    for io in it["store_to"]:
                        L.dsp_STORE(io)
                else:
                    for _ in range(it["stores"]):
                        store()
                n += 1

    prog = enc.encode(build, 2 if fmt == 2 else 6, F44100, F48000, max_io=1024, capacity=capacity)
    return prog, nin[0], nout[0], words


def has_fir(it):
    return bool(it["taps"]) and it["odd"] is None


def is_handed(it):
    return has_fir(it) and (it["slot"] is not None or it["finish"] in ("tpdf", "gain", "tpdf_gain"))


def fir_counts(c):
    """what mem_fir_info() says of a core: (trunks with a FIR, branches with a FIR, those of these branches that are handed)"""
    b = [it for it in c["items"] if it["kind"] == "branch" and has_fir(it)]
    return (sum(it["kind"] == "trunk" and has_fir(it) for it in c["items"]), len(b), sum(is_handed(it) for it in b))


def mem_counts(c):
    return mp.counts(c)


def tail_counts(c):
    """what fir_tail_info() says of a core: (handed FIR chains, those of them with a delay)"""
    h = [it for it in c["items"] if it["kind"] != "trunk" and is_handed(it)]
    return (len(h), sum(it["slot"] is not None for it in h))

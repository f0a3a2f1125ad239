"""Programs for the memory-word tests ("chain_mem"), built with the encoder like tests/delay_programs.py's: cores of
[TPDF_CALC] + items in program order, an item being

    trunk(key, ...)     LOAD | LOAD_GAIN, [BIQUADS], STORE_MEM(word of `key`)
    branch(key, ...)    LOAD_MEM(word of `key`), then what delay_programs.chain() describes behind its load
    plain(...)          an ordinary chain, delay_programs.chain()

A key without a trunk in its core is a word that core only reads.  Every trunk and every ordinary chain takes the next input from IO
IN, every STORE the next output from IO 0; encoded for 44.1 and 48 kHz.  program() returns the words' indices by key."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from tests import delay_programs as dp
from tests.delay_programs import F44100, F48000, FPEAK, words_of          # noqa: F401
from tests.fuzz_programs import _prototypes

OP_LOAD_MEM, OP_STORE_MEM = 39, 40
IN = 512                                                       # first input IO (the wide trees store more than 128 outputs)


def trunk(key, nsec=2, load_gain=0.5, odd=None):
    """odd: a trunk the lowering refuses -- "store", "sat", "delay" (that opcode behind the STORE_MEM), "front" (the STORE_MEM in front of the
    bank), "between" (between two banks), "fir" (a DSP_FIR in front of it), "mux" (a LOAD_MUX head), "from_mem" (a LOAD_MEM head)"""
    return dict(kind="trunk", key=key, nsec=nsec, load_gain=load_gain, odd=odd)


def branch(key, **kw):
    """delay_programs.chain()'s arguments (load_gain is unused); odd "fir": a DSP_FIR behind the bank"""
    kw.setdefault("slot", None)
    c = dp.chain(**kw)
    c.update(kind="branch", key=key)
    return c


def plain(**kw):
    """odd "gain_of": the chain's LOAD_GAIN takes its gain from the memory word `key`; "mux": a LOAD_MUX head; "fir": a DSP_FIR behind the bank"""
    key = kw.pop("key", None)
    kw.setdefault("slot", None)
    c = dp.chain(**kw)
    c.update(kind="plain", key=key)
    return c


def core(items, calc=None):
    return dict(items=items, calc=calc)


def program(fmt, cores, pairs=()):
    """-> (program words, number of inputs, number of outputs, {key: word index}).  pairs: keys laid out as one dspMem_LocationMultiple(2)
    each (the second word pair is unused): room to move an opcode's offset by one word"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.dsp_LOAD_MEM.argtypes = [C.c_int]
    L.dsp_STORE_MEM.argtypes = [C.c_int]
    nin, nout, words = [0], [0], {}

    def build(L):
        L.dsp_PARAM()
        banks, lines, n = {}, {}, 0
        for c in cores:
            for it in c["items"]:
                if it["nsec"]:
                    banks[n] = L.dspBiquad_Sections(it["nsec"])
                    for k in range(it["nsec"]):
                        L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * (n % 150) + 190.0 * (k % 30), 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
                if it.get("odd") == "between":
                    banks[-1 - n] = L.dspBiquad_Sections(1)
                    L.dsp_Filter2ndOrder(FPEAK, 500.0, 0.9, 1.01)
                n += 1
        n = 0
        for c in cores:
            for it in c["items"]:
                if it["kind"] != "trunk" and it["slot"] and it["form"] == "param":
                    lines[n] = L.dspDelay_MicroSec_Max_Default(it["max_us"], it["us"])
                n += 1
        odds = {it.get("odd") for c in cores for it in c["items"]}
        fir = mux = None
        if "fir" in odds:
            taps = np.linspace(0.3, -0.1, 8).astype(np.float32)
            fir = L.dspFir_Impulses()
            for _ in (F44100, F48000):
                L.dspFir_ImpulseData(taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps))
        if "mux" in odds:
            mux = L.dspLoadMux_Inputs(2)
            L.dspLoadMux_Data(IN, 0.3)
            L.dspLoadMux_Data(IN + 1, -0.2)
        for c in cores:
            for it in c["items"]:
                if it["key"] is not None and it["key"] not in words:
                    words[it["key"]] = L.dspMem_LocationMultiple(2) if it["key"] in pairs else L.dspMem_Location()

        def delay(it, n):
            if it["form"] == "param":
                L.dsp_DELAY(lines[n])
            else:
                L.dsp_DELAY_FixedMicroSec(it["us"])

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
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            for it in c["items"]:
                odd = it.get("odd")
                if it["kind"] == "trunk":
                    if odd == "mux":
                        L.dsp_LOAD_MUX(mux)
                    elif odd == "from_mem":
                        L.dsp_LOAD_MEM(words[it["key"]])
                    else:
                        load(it)
                    if odd == "front":
                        L.dsp_STORE_MEM(words[it["key"]])
                    if it["nsec"]:
                        L.dsp_BIQUADS(banks[n])
                    if odd == "fir":
                        L.dsp_FIR(fir)
                    if odd == "between":
                        L.dsp_STORE_MEM(words[it["key"]])
                        L.dsp_BIQUADS(banks[-1 - n])
                        L.dsp_SAT0DB()
                        store()
                    elif odd == "front":
                        L.dsp_SAT0DB()
                        store()
                    else:
                        L.dsp_STORE_MEM(words[it["key"]])
                    if odd == "store":
                        store()
                    elif odd == "sat":
                        L.dsp_SAT0DB()
                        store()
                    elif odd == "delay":
                        L.dsp_DELAY_FixedMicroSec(1000)
                        store()
                    n += 1
                    continue
                if it["kind"] == "branch":
                    L.dsp_LOAD_MEM(words[it["key"]])
                elif odd == "gain_of":
                    L.dsp_LOAD_GAIN(IN + nin[0], words[it["key"]])
                    nin[0] += 1
                elif odd == "mux":
                    L.dsp_LOAD_MUX(mux)
                else:
                    load(it)
                if it["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if odd == "fir":
                    L.dsp_FIR(fir)
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
                for _ in range(it["stores"]):
                    store()
                n += 1

    prog = enc.encode(build, 2 if fmt == 2 else 6, F44100, F48000, max_io=1024, capacity=1 << 20)
    return prog, nin[0], nout[0], words


def counts(c):
    """what mem_info() says of a core: (trunks, branches, branches of words the core does not write)"""
    written = {it["key"] for it in c["items"] if it["kind"] == "trunk"}
    b = [it for it in c["items"] if it["kind"] == "branch"]
    return (len(written), len(b), sum(it["key"] not in written for it in b))


def mem_ops(prog):
    """the LOAD_MEM and STORE_MEM opcodes in program order: (opcode word, target word)"""
    at = sorted(words_of(prog, OP_LOAD_MEM) + words_of(prog, OP_STORE_MEM))
    return [(op, op + int(np.int32(prog[op + 1]))) for op in at]


def set_word(buf, word, value, fmt):
    """both words of a memory word: `value` as the format's accumulator (a double, or in format 2 the 64-bit product of an s.31 sample
    and a Q4.28 gain, which BIQUADS and SAT0DB shift down by 28 bits)"""
    raw = np.array([int(round(value * (1 << 59)))], dtype=np.int64) if fmt == 2 else np.array([value], dtype=np.float64)
    buf[word:word + 2] = raw.view(np.uint32)

"""Programs for the "chain_ways" tests, built with the encoder like tests/firtree_programs.py's: cores of [TPDF_CALC] +
items in program order, an item being

    chain(...)                 LOAD | LOAD_GAIN | LOAD_MEM(word of `key`), then a way
    fork(head, way_a, way_b)   HEAD, COPYXY, <way A>, SWAPXY, <way B>   (head(): a LOAD, a LOAD_GAIN, or the LOAD_MEM of a key)
    trunk(key, ...)            LOAD | LOAD_GAIN, [BIQUADS], STORE_MEM(word of `key`)
    raw([...])                 opcodes as they are given -- the forms the lowering refuses

and a way()  [BIQUADS], [ops], [FIR], [DELAY in slot A], [SAT0DB | dressed finish | none], [DELAY in slot B], STORE+  with
ops=[("gain", g) | "neg", ...] a run of DSP_GAIN and DSP_NEGX.  Every LOAD takes the next input from IO IN, every STORE the next output
from IO 0; encoded for 44.1 and 48 kHz (an impulse per rate).  program() returns the memory words' indices by key."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from tests.delay_programs import F44100, F48000, samples          # noqa: F401  (the tests take them from here)
from tests.finish_programs import FPEAK, resealed, words_of       # noqa: F401
from tests.firtail_programs import impulse
from tests.fuzz_programs import _prototypes
from tests.memtree_programs import IN, set_word                   # noqa: F401

OP_SWAPXY, OP_COPYXY, OP_NEGX, OP_GAIN = 11, 12, 23, 41          # include/avdsp_format.h
XY = ("COPYYX", "CLRXY", "ADDXY", "ADDYX", "SUBXY", "SUBYX", "MULXY", "DIVXY", "DIVYX", "AVGXY", "AVGYX", "NEGY")


def way(nsec=0, ops=(), taps=0, slot=None, form="fixed", us=0, max_us=None, finish="sat", gain=0.9, stores=1):
    """finish: "sat", "none", "tpdf", "gain", "tpdf_gain"; slot: "A", "B" or None; form: "fixed" or "param" """
    return dict(nsec=nsec, ops=list(ops), taps=taps, slot=slot, form=form, us=us, max_us=max_us if max_us is not None else 2 * us + 50,
                finish=finish, gain=gain, stores=stores)


def head(load_gain=0.5, key=None):
    return dict(load_gain=load_gain, key=key)


def chain(load_gain=0.5, key=None, **kw):
    return dict(kind="chain", head=head(load_gain, key), ways=[way(**kw)])


def fork(hd, way_a, way_b):
    return dict(kind="fork", head=hd, ways=[way_a, way_b])


def trunk(key, nsec=1, load_gain=0.5):
    return dict(kind="trunk", head=head(load_gain), key=key, nsec=nsec, ways=[])


def raw(steps):
    """steps: ("load", gain | None), ("load_mem", key), ("load_mux",), ("copyxy",), ("swapxy",), ("biquads", n), ("gain", g), ("gain_of", key: the GAIN
    takes its parameter from that memory word), ("neg",),
    ("fir", taps), ("delay", us), ("sat",), ("tpdf",), ("store",), ("store_mem", key), ("xy", name of XY), ("nop",)"""
    return dict(kind="raw", steps=list(steps), ways=[])


def core(items, calc=None):
    return dict(items=items, calc=calc)


def _way_steps(w):
    s = []
    if w["nsec"]:
        s.append(("biquads", w["nsec"]))
    for op in w["ops"]:
        s.append(("neg",) if op == "neg" else ("gain", op[1]))
    if w["taps"]:
        s.append(("fir", w["taps"]))
    d = ("delay", w["us"], w["form"], w["max_us"])
    if w["slot"] == "A":
        s.append(d)
    f = w["finish"]
    if f != "none":
        s.append({"sat": ("sat",), "tpdf": ("tpdf",), "gain": ("sat_gain", w["gain"]), "tpdf_gain": ("tpdf_gain", w["gain"])}[f])
    if w["slot"] == "B":
        s.append(d)
    return s + [("store",)] * w["stores"]


def steps_of(it):
    if it["kind"] == "raw":
        return it["steps"]
    h = it["head"]
    s = [("load_mem", h["key"])] if h["key"] is not None else [("load", h["load_gain"])]
    if it["kind"] == "trunk":
        return s + ([("biquads", it["nsec"])] if it["nsec"] else []) + [("store_mem", it["key"])]
    if it["kind"] == "fork":
        return s + [("copyxy",)] + _way_steps(it["ways"][0]) + [("swapxy",)] + _way_steps(it["ways"][1])
    return s + _way_steps(it["ways"][0])


def program(fmt, cores, capacity=1 << 21, max_io=1024):
    """-> (program words, number of inputs, number of outputs, {key: word index})"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.dsp_LOAD_MEM.argtypes = [C.c_int]
    L.dsp_STORE_MEM.argtypes = [C.c_int]
    nin, nout, words = [0], [0], {}
    steps = [[steps_of(it) for it in c["items"]] for c in cores]
    flat = [st for c in steps for it in c for st in it]

    def build(L):
        L.dsp_PARAM()
        banks, firs, lines = {}, {}, {}
        for n, st in enumerate(flat):
            if st[0] == "biquads":
                banks[n] = L.dspBiquad_Sections(st[1])
                for k in range(st[1]):
                    L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * (n % 150) + 190.0 * (k % 30), 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
        for n, st in enumerate(flat):
            if st[0] == "delay" and len(st) > 2 and st[2] == "param":
                lines[n] = L.dspDelay_MicroSec_Max_Default(st[3], st[1])
        for n, st in enumerate(flat):
            if st[0] == "fir":
                firs[n] = L.dspFir_Impulses()
                for fs in (44100, 48000):
                    t = impulse(st[1], n, fs)
                    L.dspFir_ImpulseData(t.ctypes.data_as(C.POINTER(C.c_float)), len(t))
        for st in flat:
            if st[0] in ("load_mem", "store_mem", "gain_of") and st[1] not in words:
                words[st[1]] = L.dspMem_Location()
        mux = None
        if any(st[0] == "load_mux" for st in flat):
            L.dsp_PARAM()
            mux = L.dspLoadMux_Inputs(2)
            L.dspLoadMux_Data(IN, 0.3)
            L.dspLoadMux_Data(IN + 1, -0.2)
        n = 0
        for c, its in zip(cores, steps):
            L.dsp_CORE()
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            for it in its:
                for st in it:
                    k = st[0]
                    if k == "load":
                        if st[1] is None:
                            L.dsp_LOAD(IN + nin[0])
                        else:
                            L.dsp_LOAD_GAIN_Fixed(IN + nin[0], st[1])
                        nin[0] += 1
                    elif k == "load_mem":
                        L.dsp_LOAD_MEM(words[st[1]])
                    elif k == "store_mem":
                        L.dsp_STORE_MEM(words[st[1]])
                    elif k == "load_mux":
                        L.dsp_LOAD_MUX(mux)
                        nin[0] = max(nin[0], 2)
                    elif k == "copyxy":
                        L.dsp_COPYXY()
                    elif k == "swapxy":
                        L.dsp_SWAPXY()
                    elif k == "biquads":
                        L.dsp_BIQUADS(banks[n])
                    elif k == "gain":
                        L.dsp_GAIN_Fixed(st[1])
                    elif k == "gain_of":
                        L.dsp_GAIN(words[st[1]])
                    elif k == "neg":
                        L.dsp_NEGX()
                    elif k == "fir":
                        L.dsp_FIR(firs[n])
                    elif k == "delay":
                        if n in lines:
                            L.dsp_DELAY(lines[n])
                        else:
                            L.dsp_DELAY_FixedMicroSec(st[1])
                    elif k == "sat":
                        L.dsp_SAT0DB()
                    elif k == "tpdf":
                        L.dsp_SAT0DB_TPDF()
                    elif k == "sat_gain":
                        L.dsp_SAT0DB_GAIN_Fixed(st[1])
                    elif k == "tpdf_gain":
                        L.dsp_SAT0DB_TPDF_GAIN_Fixed(st[1])
                    elif k == "store":
                        L.dsp_STORE(nout[0])
                        nout[0] += 1
                    elif k == "xy":
                        getattr(L, "dsp_" + st[1])()
                    elif k == "nop":
                        L.dsp_NOP()
                    else:
                        raise ValueError(st)
                    n += 1

    prog = enc.encode(build, 2 if fmt == 2 else 6, F44100, F48000, max_io=max_io, capacity=capacity)
    return prog, nin[0], nout[0], words


def counts(c):
    """what ways_info() and core_info()["chains"] say of a core: (forks, chains with a run of GAIN / NEGX), chains"""
    forks = sum(it["kind"] == "fork" for it in c["items"])
    ops = sum(bool(w["ops"]) for it in c["items"] for w in it["ways"])
    chains = sum(len(it["ways"]) if it["kind"] != "trunk" else 1 for it in c["items"])
    return (forks, ops), chains


def gain_words(prog):
    """per DSP_GAIN, in program order: the program word of its parameter"""
    return [at + int(np.int32(prog[at + 1])) for at in words_of(prog, OP_GAIN)]

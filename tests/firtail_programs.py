"""Programs for the handed-FIR tests ("fir_tail"), built with the encoder like tests/delay_programs.py's: cores of
[TPDF_CALC] + N x (LOAD | LOAD_GAIN, [BIQUADS], [FIR], [DELAY in slot A], [SAT0DB | dressed finish | none], [DELAY in slot B], STORE+)
with inputs at IO IN.., outputs from IO 0, encoded for 44.1 and 48 kHz (an impulse per rate)."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from tests.delay_programs import F44100, F48000, FACTOR, OP_DELAY, line_words, samples, us_words      # noqa: F401  (the tests take them from here)
from tests.finish_programs import FINISHES, FPEAK, IN, resealed, words_of          # noqa: F401
from tests.fuzz_programs import _prototypes

OP_FIR = 51


def impulse(taps, seed, fs=48000):
    """the impulse of `taps` taps at 48 kHz; at 44.1 kHz another one, of another length"""
    n = taps if fs == 48000 else max(1, (2 * taps) // 3)
    rng = np.random.default_rng(1000 * seed + n)
    return (rng.standard_normal(n) * (0.7 / np.sqrt(n))).astype(np.float32)


def chain(nsec=2, taps=64, slot="A", form="fixed", us=1000, max_us=None, finish="tpdf_gain", gain=0.9, stores=1, load_gain=0.5, bank=None, odd=None):
    """taps: the FIR's length at 48 kHz (0: no DSP_FIR); bank: chains of one number share one impulse bank (else each has its own);
    slot: "A" (in front of the SAT0DB slot), "B" (behind it), None (no delay); form: "fixed" or "param"; finish: "sat", "none", "tpdf",
    "gain", "tpdf_gain"; odd: "bypass" (a DSP_FIR whose impulses have length 0), "pure_delay" (the FIR's delay variant), "dp", "d1"
    (that delay opcode in slot A), "front" (the delay in front of the FIR), "two_firs" (a second DSP_FIR behind the first),
    "mux" (a LOAD_MUX head)"""
    return dict(nsec=nsec, taps=taps, slot=slot, form=form, us=us, max_us=max_us if max_us is not None else 2 * us + 50, finish=finish,
                gain=gain, stores=stores, load_gain=load_gain, bank=bank, odd=odd)


def core(chains, calc=None):
    return dict(chains=chains, calc=calc)


def program(fmt, cores, capacity=1 << 20):
    """-> (program words, number of inputs, number of outputs)"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    nin = sum(len(c["chains"]) for c in cores)
    nout = [0]

    def build(L):
        L.dsp_PARAM()
        banks, lines, firs, n = {}, {}, {}, 0
        for c in cores:
            for ch in c["chains"]:
                if ch["nsec"]:
                    banks[n] = L.dspBiquad_Sections(ch["nsec"])
                    for k in range(ch["nsec"]):
                        L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * n + 190.0 * k, 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
                n += 1
        n = 0
        for c in cores:
            for ch in c["chains"]:
                if ch["slot"] and ch["form"] == "param":
                    lines[n] = L.dspDelay_MicroSec_Max_Default(ch["max_us"], ch["us"])
                n += 1
        n = 0
        for c in cores:
            for ch in c["chains"]:
                key = ("bank", ch["bank"]) if ch["bank"] is not None else ("chain", n)
                if (ch["taps"] or ch["odd"] in ("bypass", "pure_delay")) and key not in firs:
                    firs[key] = L.dspFir_Impulses()
                    for fs in (44100, 48000):                  # (an impulse per rate)
                        if ch["odd"] == "pure_delay":
                            L.dspFir_Delay(5)
                        else:
                            t = np.zeros(0, np.float32) if ch["odd"] == "bypass" else impulse(ch["taps"], n if ch["bank"] is None else 500 + ch["bank"], fs)
                            L.dspFir_ImpulseData(t.ctypes.data_as(C.POINTER(C.c_float)), len(t))
                ch["_fir"] = firs.get(key)
                n += 1
        mux = None
        if any(ch["odd"] == "mux" for c in cores for ch in c["chains"]):
            mux = L.dspLoadMux_Inputs(2)
            L.dspLoadMux_Data(IN, 0.3)
            L.dspLoadMux_Data(IN + 1, -0.2)
        n = 0

        def delay(ch, n):
            if ch["odd"] == "dp":
                L.dsp_DELAY_DP_FixedMicroSec(ch["us"])
            elif ch["odd"] == "d1":
                L.dsp_DELAY_1()
            elif ch["form"] == "param":
                L.dsp_DELAY(lines[n])
            else:
                L.dsp_DELAY_FixedMicroSec(ch["us"])

        for c in cores:
            L.dsp_CORE()
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            for ch in c["chains"]:
                odd = ch["odd"]
                if odd == "mux":
                    L.dsp_LOAD_MUX(mux)
                elif ch["load_gain"] is None:
                    L.dsp_LOAD(IN + n)
                else:
                    L.dsp_LOAD_GAIN_Fixed(IN + n, ch["load_gain"])
                if ch["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if odd == "front":
                    L.dsp_DELAY_FixedMicroSec(ch["us"])
                if ch["_fir"] is not None:
                    L.dsp_FIR(ch["_fir"])
                    if odd == "two_firs":
                        L.dsp_FIR(ch["_fir"])
                if ch["slot"] == "A" and odd != "front":
                    delay(ch, n)
                f = ch["finish"]
                if f == "sat":
                    L.dsp_SAT0DB()
                elif f == "tpdf":
                    L.dsp_SAT0DB_TPDF()
                elif f == "gain":
                    L.dsp_SAT0DB_GAIN_Fixed(ch["gain"])
                elif f == "tpdf_gain":
                    L.dsp_SAT0DB_TPDF_GAIN_Fixed(ch["gain"])
                if ch["slot"] == "B":
                    delay(ch, n)
                for _ in range(ch["stores"]):
                    L.dsp_STORE(nout[0])
                    nout[0] += 1
                n += 1

    prog = enc.encode(build, 6, F44100, F48000, max_io=256, capacity=capacity)
    return prog, nin, nout[0]


def handed(chains):
    """(handed FIR chains, those of them with a delay) of a core's chain list, as dspRuntimeFirTailInfo counts them"""
    h = [c for c in chains if c["taps"] and c["odd"] is None and (c["slot"] or c["finish"] in ("tpdf", "gain", "tpdf_gain"))]
    return (len(h), sum(1 for c in h if c["slot"]))


def fir_words(prog):
    """per DSP_FIR, in program order: its opcode word"""
    return words_of(prog, OP_FIR)

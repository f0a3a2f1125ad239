"""Programs for the delay-line tests ("chain_delay"), built with the encoder like tests/finish_programs.py's: cores of
[TPDF_CALC] + N x (LOAD | LOAD_GAIN, [BIQUADS], [DELAY in slot A], [SAT0DB | dressed finish | none], [DELAY in slot B], STORE+)
with inputs at IO IN.., outputs from IO 0, encoded for 44.1 and 48 kHz."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from avdsp_amd import progbuilder as pb
from tests.finish_programs import FPEAK, IN, resealed, words_of          # noqa: F401  (the tests take them from here)
from tests.fuzz_programs import _prototypes

F44100, F48000 = 4, 5
OP_DELAY_1, OP_DELAY, OP_DELAY_DP = 46, 47, 48
FACTOR = {48000: 206158430, 44100: 189408057}                           # (unsigned)(2^32 / 10^6 x fs), dsp_runtime.c:81-90


def samples(us, fs=48000, max_us=None):
    """the line's length in samples: the runtime's formula; max_us: the parameter form's clamp (its size is laid out at 48 kHz)"""
    n = (us * FACTOR[fs]) >> 32
    return n if max_us is None else min(n, (max_us * 48000 + 500000) // 1000000)      # (the encoder rounds the size it lays out)


def chain(nsec=2, slot="A", form="fixed", us=1000, max_us=None, finish="sat", gain=0.9, stores=1, load_gain=0.5, odd=None):
    """slot: "A" (in front of the SAT0DB slot), "B" (behind it), None (no delay); form: "fixed" (dsp_DELAY_FixedMicroSec) or "param"
    (dsp_DELAY of a dspDelay_MicroSec_Max_Default(max_us, us)); finish: "sat", "none", "tpdf", "gain", "tpdf_gain";
    odd: a chain the lowering refuses -- "dp", "d1" (that opcode in slot A), "head" (the delay in front of the banks), "stored" (behind the
    first STORE), "two" (a delay in both slots), "fir", "mux" (that head), "sat_twice" (SAT0DB, DELAY, SAT0DB)"""
    return dict(nsec=nsec, slot=slot, form=form, us=us, max_us=max_us if max_us is not None else 2 * us + 50, finish=finish, gain=gain,
                stores=stores, load_gain=load_gain, odd=odd)


def core(chains, calc=None):
    return dict(chains=chains, calc=calc)


def program(fmt, cores):
    """-> (program words, number of inputs, number of outputs)"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    nin = sum(len(c["chains"]) for c in cores)
    nout = [0]

    def build(L):
        L.dsp_PARAM()
        banks, lines, n = {}, {}, 0
        for c in cores:
            for ch in c["chains"]:
                if ch["nsec"]:
                    banks[n] = L.dspBiquad_Sections(ch["nsec"])
                    for k in range(ch["nsec"]):
                        L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * n + 190.0 * k, 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
                n += 1
        n = 0
        for c in cores:                                        # (the delay parameters behind the banks: the header's maxOpcode takes a
            for ch in c["chains"]:                             # [samples : us] word in front of a bank's head for an opcode, like the reference's)
                if ch["slot"] and ch["form"] == "param":
                    lines[n] = L.dspDelay_MicroSec_Max_Default(ch["max_us"], ch["us"])
                n += 1
        odds = {ch["odd"] for c in cores for ch in c["chains"]}
        fir = mux = None
        if "fir" in odds:
            taps = np.linspace(0.3, -0.1, 8).astype(np.float32)
            fir = L.dspFir_Impulses()
            for _ in (F44100, F48000):                         # (an impulse per rate)
                L.dspFir_ImpulseData(taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps))
        if "mux" in odds:
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
                if odd == "head":
                    L.dsp_DELAY_FixedMicroSec(ch["us"])
                if ch["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if odd == "fir":
                    L.dsp_FIR(fir)
                if ch["slot"] == "A" or odd == "two":
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
                    if odd == "sat_twice":
                        L.dsp_SAT0DB()
                for k in range(ch["stores"]):
                    L.dsp_STORE(nout[0])
                    nout[0] += 1
                    if odd == "stored" and k == 0:
                        L.dsp_DELAY_FixedMicroSec(ch["us"])
                n += 1

    prog = enc.encode(build, 2 if fmt == 2 else 6, F44100, F48000, max_io=256, capacity=1 << 19)
    return prog, nin, nout[0]


def us_words(prog):
    """per DSP_DELAY of the parameter form, in program order: the word that holds its 16-bit microsecond value"""
    out = []
    for op in words_of(prog, OP_DELAY):
        off = int(np.int32(prog[op + 3]))
        if off:
            out.append(op + off)
    return out


def line_words(prog):
    """per DSP_DELAY, in program order: the index word of its line, as an index into the state area"""
    return [int(prog[op + 2]) for op in words_of(prog, OP_DELAY)]

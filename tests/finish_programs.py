"""Programs for the dressed-finish tests ("chain_finish"), built with the encoder like tests/test_gpu_strands.py's:
cores of  [TPDF_CALC] + N x (LOAD | LOAD_GAIN, [BIQUADS], <finish>, STORE+)  with inputs at IO IN.., outputs from IO 0."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from avdsp_amd import progbuilder as pb
from tests.fuzz_programs import _prototypes

FPEAK, F48000 = 74, 5
IN = 128
OP_TPDF_CALC, OP_SAT0DB_GAIN, OP_SAT0DB_TPDF_GAIN = 7, 44, 45
FINISHES = ("tpdf", "gain", "tpdf_gain")


def chain(nsec=2, finish="tpdf", gain=0.9, stores=1, load_gain=0.5, head=None):
    """finish: "sat" (plain SAT0DB), "none", or one of FINISHES; head: None, "fir", "mux", "tpdf_op" (a DSP_TPDF behind the load),
    "calc" (a TPDF_CALC behind the load)"""
    return dict(nsec=nsec, finish=finish, gain=gain, stores=stores, load_gain=load_gain, head=head)


def core(chains, calc=None):
    """calc: None, or the width word of the DSP_TPDF_CALC at the head of the core"""
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
        banks, n = {}, 0
        for c in cores:
            for ch in c["chains"]:
                if ch["nsec"]:
                    banks[n] = L.dspBiquad_Sections(ch["nsec"])
                    for k in range(ch["nsec"]):
                        L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * n + 190.0 * k, 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
                n += 1
        heads = {ch["head"] for c in cores for ch in c["chains"]}
        fir = mux = None
        if "fir" in heads:
            taps = np.linspace(0.3, -0.1, 8).astype(np.float32)
            fir = L.dspFir_Impulses()
            L.dspFir_ImpulseData(taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps))
        if "mux" in heads:
            mux = L.dspLoadMux_Inputs(2)
            L.dspLoadMux_Data(IN, 0.3)
            L.dspLoadMux_Data(IN + 1, -0.2)
        n = 0
        for c in cores:
            L.dsp_CORE()
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            for ch in c["chains"]:
                if ch["head"] == "mux":
                    L.dsp_LOAD_MUX(mux)
                elif ch["load_gain"] is None:
                    L.dsp_LOAD(IN + n)
                else:
                    L.dsp_LOAD_GAIN_Fixed(IN + n, ch["load_gain"])
                if ch["head"] == "calc":
                    L.dsp_TPDF_CALC(0)
                if ch["head"] == "tpdf_op":
                    L.dsp_TPDF(20)
                    L.dsp_LOAD_GAIN_Fixed(IN + n, 0.5)
                if ch["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if ch["head"] == "fir":
                    L.dsp_FIR(fir)
                f = ch["finish"]
                if f == "sat":
                    L.dsp_SAT0DB()
                elif f == "tpdf":
                    L.dsp_SAT0DB_TPDF()
                elif f == "gain":
                    L.dsp_SAT0DB_GAIN_Fixed(ch["gain"])
                elif f == "tpdf_gain":
                    L.dsp_SAT0DB_TPDF_GAIN_Fixed(ch["gain"])
                for _ in range(ch["stores"]):
                    L.dsp_STORE(nout[0])
                    nout[0] += 1
                n += 1

    prog = enc.encode(build, 2 if fmt == 2 else 6, F48000, F48000, max_io=256, capacity=1 << 18)
    return prog, nin, nout[0]


def words_of(prog, op):
    """word indices of the opcodes `op` in the opcode stream"""
    pos, at = 0, []
    while True:
        skip, code = int(prog[pos]) & 0xFFFF, int(prog[pos]) >> 16
        if skip == 0:
            return at
        if code == op:
            at.append(pos)
        pos += skip


def resealed(prog):
    prog[3] = pb.checksum(prog)[0]
    return prog

"""Programs for the "mux_tail" tests, built with the encoder like tests/firtail_programs.py's: cores of
[TPDF_CALC] + N x (LOAD_MUX | LOAD | LOAD_GAIN, [BIQUADS], [FIR], [DELAY in slot A], [SAT0DB | dressed finish | none], [DELAY in slot B],
STORE+) with inputs at IO IN.., outputs from IO 0, encoded for 44.1 and 48 kHz (an impulse per rate)."""
import ctypes as C

import numpy as np

from avdsp_amd import encoder as enc
from avdsp_amd import progbuilder as pb
from tests.delay_programs import F44100, F48000, FACTOR, OP_DELAY, line_words, samples, us_words      # noqa: F401  (the tests take them from here)
from tests.finish_programs import FINISHES, FPEAK, resealed, words_of          # noqa: F401
from tests.firtail_programs import impulse
from tests.fuzz_programs import _prototypes

IN = 512                                                       # first input IO (the five-kinds core stores more than 128 outputs)
OP_LOAD_MUX = pb.OP_LOAD_MUX


def chain(mux=None, nsec=0, taps=0, slot=None, form="fixed", us=1000, max_us=None, finish="sat", gain=0.9, stores=1, load_gain=0.5, inp=0, odd=None):
    """mux: the LOAD_MUX list [(input, gain)], or None: LOAD / LOAD_GAIN (load_gain None / a gain) of input `inp`;
    taps: the FIR's length at 48 kHz (0: no DSP_FIR); slot: "A" (in front of the SAT0DB slot), "B" (behind it), None (no delay);
    form: "fixed" or "param"; finish: "sat", "none", "tpdf", "gain", "tpdf_gain"; odd: a chain the lowering refuses -- "dp", "d1" (that
    delay opcode in slot A), "two" (a delay in both slots), "head" (the delay in front of the banks), "front" (the delay in front of the
    FIR)"""
    return dict(mux=mux, nsec=nsec, taps=taps, slot=slot, form=form, us=us, max_us=max_us if max_us is not None else max(2 * us + 50, 50),
                finish=finish, gain=gain, stores=stores, load_gain=load_gain, inp=inp, odd=odd)


def core(chains, calc=None):
    return dict(chains=chains, calc=calc)


def program(fmt, cores, capacity=1 << 21):
    """-> (program words, number of inputs, number of outputs)"""
    L = enc.lib()
    _prototypes(L)
    L.dspFir_ImpulseData.argtypes = [C.POINTER(C.c_float), C.c_int]
    every = [ch for c in cores for ch in c["chains"]]
    nin = 1 + max([io for ch in every if ch["mux"] for io, _ in ch["mux"]] + [ch["inp"] for ch in every if not ch["mux"]])
    nout = [0]

    def build(L):
        L.dsp_PARAM()
        banks, lines, firs, tables = {}, {}, {}, {}
        # (the tables and the delay parameters in PARAM regions of their own, the latter last: the header's maxOpcode takes a [samples : us]
        # word in front of a bank's, an impulse's or a table's head for an opcode, like the reference's)
        for n, ch in enumerate(every):
            if ch["nsec"]:
                banks[n] = L.dspBiquad_Sections(ch["nsec"])
                for k in range(ch["nsec"]):
                    L.dsp_Filter2ndOrder(FPEAK, 120.0 + 37 * (n % 97) + 190.0 * k, 0.8 + 0.05 * (k % 5), 1.02 if k % 2 else 0.97)
        for n, ch in enumerate(every):
            if ch["taps"]:
                firs[n] = L.dspFir_Impulses()
                for fs in (44100, 48000):                      # (an impulse per rate)
                    t = impulse(ch["taps"], n, fs)
                    L.dspFir_ImpulseData(t.ctypes.data_as(C.POINTER(C.c_float)), len(t))
        L.dsp_PARAM()
        for n, ch in enumerate(every):
            if ch["mux"]:
                tables[n] = L.dspLoadMux_Inputs(len(ch["mux"]))
                for io, g in ch["mux"]:
                    L.dspLoadMux_Data(IN + io, g)
        L.dsp_PARAM()
        for n, ch in enumerate(every):
            if ch["slot"] and ch["form"] == "param":
                lines[n] = L.dspDelay_MicroSec_Max_Default(ch["max_us"], ch["us"])

        def delay(ch, n):
            if ch["odd"] == "dp":
                L.dsp_DELAY_DP_FixedMicroSec(ch["us"])
            elif ch["odd"] == "d1":
                L.dsp_DELAY_1()
            elif ch["form"] == "param":
                L.dsp_DELAY(lines[n])
            else:
                L.dsp_DELAY_FixedMicroSec(ch["us"])

        n = 0
        for c in cores:
            L.dsp_CORE()
            if c["calc"] is not None:
                L.dsp_TPDF_CALC(c["calc"])
            for ch in c["chains"]:
                odd = ch["odd"]
                if ch["mux"]:
                    L.dsp_LOAD_MUX(tables[n])
                elif ch["load_gain"] is None:
                    L.dsp_LOAD(IN + ch["inp"])
                else:
                    L.dsp_LOAD_GAIN_Fixed(IN + ch["inp"], ch["load_gain"])
                if odd == "head":
                    L.dsp_DELAY_FixedMicroSec(ch["us"])
                if ch["nsec"]:
                    L.dsp_BIQUADS(banks[n])
                if odd == "front":
                    L.dsp_DELAY_FixedMicroSec(ch["us"])
                if ch["taps"]:
                    L.dsp_FIR(firs[n])
                if (ch["slot"] == "A" and odd not in ("head", "front")) or odd == "two":
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

    prog = enc.encode(build, 2 if fmt == 2 else 6, F44100, F48000, max_io=1024, capacity=capacity)
    return prog, nin, nout[0]


# ---- what the info calls have to say of a chain list --------------------------------------------------------------------------------------
def dressed(c):
    return c["finish"] in FINISHES


def kind(c):
    """the five kinds of DESIGN.md 4.2i's table for a chain behind a LOAD_MUX head ("plain" / "other head" for the rest)"""
    if not c["mux"]:
        return "other head"
    if c["taps"] and (c["slot"] or dressed(c)):
        return "fir_handed"
    if c["taps"] or not (c["slot"] or dressed(c)):
        return "plain"
    if c["nsec"]:
        return "cascade_handed" if c["slot"] else "cascade_dressed"
    return "stage_handed" if c["slot"] else "stage_finished"


def counts(chains, fs=48000):
    """mux_tail_info, finish_info()[0], delay_info, fir_tail_info of a core of these chains (which holds a LOAD_MUX head) with every option on"""
    d = [c for c in chains if c["slot"]]
    h = [c for c in chains if c["taps"] and (c["slot"] or dressed(c))]
    longest = max([samples(c["us"], fs, c["max_us"] if c["form"] == "param" else None) for c in d] + [0])
    return dict(mux_tail=(sum(map(dressed, chains)), len(d), sum(kind(c) in ("stage_handed", "stage_finished") for c in chains)),
                dressed=sum(map(dressed, chains)), delay=(len(d), longest), fir_tail=(len(h), sum(1 for c in h if c["slot"])))


# ---- the five kinds in one core (tests/test_gpu_muxtail.py) --------------------------------------------------------------------------------
SECS = [0, 2, 0, 1, 16, 0, 17, 40]
SLOTS = [None, "A", "B"]
FIN = ["tpdf_gain", "sat", "tpdf", "none", "gain"]
US = [1000, 20, 21, 63, 25000]                                # lines of 47, 0 (bypass), 1, 3 and 1199 (longer than a launch) samples at 48 kHz
NIN = 40


def _tail(i, **kw):
    us = US[(i + i // 3) % 5]
    d = dict(nsec=SECS[i % 8], slot=SLOTS[(i + i // 5) % 3], form=("fixed", "param")[(i // 2) % 2], us=us, max_us=max(us, 50), finish=FIN[(i + i // 5) % 5],
             gain=0.9 + 0.01 * (i % 7), stores=2 if i % 3 == 1 else 1)
    d.update(kw)
    return d


def _gains(rng, n):
    return [float(np.float32(v)) for v in rng.uniform(0.02, 0.45, n) * rng.choice([-1.0, 1.0], n)]


def five_kinds_chains(seed=5):
    """Three mix groups interleaved -- 16 chains on a list of 3 entries, 17 on one of 33, 65 on one of 6 (kpad 4, 36, 8) --, 15 chains of
    one more sequence (under the group minimum: mux_plain), four private lists, six LOAD / LOAD_GAIN chains; sections, slots, forms, line
    lengths, finishes and store counts cycle through all of them with periods of their own.  -> (chains, group of each chain)"""
    rng = np.random.default_rng(seed)
    seqs = {"g16": [3, 0, 7], "g17": [(5 * j + 1) % NIN for j in range(33)], "g65": [9, 8, 2, 30, 31, 39], "p15": [4, 5, 6, 11, 12]}
    left = {"g16": 16, "g17": 17, "g65": 65, "p15": 15, "private": 4, "load": 6}
    order = ["g65", "g16", "g65", "g17", "p15", "g65", "load", "g65", "g17", "private", "g16", "g65"]
    chains, group, k = [], [], 0
    while any(left.values()):
        g = order[k % len(order)]
        k += 1
        if not left[g]:
            continue
        left[g] -= 1
        i = len(chains)
        if g == "load":
            over = [dict(nsec=0, slot=None, finish="tpdf_gain"), dict(nsec=0, slot="A"), dict(nsec=2, slot="B", finish="gain"), dict(nsec=0, slot=None, finish="sat"),
                    dict(nsec=1, slot=None, finish="gain"), dict(nsec=0, slot="B", finish="tpdf")][left[g]]
            chains.append(chain(None, inp=int(rng.integers(0, NIN)), load_gain=None if i % 2 else 0.6, **_tail(i, **over)))
        elif g == "private":
            n = int(rng.integers(1, 9))
            chains.append(chain(list(zip([int(v) for v in rng.integers(0, NIN, n)], _gains(rng, n))), **_tail(i)))
        else:
            chains.append(chain(list(zip(seqs[g], _gains(rng, len(seqs[g])))), **_tail(i)))
        group.append(g)
    return chains, group


def reference_shape_cores(finish="sat", n_cores=4):
    """the reference's generic DAC program (dspprogs/oktodac.c, dspDACStereoDsp4channels), per core:
    LOAD_MUX(2) -> BIQUADS(12) -> SAT0DB -> DELAY(param, max 5000 us, default 0) -> STORE, STORE"""
    return [core([chain([(2 * k, 0.5), (2 * k + 1, -0.25 + 0.1 * k)], nsec=12, slot="B", form="param", us=0, max_us=5000, finish=finish, gain=0.95, stores=2)],
                 calc=0 if finish in FINISHES and k == 0 else None) for k in range(n_cores)]


def small_core(gain=0.9):
    """every kind once or twice: a 17-chain group (mux_tile where the format has it) and private lists (mux_plain)"""
    rng = np.random.default_rng(8)
    tails = [dict(nsec=0, finish="tpdf_gain"), dict(nsec=0, slot="A", us=1000, finish="tpdf"), dict(nsec=2, finish="gain"), dict(nsec=2, slot="B", form="param", us=63, finish="tpdf_gain"),
             dict(nsec=0, finish="sat"), dict(nsec=0, slot="B", us=21, finish="sat"), dict(nsec=17, slot="A", us=63, finish="none"), dict(nsec=1, finish="sat"),
             dict(nsec=0, slot="A", form="param", us=2100, finish="gain", stores=2)]
    chains = [chain(list(zip([1, 0, 3, 2, 4], _gains(rng, 5))), gain=gain, **tails[i % 9]) for i in range(17)]
    chains += [chain(list(zip([int(v) for v in rng.integers(0, 5, 3)], _gains(rng, 3))), gain=gain, **tails[i]) for i in (0, 1, 3, 5, 8)]
    chains += [chain(None, inp=2, load_gain=None, nsec=0, slot="A", us=63, finish="tpdf", gain=gain), chain(None, inp=4, load_gain=0.5, nsec=0, finish="tpdf_gain", gain=gain)]
    return chains



def in_place_chains(O=143, I=6):
    """O dressed chains on one list of I inputs, no sections, no delay: the stage finishes every one of them"""
    rng = np.random.default_rng(3)
    return [chain(list(zip(range(I), _gains(rng, I))), finish=FINISHES[o % 3], gain=0.8 + 0.001 * o) for o in range(O)]


def shard_cores():
    """a core of a 47-chain group and a core of a 40-chain group, the kinds cycling through both"""
    rng = np.random.default_rng(12)
    ga, gb = [0, 5, 2, 7, 1], [3, 4, 6, 8, 9, 10, 11]
    tails = [dict(nsec=0, finish="tpdf_gain"), dict(nsec=0, slot="A", us=1000, finish="tpdf"), dict(nsec=2, slot="B", form="param", us=63, finish="gain"), dict(nsec=0, finish="sat"),
             dict(nsec=1, finish="tpdf"), dict(nsec=0, slot="B", form="param", us=21, finish="sat", stores=2)]
    return [core([chain(list(zip(ga, _gains(rng, 5))), **tails[i % 6]) for i in range(47)], calc=0),
            core([chain(list(zip(gb, _gains(rng, 7))), **tails[(i + 1) % 6]) for i in range(40)])]


def fir_tail_chains():
    """LOAD_MUX -> [0 / 2 sections] -> FIR(7 / 255 taps) -> [DELAY] -> SAT0DB_TPDF_GAIN -> STORE, three plain MUX+FIR chains, and a chain
    the stage hands over and one it finishes"""
    rng = np.random.default_rng(15)
    chains = []
    for i, (nsec, taps, slot) in enumerate([(0, 7, None), (2, 255, "A"), (0, 255, "B"), (2, 7, None), (2, 7, "A"), (0, 255, None)]):
        chains.append(chain(list(zip([0, 2, 1], _gains(rng, 3))), nsec=nsec, taps=taps, slot=slot, form=("fixed", "param")[i % 2], us=1000, finish="tpdf_gain", gain=0.9 + 0.01 * i))
    chains += [chain(list(zip([1, 3], _gains(rng, 2))), nsec=n, taps=t, finish=f) for n, t, f in [(0, 7, "sat"), (2, 255, "none"), (0, 33, "sat")]]
    chains += [chain(list(zip([3, 0], _gains(rng, 2))), slot="A", us=63, finish="tpdf"), chain(list(zip([3, 1], _gains(rng, 2))), finish="gain")]
    return chains


def gpu_programs():
    """every program of tests/test_gpu_muxtail.py: name -> (formats, cores)"""
    return {"five_kinds": ((2, 4, 6), [core(five_kinds_chains()[0], calc=0)]), "reference_shape": ((2, 4, 6), reference_shape_cores()),
            "in_place": ((2, 6), [core(in_place_chains(), calc=0)]), "small_core": ((2, 4, 6), [core(small_core(), calc=0)]),
            "small_core_gain_1_1": ((2, 6), [core(small_core(1.1), calc=0)]), "shard": ((4, 6), shard_cores()), "fir_tail": ((4, 6), [core(fir_tail_chains(), calc=0)])}

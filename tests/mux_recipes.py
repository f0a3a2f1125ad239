"""Mixer programs and inputs shared by tests/golden/make_mux_goldens.py (which runs the compiled reference on them), the oracle's
golden test and the GPU tests (which re-create them where the reference does not exist).  Pure numpy.

A mixer case: `outputs` chains  LOAD_MUX(list_o) -> [BIQUADS x sections] -> [FIR taps] -> [SAT0DB] -> STORE(o), inputs at IO
outputs .. outputs+inputs-1.  `lists`:
    "shared"    every list names the inputs 0 .. entries-1 in IO order (one IO sequence: one mix group), gains of its own
    "shuffled"  every list names the same seeded permutation of them
    "twice"     the shared sequence with its first IO named again in the middle and at the end
    "private"   every list is its own seeded draw of `entries` inputs, repeats allowed, in drawn order
"""
from __future__ import annotations

import numpy as np

from avdsp_amd import progbuilder as pb

LIST_KINDS = ("shared", "shuffled", "twice", "private")


def mixer_lists(recipe: dict):
    """Per output: [(input index, gain)], in list order."""
    O, I, L, kind = recipe["outputs"], recipe["inputs"], recipe["entries"], recipe["lists"]
    rng = np.random.default_rng(recipe.get("seed", 1))
    if kind == "shared":
        seq = [j % I for j in range(L)]
    elif kind == "shuffled":
        seq = [int(v) % I for v in rng.permutation(L)]
    elif kind == "twice":
        seq = [j % I for j in range(L)]
        seq[L // 2] = seq[0]
        seq[-1] = seq[0]
    elif kind != "private":
        raise ValueError(kind)
    out = []
    for _ in range(O):
        ios = seq if kind != "private" else [int(v) for v in rng.integers(0, I, L)]
        g = rng.uniform(0.02, 0.45, L) * rng.choice([-1.0, 1.0], L)
        if L >= 3:                       # a zero gain, and two at the ends of what Q4.28 / a float mantissa hold
            g[int(rng.integers(0, L))] = 0.0
            g[int(rng.integers(0, L))] = 1.9990234
            g[int(rng.integers(0, L))] = -2.0
        out.append([(io, float(np.float32(v))) for io, v in zip(ios, g)])
    return out


def mixer_program(recipe: dict) -> np.ndarray:
    fmt, O, I, S, T = recipe["fmt"], recipe["outputs"], recipe["inputs"], recipe["sections"], recipe.get("taps", 0)
    lists = mixer_lists(recipe)
    L = recipe["entries"]
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + O * (32 + 2 * L + S * 8 + T + 16))
    taps = pb.lcg_taps_all(O, T) if T else None
    pw.core()
    for o in range(O):
        pw.param()
        table = pw.mux_inputs([(O + io, g) for io, g in lists[o]])
        bank = pw.biquad_bank(pb.synth_sections(o, S, pb.F48000, pb.F48000), bypass=recipe.get("bypass", 1)) if S else None
        imp = pw.fir_impulses([taps[o]]) if T else None
        pw.load_mux(table)
        if bank is not None:
            pw.biquads(bank, S)
        if imp is not None:
            pw.fir(imp, T)
        if recipe.get("sat", 1):
            pw.sat0db()
        pw.store(o)
    return pw.end_of_code()


def mixer_input(recipe: dict, fmt: int) -> np.ndarray:
    """LCG samples; "special": Inf, NaN, subnormal and full-scale samples (float), INT_MIN / INT_MAX / +-1 (int) sprinkled in."""
    frames, ch = recipe["frames"], recipe["channels"]
    fl = fmt in (5, 6)
    x = pb.lcg_input(frames, ch, fl, seed=recipe.get("seed", 12345))
    if recipe["kind"] == "lcg":
        return x
    if recipe["kind"] != "special":
        raise ValueError(recipe["kind"])
    rng = np.random.default_rng(recipe.get("seed", 12345))
    n = max(4, frames * ch // 7)
    at = (rng.integers(0, frames, n), rng.integers(0, ch, n))
    if fl:
        vals = np.array([np.inf, -np.inf, np.nan, 1e-40, -3e-39, 5e-45, 1.0, -1.0, 0.99999994, -0.0, 3.0e38, -1.5e-38], dtype=np.float32)
        x = x.copy()
        x[at] = vals[rng.integers(0, len(vals), n)]
        xb = x.view(np.uint32)
        xb[frames // 2, 0] = 0xFFC12345          # a negative NaN with a payload
        xb[frames - 1, ch - 1] = 0x7F800001      # a signalling one
    else:
        vals = np.array([-2147483648, 2147483647, 1, -1, 0, 2147483000, -2147483000, 255], dtype=np.int64)
        x = x.copy()
        x[at] = vals[rng.integers(0, len(vals), n)].astype(np.int32)
    return x


def mixer_cases():
    """The golden cases: formats 2, 4, 6; lists of 1, 3, 17, 64, 200 entries; shared / shuffled / twice / private; 0, 2, 17
    sections; with and without FIR (formats 4, 6); with and without SAT0DB; two ragged blocks; special samples."""
    cases = []

    def add(fmt, entries, lists, sections, taps, sat, outputs, kind="special", frames=45, block=29, **extra):
        inputs = entries if lists != "private" else min(24, max(entries, 2))
        name = f"mux_f{fmt}_n{entries}_{lists}_s{sections}_t{taps}_{'sat' if sat else 'nosat'}_{kind}" + "".join(f"_{k}{v}" for k, v in extra.items())
        prog = dict(kind="mixer", fmt=fmt, outputs=outputs, inputs=inputs, entries=entries, lists=lists, sections=sections, taps=taps,
                    sat=sat, seed=len(cases) + 11, **extra)
        cases.append(dict(name=name, fmt=fmt, program=prog, input=dict(kind=kind, frames=frames, channels=inputs, seed=900 + len(cases)),
                          out_stride=outputs, in_base=outputs, out_base=0, block=block))

    for fmt in (2, 4, 6):
        fir = fmt != 2
        # every list length, shared and private, no filter (the stage's own stores) and two sections
        for n in (1, 3, 17, 64, 200):
            add(fmt, n, "shared", 0, 0, 1, 20)
            add(fmt, n, "private", 2, 0, n % 2, 18)
        add(fmt, 17, "shuffled", 2, 0, 1, 20)
        add(fmt, 17, "twice", 0, 0, 0, 20)
        add(fmt, 64, "twice", 17, 0, 1, 17)
        add(fmt, 3, "private", 17, 0, 0, 5)
        add(fmt, 200, "shuffled", 0, 0, 0, 16, kind="lcg")
        add(fmt, 3, "shared", 2, 0, 0, 16, kind="lcg", frames=70, block=64)
        add(fmt, 17, "shared", 2, 0, 1, 20, bypass=0)                 # a bypassed bank: no filter after all
        if fir:
            add(fmt, 17, "shared", 0, 33, 1, 20)                      # FIR alone behind the head
            add(fmt, 64, "private", 2, 21, 0, 18)
            add(fmt, 3, "shuffled", 17, 40, 1, 16)
            add(fmt, 1, "shared", 0, 5, 0, 3, kind="lcg")
    return cases

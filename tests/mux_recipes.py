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


# ---------------------------------------------------------------------------------------------------------------------------------------
# Several mix groups in one core (tests/test_gpu_mux_edges.py, host-only twins in tests/test_mux_lowering.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
TAILS = ("stored", "stored_nosat", "sections", "sections_nosat", "fir", "both", "two_stores")
GROUP_TAPS = 19


def grouped_mixer_program(fmt, groups, interleave=True, seed=1, fmin=pb.F48000, fmax=pb.F48000, first_out=0):
    """One core of several mix groups.  A group is (nchains, io_sequence, tail):

        io_sequence   a list of input indices: every chain of the group names them in that order (one IO sequence; a mix group for
                      mux_tile from 16 chains on), gains of its own;
                      ("private", entries, inputs [, first]): every chain its own seeded draw of `entries` of the inputs
                      first (0) .. inputs - 1;
                      ("gain", input): LOAD_GAIN chains beside the LOAD_MUX ones
        tail          one of TAILS, or a tuple of them that the group's chains take in turn:
                      "stored" / "stored_nosat"      no filter: the stage stores the chain itself, behind SAT0DB or without
                      "sections" / "sections_nosat"  2 sections
                      "fir"                          a 19-tap FIR alone (formats 4 and 6; format 2 has no FIR: "stored" there)
                      "both"                         2 sections and the FIR (format 2: the sections)
                      "two_stores"                   no filter, SAT0DB, two STOREs of the value

    Chain c stores IO first_out + c, the second STOREs follow behind the last chain's, the inputs at IO `width` .. (width = one past the
    last stored IO).  Gains are
    seeded and differ for every chain and list position; a list of 3 entries or more holds one 0.0, one 1.9990234 and one -2.0, as
    mixer_lists' do.  `interleave`: the groups' chains alternate in program order, so a tile's chain ids are not contiguous and
    its scratch columns lie scattered.  Returns (program words, meta); meta["chains"][c] = dict(group, tail, ios, gains, out, mux, result: the
    data offset of the opcode's result word)."""
    rng = np.random.default_rng(seed)
    order = []
    if interleave:
        left = [g[0] for g in groups]
        while any(left):
            for gi in range(len(groups)):
                if left[gi]:
                    left[gi] -= 1
                    order.append(gi)
    else:
        for gi, g in enumerate(groups):
            order += [gi] * g[0]
    nch = len(order)
    seen = [0] * len(groups)
    plan = []
    for gi in order:
        n, seq, tail = groups[gi]
        k = seen[gi]
        seen[gi] += 1
        t = tail if isinstance(tail, str) else tail[k % len(tail)]
        if t not in TAILS:
            raise ValueError(t)
        if fmt == 2:
            t = {"fir": "stored", "both": "sections"}.get(t, t)
        plan.append((gi, t, seq))
    extra = sum(1 for _, t, _ in plan if t == "two_stores")
    width = first_out + nch + extra
    ninputs, longest = 1, 1
    for _, seq, _ in groups:
        if isinstance(seq, tuple) and seq[0] == "private":
            ninputs, longest = max(ninputs, seq[2]), max(longest, seq[1])
        elif isinstance(seq, tuple) and seq[0] == "gain":
            ninputs = max(ninputs, seq[1] + 1)
        else:
            ninputs, longest = max(ninputs, max(seq) + 1), max(longest, len(seq))
    nf = fmax - fmin + 1
    pw = pb.ProgramWriter(fmt, fmin, fmax, capacity=64 + nch * (48 + 2 * longest + nf * (2 * 8 + GROUP_TAPS + 4)))
    taps = pb.lcg_taps_all(nch, GROUP_TAPS)
    pw.core()
    chains, second = [], first_out + nch
    for c, (gi, t, seq) in enumerate(plan):
        pw.param()
        if isinstance(seq, tuple) and seq[0] == "gain":
            ios, g, table = [seq[1]], [float(np.float32(rng.uniform(0.1, 0.9)))], None
        else:
            ios = [int(v) for v in rng.integers(seq[3] if len(seq) > 3 else 0, seq[2], seq[1])] if isinstance(seq, tuple) else list(seq)
            L = len(ios)
            g = rng.uniform(0.02, 0.45, L) * rng.choice([-1.0, 1.0], L)
            if L >= 3:
                at = rng.choice(L, 3, replace=False)
                g[at[0]], g[at[1]], g[at[2]] = 0.0, 1.9990234, -2.0
            g = [float(np.float32(v)) for v in g]
            table = pw.mux_inputs([(width + io, v) for io, v in zip(ios, g)])
        S = 2 if t in ("sections", "sections_nosat", "both") else 0
        T = GROUP_TAPS if t in ("fir", "both") else 0
        bank = pw.biquad_bank(pb.synth_sections(c, S, fmin, fmax)) if S else None
        imp = pw.fir_impulses([taps[c]] * nf) if T else None
        if table is None:
            pw.load_gain_fixed(width + ios[0], g[0])
            result = None
        else:
            result = pw.load_mux(table)
        if bank is not None:
            pw.biquads(bank, S)
        if imp is not None:
            pw.fir(imp, T)
        if t not in ("stored_nosat", "sections_nosat"):
            pw.sat0db()
        pw.store(first_out + c)
        out = [first_out + c]
        if t == "two_stores":
            pw.store(second)
            out.append(second)
            second += 1
        chains.append(dict(group=gi, tail=t, ios=ios, gains=g, out=out, mux=table is not None, result=result))
    return pw.end_of_code(), dict(width=width, inputs=ninputs, nchains=nch, chains=chains)


def mux_tables(prog):
    """word index of the table ([(36 << 16) | n] then n x [IO][gain]) of every LOAD_MUX opcode, in program order"""
    pos, at = 0, []
    while True:
        skip, code = int(prog[pos]) & 0xFFFF, int(prog[pos]) >> 16
        if skip == 0:
            return at
        if code == pb.OP_LOAD_MUX:
            at.append(pos + int(np.int32(prog[pos + 1])))
        pos += skip


def expected_mux_info(meta, group_min=16):
    """what dspRuntimeMuxInfo has to say of a grouped_mixer_program, from its lists alone"""
    runs = {}
    for ch in meta["chains"]:
        if ch["mux"]:
            runs[tuple(ch["ios"])] = runs.get(tuple(ch["ios"]), 0) + 1
    big = [n for n in runs.values() if n >= group_min]
    return dict(mux_chains=sum(runs.values()), groups=len(big), grouped_chains=sum(big), longest_list=max(len(k) for k in runs))


ALL_TAILS = ("stored", "sections", "fir", "both", "stored_nosat", "sections_nosat", "two_stores")

SEAM_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 28, 29, 31, 32, 33, 35, 36, 37, 60, 63, 64, 65, 67, 68, 69, 96, 97, 127, 128, 129, 95)
SEAM_INPUTS = 40
ROW_TAIL_GROUPS = (16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 80, 129)


def check_seam_lengths():
    """what SEAM_LENGTHS is for: both sides of every chunk end up to 128, every residue mod 4 (the k-step's padding), and next to
    every chunk end a length on each side that is no multiple of 4"""
    for c in (32, 64, 96, 128):
        assert {c - 1, c, c + 1} <= set(SEAM_LENGTHS)
    assert {n % 4 for n in SEAM_LENGTHS} == {0, 1, 2, 3}
    assert {n % 4 for n in SEAM_LENGTHS if 28 <= n <= 37} == {n % 4 for n in SEAM_LENGTHS if 60 <= n <= 69} == {0, 1, 3}
    assert len(set(SEAM_LENGTHS)) == len(SEAM_LENGTHS) == 29 and max(SEAM_LENGTHS) == 129
    assert {(min(32, n) + 3) // 4 for n in SEAM_LENGTHS} == {1, 2, 3, 7, 8}             # k-steps of a first chunk


def several_groups(fmt):
    """16 x 3, 17 x 33 and 70 x 64 entries on three orders of the same 64 inputs, 15 x 5 (no group), 3 private lists, 2 LOAD_GAIN"""
    perm = [int(v) for v in np.random.default_rng(64).permutation(64)]
    return grouped_mixer_program(fmt, [
        (16, list(range(3)), ALL_TAILS),
        (17, list(range(63, 30, -1)), ("sections", "stored", "both")),
        (70, perm, ("stored", "fir", "sections_nosat", "two_stores", "both")),
        (15, [9, 8, 7, 6, 5], ("stored_nosat", "sections")),
        (3, ("private", 4, 64), ("stored", "sections", "fir")),
        (2, ("gain", 11), ("sections", "stored")),
    ], seed=101)


def list_seams(fmt):
    """a group of 16 chains per length of SEAM_LENGTHS: group g names input (j + g) mod 40 at position j; even groups are stored by
    the stage, odd ones sit behind two sections"""
    return grouped_mixer_program(fmt, [(16, [(j + g) % SEAM_INPUTS for j in range(L)], "stored" if g % 2 == 0 else "sections")
                                       for g, L in enumerate(SEAM_LENGTHS)], seed=202)


def row_tails(fmt):
    """groups of ROW_TAIL_GROUPS chains on 6-entry lists (kpad 8): group g names inputs g, g + 1, .. g + 5 mod 12"""
    return grouped_mixer_program(fmt, [(n, [(g + j) % 12 for j in range(6)], ALL_TAILS[g % 7:] + ALL_TAILS[:g % 7])
                                       for g, n in enumerate(ROW_TAIL_GROUPS)], seed=303)


def shard_group(fmt, nchains):
    """one group of `nchains` x 12 entries, sections and stage-stored tails in turn"""
    return grouped_mixer_program(fmt, [(nchains, [(5 * j + 3) % 12 for j in range(12)], ("sections", "stored", "stored_nosat"))], seed=404)


def live_edit(fmt):
    """groups of 17 (7 entries) and 16 (5 entries) chains and 3 private lists, in group order: chains 0 .. 16, 17 .. 32, 33 .. 35"""
    return grouped_mixer_program(fmt, [
        (17, [0, 1, 2, 3, 4, 5, 6], ("sections", "stored")),
        (16, [6, 4, 2, 0, 1], ("stored", "sections_nosat")),
        (3, ("private", 4, 7), ("stored", "sections")),
    ], interleave=False, seed=505)


def small_mixer(fmt, fir=False, fmin=pb.F48000, fmax=pb.F48000):
    """20 outputs of 5 inputs, half stored by the stage and half behind 2 sections (`fir`: behind the FIR, alone or with sections)"""
    tails = ("fir", "both", "stored", "sections") if fir else ("stored", "sections")
    return grouped_mixer_program(fmt, [(20, [0, 1, 2, 3, 4], tails)], seed=606, fmin=fmin, fmax=fmax)


def windows_program(fmt):
    """a group of 16 and 5 private lists on inputs 10 .. 16; the chains store IO 5 .."""
    return grouped_mixer_program(fmt, [
        (16, [12, 10, 16, 11], ("stored", "sections", "two_stores")),
        (5, ("private", 3, 17, 10), ("stored_nosat", "sections")),
    ], seed=707, first_out=5)


def stored_program(fmt, nchains=136):
    """`nchains` chains of one 6-entry sequence, all stored by the stage (three tiles, the last of 8 rows) and 7 private lists"""
    return grouped_mixer_program(fmt, [
        (nchains, [5, 0, 3, 1, 4, 2], ("stored", "stored_nosat")),
        (7, ("private", 3, 6), ("stored", "stored_nosat")),
    ], seed=808)


EDGE_PROGRAMS = dict(several_groups=several_groups, list_seams=list_seams, row_tails=row_tails,
                     shard_40=lambda fmt: shard_group(fmt, 40), shard_47=lambda fmt: shard_group(fmt, 47), live_edit=live_edit,
                     small_mixer=small_mixer, small_mixer_fir=lambda fmt: small_mixer(fmt, True), windows=windows_program,
                     stored=stored_program)

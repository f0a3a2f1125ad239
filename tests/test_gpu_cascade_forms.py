"""The cascade kernels in every form a default launch can take, at every block-length seam, against the oracle -- outputs and state
bit for bit in formats 2, 4 and 6: the cascade does the reference's operations in the reference's order, there is no tolerance here.

    a  biquad_pipe<FMT, 1 | 2 | 4 | 8>: groups of 4097 chains of one section count below 9.  cascade_groups gives fewer than 16 lanes per
       chain only to a group of more than 4096 chains (tests/cascade_shapes.py, pinned on the CPU by tests/test_plan_layout.py), so no
       other test launches these forms.  What they have and biquad_row has not: several chains per 16-lane row in the store mapping
       (oslot, d, ostep), section-0 lanes in the middle of a row, batches of NB = P steps, a replay mask over sub-rows of a wave,
       sections < P, and -- with 4097 chains -- a last workgroup of one chain behind xcd_remap with seven empty ones after it.
    b  the Inf / NaN replay of such a group: chains that share a row and a wave with replayed ones stay untouched.
    c  two narrow groups beside the merged biquad_row launch in one core, fanned out over the streams and one after the other.
    d  biquad_row<6>, biquad_row<4>, biquad_row<4, true> and biquad_row_i64 at EVERY block length from 1 to 224 frames, on the merged
       table and with a launch per section count.

The block lengths follow the kernels' loops.  biquad_pipe: masked batches while the pipeline fills (2 nsec - 1 steps), a steady loop
unrolled by three from batch bs = ceil(ceil((2 nsec - 1) / NB) / 3) * 3 to be = (B / NB - 4) / 3 * 3, masked batches that drain; every
length from 1 to NB (bs + 11) has fill-only blocks, the first steady triple, a second one and every exit from the loop.  The row
kernels step in batches of 16 frames: blocks below 96 frames take a plain loop, longer ones three written-out head batches, a steady
loop unrolled by SIX (it first runs at 144 frames, a second time at 240) and tail batches; 1 .. 224 has every number of tail batches
behind one turn of that loop, and a few longer blocks behind the list reach the second and third turn."""
import functools

import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import cascade_shapes as cs

pytestmark = pytest.mark.gpu

NIN = 61                        # shared input columns: chain i reads column i mod 61 (neighbours in a row never share one)


@pytest.fixture(autouse=True)
def _release():
    yield
    L = rt.lib()
    L.dspRuntimeSetOption(b"group_fanout", 1)
    L.dspRuntimeRelease()


def chain(nsec, i, *, stores=1, taps=0, col=None):
    """What a lane decides per chain varies with the chain's number on periods that no row, wave or workgroup shares: plain LOAD or
    LOAD_GAIN (three gains), with or without SAT0DB."""
    return dict(nsec=nsec, col=i % NIN if col is None else col, gain=None if i % 3 == 1 else (0.5, 1.0, 0.8125)[i % 7 % 3],
                sat=i % 5 in (0, 2, 3), stores=stores, taps=taps, seed=i)


def build(fmt, *cores):
    """A core per list of chains: chain k = PARAM{bank [, impulse]} LOAD | LOAD_GAIN, BIQUADS, [FIR], [SAT0DB], STORE [, STORE].  Outputs at
    IO 0 .. nout - 1 (every STORE a column of its own, in program order), inputs at IO nout ...  Returns (program, nout)."""
    chains = [c for core in cores for c in core]
    nout = sum(c["stores"] for c in chains)
    words = 64 + 8 * len(cores) + sum(24 + 9 * c["nsec"] + (c["taps"] + 8 if c["taps"] else 0) + 2 * c["stores"] for c in chains)
    pw = pb.ProgramWriter(fmt, capacity=words)
    at = 0
    for core in cores:
        pw.core()
        for c in core:
            pw.param()
            bank = pw.biquad_bank(pb.synth_sections(c["seed"], c["nsec"], pb.F48000, pb.F48000))
            imp = pw.fir_impulses([pb.lcg_taps(c["seed"], c["taps"])]) if c["taps"] else None
            if c["gain"] is None: pw.load(nout + c["col"])
            else: pw.load_gain_fixed(nout + c["col"], c["gain"])
            pw.biquads(bank, c["nsec"])
            if imp is not None: pw.fir(imp, c["taps"])
            if c["sat"]: pw.sat0db()
            for _ in range(c["stores"]):
                pw.store(at); at += 1
    return pw.end_of_code(), nout


def play_oracle(fmt, prog, nout, x, blocks, state_after):
    """The oracle's outputs of all the blocks and its state area after the blocks whose index is in `state_after`."""
    o = po.OracleProgram(fmt, prog)
    out = np.zeros((len(x), nout), dtype=po.sample_dtype(fmt))
    state, pos = {}, 0
    for k, b in enumerate(blocks):
        o.run_block(x[pos:pos + b], nout, nout, out=out[pos:pos + b])
        if k in state_after:
            state[k] = o.state.copy()
        pos += b
    return dict(out=out, state=state)


def play(fmt, prog, nout, x, blocks, state_after, what, fanout=1, reference=None):
    """The blocks one after the other through the device; outputs compared with the oracle's (`reference`: what play_oracle has recorded)
    after every block, the state area after the blocks of `state_after` only (a sync downloads the whole area)."""
    ref = reference if reference is not None else play_oracle(fmt, prog, nout, x, blocks, state_after)
    r = rt.Runtime(fmt, prog)
    try:
        r.set_option("group_fanout", fanout)
        pos = 0
        for k, b in enumerate(blocks):
            got = r.run_block(x[pos:pos + b], nout, nout)
            bad = np.nonzero((got.view(np.uint32) != ref["out"][pos:pos + b].view(np.uint32)).any(axis=0))[0]
            assert bad.size == 0, f"{what}: block {k} ({b} frames at {pos}): {bad.size} output columns differ, the first {bad[:12].tolist()}"
            if k in state_after:
                bad = np.nonzero(r.sync_state() != ref["state"][k])[0]
                assert bad.size == 0, f"{what}: state after block {k} ({b} frames at {pos}): {bad.size} words differ, the first {bad[:12].tolist()}"
            pos += b
    finally:
        r.set_option("group_fanout", 1)
        r.release()


# ---------------------------------------------------------------- a. the narrow forms
def narrow_chains(fmt, nsec, P, n=cs.NARROW_CHAINS):
    """n chains of one section count.  The special ones sit where the store mapping is most likely wrong -- r = 16 / P chains share a
    row, cpb = 256 / P a workgroup: two STOREs on chains 0 (first of a row), r - 1 (last of a row), cpb - 1 (last of a workgroup), cpb and
    3 cpb + r; in formats 4 and 6 a FIR of 3 to 5 taps behind chains r, 2 r - 1, 2 cpb - 1 and 2 cpb (ring stores, the to_ring word of
    flush_word).  Chain n - 1 = 4096, alone in its workgroup, and chain 4095, the last of the last full one, take one kind each; which
    one turns with the format and the section count, so that every P has both kinds at chain 4096."""
    r, cpb = 16 // P, 256 // P
    two = [0, r - 1, cpb - 1, cpb, 3 * cpb + r]
    fir = [r, 2 * r - 1, 2 * cpb - 1, 2 * cpb] if fmt != 2 else []
    fir_last = fmt != 2 and (nsec + fmt // 2) % 2 == 1
    (fir if fir_last else two).append(n - 1)
    (two if fir_last or fmt == 2 else fir).append(n - 2)
    assert len(set(two + fir)) == len(two) + len(fir)
    chains = [chain(nsec, i) for i in range(n)]
    for i in two: chains[i] = chain(nsec, i, stores=2)
    for k, i in enumerate(fir): chains[i] = chain(nsec, i, taps=3 + k % 3)
    return chains


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("nsec, n, P", cs.NARROW)
def test_narrow_forms(fmt, nsec, n, P):
    """biquad_pipe<fmt, P> over a group of 4097 chains: every block length from 1 to NB (bs + 11) -- 14 / 28 / 56 / 112 frames for
    P = 1 / 2 / 4 / 8 -- ascending, then [1, 1, 7, 1] (x1 / y1 handed over on one-frame blocks), then 1041 frames (two launches).
    State after each of the first three blocks, after the one-frame run and at the end.

    Trimmed: P = 8 in formats 4 and 6 (sections 5, 7, 8) -- the ascending list ends at 104 frames, not 112.  The oracle's 7379 frames of
    those six cases took 4.6 to 6.8 s on the CPU (2.4 * 10^8 section steps of bit-field products), every other case 0.1 to 2.3 s.  104
    = NB (bs + 10) is the first block whose steady loop makes two turns (be = (13 - 4) / 3 * 3 = 9, bs = 3), so the list keeps fill-only
    blocks, the first steady triple with each of its exits and the second triple; what it loses is the second triple's exit with one
    drain batch more (105 .. 112).  The oracle's work falls by an eighth only, to 6 s at most on the same CPU: the rest is lengths that
    must stay -- two steady triples, the one-frame blocks and the 1041-frame block over 4097 chains."""
    trimmed = P == 8 and fmt != 2
    blocks, top = cs.narrow_block_lengths(nsec, P, trimmed)
    assert top == (104 if trimmed else {1: 14, 2: 28, 4: 56, 8: 112}[P]) and blocks[top:] == [1, 1, 7, 1, 1041]
    prog, nout = build(fmt, narrow_chains(fmt, nsec, P, n))
    x = pb.lcg_input(sum(blocks), NIN, fmt == 6, seed=100 * fmt + nsec)
    play(fmt, prog, nout, x, blocks, {0, 1, 2, top + 3, len(blocks) - 1}, f"format {fmt}, {nsec} sections on {P} lanes")


# ---------------------------------------------------------------- b. Inf and NaN in a narrow group
@pytest.mark.parametrize("nsec, n, P", cs.NARROW_REPLAY)
def test_replay_in_sub_row_chains(nsec, n, P):
    """Format 6.  Wave 5 of the launch holds chains w .. w + 64 / P - 1.  Three of them meet an odd sample, each in an input column of its
    own: +Inf in the middle of block 0 (chain w + 1, inside a row), a NaN in the LAST frame of block 0 (the last chain of the wave: when
    the block ends the trace sits in the state), -Inf in block 1 (the first chain of the wave's second row); chain 4096, alone in its
    workgroup, a NaN as well.  The replayed chains must be the oracle's -- and so must every other chain, those of the same row and
    wave above all: outputs of every block, state after every block, two clean blocks behind."""
    per_wave = 64 // P
    w = 5 * per_wave
    odd = {w + 1: NIN, w + per_wave - 1: NIN + 1, w + 16 // P: NIN + 2, n - 1: NIN + 3}
    assert len(odd) == 4
    prog, nout = build(6, [chain(nsec, i, col=odd.get(i)) for i in range(n)])
    blocks = [40, 23, 17, 9]
    x = np.concatenate([pb.lcg_input(sum(blocks), NIN, True, seed=nsec), pb.lcg_input(sum(blocks), 4, True, seed=50 + nsec)], axis=1)
    xi = x.view(np.uint32)
    xi[5, NIN] = 0x7F800000; xi[39, NIN + 1] = 0x7FC00001; xi[40 + 20, NIN + 2] = 0xFF800000; xi[40 + 22, NIN + 3] = 0xFFC12345
    play(6, prog, nout, x, blocks, {0, 1, 2, 3}, f"format 6, {nsec} sections on {P} lanes, Inf / NaN")


# ---------------------------------------------------------------- c. several groups in one core
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_narrow_groups_beside_the_merged_row_launch(fmt):
    """cs.MIXED: 4097 chains of 2 sections (P = 2) and 4097 of 5 (P = 8), alternating in the program, and seven chains of 6, 9 and 16
    sections spread among them, which the merged row table takes (the first of them with two STOREs, one of 9 sections -- formats 4 and
    6 -- in front of a FIR).  With "group_fanout" 1 the two biquad_pipe launches go out on side streams beside the biquad_row launch;
    with 0 the five groups follow each other on one stream.  Ragged blocks, one reference for both."""
    assert [P for _, _, P in cs.MIXED] == [2, 8, 16, 16, 16]
    (na, count, _), (nb, _, _) = cs.MIXED[:2]
    secs = [na if k % 2 == 0 else nb for k in range(2 * count)]
    few = [nsec for nsec, k, _ in cs.MIXED[2:] for _ in range(k)]
    for k, nsec in enumerate(few):
        secs.insert(1 + 1171 * k, nsec)
    chains = [chain(nsec, i) for i, nsec in enumerate(secs)]
    chains[1] = chain(secs[1], 1, stores=2)
    if fmt != 2:
        i = secs.index(9)
        chains[i] = chain(9, i, taps=4)
    assert sorted((nsec, secs.count(nsec)) for nsec in set(secs)) == sorted((nsec, k) for nsec, k, _ in cs.MIXED)
    prog, nout = build(fmt, chains)
    blocks = [33, 1, 100, 7, 16, 2]
    x = pb.lcg_input(sum(blocks), NIN, fmt == 6, seed=fmt)
    after = {0, 1, len(blocks) - 1}
    ref = play_oracle(fmt, prog, nout, x, blocks, after)
    for fanout in (1, 0):
        play(fmt, prog, nout, x, blocks, after, f"format {fmt}, group_fanout {fanout}", fanout=fanout, reference=ref)


# ---------------------------------------------------------------- d. the row kernels at every block length
ROW_TOP = 224                                           # 16 * (3 + 11), by the rule of the narrow forms
ROW_BLOCKS = list(range(1, ROW_TOP + 1)) + [1, 1, 7, 1] + [240, 255, 257, 337]      # (behind the list: two and three turns of the steady loop)
ROW_STATE_AFTER = {0, 1, 2, ROW_TOP + 3, len(ROW_BLOCKS) - 1}


@functools.lru_cache(maxsize=None)
def row_case(fmt):
    """Core 1: chains of 1 .. 16 sections (cs.ROWS); in formats 4 and 6 a second set of 16 in front of a 3-tap FIR; three chains with two
    STOREs (2, 9 and 16 sections: their waves take the general flush, the others the lean steady stores).  Every section count of that
    core has chains that store samples, so its format-4 launches are biquad_row<4, true> (the accumulator leaves the cascade), on the
    merged table and apart.  Core 2 (formats 4 and 6): sixteen chains more, 1 .. 16 sections, ALL in front of a FIR -- biquad_row<4>, and
    biquad_row<6> with nothing but ring stores.  The 26 000 frames take the FIR chains' rings of 4096 floats past their end six times, at
    positions that are no multiple of 16.  The oracle runs once per format."""
    core = [chain(nsec, nsec - 1) for nsec, _, _ in cs.ROWS]
    if fmt != 2:
        core += [chain(nsec, 16 + nsec - 1, taps=3) for nsec, _, _ in cs.ROWS]
    core += [chain(nsec, 32 + k, stores=2) for k, nsec in enumerate((2, 9, 16))]
    fed = [chain(nsec, 35 + nsec - 1, taps=3) for nsec, _, _ in cs.ROWS] if fmt != 2 else []
    prog, nout = build(fmt, core, fed) if fed else build(fmt, core)
    x = pb.lcg_input(sum(ROW_BLOCKS), NIN, fmt == 6, seed=7 + fmt)
    return prog, nout, x, play_oracle(fmt, prog, nout, x, ROW_BLOCKS, ROW_STATE_AFTER)


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("fanout", [1, 0])
def test_row_kernels_at_every_block_length(fmt, fanout):
    """Every block length from 1 to 224, ascending, then [1, 1, 7, 1], then 240, 255, 257 and 337 frames: once on the merged table
    ("group_fanout" 1: one launch per core, rows of sixteen lengths) and once with a launch per section count.  State after the first
    three blocks, after the one-frame run and at the end."""
    assert ROW_BLOCKS[:ROW_TOP] == list(range(1, 225)) and ROW_BLOCKS[ROW_TOP:ROW_TOP + 4] == [1, 1, 7, 1]
    prog, nout, x, ref = row_case(fmt)
    play(fmt, prog, nout, x, ROW_BLOCKS, ROW_STATE_AFTER, f"format {fmt}, group_fanout {fanout}", fanout=fanout, reference=ref)

"""fir_shared<FMT, R> with R FORCED through "fir_rows" and proved through "fir_shared_rows": every row-tile variant
(R = 1, 2, 4 in format 6; 1, 2 in format 4) against the oracle, word for word -- the outputs of every block and the state at the end --
on both sides of the k-step count's seams, on the edges of a wave's 16 R and a workgroup's 64 R frames, on ragged column groups, across
the wrap of the FIR ring, with Inf / NaN / subnormal samples, and with a LOAD_MUX head in front of the shared bank."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

DEFAULTS = (("fir_shared", 1), ("overlap", 0), ("fir_split", 0), ("fir_impl", 1), ("generic", 0), ("fir_rows", 0))


@pytest.fixture(autouse=True)
def _release():
    # (options are process-wide defaults: what an earlier test module left set would take the path away)
    for k, v in DEFAULTS:
        rt.lib().dspRuntimeSetOption(k.encode(), v)
    yield
    for k, v in DEFAULTS:
        rt.lib().dspRuntimeSetOption(k.encode(), v)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def expected_rows(fmt, rows, B):
    """launch_fir_shared: the requested row tiles, halved while a workgroup of 64 R frames would be twice the block or more, and two at
    the most in format 4"""
    while rows > 1 and 32 * rows >= B:
        rows //= 2
    return min(rows, 2) if fmt == 4 else rows


_INPUTS, _ORACLE = {}, {}


def lcg(frames, ch, fmt, seed):
    """LCG samples, made once per shape and seed and never written to (the tests that plant special values copy them)"""
    key = (frames, ch, fmt == 6, seed)
    if key not in _INPUTS:
        x = pb.lcg_input(frames, ch, fmt == 6, seed=seed)
        x.setflags(write=False)
        _INPUTS[key] = x
    return _INPUTS[key]


def oracle(key, fmt, prog, x, out_stride, in_base):
    """(outputs of the whole input, state behind it) from the oracle: once per `key`, shared by the R variants (a chain program computes
    the same frames however they are cut into blocks), read-only"""
    if key not in _ORACLE:
        o = po.OracleProgram(fmt, prog)
        assert o.rc > 0
        out = o.run_block(x, out_stride, in_base)
        state = o.state.copy()
        out.setflags(write=False)
        state.setflags(write=False)
        _ORACLE[key] = (out, state)
    return _ORACLE[key]


def run_vs_oracle(key, fmt, rows, prog, x, blocks, T, C, shared_chains, out_stride=None, in_base=None, generic=0, seen=None):
    """The program over x in `blocks` with "fir_rows" `rows`: every block's outputs and the final state against the oracle, and after
    every block the path ("fir_shared_chains") and the R that ran ("fir_shared_rows").  x has exactly sum(blocks) frames."""
    out_stride = C if out_stride is None else out_stride
    in_base = out_stride if in_base is None else in_base
    assert sum(blocks) == len(x)
    want, want_state = oracle(key, fmt, prog, x, out_stride, in_base)
    r = rt.Runtime(fmt, prog)
    assert r.rc > 0
    r.set_option("generic", generic)
    r.set_option("fir_rows", rows)
    pos = 0
    for b in blocks:
        got = r.run_block(x[pos:pos + b], out_stride, in_base)
        ran = r.get_option("fir_shared_rows")
        diff = words(got) != words(want[pos:pos + b])
        if diff.any():
            cols = np.nonzero(diff.any(axis=0))[0]
            frames = np.nonzero(diff.any(axis=1))[0]
            raise AssertionError(f"format {fmt}, fir_rows {rows} (ran R = {ran}), T = {T}, C = {C}, block at frame {pos} ({b} frames): columns "
                                 f"{cols[:8].tolist()} differ ({cols.size} in all), first at frame {pos + frames[0]} (frame {frames[0]} of the "
                                 f"block, {frames.size} frames in all)")
        if not generic:
            what = f"format {fmt}, fir_rows {rows}, T = {T}, C = {C}, block at frame {pos} ({b} frames)"
            assert r.get_option("fir_shared_chains") == shared_chains, what
            assert ran == expected_rows(fmt, rows, b), what
            if seen is not None:
                seen.add(ran)
        pos += b
    bad = np.nonzero(r.sync_state() != want_state)[0]
    assert bad.size == 0, f"format {fmt}, fir_rows {rows}, T = {T}, C = {C}: state words {bad[:8].tolist()} differ ({bad.size} in all)"
    return r


# ---- a. the seams of S = 16 ceil(((T + 16 R + 3) >> 2) / 16) for every R, last chunks of 16 / 32 / 48 / 64 k-steps ----------------------

SEAM_TAPS = ((1, 2, 3, 5, 32, 33, 48, 49, 64, 65, 96),
             (97, 112, 113, 128, 129, 160, 161, 176, 177, 192, 193),
             (224, 225, 240, 241, 256, 257, 321, 1249, 4100))
CASCADE_TAPS = (3, 49, 113, 177, 241, 1249)
SEAM_FRAMES = 1500


def seam_blocks(R):
    head = [64 * R + 1, 48 * R - 1, 700, 32 * R + 1]
    return head + [SEAM_FRAMES - sum(head)]                            # (the same frames for every R: one oracle run serves the three)


def ksteps(T, R):
    return ((T + 16 * R + 3) // 4 + 15) // 16 * 16


def test_the_tap_counts_sit_on_the_seams():
    """what the lists above are for: every R meets both sides of each of its S seams up to 257 taps, and last chunks of every length"""
    taps = [t for g in SEAM_TAPS for t in g]
    for R in (1, 2, 4):
        seams = [64 * m - 16 * R for m in range(1, 6) if 0 < 64 * m - 16 * R <= 256]
        assert len(seams) == 4
        for seam in seams:
            assert seam in taps and seam + 1 in taps and ksteps(seam + 1, R) == ksteps(seam, R) + 16
        assert {ksteps(t, R) % 64 for t in taps} == {0, 16, 32, 48}
        assert any(ksteps(t, R) == 64 for t in taps)


@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("group", range(len(SEAM_TAPS)))
def test_tap_seams_fir_only(group, rows, fmt):
    C = 19                                                               # one full column group and a tail of 3
    x = lcg(SEAM_FRAMES, C, fmt, 31)
    seen = set()
    for T in SEAM_TAPS[group]:
        prog = pb.synth_program(fmt, C, 0, T, fir_banks=1)
        run_vs_oracle(("a", fmt, 0, T), fmt, rows, prog, x, seam_blocks(rows), T, C, C, seen=seen).release()
    assert seen == {expected_rows(fmt, rows, 700)}


@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_tap_seams_behind_a_cascade(rows, fmt):
    C = 19
    x = lcg(SEAM_FRAMES, C, fmt, 31)
    seen = set()
    for T in CASCADE_TAPS:
        prog = pb.synth_program(fmt, C, 2, T, fir_banks=1)
        run_vs_oracle(("a", fmt, 2, T), fmt, rows, prog, x, seam_blocks(rows), T, C, C, seen=seen).release()
    assert seen == {expected_rows(fmt, rows, 700)}


# ---- b. blocks on the edges of a wave (16 R frames) and of a workgroup (64 R), the demotion below 32 R, R changing over one ring --------

def edge_blocks(R):
    return [64 * R, 64 * R + 1, 64 * R - 1, 16 * R, 16 * R + 1, 32 * R, 32 * R + 1, 48 * R - 1, 48 * R, 128 * R + 16 * R + 3, 1, 17, 1024]


@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_frame_edges(rows, fmt):
    T, C = 70, 17                                                        # a tail of one column: wave 0 alone stages it
    blocks = edge_blocks(rows)
    x = lcg(sum(blocks), C, fmt, 37)
    seen = set()
    for S in (0, 1):
        prog = pb.synth_program(fmt, C, S, T, fir_banks=1)
        run_vs_oracle(("b", fmt, S, len(x)), fmt, rows, prog, x, blocks, T, C, C, seen=seen).release()
    # (blocks of 32 R frames or fewer run at a smaller R over the histories the larger R left, and the other way round)
    want = {1: {1}, 2: {1, 2}, 4: {1, 2, 4}}[rows]
    assert seen == ({min(v, 2) for v in want} if fmt == 4 else want)
    if fmt == 4 and rows == 4:
        assert expected_rows(4, 4, 1024) == 2 and 4 not in seen


# ---- c. ragged column groups, two STOREs of one chain, a chain without SAT0DB ------------------------------------------------------------

def banks_program(fmt, T, bank_of, twice, nosat):
    """chain c: LOAD_GAIN(IO O + c) -> [2 sections where c % 3 == 0] -> FIR(bank bank_of[c]) -> [SAT0DB] -> STORE(c); chain `twice` stores
    to IO C as well, chain `nosat` has no SAT0DB.  O = C + 1 outputs."""
    C = len(bank_of)
    O = C + 1
    nbanks = 1 + max(bank_of)
    taps = pb.lcg_taps_all(nbanks, T)
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + nbanks * (T + 16) + C * 64)
    pw.core()
    pw.param()
    banks = [pw.fir_impulses([taps[b]]) for b in range(nbanks)]
    for c in range(C):
        pw.param()
        sect = pw.biquad_bank(pb.synth_sections(c, 2, pb.F48000, pb.F48000)) if c % 3 == 0 else None
        pw.load_gain_fixed(O + c, 0.75)
        if sect is not None:
            pw.biquads(sect, 2)
        pw.fir(banks[bank_of[c]], T)
        if c != nosat:
            pw.sat0db()
        pw.store(c)
        if c == twice:
            pw.store(C)
    return pw.end_of_code(), C, O


TAIL_BLOCKS = [200, 65, 1, 300]


def run_tails(name, fmt, rows, bank_of, shared_chains, groups):
    T = 129
    C = len(bank_of)
    prog, C, O = banks_program(fmt, T, bank_of, twice=C - 1, nosat=2)   # (the last real column of the tail stores twice)
    x = lcg(sum(TAIL_BLOCKS), C, fmt, 41)
    r = run_vs_oracle(("c", fmt, name), fmt, rows, prog, x, TAIL_BLOCKS, T, C, shared_chains, out_stride=O)
    assert r.get_option("fir_shared_groups") == groups
    return r


@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_column_tails(rows, fmt):
    for C in (16, 18, 21, 31, 33):                                       # tails of 0, 2, 5, 15 and 1 columns
        run_tails(C, fmt, rows, [0] * C, C, 1).release()
    run_tails("18+17", fmt, rows, [c % 2 for c in range(35)], 35, 2).release()


@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_a_bank_of_16_beside_one_of_15(rows, fmt):
    bank_of = [c % 2 if c < 30 else 0 for c in range(31)]                # bank 0: 16 chains, bank 1: 15 (they stay on fir_tile)
    assert bank_of.count(0) == 16 and bank_of.count(1) == 15
    r = run_tails("16+15", fmt, rows, bank_of, 16, 1)
    assert r.fir_group_info() == dict(groups=1, grouped_chains=16, largest_group=16)


# ---- d. the wrap of the FIR ring inside a block, twice ------------------------------------------------------------------------------------

def ring_length(T):
    """The plan's FIR ring (avdsp_kernels.hip, plan build): pow2ceil(max_taps + kAhead * kFirChunk + 16 * fir_gpc + 16 * (kNG + 4) + 64)
    with kAhead = 3, kFirChunk = 1024, kNG = 2 and fir_gpc = fir_groups_per_chunk(max_taps) <= kMaxGpc = 56: 4096 frames up to some
    hundred taps (T = 49: 49 + 3072 + 64 + 96 + 64), 8192 from there (T = 1030)."""
    G = (T + 30) >> 4
    nc = (G + 55) // 56
    gpc = min(((G + nc - 1) // nc + 1) // 2 * 2, 56)
    need = T + 3 * 1024 + 16 * gpc + 16 * 6 + 64
    return 1 << (need - 1).bit_length()


def test_ring_lengths_assumed():
    assert ring_length(49) == 4096 and ring_length(1030) == 8192


@pytest.mark.parametrize("fmt,rows", [(6, 1), (6, 2), (6, 4), (4, 2)])
@pytest.mark.parametrize("S", [0, 1], ids=["fir_only", "behind_a_section"])      # fir_feed's two writes per sample; the cascade's appends
@pytest.mark.parametrize("T", [49, 1030])
def test_ring_wrap(T, S, fmt, rows):
    C, B = 20, 700
    ring = ring_length(T)                                                # 4096 (T = 49) and 8192 (T = 1030) frames as sized today
    nblocks = 2 * ring // B + 1                                          # the write position passes the ring's end twice, inside a block
    assert ring % B and (2 * ring) % B and nblocks * B > 2 * ring
    x = lcg(nblocks * B, C, fmt, 43)
    if fmt == 6:                                                         # Inf in the last frame before the wrap, NaN in the first behind it:
        x = x.copy()                                                     # the re-sum of the outputs around them reads across the wrap
        for k in (1, 2):
            x[k * ring - 1, 7] = np.inf
            x[k * ring, 7] = np.float32(np.nan)
    prog = pb.synth_program(fmt, C, S, T, fir_banks=1)
    run_vs_oracle(("d", fmt, S, T), fmt, rows, prog, x, [B] * nblocks, T, C, C)


# ---- e. Inf / NaN / subnormals at R = 2 and R = 4 -----------------------------------------------------------------------------------------

def bits(v):
    return np.uint32(v).view(np.float32)


@pytest.mark.parametrize("rows", [2, 4])
def test_special_values(rows):
    fmt, T = 6, 65
    R = rows
    blocks = [64 * R + 5, 37, 16 * R + 3, 700, 1024, 48 * R - 1, 333]
    bank_of = [0] * 21                                                   # column groups of 16 and 5
    prog, C, O = banks_program(fmt, T, bank_of, twice=-1, nosat=-1)
    starts = np.cumsum([0] + blocks)
    x = lcg(sum(blocks), C, fmt, 47).copy()
    special = (20, 5, 9)                                                 # the tail's last real column, a column of the full group, a chain behind a cascade
    for col in special:
        x[3, col] = np.inf
        x[40, col] = -np.inf
        x[300, col] = np.float32(np.nan)
        x[301, col] = bits(0x7FC12345)                                   # a NaN with payload bits
        x[900:905, col] = bits(0x00000123)                               # subnormals
        x[1500:1510, col + 1 if col < 20 else 0] = bits(0x80000007)
        x[2000, col] = np.inf
        x[starts[1] - 1, col] = bits(0x7F800001)                         # a signalling NaN in the last frame of block 0: frame 4 of the last,
        x[starts[3] - 1, col] = bits(0xFFC12345)                         # partially active wave; a negative NaN with payload ending block 2
        x[starts[3] + 700 // (16 * R) * (16 * R) + 1, col] = -np.inf     # block 3 (700 frames): in its last wave, 700 % 16 R frames of it active
        x[starts[6] - 1, col] = np.inf
    want, _ = oracle(("e", rows), fmt, prog, x, O, O)
    r = rt.Runtime(fmt, prog)
    r.set_option("fir_rows", rows)
    calm = [c for c in range(C) if c not in special]
    pos = 0
    for b in blocks:                                                     # first the neighbours alone: a special column must not leak
        got = r.run_block(x[pos:pos + b], O, O)
        bad = [c for c in calm if (words(got[:, c]) != words(want[pos:pos + b, c])).any()]
        assert not bad, f"fir_rows {rows}, block at frame {pos} ({b} frames): columns {bad} beside the special columns {special} differ"
        pos += b
    r.release()
    run_vs_oracle(("e", rows), fmt, rows, prog, x, blocks, T, C, C, out_stride=O)


# ---- f. a LOAD_MUX head in front of a shared bank -----------------------------------------------------------------------------------------

def mixer_on_one_bank(fmt, T=97, M=20, P=4, I=5):
    """M chains LOAD_MUX(5 inputs) -> [2 sections on every third] -> FIR(the one bank) -> SAT0DB -> STORE and P chains LOAD_GAIN -> FIR(the
    same bank) -> SAT0DB -> STORE.  The first 16 lists name the inputs in IO order (a mix group), the others backwards."""
    O = M + P
    taps = pb.lcg_taps_all(1, T)
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=256 + T + O * 96)
    pw.core()
    pw.param()
    bank = pw.fir_impulses([taps[0]])
    for o in range(O):
        pw.param()
        if o < M:
            ios = range(I) if o < 16 else range(I - 1, -1, -1)
            table = pw.mux_inputs([(O + j, float(g)) for j, g in zip(ios, pb.mixer_gains(o, I))])
            sect = pw.biquad_bank(pb.synth_sections(o, 2, pb.F48000, pb.F48000)) if o % 3 == 0 else None
            pw.load_mux(table)
            if sect is not None:
                pw.biquads(sect, 2)
        else:
            pw.load_gain_fixed(O + o % I, 0.5)
        pw.fir(bank, T)
        pw.sat0db()
        pw.store(o)
    return pw.end_of_code(), O, I


@pytest.mark.parametrize("fmt", [6, 4])
def test_mux_head_in_front_of_a_shared_bank(fmt):
    T = 97
    prog, O, I = mixer_on_one_bank(fmt, T)
    blocks = [129, 1, 63, 300, 65, 130]
    x = lcg(sum(blocks), I, fmt, 53)
    for rows in (1, 2):
        r = run_vs_oracle(("f", fmt), fmt, rows, prog, x, blocks, T, O, 24)
        assert r.mux_info()["mux_chains"] == 20
        assert r.fir_group_info() == dict(groups=1, grouped_chains=24, largest_group=24)
        r.release()
    r = run_vs_oracle(("f", fmt), fmt, 0, prog, x, blocks, T, O, 0, generic=1)     # and the interpreter
    assert r.core_info()["chains"] == 0

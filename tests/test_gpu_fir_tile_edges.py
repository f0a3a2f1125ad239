"""fir_tile's edges: a row tile's MFMA is not issued where its taps operand is all padding -- compiled out of a launch's first
group of 16 k-steps, compared away step by step in the groups that reach beyond the last tap -- and a launch whose plan has no
FIR-only chain skips the look for them.  Against the oracle, bit for bit, output and final state: tap counts on both sides of
every seam the trimming has (shorter than the front trim, a whole dead group from the rounding of the k-steps to 16, one chunk and
several), every row count, both chunk boundaries, FIR-only and behind a cascade, both float models; ragged and short blocks;
the opt-in tap split (its own tolerance); Inf, NaN and subnormal samples on the frames that only padding taps used to touch;
FIR-only and cascaded chains mixed in one workgroup."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release():
    yield
    rt.lib().dspRuntimeSetOption(b"fir_rows", 0)
    rt.lib().dspRuntimeSetOption(b"fir_split", 0)
    rt.lib().dspRuntimeSetOption(b"fir_lean", -1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_vs_oracle(fmt, prog, x, C, blocks, rows, fir_lean):
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    r.set_option("fir_impl", 1)
    r.set_option("fir_rows", rows)
    r.set_option("fir_lean", fir_lean)
    pos = 0
    for b in blocks:
        want = o.run_block(x[pos:pos + b], C, C)
        got = r.run_block(x[pos:pos + b], C, C)
        bad = np.nonzero((words(got) != words(want)).any(axis=0))[0]
        assert bad.size == 0, f"rows {rows} lean {fir_lean}: block at frame {pos} ({b} frames): channels {bad[:8].tolist()} differ, " \
                              f"first frame {int(np.argmax((words(got) != words(want)).any(axis=1)))}"
        pos += b
    assert (r.sync_state() == o.state).all(), "state differs after the last block"


ROWS = [1, 2, 4]
SEAM_TAPS = [1, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 1030, 4095, 4096, 4097]
RAGGED = [1, 37, 256, 257, 513, 1024]       # one, two and four tiles of a one-row-tile wave, and a partial one of each


@pytest.mark.parametrize("fir_lean", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("fmt,S", [(6, 0), (6, 2), (4, 0), (4, 2)])
@pytest.mark.parametrize("taps", SEAM_TAPS)
def test_tap_counts_around_the_trimmed_groups(taps, fmt, S, rows, fir_lean):
    C = 3
    prog = pb.synth_program(fmt, C, S, taps)
    blocks = RAGGED + [1024, 300]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=taps + 7 * rows + S)
    run_vs_oracle(fmt, prog, x, C, blocks, rows, fir_lean)


@pytest.mark.parametrize("fir_lean", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("fmt,C,S,T", [(6, 5, 0, 49), (6, 9, 2, 1030), (4, 6, 1, 4097), (6, 4, 0, 4096)])
def test_ragged_and_short_blocks_meet_the_trimmed_groups(rows, fmt, C, S, T, fir_lean):
    """every block length twice and in both orders: the ring wraps, and a chain's waves are 1, 2 or 4 tiles of its block"""
    prog = pb.synth_program(fmt, C, S, T)
    blocks = RAGGED + RAGGED[::-1] + [1024, 256, 1, 513]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=T + C + rows)
    run_vs_oracle(fmt, prog, x, C, blocks, rows, fir_lean)


@pytest.mark.parametrize("fmt,S", [(6, 0), (6, 2), (4, 0)])
@pytest.mark.parametrize("taps", SEAM_TAPS)
def test_tap_split_with_the_trimmed_halves(taps, fmt, S):
    """"fir_split" 1: each half of a tile's k-steps trims its own outer end only; the two partial sums are not the reference's
    summation order, so the check is the float-mode tolerance of the split's own test (1e-6 of the block's peak), the state bit for bit"""
    C = 4
    prog = pb.synth_program(fmt, C, S, taps)
    blocks = RAGGED + [1024]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=C + taps)
    starts = np.cumsum([0] + blocks[:-1])
    o = po.OracleProgram(fmt, prog)
    want = np.concatenate([o.run_block(x[p:p + b], C, C) for p, b in zip(starts, blocks)])
    r = rt.Runtime(fmt, prog)
    r.set_option("fir_split", 1)
    assert r.get_option("fir_split") == 1
    got = np.concatenate([r.run_block(x[p:p + b], C, C) for p, b in zip(starts, blocks)])
    if fmt == 6:
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        peak = np.abs(want.astype(np.float64)).max()
    else:
        err = np.abs(got.astype(np.int64) - want.astype(np.int64)).max()
        peak = np.abs(want.astype(np.int64)).max()
    assert err <= 1e-6 * peak, f"max abs error {err} against a peak of {peak}"
    assert (r.sync_state() == o.state).all(), "the delay lines do not depend on the summation order"


ODD = [0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F812345, 0x00000012, 0x80000400, 0x007FFFFF]


@pytest.mark.parametrize("fir_lean", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("S", [0, 2])
@pytest.mark.parametrize("taps", [5, 48, 300, 1030, 4096])
def test_odd_samples_at_both_outer_ends_of_a_tile_window(taps, S, rows, fir_lean):
    """Inf, NaN, exponent-255 and subnormal samples on the frames a tile's window holds but only padding taps multiply -- F0 - T and
    below, F0 + tile and above -- and inside the window, each kind of place in a channel of its own (so that a tile whose odd samples
    meet padding only is not summed again for another reason), one channel with all of them, one clean"""
    C = 5
    tile = 256 * rows
    blocks = [1024, 1024, 513, 1024]
    n = sum(blocks)
    x = pb.lcg_input(n, C, True, seed=taps + rows)
    xv = x.view(np.uint32)
    starts = np.cumsum([0] + blocks[:-1])
    k = 0
    for p, b in zip(starts[1:], blocks[1:]):
        for f0 in range(0, b, tile):
            below = [p + f0 - taps - d for d in (0, 1, 2, 3, 17, 60)]
            above = [p + f0 + tile + d for d in (0, 1, 2, 3)]
            inside = [p + f0 - taps + 1, p + f0 - 1, p + f0, p + f0 + tile - 1]
            for ch, frames in ((0, below), (1, above), (2, inside), (3, below + above + inside)):
                for f in frames:
                    if 0 <= f < n:
                        xv[f, ch] = ODD[k % len(ODD)]
                        k += 1
    prog = pb.synth_program(6, C, S, taps)
    run_vs_oracle(6, prog, x, C, blocks, rows, fir_lean)


def _mixed_program(fmt, C, S, T, fir_only):
    """synth_program's chains, but those in fir_only have no biquads in front of their FIR"""
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + C * (T + 64 + 16 * S))
    taps = pb.lcg_taps_all(C, T)
    pw.core()
    for c in range(C):
        pw.param()
        bank = None if c in fir_only else pw.biquad_bank(pb.synth_sections(c, S, pb.F48000, pb.F48000))
        imp = pw.fir_impulses([taps[c]])
        pw.load_gain_fixed(C + c, 1.0)
        if bank is not None:
            pw.biquads(bank, S)
        pw.fir(imp, T)
        pw.sat0db()
        pw.store(c)
    return pw.end_of_code()


@pytest.mark.parametrize("fir_lean", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("fmt,T", [(6, 49), (6, 1030), (4, 300)])
@pytest.mark.parametrize("fir_only", [(), (0, 1, 2, 3, 4, 5, 6, 7, 8), (1, 2, 7), (0, 5, 6, 8)])
def test_fir_only_and_cascaded_chains_in_one_launch(fir_only, fmt, T, rows, fir_lean):
    """nine chains -- the four chains of a short block's workgroup, or the four waves of four row tiles, hold both kinds -- with
    none, all or some of them FIR-only: the launch looks for FIR-only chains exactly when its plan has one"""
    C, S = 9, 2
    prog = _mixed_program(fmt, C, S, T, set(fir_only))
    blocks = [1024, 37, 256, 513, 1024]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=T + len(fir_only))
    run_vs_oracle(fmt, prog, x, C, blocks, rows, fir_lean)

"""fir_tile's window image as a ring of columns (four row tiles, lean boundary): the prologue stages 22 columns of 64
samples, every later chunk boundary only the columns its chunk adds, into the places of those that died; a lane's column pointer
steps down once per group of 16 k-steps and wraps; physical column 0 mirrors column 22.  Against the oracle, bit for bit, outputs
and final state, four row tiles and the lean boundary forced, formats 4 and 6: tap counts on both sides of every column event (the
first new column, the pointer's first and second wrap, the last chunk of 4096 taps, a last chunk of one group, chunks shorter than
the longest), every block-length seam with the float ring wrapping under the window, Inf / NaN / subnormal samples in a column of
the prologue, in one staged later and in the mirrored one, FIR-only and cascaded chains in one workgroup, a handed launch
("fir_tail").  fir_mfma (fir_impl 2) runs the same cases as a second opinion.  The oracle's results are computed once per case,
shared between the two, and never written."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import firtail_programs as fp

pytestmark = pytest.mark.gpu

IMPLS = [1, 2]
FMTS = [6, 4]


@pytest.fixture(autouse=True)
def _release():
    yield
    for key, v in (("fir_tail", 0), ("chain_delay", 0), ("chain_finish", 0), ("fir_impl", 1), ("fir_rows", 0), ("fir_lean", -1)):
        rt.Runtime.set_global_option(key, v)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def chains_program(fmt, taps, secs):
    """one chain per entry: secs[c] biquad sections (0: a FIR alone) in front of a FIR of taps[c] taps, its own impulse"""
    C = len(taps)
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + sum(t + 64 + 16 * s for t, s in zip(taps, secs)))
    pw.core()
    for c in range(C):
        pw.param()
        bank = pw.biquad_bank(pb.synth_sections(c, secs[c], pb.F48000, pb.F48000)) if secs[c] else None
        imp = pw.fir_impulses([pb.lcg_taps_all(1, taps[c], channel_base=c)[0]])
        pw.load_gain_fixed(C + c, 1.0)
        if bank is not None:
            pw.biquads(bank, secs[c])
        pw.fir(imp, taps[c])
        pw.sat0db()
        pw.store(c)
    return pw.end_of_code()


_REF = {}


def reference(key, fmt, prog, x, C, blocks):
    if key not in _REF:
        o = po.OracleProgram(fmt, prog)
        outs, pos = [], 0
        for b in blocks:
            outs.append(o.run_block(x[pos:pos + b], C, C))
            pos += b
        state = o.state.copy()
        for v in outs + [state]:
            v.flags.writeable = False
        _REF[key] = (outs, state)
    return _REF[key]


def run_vs_reference(key, fmt, prog, x, C, blocks, impl):
    outs, state = reference(key, fmt, prog, x, C, blocks)
    r = rt.Runtime(fmt, prog)
    r.set_option("fir_impl", impl)
    r.set_option("fir_rows", 4)
    r.set_option("fir_lean", 1)
    pos = 0
    for b, want in zip(blocks, outs):
        got = r.run_block(x[pos:pos + b], C, C)
        bad = np.nonzero((words(got) != words(want)).any(axis=0))[0]
        assert bad.size == 0, f"fir_impl {impl}: block at frame {pos} ({b} frames): channels {bad[:8].tolist()} differ, " \
                              f"first frame {int(np.argmax((words(got) != words(want)).any(axis=1)))}"
        pos += b
    assert (r.sync_state() == state).all(), "state differs after the last block"


# k-steps: S = ((T + 67) / 4 rounded up to 16), chunks of ck <= 96, a column per 64 samples of reach.
#  1 .. 65: one chunk, the first column beyond the 16 of the tile itself;  380: two chunks of 64 and 48 k-steps (4 and 3 columns:
#  the boundary writes live columns again);  1343 .. 1345, 1407 .. 1409: 22 columns in, the pointer's first wrap;  1900: five full
#  chunks and a last one of a single group;  2752, 2753: the second wrap;  4095 .. 4097: eleven chunks, the last of five groups
WRAP_TAPS = {"first": [1, 63, 64, 65, 1343, 1344, 1345, 1900], "second": [1407, 1408, 1409, 2752, 2753, 4095, 4096, 4097]}


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("which", sorted(WRAP_TAPS))
def test_tap_counts_across_every_column_event(which, fmt, impl):
    """eight chains of eight tap counts in one launch: the four waves of a workgroup wrap at different groups"""
    taps = WRAP_TAPS[which]
    C = len(taps)
    prog = chains_program(fmt, taps, [0] * C)
    blocks = [1024, 1024, 1024]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=17 + len(which))
    run_vs_reference(("taps", which, fmt), fmt, prog, x, C, blocks, impl)


SEAM_BLOCKS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("T", [1345, 4096])
def test_block_lengths_and_the_float_ring_wrapping_under_the_window(T, fmt, impl):
    """three full blocks, every seam length, then full blocks until the float ring (4096 or 8192 frames) has wrapped: from there on
    a window's columns lie on both sides of the ring's end, in the prologue's fetch and in the later ones"""
    C = 4
    prog = chains_program(fmt, [T, T - 1, 380, T], [0, 1, 0, 2])
    blocks = [1024, 1024, 1024] + SEAM_BLOCKS + [1024, 513, 1024, 1024, 700, 1024, 1024]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=T)
    assert sum(blocks) > 8192 + 2048
    run_vs_reference(("blocks", T, fmt), fmt, prog, x, C, blocks, impl)


INF, NINF, NAN, BIGEXP, SUB, NSUB = 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F812345, 0x00000012, 0x80000400


@pytest.mark.parametrize("impl", IMPLS)
def test_odd_samples_in_prologue_later_and_mirrored_columns(impl):
    """Column D of a tile at frame p holds frames p - 3 + 64 (16 - D) + row.  D = 3 and 20: staged in the prologue; D = 30 and 50:
    staged at the second and the sixth boundary; D = 0, 22, 44: physical column 22, mirrored into the guard (D = 0: rows 0 .. 2 are
    frames of the block itself).  Subnormals go through the image (the conversion flushes them); an Inf or a NaN makes the tile's
    sums non-finite and the tile is summed again the reference's way.  Each kind of place in a channel of its own, one channel with
    all of them, one clean."""
    C, T = 8, 4096
    blocks = [1024, 1024, 1024, 513]
    n = sum(blocks)
    x = pb.lcg_input(n, C, True, seed=29)
    xv = x.view(np.uint32)

    def col(p, D, rows):
        return [p - 3 + 64 * (16 - D) + r for r in rows]

    for p in (2048, 3072):
        prologue = col(p, 3, (0, 31, 63)) + col(p, 20, (1, 62))
        later = col(p, 30, (0, 40, 63)) + col(p, 50, (5, 63))
        mirrored = col(p, 0, (0, 1, 2)) + col(p, 22, (0, 33, 63)) + col(p, 44, (7, 63))
        for ch, frames, kinds in ((0, prologue, (SUB, NSUB)), (1, later, (SUB, NSUB)), (2, mirrored, (NSUB, SUB)),
                                  (3, prologue, (INF, BIGEXP)), (4, later, (NAN, NINF)), (5, mirrored, (INF, NAN)),
                                  (7, prologue + later + mirrored, (SUB, INF, NSUB, NAN, BIGEXP, NINF))):
            for i, f in enumerate(frames):
                if 0 <= f < n:
                    xv[f, ch] = kinds[i % len(kinds)]
    prog = chains_program(6, [T] * C, [0] * C)
    run_vs_reference(("odd",), 6, prog, x, C, blocks, impl)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fir_only", [(1, 2, 7), (0, 5, 6, 8)])
def test_fir_only_and_cascaded_chains_in_one_workgroup(fir_only, fmt, impl):
    """nine chains, four to a workgroup, of tap counts that wrap at different groups, some of them a FIR alone"""
    taps = [4096, 1345, 2753, 380, 65, 1409, 1900, 3000, 4097]
    secs = [0 if c in fir_only else 2 for c in range(len(taps))]
    C = len(taps)
    prog = chains_program(fmt, taps, secs)
    blocks = [1024, 37, 600, 1024]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=len(fir_only))
    run_vs_reference(("mixed", fir_only, fmt), fmt, prog, x, C, blocks, impl)


@pytest.mark.parametrize("fmt", FMTS)
def test_handed_chains(fmt):
    """"fir_tail": the HAND form of the same kernel -- a delay or a dressed finish behind FIRs that wrap the column ring; the chains
    must be handed (dspRuntimeFirTailInfo), then outputs and state against the oracle after each block"""
    taps = [4096, 1345, 2753, 380, 4097]
    chains = [fp.chain(nsec=(2, 0, 1, 0, 3)[i], taps=t, slot=("A", "B", None, "B", "A")[i], us=(1000, 20, 21, 300, 50)[i], max_us=1000,
                       finish=("tpdf_gain", "tpdf", "gain", "sat", "none")[i], gain=0.9 + 0.01 * i) for i, t in enumerate(taps)]
    prog, nin, nout = fp.program(fmt, [fp.core(chains, calc=0)])
    blocks = [1024, 600, 1024, 1024]
    x = pb.lcg_input(sum(blocks), nin, fmt == 6, seed=41)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    for key in ("chain_finish", "chain_delay", "fir_tail"):
        r.set_option(key, 1)
    r.set_option("fir_rows", 4)
    assert r.core_info(0)["chains"] == len(chains), r.last_error()
    assert r.fir_tail_info(0) == fp.handed(chains) and fp.handed(chains)[0] == len(chains)
    pos = 0
    for b in blocks:
        want = o.run_block(x[pos:pos + b], nout, fp.IN)
        got = r.run_block(x[pos:pos + b], nout, fp.IN)
        bad = np.nonzero((words(got) != words(want)).any(axis=0))[0]
        assert bad.size == 0, f"block at frame {pos} ({b} frames): outputs {bad[:8].tolist()} differ"
        assert (r.sync_state() == o.state).all(), f"state differs after the block at frame {pos}"
        pos += b

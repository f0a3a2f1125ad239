"""The teeth fir_tile's window ring never got (profiles/fir_window_ring.md, "Teeth"): tests/fir_ring_model.py transcribes the ring's
integer arithmetic and tracks which frame every window operand of every issued MFMA comes from.  (1) For 1 .. 8000 taps every read
is the picture's (lane (a, k) at k-step s multiplies x[F0 + 64 a - (m + k)], m = -64 + 4 s), and every MFMA that has a
real tap is issued.  (2) Each of a list of slips -- the wrap of the column pointer a column short or late, the guard left stale,
pc0 or Dhi off by one, five columns staged for six, a prologue of 21 columns, the pointer stepped a k-step early or late -- is made
in the model, and the tap counts that run through the ring kernel on a GPU (tests/test_gpu_fir_window_ring.py,
tests/test_gpu_fir_ring_routes.py, program DEEP of tests/state_scripts.py) must contain one at which the slip puts a wrong frame
under a real tap: a slip that none of them sees means a GPU case is missing.  Nothing here runs a wrong kernel anywhere."""
import numpy as np
import pytest

from tests import fir_ring_cases as rc
from tests import fir_ring_model as fm

TAPS = rc.ring_tap_counts()


def test_every_read_is_the_pictures_for_1_to_8000_taps():
    seen = None
    for T in range(1, 8001):
        Sall, nch, ck, slast = fm.chunking(T)
        s, frames, issued = fm.wave(T)
        assert (s == np.arange(len(s))).all() and len(s) == slast + 1 <= Sall, T
        if (Sall, slast) != seen:                            # (the reads depend on T through these two alone)
            seen = (Sall, slast)
            used = issued.any(axis=1)
            bad = (frames != fm.picture(s)) & used[:, None]
            assert not bad.any(), f"{T} taps: k-step {int(s[bad.any(axis=1)][0])}, lanes {np.nonzero(bad[bad.any(axis=1)][0])[0][:8].tolist()} read another frame than the picture's"
            assert frames[used].min() > fm.UNSET
        need = fm.real(T, s).any(axis=2)                     # [n][r]: the MFMA has a tap
        assert (issued | ~need).all(), f"{T} taps: an MFMA with a real tap is not issued"
        assert not (issued & ~need)[s > slast - 12].any(), f"{T} taps: an MFMA of padding alone is issued in the guarded groups"
    assert fm.wrong_reads(4096)[0] == 4112 and fm.wrong_reads(4097)[0] == 4116 and fm.wrong_reads(2048)[0] == 2064      # DESIGN.md 4.2, "the edges of the tap loop"


def test_the_model_reports_every_issued_mfma():
    got = list(fm.mfmas(65))
    assert len(got) == fm.wrong_reads(65)[0] == 84
    s, r, frames = got[0]
    assert (s, r) == (0, 3) and frames.shape == (64,)      # the launch's first group: row tile 3 alone has taps at step 0
    assert (frames == 64 * (np.arange(64) & 15) + 64 - (np.arange(64) >> 4)).all()


@pytest.mark.parametrize("name", sorted(fm.MUTATIONS))
def test_a_slip_in_the_ring_is_seen_by_a_tap_count_the_gpu_cases_run(name):
    mut = fm.MUTATIONS[name]
    seeing = [T for T in TAPS if fm.sees(T, mut)]
    assert seeing, f"{name}: none of the tap counts {TAPS} puts a wrong frame under a real tap"
    # a slip in the later boundaries or in the wrap cannot show in a FIR of one chunk: the model must say so too
    if name not in ("the prologue stages 21 columns, the newest missing", "the pointer steps in front of step 13", "the pointer steps in front of step 15"):
        assert not fm.sees(1, mut) and not fm.sees(65, mut), name


def test_the_tap_counts_are_the_gpu_cases():
    from tests import state_scripts as ss
    assert {1345, 2753, 4096, 4097, 1409, 1900, 380, 65, 3000, 1407, 300} <= set(TAPS)
    assert set(TAPS) >= {t for _, t in rc.BASE} | {t for _, t in ss.DEEP_CHAINS} | set(rc.TREE_TAPS)

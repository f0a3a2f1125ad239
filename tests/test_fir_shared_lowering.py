"""Host-only checks of the shared-impulse FIR grouping: dspRuntimeFirGroupInfo reports the groups of 16 chains or
more whose DSP_FIR points at one impulse bank at the current rate, among the rank's chains, and synth_program's `fir_banks`
leaves the programs it made before word for word.  No GPU: nothing here runs a block."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt


@pytest.fixture(autouse=True)
def _release():
    yield
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def groups(fmt, prog, fs=48000):
    r = rt.Runtime(fmt, prog, fs=fs)
    return r, r.fir_group_info()


@pytest.mark.parametrize("fmt", [4, 6])
def test_one_bank_is_one_group(fmt):
    _, g = groups(fmt, pb.synth_program(fmt, 40, 2, 61, fir_banks=1))
    assert g == dict(groups=1, grouped_chains=40, largest_group=40)


def test_three_banks_are_three_groups():
    _, g = groups(6, pb.synth_program(6, 50, 0, 64, fir_banks=3))
    assert g == dict(groups=3, grouped_chains=50, largest_group=17)


def test_below_the_threshold_no_group():
    _, g = groups(6, pb.synth_program(6, 15, 1, 33, fir_banks=1))
    assert g == dict(groups=0, grouped_chains=0, largest_group=0)
    _, g = groups(6, pb.synth_program(6, 40, 0, 64, fir_banks=3))     # 14 / 13 / 13 chains
    assert g["groups"] == 0


def test_private_impulses_no_group():
    for shared_taps in (False, True):                                   # equal values in separate banks are separate banks
        _, g = groups(6, pb.synth_program(6, 64, 2, 61, shared_taps=shared_taps))
        assert g == dict(groups=0, grouped_chains=0, largest_group=0)


def test_mixed_banks_and_private_chains():
    """24 + 20 chains on two interleaved banks, 9 private ones behind them"""
    C, T = 53, 37
    taps = pb.lcg_taps_all(C, T)
    pw = pb.ProgramWriter(6, pb.F48000, pb.F48000, capacity=64 + C * (T + 64) + 2 * (T + 16))
    pw.core()
    pw.param()
    banks = [pw.fir_impulses([taps[0]]), pw.fir_impulses([taps[1]])]
    for c in range(C):
        pw.param()
        imp = banks[c % 2] if c < 40 else banks[0] if c < 44 else pw.fir_impulses([taps[c]])
        pw.load_gain_fixed(C + c, 1.0)
        pw.fir(imp, T)
        pw.sat0db()
        pw.store(c)
    _, g = groups(6, pw.end_of_code())
    assert g == dict(groups=2, grouped_chains=44, largest_group=24)


def two_rate_program(C, T):
    """rate 44.1k: every chain on one bank; rate 48k: every chain on its own impulse"""
    taps = pb.lcg_taps_all(C + 1, T)
    pw = pb.ProgramWriter(6, pb.F44100, pb.F48000, capacity=64 + C * (2 * T + 64) + 2 * T + 64)
    pw.core()
    pw.param()
    shared = pw.fir_impulses([taps[0], taps[0]])
    for c in range(C):
        pw.param()
        own = pw.fir_impulses([taps[c + 1], taps[c + 1]])
        pw.load_gain_fixed(C + c, 1.0)
        pw.fir([shared[0], own[1]], T)
        pw.sat0db()
        pw.store(c)
    return pw.end_of_code()


def test_groups_follow_the_rate():
    r, g = groups(6, two_rate_program(32, 20), fs=44100)
    assert g == dict(groups=1, grouped_chains=32, largest_group=32)
    assert r.reset(48000) == 0
    assert r.fir_group_info() == dict(groups=0, grouped_chains=0, largest_group=0)
    assert r.reset(44100) == 0
    assert r.fir_group_info()["grouped_chains"] == 32


def test_pure_delay_fir_runs_on_the_interpreter():
    prog = pb.synth_program(6, 32, 0, 8, fir_banks=1)
    # the bank's length word: PARAM head, section header [(51 << 16) | nF], then the (odd-indexed) length word
    at = [j for i in range(len(prog) - 2) if prog[i] == (pb.OP_FIR << 16) | 1 for j in (i + 1, i + 2) if prog[j] == 8]
    assert at, "bank not found"
    prog = prog.copy()
    prog[at[0]] = (2 << 16) | 8                                          # length >> 16: the pure-delay variant
    r, g = groups(6, prog)
    assert r.core_info()["chains"] == 0
    assert g == dict(groups=0, grouped_chains=0, largest_group=0)


def test_formats_without_the_chain_fir_have_no_groups():
    prog = pb.synth_program(6, 32, 2, 16, fir_banks=1)
    for fmt in (3, 5):
        _, g = groups(fmt, prog)
        assert g["groups"] == 0


def test_shard_counts_the_ranks_chains():
    prog = pb.synth_program(6, 96, 1, 40, fir_banks=2)                  # 48 + 48 chains, interleaved
    rt.lib().dspRuntimeSetShard(1, 3)                                    # chains 32 .. 63: 16 of each bank
    r = rt.Runtime(6, prog)
    assert r.shard_info()["nchains"] == 32
    assert r.fir_group_info() == dict(groups=2, grouped_chains=32, largest_group=16)
    rt.lib().dspRuntimeSetShard(0, 1)
    r.release()
    r = rt.Runtime(6, prog)
    assert r.fir_group_info() == dict(groups=2, grouped_chains=96, largest_group=48)


@pytest.mark.parametrize("args", [(6, 8, 4, 300), (6, 40, 16, 64), (4, 17, 0, 65), (2, 64, 16, 0), (6, 5, 3, 7),
                                  (6, 12, 2, 33, pb.F44100, pb.F96000), (4, 3, 1, 5, pb.F48000, pb.F48000, 1.0, True)])
def test_fir_banks_none_is_word_for_word(args):
    a = pb.synth_program(*args)
    b = pb.synth_program(*args, fir_banks=None)
    assert a.dtype == b.dtype and len(a) == len(b) and (a == b).all()


def test_fir_banks_layout():
    prog = pb.synth_program(6, 6, 0, 5, fir_banks=2)
    r = rt.Runtime(6, prog)
    assert r.core_info() == dict(chains=6, max_sections=0, max_taps=5)
    with pytest.raises(ValueError):
        pb.synth_program(6, 6, 0, 5, fir_banks=0)


def test_options():
    r = rt.Runtime(6, pb.synth_program(6, 16, 0, 5, fir_banks=1))
    assert r.get_option("fir_shared") == 1
    assert r.get_option("fir_shared_chains") == 0 and r.get_option("fir_shared_groups") == 0 and r.get_option("fir_shared_rows") == 0
    r.set_option("fir_shared", 0)
    assert r.get_option("fir_shared") == 0
    r.set_option("fir_shared", 1)
    with pytest.raises(rt.AvdspError):
        r.set_option("fir_shared", 2)
    with pytest.raises(rt.AvdspError):
        r.set_option("fir_shared_chains", 3)
    with pytest.raises(rt.AvdspError):
        r.set_option("fir_shared_rows", 2)

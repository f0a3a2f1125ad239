"""fir_shared<FMT, R>: chains that point at one impulse bank as the 16 columns of the FIR tile, against the oracle
bit for bit -- outputs and the FIR histories -- and against the per-chain path (fir_tile) on the full-size program; the places the
path is not taken keep today's kernels (and say so through "fir_shared_chains")."""
import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

BLOCKS = [1024, 1, 37, 64, 256, 257, 700, 128]


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


def run_vs_oracle(fmt, prog, x, C, blocks, shared_chains, options=None, in_base=None, out_base=0, edit=None):
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    pos = 0
    for bi, b in enumerate(blocks):
        if edit is not None:
            edit(bi, r, o)
        want = o.run_block(x[pos:pos + b], C, C if in_base is None else in_base)
        got = r.run_block(x[pos:pos + b], C, C if in_base is None else in_base)
        bad = np.nonzero((words(got) != words(want)).any(axis=0))[0]
        assert bad.size == 0, f"block at frame {pos} ({b} frames): columns {bad[:8].tolist()} differ"
        assert r.get_option("fir_shared_chains") == shared_chains
        pos += b
    assert (r.sync_state() == o.state).all(), "FIR histories / cascade state differ"
    return r


@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("C", [16, 17, 40, 64])
def test_one_bank_against_the_oracle(fmt, C):
    x = pb.lcg_input(sum(BLOCKS), C, fmt == 6, seed=C)
    for S, Ts in ((0, (1, 3, 4, 61, 64, 65, 257, 1030)), (2, (3, 64, 257, 1030))):      # FIR-only chains, chains behind a cascade
        for T in Ts:
            prog = pb.synth_program(fmt, C, S, T, fir_banks=1)
            r = run_vs_oracle(fmt, prog, x, C, BLOCKS, C)
            assert r.get_option("fir_shared_groups") == 1
            r.release()


def mixed_program(T):
    """banks of 24 and 20 chains, interleaved over IO 0 .. 43, and 9 chains with impulses of their own (IO 44 .. 52)"""
    C = 53
    taps = pb.lcg_taps_all(C, T)
    pw = pb.ProgramWriter(6, pb.F48000, pb.F48000, capacity=64 + C * (T + 64) + 2 * (T + 16))
    pw.core()
    pw.param()
    banks = [pw.fir_impulses([taps[0]]), pw.fir_impulses([taps[1]])]
    for c in range(C):
        pw.param()
        bank = pw.biquad_bank(pb.synth_sections(c, 2, pb.F48000, pb.F48000)) if c % 3 == 0 else None
        imp = banks[c % 2] if c < 40 else banks[0] if c < 44 else pw.fir_impulses([taps[c]])
        pw.load_gain_fixed(C + c, 1.0)
        if bank is not None:
            pw.biquads(bank, 2)
        pw.fir(imp, T)
        pw.sat0db()
        pw.store(c)
    return pw.end_of_code(), C


def test_mixed_program():
    prog, C = mixed_program(129)
    x = pb.lcg_input(sum(BLOCKS), C, True, seed=7)
    r = run_vs_oracle(6, prog, x, C, BLOCKS, 44)
    assert r.get_option("fir_shared_groups") == 2
    assert r.fir_group_info() == dict(groups=2, grouped_chains=44, largest_group=24)


def test_special_values_in_one_column():
    C, T = 20, 65
    prog = pb.synth_program(6, C, 0, T, fir_banks=1)
    x = pb.lcg_input(sum(BLOCKS), C, True, seed=11)
    col = 5
    x[3, col] = np.inf
    x[40, col] = -np.inf
    x[300, col] = np.float32(np.nan)
    x[301, col] = np.uint32(0x7FC12345).view(np.float32)                # a NaN with payload bits
    x[900:905, col] = np.uint32(0x00000123).view(np.float32)           # subnormals
    x[1500:1510, col + 1] = np.uint32(0x80000007).view(np.float32)
    x[2000, col] = np.inf
    run_vs_oracle(6, prog, x, C, BLOCKS, C)


def test_live_bank_edit():
    C, T = 24, 97
    prog = pb.synth_program(6, C, 1, T, fir_banks=1)
    at = [j for i in range(len(prog) - 2) if prog[i] == (pb.OP_FIR << 16) | 1 for j in (i + 1, i + 2) if prog[j] == T][0] + 1

    def edit(bi, r, o):
        if bi == 3:                                                      # a new impulse in the one bank, between two blocks
            new = (pb.lcg_taps_all(1, T, 999)[0] * 0.5).astype(np.float32).view(np.uint32)
            r.buf[at:at + T] = new
            o.buf[at:at + T] = new
            r.upload_params()
    x = pb.lcg_input(sum(BLOCKS), C, True, seed=13)
    run_vs_oracle(6, prog, x, C, BLOCKS, C, edit=edit)


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


def test_rate_change_regroups():
    """dspRuntimeReset to the other rate mid-stream: the chains regroup by that rate's impulses (none at 48k), and back"""
    C, T = 32, 70
    prog = two_rate_program(C, T)
    steps = ((44100, 700), (44100, 700), (48000, 700), (48000, 300), (44100, 400))
    x = pb.lcg_input(sum(b for _, b in steps), C, True, seed=17)
    o = po.OracleProgram(6, prog, fs=44100)
    r = rt.Runtime(6, prog, fs=44100)
    pos, fs_now = 0, 44100
    for k, (fs, b) in enumerate(steps):
        if fs != fs_now:
            assert r.reset(fs) == 0 and o.reset(fs) == 0
            fs_now = fs
        want = o.run_block(x[pos:pos + b], C, C)
        got = r.run_block(x[pos:pos + b], C, C)
        assert (words(got) == words(want)).all(), f"block {k} at {fs}"
        assert r.get_option("fir_shared_chains") == (C if fs == 44100 else 0)
        pos += b
    assert (r.sync_state() == o.state).all()


def test_full_size_shared_against_per_chain():
    """the north-star shape with one bank: 4096 chains x 4096 taps, fir_shared 1 against 0 (fir_tile), bit for bit"""
    C, T = 4096, 4096
    prog = pb.synth_program(6, C, 2, T, fir_banks=1)
    blocks = [64, 256, 1024, 64]
    x = pb.lcg_input(sum(blocks), C, True, seed=19)
    outs = []
    for shared in (1, 0):
        r = rt.Runtime(6, prog)
        r.set_option("fir_shared", shared)
        pos, got = 0, []
        for b in blocks:
            got.append(r.run_block(x[pos:pos + b], C, C))
            assert r.get_option("fir_shared_chains") == (C if shared else 0)
            pos += b
        outs.append((np.concatenate(got), r.sync_state()))
        r.release()
    assert (words(outs[0][0]) == words(outs[1][0])).all()
    assert (outs[0][1] == outs[1][1]).all()


@pytest.mark.parametrize("opt", [{"overlap": 1}, {"overlap": 2}, {"fir_split": 1}, {"fir_shared": 0}, {"fir_impl": 3}])
def test_fallbacks_keep_todays_path(opt):
    C, T = 32, 300
    prog = pb.synth_program(6, C, 2, T, fir_banks=1)
    x = pb.lcg_input(sum(BLOCKS), C, True, seed=23)
    if "overlap" in opt:                                                 # (the mode's contract: device-resident blocks, inputs complete)
        import torch
        from avdsp_amd import devmem as dm
        o = po.OracleProgram(6, prog)
        r = rt.Runtime(6, prog)
        r.set_option("overlap", opt["overlap"])
        st = torch.cuda.current_stream().cuda_stream
        pos = 0
        for b in BLOCKS:
            xd = dm.to_device(x[pos:pos + b].copy())
            yd = torch.zeros((b, C), dtype=xd.dtype, device="cuda")
            torch.cuda.synchronize()
            r.run_block_device(xd.data_ptr(), C, C, yd.data_ptr(), C, 0, b, st)
            torch.cuda.synchronize()
            want = o.run_block(x[pos:pos + b], C, C)
            assert (words(dm.to_host(yd)) == words(want)).all()
            assert r.get_option("fir_shared_chains") == 0
            pos += b
        assert (r.sync_state() == o.state).all()
        return
    if "fir_split" in opt:                                               # (not bit-exact by design: against fir_shared 0)
        outs = []
        for shared in (1, 0):
            r = rt.Runtime(6, prog)
            r.set_option("fir_split", 1)
            r.set_option("fir_shared", shared)
            outs.append(r.run_block(x[:1024], C, C))
            assert r.get_option("fir_shared_chains") == 0
            r.release()
        assert (words(outs[0]) == words(outs[1])).all()
        return
    run_vs_oracle(6, prog, x, C, BLOCKS, 0, options=opt)


def test_chain_instances_keep_todays_path():
    from tests.test_gpu_instances import _chain_instances_vs_oracle
    prog = pb.synth_program(6, 20, 2, 130, fir_banks=1)
    r = _chain_instances_vs_oracle(6, prog, 20, 3, [256, 64, 700, 1])
    assert r.get_option("fir_shared_chains") == 0
    r.release()


def test_shard_of_a_shared_program():
    C, T = 96, 200
    prog = pb.synth_program(6, C, 1, T, fir_banks=2)                     # 48 + 48 chains, interleaved
    x = pb.lcg_input(sum(BLOCKS), C, True, seed=29)
    o = po.OracleProgram(6, prog)
    want = o.run_block(x, C, C)
    rt.lib().dspRuntimeSetShard(1, 3)
    r = rt.Runtime(6, prog)
    si = r.shard_info()
    lo, n = si["first_chain"], si["nchains"]
    assert (lo, n) == (32, 32)
    pos, got = 0, []
    for b in BLOCKS:
        got.append(r.run_block(x[pos:pos + b, lo:lo + n], n, C + lo, out_io_base=lo))
        assert r.get_option("fir_shared_chains") == 32 and r.get_option("fir_shared_groups") == 2
        pos += b
    assert (words(np.concatenate(got)) == words(want[:, lo:lo + n])).all()

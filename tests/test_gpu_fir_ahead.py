"""Staged FIR launches ("fir_ahead"): under "overlap" 1 the FIRs of consecutive blocks run on two streams of the
library's own, each into a staging block, and a copy on the caller's stream moves the columns the FIR chains stored into the
caller's block.  The contract is "overlap" 1's: ONE output block may serve every call, and it is only ever written in the caller's
stream order.  Every case forces the path ("fir_ahead" 1), asks "fir_ahead_now" whether it was taken, enqueues its blocks back to
back without host synchronisation and holds every block's output and the state to the oracle word for word.

The FIR-only shape (no cascade) has no overlap mode at all (overlap_ok): it stays on the direct path, "fir_ahead_now" 0, same bits."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(test):
    """a GPU test: marked, and behind the fixture that loads the library and leaves its options as it found them (the rule tests at
    the end of the file need neither)"""
    return pytest.mark.gpu(pytest.mark.usefixtures("_options_back")(test))


BLOCKS = [1024, 333, 100, 1024, 100, 333]            # six calls; 333 and 100 are ragged tiles
SENT = 0x5EA1AB1E                                    # what unused columns and rows of an output block hold
SHAPES = {"f6": (6, 40, 8, 700), "f6_fir_only": (6, 8, 0, 64), "f4": (4, 24, 4, 300)}
SLEEP_CYCLES = 5_000_000                             # torch.cuda._sleep: a few milliseconds, far longer than a FIR of these sizes


@pytest.fixture
def _options_back():
    """options are process-wide: the tests here set every one they depend on, and leave the process as they found it"""
    rt.lib().dspRuntimeRelease()
    found = [(key, rt.lib().dspRuntimeGetOption(key.encode())) for key in ("fir_impl", "biquad_impl", "ready_words")]
    yield
    rt.lib().dspRuntimeRelease()
    for key, v in found + [("fir_ahead", -1), ("overlap", 0), ("fir_rows", 0), ("fir_tail", 0), ("chain_delay", 0), ("chain_finish", 0)]:
        rt.Runtime.set_global_option(key, v)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def chain_program(fmt, C, S, T, stores=1, gap=1):
    """pb.synth_program's chains with `stores` STOREs each, `gap` IOs apart: chain c stores IOs gap * stores * c .. + stores - 1.
    Inputs at IO `nout` .. ; -> (program, nout)"""
    nout = gap * stores * C
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + C * (48 + 8 * S + T + 8 * stores))
    taps = pb.lcg_taps_all(C, T)
    pw.core()
    for c in range(C):
        pw.param()
        bank = pw.biquad_bank(pb.synth_sections(c, S, pb.F48000, pb.F48000))
        imp = pw.fir_impulses([taps[c]])
        pw.load_gain_fixed(nout + c, 1.0)
        pw.biquads(bank, S)
        pw.fir(imp, T)
        pw.sat0db()
        for k in range(stores):
            pw.store(gap * stores * c + k)
    return pw.end_of_code(), nout


_REF = {}


def reference(name):
    """program, input, the oracle's output of every block and its state after every block -- computed once, shared, never written.
    -> (fmt, C, nout, in_base, prog, x, outs, states)"""
    if name not in _REF:
        if name in SHAPES:
            fmt, C, S, T = SHAPES[name]
            prog, nout = pb.synth_program(fmt, C, S, T), C
        elif name == "grouped":                       # two impulse banks of 16 chains each: the plans of the shared-impulse path
            fmt, C = 6, 32
            prog, nout = pb.synth_program(fmt, C, 4, 200, fir_banks=2), C
        elif name == "two_stores":                    # 5 chains x 2 stores: ten columns in a row, not a multiple of 16 bytes
            fmt, C = 6, 5
            prog, nout = chain_program(fmt, C, 3, 200, stores=2)
        else:                                         # "gapped": every other column, the ones between belong to nobody
            fmt, C = 6, 12
            prog, nout = chain_program(fmt, C, 3, 200, gap=2)
        x = pb.lcg_input(sum(BLOCKS), C, fmt == 6, seed=77)
        o = po.OracleProgram(fmt, prog)
        outs, states = [], []
        for a, n in cut(BLOCKS):
            outs.append(o.run_block(x[a:a + n], nout, nout))
            states.append(o.state.copy())
        for v in outs + states + [x, prog]:
            v.flags.writeable = False
        _REF[name] = (fmt, C, nout, nout, prog, x, outs, states)
    return _REF[name]


def staged_runtime(fmt, prog, fir_rows=0):
    r = rt.Runtime(fmt, prog)
    r.set_option("fir_impl", 1)                              # (options are process-wide: whatever an earlier test left)
    r.set_option("biquad_impl", 1)
    r.set_option("ready_words", -1)
    r.set_option("overlap", 1)
    r.set_option("fir_ahead", 1)
    r.set_option("fir_rows", fir_rows)
    assert r.get_option("fir_ahead") == 1 and r.get_option("fir_ahead_now") == 0
    return r


def device_inputs(x):
    import torch
    xd = [dm.to_device(x[a:a + n].copy()) for a, n in cut(BLOCKS)]
    torch.cuda.synchronize()                                 # the overlap mode's contract: inputs complete when the call is made
    return xd


def check_block(clone, want, nout, what):
    """the block's columns hold the oracle's words; every other word of the output block still holds the sentinel"""
    got = dm.to_host(clone).view(np.uint32)
    n = want.shape[0]
    assert (got[:n, :nout] == words(want)).all(), f"{what}: output differs from the oracle"
    assert (got[:n, nout:] == SENT).all(), f"{what}: a column outside the chains' was written"
    assert (got[n:] == SENT).all(), f"{what}: a frame behind the block was written"


def run_one_buffer(r, xd, C, in_base, nout, width, expect, sleep=False, between=None):
    """six calls into ONE output block of `width` words per frame (sentinels refilled in stream order in front of every call),
    cloned on the caller's stream behind each call -- with `sleep`, behind a spin of a few milliseconds queued between the call and
    its clone, so that the next call is made long before the clone runs.  -> the clones"""
    import torch
    st = torch.cuda.current_stream().cuda_stream             # the NULL stream, as a plain host hands it over
    y = torch.empty((1024, width), dtype=torch.int32, device="cuda")
    clones = []
    for k, n in enumerate(BLOCKS):
        if between is not None:
            between(k)
        y.fill_(SENT)
        r.run_block_device(xd[k].data_ptr(), C, in_base, y.data_ptr(), width, 0, n, st)
        assert r.get_option("fir_ahead_now") == expect, f"call {k}: {r.core_info(0)}, overlap {r.get_option('overlap')}, fir_impl {r.get_option('fir_impl')}"
        if sleep:
            torch.cuda._sleep(SLEEP_CYCLES)
        clones.append(y.clone())
    torch.cuda.synchronize()
    return clones


@gpu
@pytest.mark.parametrize("fir_rows", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_output_block_serves_every_call(name, fir_rows):
    """(a) one output block, cloned behind each call; (b) the same with a spin between call and clone: a FIR that wrote the
    caller's block early would put block k + 1 into clone k"""
    fmt, C, nout, in_base, prog, x, outs, states = reference(name)
    expect = 0 if name == "f6_fir_only" else 1
    xd = device_inputs(x)
    for sleep in (False, True):
        r = staged_runtime(fmt, prog, fir_rows)
        assert r.get_option("fir_ahead_apart") == -1         # (not tried yet)
        clones = run_one_buffer(r, xd, C, in_base, nout, nout, expect, sleep=sleep)
        assert r.get_option("fir_ahead_apart") in ((0, 1) if expect else (-1,))
        for k, c in enumerate(clones):
            check_block(c, outs[k], nout, f"{name}, fir_rows {fir_rows}, sleep {sleep}, block {k}")
        assert (r.sync_state() == states[-1]).all()
        assert r.get_option("ready_timeouts") == 0
        r.release()


@gpu
@pytest.mark.parametrize("name", ["f6", "f4"])
def test_wide_window_keeps_its_sentinels(name):
    """(c) an output window five words wider than the chains (an odd stride: the word-wise copy), ragged blocks in a 1024-frame
    buffer: the unused columns and the frames behind a block's last one are never written"""
    fmt, C, nout, in_base, prog, x, outs, states = reference(name)
    xd = device_inputs(x)
    r = staged_runtime(fmt, prog)
    clones = run_one_buffer(r, xd, C, in_base, nout, nout + 5, 1, sleep=True)
    for k, c in enumerate(clones):
        check_block(c, outs[k], nout, f"{name}, wide window, block {k}")
    assert (r.sync_state() == states[-1]).all()
    r.release()


@gpu
@pytest.mark.parametrize("name", ["two_stores", "gapped"])
def test_two_stores_and_gapped_columns(name):
    """(d) chains that store twice (ten columns: no 16-byte run) and chains that store every other column: the columns between
    them are nobody's and keep their sentinels"""
    import torch
    fmt, C, nout, in_base, prog, x, outs, states = reference(name)
    xd = device_inputs(x)
    r = staged_runtime(fmt, prog)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((1024, nout), dtype=torch.int32, device="cuda")
    clones = []
    for k, n in enumerate(BLOCKS):
        y.fill_(SENT)
        r.run_block_device(xd[k].data_ptr(), C, in_base, y.data_ptr(), nout, 0, n, st)
        assert r.get_option("fir_ahead_now") == 1
        torch.cuda._sleep(SLEEP_CYCLES)
        clones.append(y.clone())
    torch.cuda.synchronize()
    stored = np.zeros(nout, bool)
    stored[[c for c in range(nout) if name == "two_stores" or c % 2 == 0]] = True
    for k, c in enumerate(clones):
        got, n = dm.to_host(c).view(np.uint32), BLOCKS[k]
        assert (got[:n, stored] == words(outs[k])[:, stored]).all(), f"{name}, block {k}"
        assert (got[:n, ~stored] == SENT).all() and (got[n:] == SENT).all(), f"{name}, block {k}: a word of nobody's was written"
    assert (r.sync_state() == states[-1]).all()
    r.release()


@gpu
def test_state_calls_option_switches_and_release_in_flight():
    """(e) dspRuntimeSyncState and dspRuntimeUploadState in the middle of the six blocks, "fir_ahead" 1 -> 0 -> 1 between blocks,
    then a release with staged blocks in flight"""
    import torch
    fmt, C, nout, in_base, prog, x, outs, states = reference("f6")
    xd = device_inputs(x)
    r = staged_runtime(fmt, prog)
    seen = {}

    def between(k):
        if k == 3:                                           # blocks 0 .. 2 are in flight
            seen["state"] = r.sync_state().copy()
            r.upload_state()
        if k == 4:
            r.set_option("fir_ahead", 0)
        if k == 5:
            r.set_option("fir_ahead", 1)

    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((1024, nout), dtype=torch.int32, device="cuda")
    clones = []
    for k, n in enumerate(BLOCKS):
        between(k)
        r.run_block_device(xd[k].data_ptr(), C, in_base, y.data_ptr(), nout, 0, n, st)
        assert r.get_option("fir_ahead_now") == (0 if k == 4 else 1)
        clones.append(y[:n].clone())
    torch.cuda.synchronize()
    assert (seen["state"] == states[2]).all()
    for k, c in enumerate(clones):
        assert (dm.to_host(c).view(np.uint32) == words(outs[k])).all(), f"block {k}"
    assert (r.sync_state() == states[-1]).all()
    for k in range(3):                                       # staged blocks in flight when the program goes
        r.run_block_device(xd[0].data_ptr(), C, in_base, y.data_ptr(), nout, 0, 1024, st)
    r.release()
    torch.cuda.synchronize()
    r = staged_runtime(fmt, prog)                            # ... and the next program finds the device as it should be
    r.run_block_device(xd[0].data_ptr(), C, in_base, y.data_ptr(), nout, 0, 1024, st)
    torch.cuda.synchronize()
    assert (dm.to_host(y).view(np.uint32) == words(outs[0])).all()
    r.release()


@gpu
def test_in_place_call_takes_the_direct_path():
    """(f) input and output windows in the same memory: never staged, same bits"""
    import torch
    fmt, C, nout, in_base, prog, x, outs, states = reference("f6")
    r = staged_runtime(fmt, prog)
    st = torch.cuda.current_stream().cuda_stream
    for k, (a, n) in enumerate(cut(BLOCKS)):
        buf = dm.to_device(x[a:a + n].copy())
        torch.cuda.synchronize()
        r.run_block_device(buf.data_ptr(), C, in_base, buf.data_ptr(), C, 0, n, st)
        assert r.get_option("fir_ahead_now") == 0
        torch.cuda.synchronize()
        assert (dm.to_host(buf).view(np.uint32) == words(outs[k])).all(), f"block {k}"
    assert (r.sync_state() == states[-1]).all()
    r.release()


@gpu
def test_plans_with_impulse_groups_take_the_direct_path():
    """(f) a plan whose FIR chains are all grouped by impulse bank makes its per-chain taps when a launch first needs them, on that
    launch's stream: it is never staged ("fir_ahead_now" 0), and neither is a launch of fir_stream's ("fir_impl" 3, whose operand
    ring is made the same way) -- same bits, one output block for every call, a spin between call and clone"""
    fmt, C, nout, in_base, prog, x, outs, states = reference("grouped")
    xd = device_inputs(x)
    r = staged_runtime(fmt, prog)
    g = r.fir_group_info(0)
    assert g["groups"] == 2 and g["grouped_chains"] == C
    clones = run_one_buffer(r, xd, C, in_base, nout, nout, 0, sleep=True)
    for k, c in enumerate(clones):
        check_block(c, outs[k], nout, f"grouped, block {k}")
    assert (r.sync_state() == states[-1]).all()
    r.release()
    fmt, C, nout, in_base, prog, x, outs, states = reference("f6")
    xd = device_inputs(x)
    r = staged_runtime(fmt, prog)
    r.set_option("fir_impl", 3)
    clones = run_one_buffer(r, xd, C, in_base, nout, nout, 0, sleep=True)
    for k, c in enumerate(clones):
        check_block(c, outs[k], nout, f"fir_impl 3, block {k}")
    assert (r.sync_state() == states[-1]).all()
    r.release()


@gpu
def test_fir_tail_plan_takes_the_direct_path():
    """(f) a plan with handed FIR chains has no overlap mode: never staged, same bits"""
    from tests import firtail_programs as fp
    chains = [fp.chain(nsec=2, taps=64, slot="A"), fp.chain(nsec=3, taps=200, slot=None, finish="sat"), fp.chain(nsec=1, taps=33, slot="B", finish="gain")]
    prog, nin, nout = fp.program(6, [fp.core(chains, calc=0)])
    x = pb.lcg_input(sum(BLOCKS), nin, True, seed=3)
    o = po.OracleProgram(6, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    for key in ("fir_impl", "biquad_impl", "chain_finish", "chain_delay", "fir_tail", "overlap", "fir_ahead"):
        r.set_option(key, 1)
    assert r.fir_tail_info(0) == fp.handed(chains) and fp.handed(chains)[0] == 2
    for k, (a, n) in enumerate(cut(BLOCKS)):
        want = o.run_block(x[a:a + n], nout, fp.IN)
        got = r.run_block(x[a:a + n], nout, fp.IN)
        assert r.get_option("fir_ahead_now") == 0
        assert (words(got) == words(want)).all(), f"block {k}"
    assert (r.sync_state() == o.state).all()
    r.release()


# ---------------------------------------------------------------- the rule, without a GPU
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("firahead") / "fir_ahead_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "fir_ahead_driver.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def ask(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


def test_rule_takes_the_north_star_and_leaves_the_shards(driver):
    """(g) fir_ahead_by_plan: launches of more than a chip of waves at a time -- the north star (4096 chains x 4096 taps) and a
    2048-chain x 4096-tap plan -- are staged; north8 (512 x 4096), cfg5s (2048 x 2048) and cfg4 (256 x 4096) are not"""
    assert ask(driver, "rule", 4096, 4096, 1024) == "1"
    assert ask(driver, "rule", 2048, 4096, 1024) == "1"
    assert ask(driver, "rule", 512, 4096, 1024) == "0"
    assert ask(driver, "rule", 2048, 2048, 1024) == "0"
    assert ask(driver, "rule", 256, 4096, 1024) == "0"


def test_staging_cap_and_column_lists(driver):
    """a staging block is 1024 frames of the caller's window, 64 MB at the most; the copy's columns are the FIR chains' stores in
    ascending order, one run or a list"""
    assert ask(driver, "stage", 4096) == str(1024 * 4096)
    assert ask(driver, "stage", 16384) == str(1024 * 16384)
    assert ask(driver, "stage", 16385) == "0" and ask(driver, "stage", 0) == "0"
    assert ask(driver, "cols", 1, 2, 1, 0, 1, 1, 1, 3) == "run: 0 1 2 3"
    assert ask(driver, "cols", 2, 4, 5, 2, 6, 7) == "run: 4 5 6 7"
    assert ask(driver, "cols", 1, 0, 1, 2, 1, 4) == "list: 0 2 4"
    assert ask(driver, "cols", 0) == "list:"

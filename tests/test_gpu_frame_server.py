"""The frame server ("frame_server"): dspRuntime_N calls of interpreter cores served by one resident wave per program
must give what the launch per call gives -- the reference's outputs and state, bit for bit -- whatever runs between the frames."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR, check_against_golden, make_input, make_program
from tests.test_gpu_parity import sha

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(GOLDEN_DIR, "manifest.json")) as _f:
    B1_CASES = [c for c in json.load(_f)["cases"] if c["name"].endswith("_b1")]


@pytest.fixture(autouse=True)
def _server_on():
    L = rt.lib()
    L.dspRuntimeRelease()
    assert L.dspRuntimeSetOption(b"frame_server", 1) == 0
    yield
    L.dspRuntimeRelease()
    L.dspRuntimeSetOption(b"frame_server", 0)
    L.dspRuntimeSetOption(b"frame_server_idle_us", 1000)


def frames_like_the_parity_test(r, x, out_stride, in_base, scratch):
    """test_gpu_parity.py::test_general_interpreter_single_frame_and_store_mem's loop: cores in order on one samples[] array"""
    got = np.zeros((len(x), out_stride), dtype=x.dtype)
    frame = np.zeros(max(scratch, 64), dtype=x.dtype)
    for n in range(len(x)):
        frame[in_base:in_base + x.shape[1]] = x[n]
        for core in range(len(r.cores)):
            r.run_frame(frame, core)
        got[n] = frame[:out_stride]
        frame[:out_stride] = 0
    return got


def counters(r):
    return {k: r.get_option("frame_server_" + k) for k in ("frames", "launches", "fallbacks")}


@pytest.mark.parametrize("case", B1_CASES, ids=lambda c: c["name"])
def test_goldens_frame_by_frame(case):
    fmt = case["fmt"]
    prog = make_program(case["program"])
    x = make_input(case["input"], fmt)
    r = rt.Runtime(fmt, prog, fs=case["fs"], random=case["random"], dither=case["dither"])
    assert r.rc == case["init_rc"]
    assert r.get_option("frame_server") == 1
    out = frames_like_the_parity_test(r, x, case["out_stride"], case["in_base"], case["scratch"])
    c = counters(r)
    check_against_golden(case, out, r.sync_state(), sha)
    assert c["frames"] == len(x) * len(r.cores) and c["fallbacks"] == 0 and c["launches"] >= 1, c


def oracle_frames(fmt, prog, seed):
    """random programs of tests/fuzz_programs.py frame by frame, the samples[] array kept by the caller on both sides"""
    from tests.fuzz_programs import IN_BASE, N_IN, N_OUT, random_program
    prog = random_program(seed, fmt)
    x = pb.lcg_input(120, N_IN, fmt in (5, 6), seed=seed)
    o = po.OracleProgram(fmt, prog, fs=48000, random=seed, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=seed, dither=24)
    assert r.rc == o.rc
    if r.rc < 0:
        return None
    want = o.run_block(x, N_OUT, IN_BASE, 0, block=1, frame=np.zeros(256, dtype=np.uint32))
    got = np.zeros_like(want)
    frame = np.zeros(256, dtype=want.dtype)
    for n in range(len(x)):
        for core in range(len(r.cores)):
            frame[:N_OUT] = got[n]
            frame[IN_BASE:IN_BASE + N_IN] = x[n]
            r.run_frame(frame, core)
            got[n] = frame[:N_OUT]
    return r, o, prog, got, want


@pytest.mark.parametrize("seed", [3, 17, 40])
def test_random_programs_frame_by_frame(seed):
    for fmt in (2, 3, 4, 5, 6):
        res = oracle_frames(fmt, None, seed)
        if res is None:
            continue
        r, o, prog, got, want = res
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=0))[0]
        assert bad.size == 0, f"seed {seed} DSP_FORMAT {fmt}: output columns {list(bad)} differ"
        r.sync_state()
        n = int(prog[1]) + int(prog[2])
        assert (r.buf[12:n] == o.buf[12:n]).all(), f"seed {seed} DSP_FORMAT {fmt}: buffer differs"
        assert r.get_option("frame_server_frames") == 120 * len(r.cores)
        assert r.get_option("frame_server_fallbacks") == 0
        r.release()


def _dacdiy(random=3):
    prog = np.fromfile(os.path.join(GOLDEN_DIR, "dacdiy1.bin"), dtype=np.uint32)
    return prog, po.OracleProgram(2, prog, fs=48000, random=random, dither=24), rt.Runtime(2, prog, fs=48000, random=random, dither=24)


def test_calls_between_frames_see_and_set_the_state():
    prog, o, r = _dacdiy()
    x = pb.lcg_input(200, 16, False, seed=5)

    def frames(a, b):
        want = o.run_block(x[a:b], 32, 8, 0, scratch_len=40, block=1)
        got = frames_like_the_parity_test(r, x[a:b], 32, 8, 40)
        assert (got == want).all(), f"frames {a}..{b} differ"

    frames(0, 20)
    ck = r.sync_state().copy()                              # dspRuntimeSyncState mid-stream
    assert (ck == o.state).all()
    frames(20, 40)
    r.state[:] = ck; o.state[:] = ck                        # dspRuntimeUploadState of an earlier checkpoint
    r.upload_state()
    frames(40, 60)
    assert (r.sync_state() == o.state).all()
    r.upload_params()                                       # dspRuntimeUploadParams (the plans are made again)
    frames(60, 80)
    assert r.reset(48000, 3, 24) == 0 and o.reset(48000, 3, 24) == 0      # dspRuntimeReset
    frames(80, 100)
    want = o.run_block(x[100:140], 32, 8, 0, scratch_len=40)      # a dspRuntimeBlockAll block
    got = r.run_block_all(x[100:140], 32, 8, 0)
    assert (got == want).all()
    frames(140, 200)
    assert (r.sync_state() == o.state).all()
    n = int(prog[1])
    assert (r.buf[:n] == o.buf[:n]).all()
    assert r.get_option("frame_server_fallbacks") == 0 and r.get_option("frame_server_frames") > 0


def test_the_server_leaves_when_idle_and_comes_back():
    prog, o, r = _dacdiy()
    r.set_option("frame_server_idle_us", 200)
    x = pb.lcg_input(40, 16, False, seed=9)
    want = o.run_block(x, 32, 8, 0, scratch_len=40, block=1)
    got = frames_like_the_parity_test(r, x[:20], 32, 8, 40)
    before = r.get_option("frame_server_launches")
    time.sleep(5 * 200e-6 + 0.002)
    got2 = frames_like_the_parity_test(r, x[20:21], 32, 8, 40)
    assert r.get_option("frame_server_launches") == before + 1
    got3 = frames_like_the_parity_test(r, x[21:], 32, 8, 40)
    assert (np.concatenate([got, got2, got3]) == want).all()
    assert (r.sync_state() == o.state).all()
    assert r.get_option("frame_server_fallbacks") == 0


def test_two_programs_alternate_and_one_is_released():
    p1 = np.fromfile(os.path.join(GOLDEN_DIR, "crossoverLV6.bin"), dtype=np.uint32)
    p2 = np.fromfile(os.path.join(GOLDEN_DIR, "dacdiy1.bin"), dtype=np.uint32)
    o1, o2 = po.OracleProgram(2, p1, fs=48000, random=1, dither=24), po.OracleProgram(2, p2, fs=48000, random=2, dither=24)
    r1, r2 = rt.Runtime(2, p1, fs=48000, random=1, dither=24), rt.Runtime(2, p2, fs=48000, random=2, dither=24)
    x = pb.lcg_input(60, 16, False, seed=21)
    w1 = o1.run_block(x[:40], 32, 8, 0, scratch_len=40, block=1)          # (r1 runs 40 frames, then goes)
    w2 = o2.run_block(x, 32, 8, 0, scratch_len=40, block=1)
    g1 = np.zeros_like(w1); g2 = np.zeros_like(w2)
    for n in range(40):
        g1[n] = frames_like_the_parity_test(r1, x[n:n + 1], 32, 8, 40)[0]
        g2[n] = frames_like_the_parity_test(r2, x[n:n + 1], 32, 8, 40)[0]
    assert (g1 == w1).all() and (g2[:40] == w2[:40]).all()
    s1 = r1.sync_state().copy()
    r1.release()
    g2[40:] = frames_like_the_parity_test(r2, x[40:], 32, 8, 40)
    assert (g2 == w2).all()
    assert (r2.sync_state() == o2.state).all()
    assert (s1 == o1.state).all()
    assert r2.get_option("frame_server_fallbacks") == 0


def test_option_off_and_chain_programs():
    L = rt.lib()
    assert L.dspRuntimeSetOption(b"frame_server", 0) == 0
    prog, o, r = _dacdiy()
    x = pb.lcg_input(30, 16, False, seed=4)
    want = o.run_block(x, 32, 8, 0, scratch_len=40, block=1)
    assert (frames_like_the_parity_test(r, x, 32, 8, 40) == want).all()
    assert r.get_option("frame_server_launches") == 0 and r.get_option("frame_server_frames") == 0
    r.release()
    assert L.dspRuntimeSetOption(b"frame_server", 1) == 0
    for generic in (0, 1):
        cp = pb.synth_program(2, 3, 2)
        oc = po.OracleProgram(2, cp, fs=48000, dither=24)
        rc_ = rt.Runtime(2, cp, fs=48000, dither=24)
        rc_.set_option("generic", generic)
        xc = pb.lcg_input(30, 3, False, seed=8)
        want = oc.run_block(xc, 3, 3, 0, block=1, frame=np.zeros(64, dtype=np.uint32))
        got = np.zeros_like(want)
        frame = np.zeros(64, dtype=np.int32)
        for n in range(len(xc)):
            for core in range(len(rc_.cores)):
                frame[0:3] = got[n]
                frame[3:6] = xc[n]
                rc_.run_frame(frame, core)
                got[n] = frame[0:3]
        assert (got == want).all(), f"generic {generic}"
        assert (rc_.sync_state() == oc.state).all()
        assert (rc_.get_option("frame_server_frames") > 0) == bool(generic)
        rc_.release()
    L.dspRuntimeSetOption(b"generic", 0)


def test_unmodified_host_with_the_environment_variable(tmp_path):
    exe = str(tmp_path / "frame_host")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", f"-I{ROOT}/include", "-DDSP_FORMAT=2",
                           f"{ROOT}/examples/frame_host.c", f"-L{ROOT}/avdsp_amd/lib", "-lavdsp_mi355x",
                           f"-Wl,-rpath,{ROOT}/avdsp_amd/lib", "-o", exe])
    prog = np.fromfile(os.path.join(GOLDEN_DIR, "crossoverLV6.bin"), dtype=np.uint32)
    nin, in_base, nout, out_base = 8, 16, 8, 24
    x = pb.lcg_input(300, nin, False, seed=11)
    (tmp_path / "p.bin").write_bytes(prog.tobytes())
    (tmp_path / "in.raw").write_bytes(x.tobytes())
    env = dict(os.environ, AVDSP_FRAME_SERVER="1")
    res = subprocess.run([exe, str(tmp_path / "p.bin"), "48000", str(tmp_path / "in.raw"), str(nin), str(in_base),
                          str(tmp_path / "out.raw"), str(nout), str(out_base)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(str(tmp_path / "out.raw"), dtype=np.int32).reshape(300, nout)
    o = po.OracleProgram(2, prog, fs=48000, random=12345, dither=24)
    want = o.run_block(x, nout, in_base, out_base, scratch_len=40, block=1)
    assert (got == want).all()
    words = res.stdout.split("state[0..3]=")[1].split()
    assert [int(w, 16) for w in words[:4]] == [int(v) for v in o.state[:4]]

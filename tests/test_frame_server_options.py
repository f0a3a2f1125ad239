"""CPU-only checks of the frame server's options (include/avdsp_runtime.h, "frame_server"): the keys exist, the idle bound is
range-checked, the counters read 0 before any device copy exists, and AVDSP_FRAME_SERVER=1 sets the default of a fresh process."""
import os
import subprocess
import sys

import pytest

from avdsp_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore():
    L = rt.lib()
    L.dspRuntimeRelease()
    yield
    L.dspRuntimeSetOption(b"frame_server", 0)
    L.dspRuntimeSetOption(b"frame_server_idle_us", 1000)
    L.dspRuntimeRelease()


def test_frame_server_option_round_trips():
    L = rt.lib()
    assert L.dspRuntimeGetOption(b"frame_server") == 0
    assert L.dspRuntimeSetOption(b"frame_server", 1) == 0, L.dspRuntimeLastError()
    assert L.dspRuntimeGetOption(b"frame_server") == 1
    assert L.dspRuntimeSetOption(b"frame_server", 0) == 0
    assert L.dspRuntimeGetOption(b"frame_server") == 0
    assert L.dspRuntimeSetOption(b"frame_server", 2) == -1


def test_idle_bound_is_range_checked():
    L = rt.lib()
    assert L.dspRuntimeGetOption(b"frame_server_idle_us") == 1000
    for ok in (50, 20000):
        assert L.dspRuntimeSetOption(b"frame_server_idle_us", ok) == 0, L.dspRuntimeLastError()
        assert L.dspRuntimeGetOption(b"frame_server_idle_us") == ok
    for bad in (49, 20001, 0, -1):
        assert L.dspRuntimeSetOption(b"frame_server_idle_us", bad) == -1
        assert L.dspRuntimeGetOption(b"frame_server_idle_us") == 20000


def test_counters_read_zero_before_any_device_exists():
    L = rt.lib()
    for key in (b"frame_server_frames", b"frame_server_launches", b"frame_server_fallbacks"):
        assert L.dspRuntimeGetOption(key) == 0


@pytest.mark.parametrize("value, want", [("1", 1), (None, 0)])
def test_environment_sets_the_default_of_a_fresh_process(value, want):
    env = dict(os.environ)
    env.pop("AVDSP_FRAME_SERVER", None)
    if value is not None:
        env["AVDSP_FRAME_SERVER"] = value
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = "from avdsp_amd import runtime as rt; print(rt.lib().dspRuntimeGetOption(b'frame_server'))"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout.split()[-1]) == want

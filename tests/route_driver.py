"""tests/csrc/launch_route_driver.cpp for the tests that ask it (test_launch_route.py, test_gpu_launch_route.py): built against
avdsp_amd/csrc/avdsp_plan_layout.h alone with AddressSanitizer and UBSan, run as a program of its own, one JSON object per question."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACK_TO_BACK, DIRECT, OWN_FIR, STAGED = 0, 1, 2, 3
ON_CALLER, ON_FIR_TURN, ON_FIR_FIRST = 0, 1, 2           # the stream the side-by-side probe runs against

# the options as the library ships them under "overlap" 1, fir_tile and biquad_row, a plan with every table, a program without
# instances, a call that is not in place into a window of 4096 words, a kernel timer that is not sampled
DEFAULTS = dict(overlap=1, cu_split=0, fir_ahead=-1, ready_words=-1, fir_launch=-1, fir_impl=1, biquad_impl=1, nframes=1024, out_stride=4096,
                in_place=0, overlap_ok=1, n_fir=4096, max_taps=4096, n_ahead_cols=4096, instances=0, n_sh_groups=0, has_taps64=1, has_ready=1,
                inst_n=1, chain_inst=0, has_timeouts=1, timer_samples=0, n_fir_only=0, ahead_apart=0, side_by_side=0)


def build_driver(dirname):
    """the driver's path, or a text that says why it could not be built"""
    if shutil.which("g++") is None:
        return None, "no g++"
    exe = os.path.join(str(dirname), "launch_route_driver")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "launch_route_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, "sanitizer build not available here: " + r.stderr[-300:]
    return exe, ""


def ask(exe, **facts):
    unknown = set(facts) - set(DEFAULTS)
    assert not unknown, unknown
    args = [f"{k}={int(v)}" for k, v in {**DEFAULTS, **facts}.items()]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout)

"""Per-call cost of dspRuntime_N, the reference's one-frame entry point, with the frame server off and on.

For crossoverLV6.bin (2 cores) and dacdiy1.bin (4 cores), DSP_FORMAT 2 at 48 kHz: at least 20 000 core calls each way, timed one by
one on the host (perf_counter_ns around the ctypes call, so ~1 us of Python is inside every figure).  Prints the median and p99 per
core call and the real-time factor of the unmodified host loop at 48 kHz (20.83 us per frame / the mean time of a frame's calls;
above 1 = faster than real time), then one JSON line.

    python tools/frame_server_bench.py [--calls 20000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avdsp_amd import progbuilder as pb      # noqa: E402
from avdsp_amd import runtime as rt          # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FRAME_US_48K = 1e6 / 48000


def measure(name: str, server: int, calls: int) -> dict:
    L = rt.lib()
    L.dspRuntimeSetOption(b"frame_server", server)
    prog = np.fromfile(os.path.join(GOLDEN, name), dtype=np.uint32)
    r = rt.Runtime(2, prog, fs=48000, random=12345, dither=24)
    ncores = len(r.cores)
    nframes = (calls + ncores - 1) // ncores
    x = pb.lcg_input(nframes + 200, 16, False, seed=7)
    frame = np.zeros(64, dtype=np.int32)
    fn, rundata, ptr = L.dspRuntime_2, r.rundata, frame.ctypes.data
    cores = list(r.cores)
    t = np.zeros((nframes, ncores), dtype=np.int64)
    for n in range(200):                                 # warm-up: plans, the first server launch
        frame[8:24] = x[n]
        for c in cores:
            fn(c, rundata, ptr)
    for n in range(nframes):
        frame[8:24] = x[200 + n]
        for k, c in enumerate(cores):
            t0 = time.perf_counter_ns()
            rc = fn(c, rundata, ptr)
            t[n, k] = time.perf_counter_ns() - t0
            if rc < 0:
                raise RuntimeError(r.last_error())
        frame[:32] = 0
    us = t.ravel() / 1e3
    res = dict(program=name, server=server, cores=ncores, calls=int(us.size), median_us=round(float(np.median(us)), 2),
               p99_us=round(float(np.percentile(us, 99)), 2), mean_us=round(float(us.mean()), 2),
               frame_us=round(float(t.sum(axis=1).mean() / 1e3), 2),
               launches=r.get_option("frame_server_launches"), fallbacks=r.get_option("frame_server_fallbacks"))
    res["realtime_48k"] = round(FRAME_US_48K / res["frame_us"], 3)
    r.release()
    L.dspRuntimeSetOption(b"frame_server", 0)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20000)
    a = ap.parse_args()
    rows = []
    for name in ("crossoverLV6.bin", "dacdiy1.bin"):
        for server in (0, 1):
            row = measure(name, server, a.calls)
            rows.append(row)
            print(f"{name:18s} server {server}: {row['calls']} core calls, median {row['median_us']:.2f} us, p99 {row['p99_us']:.2f} us, "
                  f"frame {row['frame_us']:.2f} us -> {row['realtime_48k']:.2f} x real time at 48 kHz "
                  f"(launches {row['launches']}, fallbacks {row['fallbacks']})", flush=True)
    print(json.dumps(dict(bench="frame_server", rows=rows)))


if __name__ == "__main__":
    main()

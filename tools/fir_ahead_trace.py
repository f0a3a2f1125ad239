#!/usr/bin/env python3
"""How consecutive fir_tile dispatches follow each other, from a rocprofv3 kernel trace of bench.py:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py
    python tools/fir_ahead_trace.py DIR
Per pair of consecutive FIR launches of the trace's last third (the timed region): the launch's own start-to-end time, the time from a
launch's end to the next one's start (negative: the two are in flight together) and from start to start (the step); the copy kernel of
the staged path and the cascades beside them; and a dozen dispatches in full."""
import csv
import glob
import sys

import numpy as np

rows = []
for f in glob.glob(sys.argv[1] + "/*/*_kernel_trace.csv"):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?")))
rows.sort()
rows = rows[2 * len(rows) // 3:]


def short(n):
    return "fir" if "fir_tile" in n else "copy" if "ahead_copy" in n else "cascade" if "biquad_" in n else "ready_set" if "ready_set" in n else "other"


def line(what, v):
    v = np.asarray(v) / 1e3
    print(f"{what}: median {np.median(v):.1f} us, p10 {np.percentile(v, 10):.1f}, p90 {np.percentile(v, 90):.1f} ({len(v)})")


for kind in ("fir", "cascade", "copy", "ready_set"):
    d = [e - s for s, e, n, _ in rows if short(n) == kind]
    if d:
        line(f"{kind} start -> end", d)
firs = [r for r in rows if short(r[2]) == "fir"]
line("fir end -> next fir start", [b[0] - a[1] for a, b in zip(firs[:-1], firs[1:])])
line("fir start -> next fir start", [b[0] - a[0] for a, b in zip(firs[:-1], firs[1:])])
line("fir end -> next fir end", [b[1] - a[1] for a, b in zip(firs[:-1], firs[1:])])
print("queues of the FIR launches:", sorted({q for *_, q in firs}))
copies = [r for r in rows if short(r[2]) == "copy"]
if copies:
    # the FIR whose end precedes the copy's start most closely is the one it copies
    ends = np.array([e for _, e, _, _ in firs])
    line("fir end -> its copy's start", [c[0] - ends[ends <= c[0]].max() for c in copies if (ends <= c[0]).any()])
t0 = rows[-40][0]
print("start_us    end_us   dur_us  queue  kernel")
for s, e, n, q in rows[-40:-24]:
    print(f"{(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f}  {q:>5}  {short(n)}")

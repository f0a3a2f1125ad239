#!/usr/bin/env python3
"""Characterisation of the host's core reports and option calls (avdsp_host.c): a fixed corpus of programs -- the .bin
programs of tests/golden, random_program seeds, progbuilder.synth_program shapes, accepted programs of every *_programs module and of
mux_recipes, and seeded mutants of all of them (mutate() of tests/test_scan_fuzz.py) -- replayed under every DSP_FORMAT, with the six
lowering options all off, all on, each on alone and each off alone, unsharded and as shard 1 of 3.  Per core: the return code and the outputs of the ten
dspRuntime...Info calls and of dspRuntimeStrandInfo, and dspRuntimeLastError() after dspRuntimeCoreInfo.  Then a fixed script of
dspRuntimeSetOption / dspRuntimeGetOption calls, without a program and with one.  Host-only: no device is touched.

The fixture is data, recorded from a build of the commit BEFORE the host lowering was put in stages; tests/test_lowering_report.py
replays the corpus through the library of the tree it runs in and compares every field.  To record it again (only where a change of
behaviour is meant), build the library to record from and name it:

    python tests/golden/make_lowering_report.py [--lib path/to/libavdsp_mi355x.so] --write

Every distinct report is stored once; a case lists indices.  Runs in a process of its own: what the option calls read back depends on
what the process has set before."""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import re
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from avdsp_amd import progbuilder as pb          # noqa: E402
from avdsp_amd import runtime as rt              # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lowering_report.json.gz")
LOWERINGS = ("chain_finish", "chain_delay", "fir_tail", "mux_tail", "chain_mem", "chain_copy")
# all off, all on, each on alone, each off alone ("fir_tail" and "mux_tail" change nothing without "chain_finish" or "chain_delay")
OPTION_SETS = [(), LOWERINGS] + [(k,) for k in LOWERINGS] + [tuple(j for j in LOWERINGS if j != k) for k in LOWERINGS]
SHARDS = ((0, 1), (1, 3))
FORMATS = (2, 3, 4, 5, 6)
# (call, number of int outputs); dspRuntimeCoreInfo goes first, its refusal text is recorded
REPORTS = (("dspRuntimeCoreInfo", 3), ("dspRuntimeFirGroupInfo", 3), ("dspRuntimeMuxInfo", 4), ("dspRuntimeFinishInfo", 2),
           ("dspRuntimeDelayInfo", 2), ("dspRuntimeFirTailInfo", 2), ("dspRuntimeMuxTailInfo", 3), ("dspRuntimeMemInfo", 3),
           ("dspRuntimeCopyInfo", 2), ("dspRuntimeShardInfo", 7), ("dspRuntimeStrandInfo", 3))
UNWRITTEN = -777                                 # what an output holds before the call: a failing call leaves it
MUTANTS = 12                                     # per base program
MUTANT_SEED = 20

BINS = ("crossoverLV6.bin", "dacdiy1.bin", "dacfabriceo.bin", "dsptest1.bin", "mydspcode.bin", "tour_float.bin", "tour_int.bin",
        "enc_hilbert_2_4_9.bin", "enc_hilbert_2_5_5.bin", "enc_hilbert_6_0_13.bin", "enc_hilbert_6_4_7.bin",
        "enc_sweep_2_4_9.bin", "enc_sweep_2_5_5.bin", "enc_sweep_6_0_13.bin", "enc_sweep_6_4_7.bin")


def built_programs():
    """accepted programs of the lowering tests' builders, one Q28 and one float encoding each: [(name, words)]"""
    from tests import copy_programs as cp
    from tests import delay_programs as dp
    from tests import finish_programs as fp
    from tests import firtail_programs as ft
    from tests import memtree_programs as mt
    from tests import mux_recipes as mr
    from tests import muxtail_programs as mp
    from tests.fuzz_programs import random_program
    out = []
    m2 = [(0, 0.3), (1, -0.2)]
    src = lambda k: cp.IN + 20 + k               # noqa: E731
    for fmt in (2, 6):
        e = f"_e{fmt}"
        for seed in range(3):
            out.append((f"random{seed}{e}", random_program(seed, fmt)))
        out.append((f"synth_3x2_fir9{e}", pb.synth_program(fmt, 3, 2, 9 if fmt == 6 else 0)))
        out.append((f"synth_18x1_fir5{e}", pb.synth_program(fmt, 18, 1, 5 if fmt == 6 else 0)))       # (a FIR group of 18 in formats 4 and 6)
        out.append((f"finish{e}", fp.program(fmt, [fp.core([fp.chain(2, "tpdf_gain"), fp.chain(1, "gain")], calc=0), fp.core([fp.chain(1, "tpdf")])])[0]))
        out.append((f"delay{e}", dp.program(fmt, [dp.core([dp.chain(2, "A", "param", us=1000), dp.chain(1, "B", "fixed", us=2100)]),
                                                  dp.core([dp.chain(1, "A", "fixed", us=63, finish="tpdf")], calc=0)])[0]))
        out.append((f"firtail{e}", ft.program(fmt, [ft.core([ft.chain(2, 64, "A", "fixed", us=2100, finish="sat"), ft.chain(1, 40, "B", "param", us=1000, finish="sat")]),
                                                    ft.core([ft.chain(), ft.chain(0, 7, None, finish="gain")], calc=0)])[0]))
        out.append((f"muxtail{e}", mp.program(fmt, [mp.core([mp.chain(m2, slot="A", finish="tpdf")], calc=0),
                                                    mp.core([mp.chain(m2, nsec=1), mp.chain(None, nsec=1, slot="B", us=63, inp=3)]),
                                                    mp.core([mp.chain(m2), mp.chain(None, nsec=0, finish="gain", inp=4)])])[0]))
        out.append((f"muxtail_small{e}", mp.program(fmt, [mp.core(mp.small_core(), calc=0)])[0]))
        out.append((f"muxtail_fir{e}", mp.program(fmt, [mp.core(mp.fir_tail_chains(), calc=0)])[0]))
        out.append((f"memtree{e}", mt.program(fmt, [mt.core([mt.trunk("a", 1), mt.plain(nsec=1, finish="sat"), mt.branch("a", nsec=1, finish="sat")]),
                                                    mt.core([mt.trunk("b", 2), mt.branch("b", nsec=0, finish="tpdf"), mt.branch("c", nsec=1, slot="A", us=63, finish="sat")], calc=0)])[0]))
        c0 = cp.core([cp.copies([(src(2), 102), (src(3), 103)]), cp.plain(nsec=1, finish="sat"), cp.copies([(src(4), 104)]), cp.trunk("a", 2),
                      cp.copies([(src(5), 105), (src(6), 106), (src(7), 107)]), cp.branch("a", nsec=1, finish="tpdf"), cp.plain(nsec=0, finish="sat"),
                      cp.copies([(src(8), 108)])], calc=0, head=[cp.copies([(src(0), 100), (src(1), 101)])])
        c1 = cp.core([cp.copies([(src(k), 120 + k) for k in range(6)])])
        c2 = cp.core([cp.copies([(src(0), 130), (130, 131)]), cp.plain(nsec=1, finish="sat")])
        out.append((f"copy{e}", cp.program(fmt, [c0, c1, c2])[0]))
        out.append((f"mixer{e}", mr.small_mixer(fmt)[0]))
        out.append((f"mixer_fir{e}", mr.small_mixer(fmt, True)[0]))
    return out


def corpus():
    """[(name, program words)]: the base programs, then MUTANTS seeded mutants of each"""
    from tests.golden_recipes import GOLDEN_DIR
    from tests.test_scan_fuzz import mutate
    base = [(n, np.fromfile(os.path.join(GOLDEN_DIR, n), dtype=np.uint32)) for n in BINS] + built_programs()
    out = list(base)
    for b, (name, prog) in enumerate(base):
        rng = np.random.default_rng([MUTANT_SEED, b])
        for m in range(MUTANTS):
            out.append((f"{name}~{m}", mutate(rng, prog)))
    return out


def report_of(L, fmt, core):
    """[rc, outputs ..., dspRuntimeLastError() behind the call] per call; the text is "" where the call wrote none (a failing option
    call in front of each one puts a known text there)"""
    rep = []
    for name, nout in REPORTS:
        v = [C.c_int(UNWRITTEN) for _ in range(nout)]
        L.dspRuntimeSetOption(b"", 0)
        rc = getattr(L, name)(fmt, core, *[C.byref(x) for x in v])
        err = L.dspRuntimeLastError().decode("latin-1")
        rep.append([rc] + [x.value for x in v] + ["" if err == "unknown option ''" else err])
    return rep


def replay_program(L, prog, fmt, intern):
    """one program under one DSP_FORMAT: (dspRuntimeInit's result, cores, report indices by option set, shard and core)"""
    n = int(prog[1]) + max(int(np.int32(prog[2])), 0)
    buf = np.zeros(max(n, len(prog)) + 64, dtype=np.uint32)
    buf[:len(prog)] = prog
    base = buf.ctypes.data
    rc = L.dspRuntimeInit(base, n, 48000, 1, 24)
    cores, idx = [], []
    if rc >= 0:
        # (a mutant may hold no DSP_CORE word: dspFindCore then answers every number with the program itself, as the reference does)
        for k in range(1, 65):
            p = L.dspFindCore(base, k)
            if not p or (k > 1 and p == base):
                break
            cores.append(L.dspFindCoreBegin(p))
        for on in OPTION_SETS:
            for key in LOWERINGS:
                L.dspRuntimeSetOption(key.encode(), int(key in on))
            for rank, world in SHARDS:
                L.dspRuntimeSetShard(rank, world)
                for core in cores:
                    idx.append(intern(report_of(L, fmt, core)))
        L.dspRuntimeSetShard(0, 1)
    L.dspRuntimeRelease()
    return rc, len(cores), idx


# ---- the option script ----
# (key, a legal value, an illegal value or None); read-only keys and an unknown one have no legal value
OPTION_SCRIPT = (
    ("fir_impl", 0, None), ("biquad_impl", 2, None), ("device", 3, None), ("generic", 1, None), ("interp_impl", 0, None),
    ("strand_split", 0, None), ("strand_lanes", 2, None), ("overlap", 1, None), ("fir_rows", 2, None), ("host_split", 1, None),
    ("ready_words", 0, None), ("lane_hw", 0, None), ("fir_split", 1, None), ("rate_count_static", 3, None), ("host_pin", 1, None),
    ("fir_lean", 1, None), ("fir_shared", 0, 2), ("chain_finish", 1, 2), ("chain_delay", 1, -1), ("fir_tail", 1, 2), ("mux_tail", 1, 2),
    ("chain_mem", 1, 2), ("chain_copy", 1, -1), ("ring_wait", 5, None), ("fir_ahead", 1, 2), ("fir_launch", 2, None),
    ("profile_stride", 4, 0), ("ready_timeouts", 0, 1), ("group_fanout", 0, None), ("cu_split", 8, None), ("frame_server", 1, 2),
    ("frame_server_idle_us", 200, 49), ("ready_test", 0, None), ("profile", 1, None),
    ("fir_shared_chains", None, 1), ("fir_shared_groups", None, 1), ("fir_shared_rows", None, 1), ("fir_ahead_now", None, 1),
    ("fir_ahead_apart", None, 1), ("levels", None, 1), ("cores", None, 1), ("pieces", None, 1), ("strands", None, 1),
    ("timing_pairs_0", None, 1), ("timing_pairs_7", None, 1), ("timing_pairs_8", None, 1), ("timing_pairs_10", None, 1),
    ("side_by_side", None, 1), ("streams_remade", None, 1), ("ready_mode", None, 1), ("frame_server_frames", None, 1),
    ("frame_server_launches", None, 1), ("frame_server_fallbacks", None, 1), ("shard_rank", None, 1), ("shard_world", None, 1),
    ("chain_copies", None, 1), ("", None, 0),
)


def option_script(L):
    """[[phase, key, step, rc, error text of a failing call, read-back]]: every key read, set to an illegal value, read, set to a legal
    one, read -- without a program (the template), with a program that inherits what the template got, and on a second program after
    the options went back, which shows what a program loaded later starts from"""
    rows = []

    def walk(phase, legal=True):
        for key, good, bad in OPTION_SCRIPT:
            k = key.encode()
            steps = [("read", None), ("bad", bad)] + ([("good", good)] if legal else [])
            for step, value in steps:
                rc, err = 0, ""
                if step != "read":
                    if value is None:
                        continue
                    rc = L.dspRuntimeSetOption(k, value)
                    err = L.dspRuntimeLastError().decode("latin-1") if rc else ""
                rows.append([phase, key, step, rc, err, L.dspRuntimeGetOption(k)])

    walk("fresh, no program")
    prog = pb.synth_program(6, 3, 2, 9)
    r1 = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    walk("inherited by a program", legal=False)
    for key, good, _ in OPTION_SCRIPT:           # on the program: every legal value once more, the other way round where there is one
        if good is not None:
            v = {1: 0, 0: 1}.get(good, good + 1)
            rc = L.dspRuntimeSetOption(key.encode(), v)
            rows.append(["set on the program", key, "good", rc, L.dspRuntimeLastError().decode("latin-1") if rc else "", L.dspRuntimeGetOption(key.encode())])
    r2 = rt.Runtime(6, prog.copy(), fs=48000, random=1, dither=24)
    walk("a second program", legal=False)
    L.dspRuntimeSelect(r1.buf.ctypes.data)
    walk("the first program again", legal=False)
    L.dspRuntimeRelease()
    walk("after the release", legal=False)
    del r1, r2
    return rows


def strip_numbers(text):
    return re.sub(r"-?\d+", "#", text)


def record(lib_path=None, verbose=False):
    if lib_path:
        rt.LIB_PATH = os.path.abspath(lib_path)
    L = rt.lib()
    reports, index = [], {}

    def intern(rep):
        key = json.dumps(rep)
        if key not in index:
            index[key] = len(reports)
            reports.append(rep)
        return index[key]

    cases, slow = [], []
    for name, prog in corpus():
        crc = zlib.crc32(prog.tobytes())
        for fmt in FORMATS:
            t0 = time.perf_counter()
            rc, ncores, idx = replay_program(L, prog, fmt, intern)
            slow.append((time.perf_counter() - t0, name, fmt))
            cases.append([name, crc, fmt, rc, ncores, idx])
    for key in LOWERINGS:
        L.dspRuntimeSetOption(key.encode(), 0)
    options = option_script(L)
    if verbose:
        slow.sort(reverse=True)
        print("slowest cases:", [(round(t, 3), n, f) for t, n, f in slow[:5]], "total", round(sum(t for t, _, _ in slow), 1), "s")
    return dict(lowerings=list(LOWERINGS), option_sets=[list(o) for o in OPTION_SETS], shards=[list(s) for s in SHARDS],
                calls=[n for n, _ in REPORTS], reports=reports, cases=cases, options=options)


def summary(doc):
    """what the fixture has to show (tests/test_lowering_report.py asserts it): per format accepted chain cores and refused cores, per
    option a core whose report it changes, and the distinct refusal texts"""
    reports, nsets, nshards = doc["reports"], len(doc["option_sets"]), len(doc["shards"])
    accepted, refused, changed, texts = {}, {}, {k: 0 for k in doc["lowerings"]}, set()
    for name, crc, fmt, rc, ncores, idx in doc["cases"]:
        if rc < 0:
            continue
        at = lambda s, h, c: reports[idx[(s * nshards + h) * ncores + c]]      # noqa: E731
        for c in range(ncores):
            for s in range(nsets):
                core_info = at(s, 0, c)[0]                                         # [rc, chains, sections, taps, text]
                if core_info[0] == 0 and core_info[1] > 0:
                    accepted[fmt] = accepted.get(fmt, 0) + 1
                if core_info[-1]:
                    refused[fmt] = refused.get(fmt, 0) + 1
                    texts.add(strip_numbers(core_info[-1]))
            for k, key in enumerate(doc["lowerings"]):
                changed[key] += at(2 + k, 0, c) != at(0, 0, c) or at(2 + len(doc["lowerings"]) + k, 0, c) != at(1, 0, c)
    return dict(accepted=accepted, refused=refused, changed=changed, texts=sorted(texts))


def dump(doc, path):
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
        g.write(raw)


def load(path=FIXTURE):
    with gzip.open(path, "rb") as f:
        return json.loads(f.read().decode())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="the libavdsp_mi355x.so to record from (default: this tree's)")
    ap.add_argument("--write", action="store_true", help="write tests/golden/lowering_report.json.gz")
    ap.add_argument("--out", help="write the record to this file instead")
    a = ap.parse_args()
    t0 = time.perf_counter()
    doc = record(a.lib, verbose=True)
    s = summary(doc)
    print(f"{len(doc['cases'])} cases, {len(doc['reports'])} distinct reports, {len(doc['options'])} option steps, {time.perf_counter() - t0:.1f} s")
    print("accepted chain cores by format:", s["accepted"], " refused cores by format:", s["refused"])
    print("cores whose report an option alone changes:", s["changed"])
    print(f"{len(s['texts'])} distinct refusal texts (numbers stripped)")
    path = a.out or (FIXTURE if a.write else None)
    if path:
        dump(doc, path)
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

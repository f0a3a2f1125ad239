"""The host's core reports and option calls against a record of what they answered before the lowering was put in stages (DESIGN.md
4.8b): tests/golden/make_lowering_report.py replays its corpus -- golden programs, builder programs of every lowering, seeded mutants;
every DSP_FORMAT; the six lowering options off, on, each alone, each missing; two shards -- through the library of this tree, in a process
of its own (what options read back depends on what the process set before), and every field must equal the fixture's: return codes,
outputs and dspRuntimeLastError() of the ten dspRuntime...Info calls and dspRuntimeStrandInfo per core, and return code, text and
read-back of every step of the option script.  Host-only, no GPU."""
import os
import shutil
import subprocess
import sys

import pytest

from tests.golden import make_lowering_report as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def want():
    return mk.load()


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lowering_report") / "report.json.gz")
    env = {k: v for k, v in os.environ.items() if k not in ("AVDSP_FRAME_SERVER", "AVDSP_FIR_AHEAD")}      # (they change two defaults)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_lowering_report.py"), "--out", out],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return mk.load(out)


def test_the_fixture_shows_what_it_has_to(want):
    s = mk.summary(want)
    for fmt in mk.FORMATS:                                     # accepted chain cores and refused cores in every format
        assert s["accepted"].get(fmt, 0) > 0 and s["refused"].get(fmt, 0) > 0, (fmt, s["accepted"], s["refused"])
    for key in mk.LOWERINGS:                                   # every option changes a recorded core
        assert s["changed"][key] > 0, s["changed"]
    assert os.path.getsize(mk.FIXTURE) < 390_000


def test_same_corpus_and_calls(want, got):
    for key in ("lowerings", "option_sets", "shards", "calls"):
        assert got[key] == want[key], key
    # name, checksum of the program words, format: a difference here is a builder or mutate() that changed, not the library
    assert [c[:3] for c in got["cases"]] == [c[:3] for c in want["cases"]]


def test_every_core_report(want, got):
    calls, nshards = want["calls"], len(want["shards"])
    for w, g in zip(want["cases"], got["cases"]):
        name, _, fmt, rc, ncores, widx = w
        assert g[3:5] == [rc, ncores], f"{name}, DSP_FORMAT {fmt}: dspRuntimeInit / cores {g[3:5]}, recorded {[rc, ncores]}"
        if g[5] == widx and got["reports"] == want["reports"]:
            continue
        for k, (wi, gi) in enumerate(zip(widx, g[5])):
            wr, gr = want["reports"][wi], got["reports"][gi]
            if wr == gr:
                continue
            s, h, c = k // (nshards * ncores), k // ncores % nshards, k % ncores
            bad = [(calls[j], dict(recorded=wr[j], now=gr[j])) for j in range(len(calls)) if wr[j] != gr[j]]
            pytest.fail(f"{name}, DSP_FORMAT {fmt}, options on {want['option_sets'][s]}, shard {want['shards'][h]}, core {c}: {bad}")


def test_reports_and_options_under_the_sanitizers(tmp_path):
    """tests/csrc/report_asan_driver.c, a stand-alone program built with AddressSanitizer and UBSan and linked to the library, over the
    whole corpus: the report helper's frees on the refusal paths, the table's reads and writes of the context.  (The library itself is not
    instrumented: the sanitizer sees its heap traffic; leak detection is off, the HIP runtime it loads keeps what it allocates.)"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe, lib = str(tmp_path / "report_asan_driver"), os.path.join(ROOT, "avdsp_amd", "lib")
    cmd = ["gcc", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-std=gnu99", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "csrc", "report_asan_driver.c"), "-L" + lib, "-lavdsp_mi355x", "-Wl,-rpath," + lib, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    paths = []
    for k, (_, prog) in enumerate(mk.corpus()):
        paths.append(str(tmp_path / f"p{k:04d}.bin"))
        prog.tofile(paths[-1])
    r = subprocess.run([exe] + paths, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-500:] + r.stderr[-3000:]


def test_every_option_step(want, got):
    assert len(got["options"]) == len(want["options"])
    for w, g in zip(want["options"], got["options"]):
        assert g == w, f"[phase, key, step, rc, text, read-back] recorded {w}, now {g}"

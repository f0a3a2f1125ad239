"""The host-side tables of a chain plan (avdsp_amd/csrc/avdsp_plan_layout.h), without a GPU: the checks that keep a kernel from
following a word index out of the mirror, the launch groups and pieces of the cascades, the merged row table with its padding rows,
the tiles of the shared-FIR and mixer stages, and the choice of the FIR kernel of a launch.  tests/csrc/plan_layout_driver.cpp is
built against that header alone with AddressSanitizer and UBSan and run as a program of its own; what it prints is compared with
literal values that follow from the rules avdsp_hip_prog_add_plan and launch_fir have implemented all along.

ring_length: the rule is pow2ceil(taps + 3 * 1024 + 16 * gpc + 16 * 6 + 64); for 4096 taps gpc is 52 and the sum 8160, so the ring
is 8192 floats long, one power of two below the 16384 that DESIGN.md 2 quotes for the north star; 8192 taps give 16384."""
import json
import os
import shutil
import subprocess

import pytest

from tests import cascade_shapes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOAD_PLAIN, LOAD_MUX, RAW = 0, 3, 2          # RAW: kLoadRaw / kStoreRaw, device-side only


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("planlayout") / "plan_layout_driver")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "avdsp_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "csrc", "plan_layout_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available here: " + r.stderr[-300:])
    return exe


def run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stdout


class Desc:
    """A plan description.  Words are handed out in order: a section takes 12 (b0 .. at w, its six state words at w + 6), a FIR
    2 * taps (taps, then the delay line), a LOAD_MUX list 2 * count + 2 (the pairs, then the result word)."""

    def __init__(self, fmt, instances=0):
        self.fmt, self.instances, self.w = fmt, instances, 0
        self.sections, self.chains, self.firgroups, self.muxgroups, self.mirror = [], [], [], [], {}
        self.total_words = None

    def take(self, n):
        w, self.w = self.w, self.w + n + (n & 1)
        return w

    def chain(self, nsec=0, taps=0, bank=None, sat=0, mux=None, **over):
        i = len(self.chains)
        c = dict(in_io=i, load_mode=LOAD_PLAIN, gain_bits=0, nsec=nsec, sec_base=len(self.sections), fir_taps=taps, fir_coef_word=0,
                 fir_state_word=0, sat=sat, n_out=1, out_io=[i, 0, 0, 0], mux_word=0, mux_count=0, mux_result_word=0)
        for _ in range(nsec):
            w = self.take(12)
            self.sections.append([w, w + 6])
        if taps:
            c["fir_coef_word"] = self.take(taps) if bank is None else bank
            c["fir_state_word"] = self.take(taps)
        if mux is not None:                          # the IOs of the list
            c.update(load_mode=LOAD_MUX, mux_word=self.take(2 * len(mux)), mux_count=len(mux), mux_result_word=self.take(2))
            for k, io in enumerate(mux):
                self.mirror[c["mux_word"] + 2 * k] = io
        c.update(over)
        self.chains.append(c)
        return i

    def text(self):
        total = self.total_words if self.total_words is not None else max(self.w, 2)
        t = [self.fmt, total, self.instances, len(self.sections), len(self.chains), len(self.firgroups), len(self.muxgroups), len(self.mirror)]
        for s in self.sections:
            t += s
        for c in self.chains:
            t += [c["in_io"], c["load_mode"], c["gain_bits"], c["nsec"], c["sec_base"], c["fir_taps"], c["fir_coef_word"], c["fir_state_word"],
                  c["sat"], c["n_out"], *c["out_io"], c["mux_word"], c["mux_count"], c["mux_result_word"]]
        for g in self.firgroups + self.muxgroups:
            t += [len(g), *g]
        for w, v in self.mirror.items():
            t += [w, v]
        dressed = [(i, c["finish"]) for i, c in enumerate(self.chains) if c.get("finish")]
        if dressed:                                   # (chain(finish=...), with sat=1: a dressed finish)
            t += [len(dressed)] + [v for p in dressed for v in p]
        return " ".join(map(str, t))


def layout(driver, tmp_path, desc):
    path = str(tmp_path / "plan.txt")
    with open(path, "w") as f:
        f.write(desc.text())
    return json.loads(run(driver, "layout", path))


# ---------------------------------------------------------------- cascade groups
def test_groups_by_section_count_and_the_merged_table(driver, tmp_path):
    d = Desc(6)
    for _ in range(3): d.chain(nsec=2)
    for _ in range(2): d.chain(nsec=5)
    L = layout(driver, tmp_path, d)
    assert [(g["nsec"], g["n"], g["P"], g["ids"], g["pieces"]) for g in L["groups"]] == [(2, 3, 16, [0, 1, 2], []), (5, 2, 16, [3, 4], [])]
    m = L["merged"]
    assert m["n"] == 16 and len(m["rows"]) == 16 and len(m["lanes"]) == 256
    assert [r[0] for r in m["rows"]] == [0, 1, 2, -1, 3, 4, -1, -1] + [-1] * 8              # 3 real + 1 empty, 2 real + 2 empty, 8 empty
    assert [r[1] for r in m["rows"]] == [0, 1, 2, 0, 3, 4, 3, 3] + [3] * 8                  # an empty row reads a real row's IO
    assert [r[5] for r in m["rows"]] == [2] * 4 + [5] * 12                                  # each wave of four rows has one section count
    assert m["rows"][1] == [1, 1, 1, 1 << 16, 0, 2]                                         # plain load, no SAT0DB, no ring, one store
    # chain 0: sections at words 0 and 12 (states 6 and 18) in lanes 14 and 15 of its row
    assert m["lanes"][:16] == [[-1, -1]] * 14 + [[0, 6], [12, 18]]
    assert m["lanes"][3 * 16:4 * 16] == [[-1, -1]] * 16                                     # an empty row holds no section
    assert m["lanes"][4 * 16:5 * 16] == [[-1, -1]] * 11 + [[72 + 12 * q, 78 + 12 * q] for q in range(5)]
    assert L["groups"][0]["rows"] == m["rows"][:3] and L["groups"][0]["lanes"] == m["lanes"][:48]
    assert L["fir"] == [] and L["pass"] == [] and L["io"] == [0, 4, 0, 4]
    assert L["stores_whole_window"] == 1 and L["overlap_ok"] == 0


def test_one_section_count_makes_no_merged_table(driver, tmp_path):
    d = Desc(6)
    for _ in range(5): d.chain(nsec=3)
    L = layout(driver, tmp_path, d)
    assert len(L["groups"]) == 1 and len(L["groups"][0]["rows"]) == 5
    assert L["merged"]["n"] == 0 and L["merged"]["rows"] == [] and L["merged"]["lanes"] == []


@pytest.mark.parametrize("n, P, nrows", [(4096, 16, 4096), (4097, 8, 0)])
def test_sixteen_lane_rows_while_the_chip_has_simds_to_spare(driver, tmp_path, n, P, nrows):
    d = Desc(6)
    for _ in range(n): d.chain(nsec=8)
    g, = layout(driver, tmp_path, d)["groups"]
    assert (g["P"], g["n"], len(g["rows"]), len(g["lanes"])) == (P, n, nrows, 16 * nrows)


def uniform(n, nsec, fmt=6, **over):
    d = Desc(fmt)
    for _ in range(n): d.chain(nsec=nsec, **over)
    return d


def narrow_shapes():
    seen = []
    for shape in cs.NARROW + cs.NARROW_REPLAY + [s for s in cs.MIXED if s[2] < 16]:
        if shape not in seen: seen.append(shape)
    return seen


@pytest.mark.parametrize("nsec, n, P", narrow_shapes())
def test_the_narrow_groups_of_the_gpu_cascade_tests(driver, tmp_path, nsec, n, P):
    """tests/test_gpu_cascade_forms.py means to launch biquad_pipe<FMT, 1 | 2 | 4 | 8>; the device does not say which cascade kernel
    ran.  So the rule is held here to the shapes that file imports (tests/cascade_shapes.py): exactly these P, and no biquad_row
    records.  A failure here says that the GPU tests no longer reach the narrow forms -- move their chain counts with the rule."""
    assert P < 16 and n * 16 > 65536
    g, = layout(driver, tmp_path, uniform(n, nsec))["groups"]
    assert (g["nsec"], g["n"], g["P"], g["wide"], g["rows"], g["lanes"], g["pieces"]) == (nsec, n, P, 0, [], [], []), \
        "the GPU tests of biquad_pipe's narrow forms no longer reach them"


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_mixed_core_of_the_gpu_cascade_tests(driver, tmp_path, fmt):
    """Two narrow groups beside chains of three other section counts: the latter are 16-lane rows with records and make the merged
    table, which holds no row of the narrow groups (their launches go out beside the merged one)."""
    d = Desc(fmt)
    for nsec, n, _ in cs.MIXED:
        for _ in range(n): d.chain(nsec=nsec)
    L = layout(driver, tmp_path, d)
    assert [(g["nsec"], g["n"], g["P"]) for g in L["groups"]] == cs.MIXED
    for g in L["groups"]:
        assert len(g["rows"]) == (g["n"] if g["P"] == 16 else 0) and len(g["lanes"]) == 16 * len(g["rows"])
    narrow_ids = {i for g in L["groups"] if g["P"] < 16 for i in g["ids"]}
    merged_ids = [r[0] for r in L["merged"]["rows"] if r[0] >= 0]
    assert sorted(merged_ids) == sorted(i for g in L["groups"] if g["P"] == 16 for i in g["ids"]) and not narrow_ids & set(merged_ids)


def test_the_row_groups_of_the_gpu_cascade_tests(driver, tmp_path):
    d = Desc(6)
    for nsec, n, _ in cs.ROWS:
        for _ in range(n): d.chain(nsec=nsec)
    L = layout(driver, tmp_path, d)
    assert [(g["nsec"], g["n"], g["P"]) for g in L["groups"]] == cs.ROWS
    assert all(len(g["rows"]) == g["n"] for g in L["groups"]) and L["merged"]["n"] == 64       # 16 runs, each filled up to a wave


def test_dressed_short_chains_keep_sixteen_lanes_however_many(driver, tmp_path):
    """The WIDE form of biquad_pipe exists for 16-lane rows only: a dressed group past the threshold is not narrowed."""
    g, = layout(driver, tmp_path, uniform(cs.NARROW_CHAINS, 3, sat=1, finish=1))["groups"]
    assert (g["P"], g["wide"], g["n"], g["rows"]) == (16, 1, cs.NARROW_CHAINS, [])
    g, = layout(driver, tmp_path, uniform(cs.NARROW_CHAINS, 3, sat=1))["groups"]                 # (the same chains without the finish)
    assert (g["P"], g["wide"]) == (4, 0)


def test_a_shard_of_the_full_chip_runs_sixteen_lane_rows(driver, tmp_path):
    """set_shard(rank, 8) of 16 384 chains plans 2048 of them: the cfg5 headline tests run biquad_row, not the narrow forms."""
    g, = layout(driver, tmp_path, uniform(16384 // 8, 8))["groups"]
    assert (g["P"], g["n"], len(g["rows"])) == (16, 2048, 2048)


# ---------------------------------------------------------------- pieces
def test_piece_lengths(driver, tmp_path):
    want = {17: [9, 8], 65: [13] * 5, 100: [15, 15, 14, 14, 14, 14, 14], 129: [15] * 3 + [14] * 6, 200: [16] * 5 + [15] * 8}
    d = Desc(6)
    for nsec in want: d.chain(nsec=nsec)
    L = layout(driver, tmp_path, d)
    assert {g["nsec"]: [p["nsec"] for p in g["pieces"]] for g in L["groups"]} == want
    assert all(p["P"] == 16 and len(p["rows"]) == 1 for g in L["groups"] for p in g["pieces"])
    assert all(g["rows"] == [] for g in L["groups"]) and L["merged"]["n"] == 0
    assert len(L["dev_chains"]) == 5 + sum(len(v) - 1 for v in want.values())


@pytest.mark.parametrize("fmt", [6, 2])
def test_piece_records(driver, tmp_path, fmt):
    d = Desc(fmt)
    taps = 30 if fmt == 6 else 0                        # (a FIR has no int64 definition)
    d.chain(nsec=3)                                     # another group in front: the pieces' columns are places in THEIR group
    a = d.chain(nsec=40, taps=taps, sat=1)
    b = d.chain(nsec=40, taps=taps)
    L = layout(driver, tmp_path, d)
    g = L["groups"][1]
    assert [p["nsec"] for p in g["pieces"]] == [14, 13, 13] and g["ids"] == [a, b]
    ch = L["dev_chains"]
    assert len(ch) == 3 + 2 * 2
    for k, p in enumerate(g["pieces"]):
        last = k == 2
        assert p["ids"] == ([a, b] if last else [3 + 2 * k, 4 + 2 * k])           # new records behind the host's; the last piece is the chain's own
        assert p["raw_out"] == (not last) and p["all_fir"] == (last and fmt == 6)
        for j, cid in enumerate(p["ids"]):
            c, host = ch[cid], d.chains[(a, b)[j]]
            assert c["nsec"] == p["nsec"] and c["sec_base"] == host["sec_base"] + [0, 14, 27][k]
            assert (c["in_io"], c["load_mode"]) == ((host["in_io"], LOAD_PLAIN) if k == 0 else (j, RAW))
            if last:
                assert (c["fir_taps"], c["sat"], c["n_out"], c["out_io"]) == (taps, host["sat"], 1, host["out_io"][0])
            else:
                assert (c["fir_taps"], c["sat"], c["n_out"], c["out_io"]) == (0, RAW, 1, j)
            # flags: load mode | bit 8 SAT0DB (a raw store only in format 2) | bit 9 ring | bit 10 raw | n_out << 16
            flags = (0 if k == 0 else RAW) | (1 << 16)
            if last:
                flags |= (host["sat"] << 8) | ((1 << 9) if taps else 0)
            else:
                flags |= (1 << 10) | ((1 << 8) if fmt == 2 else 0)
            assert p["rows"][j] == [cid, c["in_io"], c["out_io"], flags, 0, p["nsec"]]
            w0 = d.sections[c["sec_base"]][0]
            assert p["lanes"][16 * j:16 * j + 16] == [[-1, -1]] * (16 - p["nsec"]) + [[w0 + 12 * q, w0 + 12 * q + 6] for q in range(p["nsec"])]
    assert L["overlap_ok"] == 0                         # (chain 0's cascade stores to the output block)


# ---------------------------------------------------------------- shared FIR, mixer stage
def test_shared_fir_tiles(driver, tmp_path):
    d = Desc(6)
    bank = d.take(100)
    for i in range(40): d.chain(nsec=1 - i % 2, taps=100, bank=bank)
    for i in range(3): d.chain(nsec=1, taps=60 + i)
    d.firgroups.append(list(range(40)))
    L = layout(driver, tmp_path, d)
    S = L["shared"]
    assert S["tiles"] == [[0, 0, 16, 100], [0, 16, 16, 100], [0, 32, 8, 100]]
    assert S["ids"] == list(range(40)) and S["rest"] == [40, 41, 42] and S["reps"] == [0]
    assert S["feed"] == list(range(1, 40, 2))           # the grouped chains without sections
    assert L["fir"] == list(range(43)) and L["max_taps"] == 100 and L["overlap_ok"] == 1        # every cascade feeds a FIR


def test_mux_tiles(driver, tmp_path):
    d = Desc(6)
    for i in range(70): d.chain(nsec=0 if i == 5 else 1, mux=[7, 3, 9, 3, 11])
    d.chain(nsec=1, in_io=20)                           # a LOAD chain beside them: its sample word is copied into its column
    d.muxgroups.append(list(range(70)))
    L = layout(driver, tmp_path, d)
    M = L["mux"]
    lw0 = d.chains[0]["mux_word"]
    assert M["tiles"] == [[0, 64, 5, 8, lw0, 0], [64, 6, 5, 8, lw0, 512]]
    assert M["kpads"] == [8] * 70 and M["rows"] == list(range(0, 560, 8)) and M["g64_len"] == 560
    assert M["tile_ids"] == list(range(70)) and M["plain"] == [70]
    assert [r[3] for r in M["recs"]] == [-1 if i == 5 else i for i in range(71)]           # column -1: the stage stores the chain itself
    assert M["recs"][0] == [lw0, 5, d.chains[0]["mux_result_word"], 0] and M["recs"][70] == [20, 0, 0, 70]
    assert L["has_mux"] == 1 and L["n_mux_stored"] == 1 and L["pass"] == []
    assert L["io"][:2] == [3, 20]                       # the IOs the lists and the LOAD chain name
    assert all((c["in_io"], c["load_mode"]) == (i, RAW if i < 70 else LOAD_PLAIN) for i, c in enumerate(L["dev_chains"]))
    assert L["overlap_ok"] == 0


def test_ring_length(driver):
    assert run(driver, "ring", 4096).split() == ["8192", "52", "4544"]         # ring floats, fir_gpc, pitch64 (see the module's docstring)
    assert run(driver, "ring", 8192).split()[0] == "16384"
    assert run(driver, "ring", 300).split() == ["4096", "20", "748"]
    assert run(driver, "ring", 416).split()[:2] == ["4096", "28"]              # 416 + 3072 + 16 * 28 + 96 + 64 = 4096: the fullest ring of 4096
    assert run(driver, "ring", 417).split()[:2] == ["8192", "28"]


# ---------------------------------------------------------------- refusals
def plain(fmt=6, instances=0):
    d = Desc(fmt, instances)
    d.chain(nsec=2, taps=0 if fmt == 2 else 20)
    d.total_words = d.w
    return d


def grouped(n=20):
    d = Desc(6)
    bank = d.take(50)
    for _ in range(n): d.chain(taps=50, bank=bank)
    return d


def mixers(fmt=6, instances=0):
    d = Desc(fmt, instances)
    for _ in range(16): d.chain(nsec=1, mux=[1, 2, 3])
    return d


def refusal_cases():
    def case(name, d, message):
        return pytest.param(d, message, id=name)
    d = plain(); d.sections[0][0] = d.total_words - 4
    yield case("coef_word_outside", d, "section 0 addresses words outside the loaded buffer")
    d = plain(); d.sections[1][1] = d.total_words - 4
    yield case("state_word_outside", d, "section 1 addresses words outside the loaded buffer")
    d = plain(); d.sections[0][0] = -1
    yield case("coef_word_negative", d, "section 0 addresses words outside the loaded buffer")
    d = plain(); d.sections[1][1] = 7
    yield case("odd_state_word", d, "section 1 addresses words outside the loaded buffer")
    d = plain(); d.chains[0]["nsec"] = 3
    yield case("section_range", d, "chain 0: bad section range")
    d = plain(); d.chains[0]["sec_base"] = -1
    yield case("section_base_negative", d, "chain 0: bad section range")
    for n_out in (0, 5):
        d = plain(); d.chains[0]["n_out"] = n_out
        yield case(f"n_out_{n_out}", d, "chain 0: bad IO")
    d = plain(); d.chains[0]["in_io"] = -1
    yield case("negative_input_io", d, "chain 0: bad IO")
    d = plain(); d.chains[0].update(n_out=2, out_io=[0, -3, 0, 0])
    yield case("negative_output_io", d, "chain 0: bad IO")
    d = plain(2); d.chains[0].update(fir_taps=4, fir_coef_word=0, fir_state_word=0)
    yield case("fir_in_format_2", d, "chain 0: FIR has no int64 definition")
    d = plain(); d.chains[0]["fir_coef_word"] = d.total_words - 19
    yield case("fir_taps_outside", d, "chain 0: FIR addresses words outside the loaded buffer")
    d = plain(); d.chains[0]["fir_state_word"] = -1
    yield case("fir_state_negative", d, "chain 0: FIR addresses words outside the loaded buffer")
    d = plain(); d.chains[0]["load_mode"] = RAW
    yield case("load_mode_2_from_the_host", d, "chain 0: load mode 2")
    yield case("mux_in_format_3", mixers(3), "LOAD_MUX chains have no kernels in format 3")
    yield case("mux_with_instances", mixers(6, 2), "LOAD_MUX chains have no chain instances")
    d = mixers(); d.chains[3]["mux_word"] = d.w - 4
    yield case("mux_list_outside", d, "chain 3: LOAD_MUX list or result word outside the loaded buffer")
    d = mixers(); d.mirror[d.chains[2]["mux_word"] + 2] = -1
    yield case("mux_entry_negative_io", d, "chain 2: LOAD_MUX entry 1 names IO -1")
    d = grouped(); d.firgroups.append(list(range(15)))
    yield case("fir_group_of_15", d, "FIR group 0: 15 chains")
    d = grouped(); d.chains[7]["fir_taps"] = 49; d.firgroups.append(list(range(20)))
    yield case("fir_group_other_tap_count", d, "FIR group 0: chain 7 is not one of its bank")
    d = grouped(); d.chains[9]["fir_coef_word"] = 2; d.firgroups.append(list(range(20)))
    yield case("fir_group_other_bank", d, "FIR group 0: chain 9 is not one of its bank")
    d = grouped(40); d.firgroups += [list(range(20)), list(range(19, 40))]
    yield case("chain_in_two_fir_groups", d, "FIR group 1: chain 19 is not one of its bank")
    d = mixers(); d.chain(nsec=1, mux=[1, 2, 3, 4]); d.muxgroups.append(list(range(17)))
    yield case("mix_group_other_list_length", d, "mix group 0: chain 16 is not one of its lists")
    d = mixers(); d.muxgroups.append(list(range(15)))
    yield case("mix_group_of_15", d, "mix group 0: 15 chains")
    d = plain(instances=3); d.sections[0][0] = 3 * ((d.total_words + 1) & ~1) - 4
    yield case("word_past_the_last_copy", d, "section 0 addresses words outside the loaded buffer")


@pytest.mark.parametrize("desc, message", list(refusal_cases()))
def test_refusals(driver, tmp_path, desc, message):
    assert layout(driver, tmp_path, desc) == {"error": message}


def test_unharmed_plans_are_accepted(driver, tmp_path):
    for d in (plain(), plain(2), grouped(), mixers()):
        assert "error" not in layout(driver, tmp_path, d)
    d = grouped(); d.firgroups.append(list(range(20)))
    assert layout(driver, tmp_path, d)["shared"]["tiles"] == [[0, 0, 16, 50], [0, 16, 4, 50]]


def test_instances_reach_every_copy_of_the_mirror(driver, tmp_path):
    d = plain(instances=3)
    stride = (d.total_words + 1) & ~1
    d.sections[0] = [2 * stride + 4, 2 * stride + 10]             # inside copy 2
    d.chains[0].update(fir_coef_word=3 * stride - 20, fir_state_word=2 * stride)
    assert "error" not in layout(driver, tmp_path, d)
    d.instances = 0                                               # ... which an ordinary plan does not have
    assert layout(driver, tmp_path, d) == {"error": "section 0 addresses words outside the loaded buffer"}


# ---------------------------------------------------------------- the FIR kernel of a launch
TILE = 1


def choice(driver, impl, n, frames=1024, fir_rows=0, fir_split=0, fir_lean=-1, cascades=1, plan_taps=None):
    fam, R, big, split, lean = map(int, run(driver, "choice", impl, n, frames, fir_rows, fir_split, fir_lean, cascades,
                                            n * 2048 if plan_taps is None else plan_taps).split())
    assert fam == impl
    return R, big, split, lean


def test_fir_tile_rows_by_cost(driver):
    got = [choice(driver, TILE, n)[0] for n in (512, 1024, 2048, 4096, 16384, 3000)]
    assert got == [1, 2, 4, 4, 4, 2]
    assert choice(driver, TILE, 4096, frames=256)[:3] == (1, 0, 0)          # 128 R >= frames: no tile of twice the block
    assert choice(driver, TILE, 4096, frames=257)[0] == 2
    assert choice(driver, TILE, 4096, frames=512, fir_rows=4)[0] == 2        # ... whoever chose the R


def test_fir_tile_long_chunks_and_tap_split(driver):
    assert choice(driver, TILE, 256)[:3] == (1, 1, 0)                        # at most a wave per SIMD: BIG
    assert choice(driver, TILE, 256, fir_split=1)[:3] == (1, 0, 1)
    assert choice(driver, TILE, 256, fir_rows=1)[:3] == (1, 0, 0)
    assert choice(driver, TILE, 257)[:3] == (1, 0, 0)                        # 1028 waves
    assert choice(driver, TILE, 1024, frames=256)[:3] == (1, 1, 0)
    assert choice(driver, TILE, 2048, fir_split=1)[:3] == (4, 0, 0)


def test_fir_tile_lean_boundary(driver):
    assert choice(driver, TILE, 256, cascades=0, plan_taps=256 * 4096)[3] == 1
    assert choice(driver, TILE, 4096, plan_taps=4096 * 4096)[3] == 1          # 16.8 M >= 12 M
    assert choice(driver, TILE, 2048, plan_taps=2048 * 4096)[3] == 0
    assert choice(driver, TILE, 4096, plan_taps=4096 * 4096, fir_lean=0)[3] == 0
    assert choice(driver, TILE, 2048, plan_taps=2048 * 4096, fir_lean=1)[3] == 1


def test_other_fir_kernels(driver):
    assert [choice(driver, 4, n)[:2] for n in (256, 1023, 1024, 2048)] == [(1, 1), (1, 0), (2, 0), (4, 0)]          # fir_flow
    assert choice(driver, 4, 256, fir_rows=1)[:2] == (1, 0) and choice(driver, 4, 4096, frames=256)[:2] == (1, 0)
    assert [choice(driver, 3, n)[0] for n in (256, 511, 512, 1024)] == [1, 1, 2, 4]                                 # fir_stream
    assert [choice(driver, 2, n)[0] for n in (512, 513)] == [2, 1]                                                  # fir_mfma's NG
    assert choice(driver, 0, 100) == (1, 0, 0, 0)


def test_fir_shared_rows(driver):
    def shared(fmt, ntiles, frames, rows=0):
        fam, R, *flags = map(int, run(driver, "shared", fmt, ntiles, frames, rows).split())
        assert fam == 5 and flags == [0, 0, 0]
        return R
    assert shared(6, 1000, 1024) == 4 and shared(4, 1000, 1024) == 2         # format 4 stops at two row tiles
    assert shared(4, 1000, 1024, rows=4) == 2 and shared(6, 1000, 1024, rows=4) == 4
    assert shared(6, 3, 1024) == 1                                           # 48 waves: one round whatever the R
    assert [shared(6, 1000, f, rows=4) for f in (129, 128, 65, 64, 33)] == [4, 2, 2, 1, 1]      # halved while 32 R >= frames
    assert [shared(6, 1000, f) for f in (129, 128, 64)] == [1, 2, 1]                            # (129 frames: 2 x 4 / 0.90 against 6 x 1 / 0.79 rounds)

"""tests/state_scripts.py without a GPU: every script played oracle against oracle, so that the player's steps mean what they say
before a device sees them; the modelled ring positions every script is written for; and the lowering of every program by the
host-only calls -- a program that fell to the interpreter would test nothing of the rings.

What "mean what they say" is: a script that only saves, syncs, switches options, replans or shards must leave the oracle's outputs
those of ONE uninterrupted block over the same input.  "load", "poke", "params" with an edit and "reset" break the stream; they are
held to their own definition: a fresh oracle that is given the state such a step left (and the edited words, and the rate)
reproduces everything up to the next such step from it, outputs and end state."""
import numpy as np
import pytest

from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import state_scripts as ss


@pytest.fixture(autouse=True)
def _release():
    yield
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def kinds(script):
    return [s[0] for s in script]


@pytest.mark.parametrize("case_id", sorted(ss.CASES))
def test_scripts_mean_what_they_say(case_id):
    prog, script, x = ss.case(case_id)
    trace = ss.play(script, prog.fmt, prog, x, device=False)
    breaking = [i for i, s in enumerate(script) if s[0] in ("load", "poke", "reset") or (s[0] == "params" and s[1])]
    assert [s.step for s in trace.segments] == [-1] + breaking
    if not breaking:
        o = po.OracleProgram(prog.fmt, prog.words, fs=prog.fs)
        want = o.run_block(x, prog.C, prog.C)
        assert (ss.words(trace.out) == ss.words(want)).all(), "an unbroken oracle run gives other outputs"
        assert (o.state == trace.segments[0].end_state).all()
    ss.replay_segments(trace, prog.fmt, prog, x)
    for i in breaking:
        seg = [s for s in trace.segments if s.step == i][0]
        before = trace.segments[trace.segments.index(seg) - 1].end_state
        if script[i][0] == "load":
            assert (seg.state == trace.saves[script[i][1]][1]).all()
        elif script[i][0] == "poke":
            (chain, pokes), = script[i][1].items()
            at = np.array([prog.fir_state[chain] + k for k, _ in pokes])
            assert (seg.state[at] == np.array([w for _, w in pokes], dtype=np.uint32)).all()
            rest = np.ones(len(before), dtype=bool)
            rest[at] = False
            assert (seg.state[rest] == before[rest]).all()
        elif script[i][0] == "reset":
            assert not seg.state.any(), "a reset leaves the zeroed data area"
            assert before.any()
        else:
            assert (seg.state == before).all(), "a parameter edit leaves the state alone"
    assert len(trace.forks) == kinds(script).count("fork")
    assert all(0 < n <= ss.FORK_FRAMES for _, _, n in trace.forks)


@pytest.mark.parametrize("case_id", sorted(ss.CASES))
def test_scripts_reach_the_ring_positions_they_name(case_id):
    name, fmt, make, args = ss.CASES[case_id]
    prog, script, x = ss.case(case_id)
    R = {"TIGHT": 4096, "MIXED": 4096, "LONG": 8192, "BANK": 4096, "LANE": 4096, "FIXED": 0, "RATES": 4096, "DEEP": 8192}[name]
    assert prog.R == R
    m = ss.model(script, R)                                   # asserts every ("at", p) and ("total", n) of the script
    assert m[-1][1] == len(x) <= (18000 if name in ("LONG", "DEEP") else 10000)
    at = lambda kind: [m[i] for i, s in enumerate(script) if s[0] == kind]
    T = prog.max_taps
    if case_id[0] == "A":
        saves = at("save")
        assert [t for _, t in saves] == [0, 1, 1025, R - 1, R, R + 1, R + T - 1, 2 * R + 1300]
        assert [p for p, _ in saves] == [0, 1, 1025, R - 1, 0, 1, T - 1, 1300]
        big = [m[i] for i, s in enumerate(script) if s == ("block", 2500)]
        assert big == [(R - 1200, 2 * R - 1200)]               # three launches: 1024 + 1024 + 452, the second crosses the ring's end
        assert kinds(script).count("fork") == len(saves) == 8
    if case_id[0] == "B":
        assert [p for p, _ in at("load")] == [4000, 200] and R > 4000
        assert at("load")[1][1] == 2 * R + 200                 # ... the second after two wraps
        assert [p for p, _ in at("poke")] == ([5124 % R, 5724 % R] if fmt == 6 else [])      # (1028 and 1628 where R is 4096)
        for i, s in enumerate(script):
            if s[0] == "poke":
                (chain, pokes), = s[1].items()
                Tc = prog.chains[chain][1]
                assert [k for k, _ in pokes] == [0, 1, Tc // 2, Tc - 2, Tc - 1] and Tc >= 300
                assert tuple(w for _, w in pokes) == (0x7F800000, 0xFFC00001, 0x7F812345, 0x00000012, 0x80000400)
        # the second poke lies between two fir_impl 4 blocks
        if fmt == 6:
            i = [j for j, s in enumerate(script) if s[0] == "poke"][1]
            assert script[i - 2:i] == [("opt", "fir_impl", 4), ("block", 300)] and script[i + 1] == ("block", 300)
    if case_id[0] == "C":
        blocks = [(i, s[1]) for i, s in enumerate(script) if s[0] == "block"][-10:]
        assert [n for _, n in blocks] == [1024, 300, 1, 1024, 257, 1024, 700, 1024, 37, 513]
        impl, first_wide = 1, None
        walk = []
        for i, s in enumerate(script):
            if s[:2] == ("opt", "fir_impl"):
                impl = s[2]
            if s[0] == "block":
                walk.append(impl)
                if impl in (3, 4) and first_wide is None:
                    first_wide = (m[i][0], s[1])
        assert walk[-10:] == [1, 4, 1, 3, 0, 2, 1, 3, 4, 1] and set(walk[:-10]) <= {1}
        p, n = first_wide
        assert (p < R < p + n) if "wrapped" in case_id else (0 < p and p + n < R)
        i = kinds(script).index("load")
        assert [s for s in script[:i] if s[:2] == ("opt", "fir_impl")][-1][2] == 3          # set for the block behind the load
        assert [s for s in script[:i] if s[:2] == ("opt", "fir_impl")][-2][2] == 1          # ... the block in front ran with 1
        syncs = [i for i, s in enumerate(script) if s[0] == "sync"]
        assert len(syncs) == 5
    if case_id[0] == "N":
        blocks = [(i, s[1]) for i, s in enumerate(script) if s[0] == "block"][-11:]
        assert [n for _, n in blocks] == [1024, 700, 513, 1024, 600, 1024, 700, 513, 1024, 600, 1024]
        opt, walk, first_other = dict(fir_impl=1, fir_rows=0, fir_lean=-1), [], None
        for i, s in enumerate(script):
            if s[0] == "opt" and s[1] in opt:
                opt[s[1]] = s[2]
            if s[0] == "block":
                walk.append((opt["fir_impl"], opt["fir_rows"], opt["fir_lean"]))
                if walk[-1] != (1, 4, 1) and first_other is None:
                    first_other = (m[i][0], s[1])
        ring = (1, 4, 1)
        assert walk[-11:] == [ring, (2, 0, -1), ring, (3, 4, 0), ring, (4, 0, 0), ring, (1, 2, 1), ring, (0, 0, -1), ring] and set(walk[:-11]) <= {ring}
        assert all(n > 512 for (_, n), w in zip(blocks, walk[-11:]) if w == ring)
        p, n = first_other
        assert (p < R < p + n) if "wrapped" in case_id else (0 < p and p + n < R)
        i = kinds(script).index("save")
        assert kinds(script[:i]).count("block") == len(walk) - 10                # behind the table's first block
        i = kinds(script).index("load")
        before = [j for j in range(i) if script[j][0] == "block"][-1]
        assert walk[kinds(script[:before]).count("block")] == (3, 4, 0)           # the block in front of the load: fir_stream
        assert [s for s in script[:i] if s[:2] == ("opt", "fir_impl")][-1][2] == 1 and [s for s in script[:i] if s[:2] == ("opt", "fir_lean")][-1][2] == 1
        assert kinds(script).count("sync") == 6
    if name == "DEEP" and case_id[0] in "ABDE":
        assert script[:2] == [("opt", "fir_rows", 4), ("opt", "fir_lean", 1)] and T == 4097
    if case_id.startswith("E-DEEP"):
        assert script[-2:] == [("block", 1024), ("sync",)]
    if case_id.startswith("D-MIXED") or case_id.startswith("D-DEEP"):
        assert [p for p, _ in at("params")] == [1300, 1324] and [p for p, _ in at("generic")] == [1324, 0]
        assert [s[2] for s in script if s[0] == "shards"] == [300, 1, 1024, 257]
        assert at("shards")[0][0] == 1324
    if case_id.startswith("D-RATES"):
        assert [p for p, _ in at("reset")] == [1300, 1324] and [s[1] for s in script if s[0] == "reset"] == [48000, 44100]
    if case_id[0] == "E":
        assert [p for p, _ in at("frames")] == [R - 2, 100] and at("frames")[1][1] == R + 100
    if case_id[0] == "F":
        assert m[-1][0] == sum(ss.F_BLOCKS[1:]) - R > 0          # the ring has wrapped behind the plans the shard step left
        assert [s[2] for s in script if s[0] == "expect"] == [17, 0, 17, 0, 17, 0, 17, 0]


@pytest.mark.parametrize("name,fmt", [(n, f) for n, (fmts, _) in ss.PROGRAMS.items() for f in fmts])
def test_programs_run_on_the_chain_kernels(name, fmt):
    prog = ss.program(name, fmt)
    assert prog.C <= 20
    r = rt.Runtime(fmt, prog.words, fs=prog.fs)
    assert r.rc >= 0 and len(r.cores) == 1
    assert r.core_info() == dict(chains=prog.C, max_sections=max(s for s, _ in prog.chains), max_taps=prog.max_taps)
    g = r.fir_group_info()
    if name == "BANK":
        assert g == dict(groups=1, grouped_chains=17, largest_group=17) and prog.banked == list(range(17))
    else:
        assert g["groups"] == 0
    assert r.shard_info() == dict(total_chains=prog.C, first_chain=0, nchains=prog.C, in_io_min=prog.C, in_io_max=2 * prog.C - 1,
                                  out_io_min=0, out_io_max=prog.C - 1)
    worlds = {s[1] for cid, c in ss.CASES.items() if c[:2] == (name, fmt) for s in ss.case(cid)[1] if s[0] == "shards"}
    assert worlds == {"MIXED": {3}, "BANK": {2}, "LANE": {3}, "FIXED": {2}, "DEEP": {3}}.get(name, set())
    for world in sorted(worlds):                               # what the "shards" steps of this program's scripts assume
        for rank in range(world):
            r.set_shard(rank, world)
            lo, n = ss.shard_range(prog.C, world, rank)
            assert n >= 1
            assert r.shard_info() == dict(total_chains=prog.C, first_chain=lo, nchains=n, in_io_min=prog.C + lo,
                                          in_io_max=prog.C + lo + n - 1, out_io_min=lo, out_io_max=lo + n - 1)
            assert r.core_info()["chains"] == prog.C        # (the core's chains, whatever the shard)
    r.set_shard(0, 1)
    if name == "BANK":                                         # 10 chains a shard: below the shared path's 16
        r.set_shard(0, 2)
        assert r.fir_group_info()["groups"] == 0
        r.set_shard(0, 1)


def test_ring_length_restated():
    assert ss.ring_length(416) == 4096 and ss.ring_length(417) == 8192
    assert ss.ring_length(300) == 4096 and ss.ring_length(4096) == 8192 and ss.ring_length(8192) == 16384
    assert ss.ring_length(1030) == 8192 and ss.ring_length(97) == 4096
    assert ss.ring_length(4097) == 8192 and ss.program("DEEP", 6).R == 8192 and ss.program("DEEP", 4).max_taps == 4097

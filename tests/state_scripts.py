"""Programs, scripts and one player for the hand-overs of FIR histories and filter state between calls ("hand-overs"):
tests/test_state_scripts.py plays every script oracle against oracle (no GPU), tests/test_gpu_state_handover.py plays them on the
device against the oracle, bit for bit.  Importing this module needs no GPU.

A program is one core of chains  LOAD_GAIN(IO C + c, gain_c) -> [BIQUADS] -> [FIR] -> SAT0DB -> STORE(IO c)  from a list of
(sections, taps) per chain -- (sections, taps, "bank"): the chain's FIR names the program's one shared impulse bank.

A script is a list of steps; play() applies every step to a po.OracleProgram and, if `device`, to an rt.Runtime:

    ("block", n)                 the next n frames of the input as one block
    ("frames", k)                the next k frames as k one-frame calls (dspRuntime_N: samples[] indexed by IO number)
    ("sync",)                    sync_state(), the whole state area against the oracle's
    ("save", name)               a sync, then a copy of the state kept under that name
    ("load", name)               that copy into both states, then upload_state()
    ("poke", {chain: [(i, w)]})  a sync, then word w at index i of the chain's FIR delay line in both states, then upload_state()
    ("opt", key, value)          dspRuntimeSetOption (device only: the oracle has one way to compute)
    ("expect", key, value)       dspRuntimeGetOption must say so (device only)
    ("params", edit_or_None)     {word: value} written into both program copies, then upload_params()
    ("generic", 0 | 1)           the core on the interpreter / back on the chain kernels
    ("shards", world, n)         a block of n frames as `world` calls, each behind set_shard(rank, world) over that shard's
                                 columns, then set_shard(0, 1); the assembled block is compared with the oracle's whole block
    ("reset", fs)                dspRuntimeReset on both
    ("fork", name)               a second oracle and a second Runtime, both fresh and given the state saved under `name`, replay
                                 up to FORK_FRAMES of the frames that followed the save: the second oracle must repeat what the
                                 first one made of them, the second Runtime what the second oracle makes, outputs and state
    ("at", p) / ("total", n)     claims that model() checks -- the modelled ring position / the frames consumed so far; the
                                 player skips them

The modelled ring position: frames of chain-kernel blocks since the plans were last built, modulo the ring length R, which is
ring_length(longest FIR) as avdsp_plan_layout.h computes it.  The plans are built anew by the first block and after "params",
"generic", "shards" and "reset".  The device's own position cannot be read; the model only says whether a script reaches the
positions it is written for and never decides what the device is compared with.

Program DEEP and its cases (scripts A, B, D, E behind RING_PREFIX, and script N) put fir_tile's window ring on both
sides of every hand-over; tests/fir_ring_cases.py lists their launches and tests/test_fir_ring_reach.py asks fir_choice about each."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po

FORK_FRAMES = 1200


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# programs
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Program:
    name: str
    fmt: int
    words: np.ndarray
    chains: list                 # (sections, taps) per chain
    fs: int = 48000
    gain_word: list = field(default_factory=list)     # per chain: the word of its LOAD_GAIN's gain
    taps_word: list = field(default_factory=list)     # per chain: the word of its first tap at rate 0 (None: no FIR)
    fir_state: list = field(default_factory=list)     # per chain: the data offset of its delay line (None: no FIR)
    banked: list = field(default_factory=list)        # chains on the shared impulse bank

    @property
    def C(self):
        return len(self.chains)

    @property
    def max_taps(self):
        return max(t for _, t in self.chains)

    @property
    def R(self):
        return ring_length(self.max_taps) if self.max_taps else 0


def chain_gain(c):
    return 0.5 + 0.03125 * c                  # exact in Q4.28 and in a float


def build(name, fmt, chains, fmin=pb.F48000, fmax=pb.F48000, fs=48000):
    nf = fmax - fmin + 1
    spec = [(ch[0], ch[1]) for ch in chains]
    banked = [c for c, ch in enumerate(chains) if len(ch) > 2 and ch[2] == "bank"]
    cap = 128 + sum(48 + S * (4 + 6 * nf) + nf * (T + 4) for S, T in spec) + nf * (max(t for _, t in spec) + 8)
    pw = pb.ProgramWriter(fmt, fmin, fmax, capacity=cap)
    C = len(spec)
    p = Program(name, fmt, None, spec, fs, banked=banked)
    pw.core()
    bank = None
    if banked:
        T = spec[banked[0]][1]
        assert all(spec[c][1] == T for c in banked)
        pw.param()
        bank = pw.fir_impulses([pb.lcg_taps(200 + f, T) for f in range(nf)])
    for c, (S, T) in enumerate(spec):
        pw.param()
        sec = pw.biquad_bank(pb.synth_sections(c, S, fmin, fmax)) if S else None
        imp = None
        if T:
            imp = bank if c in banked else pw.fir_impulses([pb.lcg_taps(c + 50 * f, T) for f in range(nf)])
        p.gain_word.append(pw.idx + 3)
        pw.load_gain_fixed(C + c, chain_gain(c))
        if sec is not None:
            pw.biquads(sec, S)
        p.fir_state.append(pw.fir(imp, T) if T else None)
        p.taps_word.append(imp[0] + 1 if T else None)
        pw.sat0db()
        pw.store(c)
    p.words = pw.end_of_code()
    return p


TIGHT_CHAINS = [(0, 416), (0, 7), (0, 1), (0, 300), (0, 49)]
MIXED_CHAINS = [(2, 416), (16, 49), (0, 300), (3, 0), (24, 7), (1, 1), (16, 0)]
LONG_CHAINS = [(1, 1030), (0, 641)]
BANK_CHAINS = [(1, 97, "bank")] * 17 + [(0, 97)] * 3
LANE_CHAINS = [(2, 120), (0, 33), (16, 0), (17, 7), (0, 300)]
FIXED_CHAINS = [(65, 0), (16, 0), (3, 0), (1, 0)]
# fir_tile's window ring (four row tiles, lean boundary): FIRs whose column pointer wraps once (1345 taps or more) and twice (2753),
# the longest one a tap past 4096; the 300-tap chain is what script B's second poke looks for
DEEP_CHAINS = [(2, 4096), (0, 1345), (1, 2753), (0, 300), (3, 4097)]

PROGRAMS = {                     # name -> (formats, maker(fmt))
    "TIGHT": ((4, 6), lambda fmt: build("TIGHT", fmt, TIGHT_CHAINS)),
    "MIXED": ((4, 6), lambda fmt: build("MIXED", fmt, MIXED_CHAINS)),
    "LONG": ((6,), lambda fmt: build("LONG", fmt, LONG_CHAINS)),
    "BANK": ((6,), lambda fmt: build("BANK", fmt, BANK_CHAINS)),
    "LANE": ((3, 5), lambda fmt: build("LANE", fmt, LANE_CHAINS)),
    "FIXED": ((2,), lambda fmt: build("FIXED", fmt, FIXED_CHAINS)),
    "RATES": ((6,), lambda fmt: build("RATES", fmt, MIXED_CHAINS, pb.F44100, pb.F48000, fs=44100)),
    "DEEP": ((4, 6), lambda fmt: build("DEEP", fmt, DEEP_CHAINS)),
}
_programs = {}


def program(name, fmt):
    assert fmt in PROGRAMS[name][0], (name, fmt)
    if (name, fmt) not in _programs:
        _programs[name, fmt] = PROGRAMS[name][1](fmt)
    return _programs[name, fmt]


def shard_range(total, world, rank):
    q, r = divmod(total, world)
    lo = rank * q + min(rank, r)
    return lo, q + (1 if rank < r else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the modelled ring position
# ---------------------------------------------------------------------------------------------------------------------------------
def ring_length(max_taps):
    """avdsp_plan_layout.h: pow2ceil(taps + 3 * 1024 + 16 * fir_groups_per_chunk(taps) + 16 * 6 + 64)"""
    G = (max_taps + 30) >> 4
    nc = (G + 55) // 56
    gpc = min(((G + nc - 1) // nc + 1) // 2 * 2, 56)
    v, p = max_taps + 3 * 1024 + 16 * gpc + 96 + 64, 1
    while p < v:
        p <<= 1
    return p


def model(script, R):
    """per step: (modelled position, frames consumed) BEFORE the step; the claims ("at", "total") are asserted on the way"""
    pos, total, generic, out = 0, 0, 0, []
    for i, st in enumerate(script):
        out.append((pos, total))
        k = st[0]
        if k == "at":
            assert pos == st[1], f"step {i}: the script claims ring position {st[1]}, the model says {pos}"
        elif k == "total":
            assert total == st[1], f"step {i}: the script claims {st[1]} frames, the model says {total}"
        elif k in ("block", "frames"):
            total += st[1]
            if not generic:
                pos += st[1]
        elif k == "shards":
            total += st[2]
            pos = 0
        elif k == "generic":
            generic, pos = st[1], 0
        elif k in ("params", "reset"):
            pos = 0
        if R:
            pos %= R
    out.append((pos, total))
    return out


def script_frames(script):
    return model([s for s in script if s[0] not in ("at", "total")], 0)[-1][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the player
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Segment:
    """what a fresh oracle needs to repeat the stream from a breaking step (or from the start) on"""
    step: int
    start: int                   # first input frame
    state: np.ndarray            # the state area at that point
    edits: dict
    fs: int
    end_state: np.ndarray | None = None       # the state where the next breaking step, or the script's end, found it


@dataclass
class Trace:
    out: np.ndarray              # the oracle's outputs, frame by frame over the whole input
    segments: list
    saves: dict                  # name -> (frames consumed at the save, state, step)
    forks: list                  # (name, first frame, frames replayed)


def _differ(step, kind, got, want, what="outputs"):
    g, w = words(got), words(want)
    if (g == w).all():
        return
    bad = np.nonzero((g != w).any(axis=0))[0]
    first = int(np.argmax((g != w).any(axis=1)))
    raise AssertionError(f"step {step} {kind}: {what} differ in channels {bad[:16].tolist()}, first at frame {first} of the step "
                         f"({np.count_nonzero(g != w)} words)")


def _same_state(step, kind, got, want, what="state"):
    if (got == want).all():
        return
    at = np.nonzero(got != want)[0]
    raise AssertionError(f"step {step} {kind}: {what} differs from the oracle's in {at.size} words, first at data offset {int(at[0])}: "
                         f"{int(got[at[0]]):#010x} against {int(want[at[0]]):#010x}")


def play(script, fmt, prog: Program, x, device=True):
    assert fmt == prog.fmt
    C, dt = prog.C, po.sample_dtype(fmt)
    x = np.ascontiguousarray(x, dtype=dt)
    assert x.shape == (script_frames(script), C), (x.shape, script_frames(script))
    o = po.OracleProgram(fmt, prog.words, fs=prog.fs)
    assert o.rc >= 0
    r = None
    if device:
        r = rt.Runtime(fmt, prog.words, fs=prog.fs)
        assert r.rc == o.rc
    out = np.zeros((len(x), C), dtype=dt)
    edits, fs, pos = {}, prog.fs, 0
    trace = Trace(out, [Segment(-1, 0, o.state.copy(), {}, fs)], {}, [])
    touched, generic_touched = {}, False

    def sync(i, kind):
        if r is not None:
            _same_state(i, kind, r.sync_state(), o.state)

    def breaks(i):
        trace.segments[-1].end_state = o.state.copy()
        return Segment(i, pos, None, dict(edits), fs)

    try:
        for i, st in enumerate(script):
            k = st[0]
            if k in ("at", "total"):
                continue
            if k == "block":
                n = st[1]
                out[pos:pos + n] = o.run_block(x[pos:pos + n], C, C)
                if r is not None:
                    _differ(i, k, r.run_block(x[pos:pos + n], C, C), out[pos:pos + n])
                pos += n
            elif k == "frames":
                for j in range(st[1]):
                    fo = np.zeros(2 * C, dtype=dt)
                    fo[C:] = x[pos]
                    fd = fo.copy()
                    assert po.lib().oracle_run(o.ctx, o.cores[0], o.data_ptr, fo.ctypes.data) >= 0
                    out[pos] = fo[:C]
                    if r is not None:
                        assert r.run_frame(fd) == 0
                        _differ(i, f"frames[{j}]", fd[None, :C], fo[None, :C])
                        _differ(i, f"frames[{j}]", fd[None, C:], fo[None, C:], "the input slots")
                    pos += 1
            elif k == "sync":
                sync(i, k)
            elif k == "save":
                sync(i, k)
                trace.saves[st[1]] = (pos, o.state.copy(), i)
            elif k == "load":
                seg = breaks(i)
                o.state[:] = trace.saves[st[1]][1]
                if r is not None:
                    r.state[:] = trace.saves[st[1]][1]
                    r.upload_state()
                seg.state = o.state.copy()
                trace.segments.append(seg)
            elif k == "poke":
                sync(i, k)
                seg = breaks(i)
                for chain, pokes in st[1].items():
                    T = prog.chains[chain][1]
                    for at, w in pokes:
                        assert 0 <= at < T
                        o.state[prog.fir_state[chain] + at] = w
                        if r is not None:
                            r.state[prog.fir_state[chain] + at] = w
                if r is not None:
                    r.upload_state()
                seg.state = o.state.copy()
                trace.segments.append(seg)
            elif k == "opt":
                if r is not None:
                    if st[1] not in touched:
                        touched[st[1]] = r.get_option(st[1])
                    r.set_option(st[1], st[2])
            elif k == "expect":
                if r is not None:
                    got = r.get_option(st[1])
                    assert got == st[2], f"step {i}: option {st[1]} reads {got}, expected {st[2]}"
            elif k == "params":
                if st[1]:
                    edits.update(st[1])
                    seg = breaks(i)
                    seg.state = o.state.copy()
                    trace.segments.append(seg)
                    for at, w in st[1].items():
                        assert 12 <= at < int(prog.words[1])
                        o.buf[at] = w
                        if r is not None:
                            r.buf[at] = w
                if r is not None:
                    r.upload_params()
            elif k == "generic":
                if r is not None:
                    generic_touched = True
                    r.set_option("generic", st[1])
            elif k == "shards":
                world, n = st[1], st[2]
                out[pos:pos + n] = o.run_block(x[pos:pos + n], C, C)
                if r is not None:
                    got = np.zeros((n, C), dtype=dt)
                    for rank in range(world):
                        r.set_shard(rank, world)
                        info = r.shard_info()
                        lo, m = info["first_chain"], info["nchains"]
                        assert (lo, m) == shard_range(C, world, rank)
                        got[:, lo:lo + m] = r.run_block(np.ascontiguousarray(x[pos:pos + n, lo:lo + m]), m, C + lo, lo)
                    r.set_shard(0, 1)
                    _differ(i, k, got, out[pos:pos + n])
                pos += n
            elif k == "reset":
                seg = breaks(i)
                fs = st[1]
                assert o.reset(fs) == 0
                if r is not None:
                    assert r.reset(fs) == 0
                seg.fs, seg.state = fs, o.state.copy()
                trace.segments.append(seg)
            elif k == "fork":
                start, saved, saved_at = trace.saves[st[1]]
                n = min(FORK_FRAMES, pos - start)
                assert n > 0 and not any(s.step > saved_at and s.start < start + n for s in trace.segments), \
                    f"step {i}: the frames behind save {st[1]!r} are not one unbroken stream"
                o2 = po.OracleProgram(fmt, prog.words, fs=fs)
                for at, w in edits.items():
                    o2.buf[at] = w
                o2.state[:] = saved
                want = o2.run_block(x[start:start + n], C, C)
                _differ(i, k, want, out[start:start + n], f"a second oracle's outputs from save {st[1]!r}")
                if r is not None:
                    r2 = rt.Runtime(fmt, prog.words, fs=fs)
                    try:
                        for at, w in edits.items():
                            r2.buf[at] = w
                        r2.state[:] = saved
                        r2.upload_state()
                        _differ(i, k, r2.run_block(x[start:start + n], C, C), want, f"a second runtime's outputs from save {st[1]!r}")
                        _same_state(i, k, r2.sync_state(), o2.state, f"a second runtime's state, {n} frames behind save {st[1]!r},")
                    finally:
                        r2.release()
                trace.forks.append((st[1], start, n))
            else:
                raise ValueError(f"step {i}: {st!r}")
        assert pos == len(x)
        trace.segments[-1].end_state = o.state.copy()
    finally:
        if r is not None:
            try:
                for key, v in touched.items():
                    r.set_option(key, v)
                if generic_touched:
                    r.set_option("generic", 0)
                r.set_shard(0, 1)
            finally:
                r.release()
    return trace


def replay_segments(trace, fmt, prog: Program, x):
    """the player's own semantics, oracle against oracle: from every breaking step (and from the start) a FRESH oracle, given the
    state that step left, runs the frames up to the next breaking step as ONE block and must give the same outputs and end state"""
    x = np.ascontiguousarray(x, dtype=po.sample_dtype(fmt))
    ends = [s.start for s in trace.segments[1:]] + [len(x)]
    for seg, end in zip(trace.segments, ends):
        o = po.OracleProgram(fmt, prog.words, fs=seg.fs)
        for at, w in seg.edits.items():
            o.buf[at] = w
        o.state[:] = seg.state
        if end > seg.start:
            _differ(seg.step, "segment", o.run_block(x[seg.start:end], prog.C, prog.C), trace.out[seg.start:end], "a fresh oracle's outputs")
        _same_state(seg.step, "segment", o.state, seg.end_state, "a fresh oracle's end state")


# ---------------------------------------------------------------------------------------------------------------------------------
# the scripts
# ---------------------------------------------------------------------------------------------------------------------------------
def blocks_to(steps, frames, chunk=4096):
    """blocks (of `chunk` frames at most) that bring the frames consumed so far to `frames`"""
    have = script_frames(steps)
    assert frames >= have
    while have < frames:
        n = min(chunk, frames - have)
        steps.append(("block", n))
        have += n


def script_A(prog, chunk=4096):
    """checkpoints at every phase of the ring"""
    R, T = prog.R, prog.max_taps
    s = [("save", "f0")]
    for total in (1, 1025, R - 1, R, R + 1, R + T - 1):
        blocks_to(s, total, chunk)
        s += [("total", total), ("at", total % R), ("save", f"f{total}")]
    blocks_to(s, 2 * R - 1200, chunk)
    s += [("at", R - 1200), ("block", 2500), ("at", 1300), ("save", "big"), ("block", 100), ("sync",)]
    s += [("fork", n) for n in ["f0"] + [f"f{t}" for t in (1, 1025, R - 1, R, R + 1, R + T - 1)] + ["big"]]
    return s


POKE_WORDS = (0x7F800000, 0xFFC00001, 0x7F812345, 0x00000012, 0x80000400)


def poke_of(prog, chain):
    T = prog.chains[chain][1]
    return {chain: list(zip((0, 1, T // 2, T - 2, T - 1), POKE_WORDS))}


def script_B(prog, pokes, chunk=4096):
    """upload at a used position; `pokes`: format 6"""
    R = prog.R
    big = max(range(prog.C), key=lambda c: prog.chains[c][1])
    other = [c for c in range(prog.C) if prog.chains[c][1] == 300][0]
    s = [("block", 1), ("block", 1024), ("total", 1025), ("save", "c")]
    blocks_to(s, 4000, chunk)
    s += [("at", 4000 % R), ("load", "c"), ("block", 100), ("block", 1024), ("sync",)]
    if pokes:
        s += [("poke", poke_of(prog, big))]
    s += [("block", 300), ("sync",), ("opt", "fir_impl", 4), ("block", 300)]
    if pokes:
        s += [("poke", poke_of(prog, other))]          # the operand ring exists: the operand of a poked word is the product's
    s += [("block", 300), ("sync",), ("opt", "fir_impl", 1)]
    blocks_to(s, 2 * R + 200, chunk)
    s += [("at", 200), ("load", "c"), ("block", 100), ("block", 1024), ("sync",)]
    return s


C_BLOCKS = [1024, 300, 1, 1024, 257, 1024, 700, 1024, 37, 513]
C_FIR_IMPL = [1, 4, 1, 3, 0, 2, 1, 3, 4, 1]
C_FIR_ROWS = [0, 1, 2, 4]


def script_C(prog, wrapped):
    """kernel switches between blocks; `wrapped`: the first fir_impl 3 / 4 block crosses the ring's end"""
    R = prog.R
    s = [("opt", "fir_impl", 1)]
    if wrapped:
        blocks_to(s, R - 150 - C_BLOCKS[0], 1024)
    for j, n in enumerate(C_BLOCKS):
        s += [("opt", "fir_impl", C_FIR_IMPL[j]), ("opt", "biquad_impl", (j + 1) % 2), ("opt", "fir_rows", C_FIR_ROWS[j % 4]),
              ("opt", "fir_lean", j % 2)]
        if j == 1:
            s += [("at", R - 150 if wrapped else 1024)]
        if j == 3:
            s += [("load", "c")]                        # between a fir_impl 1 block and a fir_impl 3 block
        s += [("block", n)]
        if j == 0:
            s += [("save", "c")]
        if j % 2:
            s += [("sync",)]
    return s


def find_edit(prog):
    """one gain and one tap, as tests/test_gpu_edge.py::test_live_parameter_edits edits them"""
    assert int(prog.words[prog.gain_word[1] - 3]) >> 16 == pb.OP_LOAD_GAIN and int(prog.words[prog.taps_word[0] - 1]) == prog.chains[0][1]
    return {prog.gain_word[1]: int(np.float32(0.37).view(np.uint32)), prog.taps_word[0] + 3: int(np.float32(0.125).view(np.uint32))}


D_SHARDS = [300, 1, 1024, 257]


def script_D(prog):
    """plans made again mid-stream"""
    tail = [("block", 300), ("block", 1024), ("sync",)]
    s = [("block", 1024), ("block", 276), ("total", 1300), ("at", 1300)]
    s += [("params", None), ("at", 0)] + tail
    s += [("params", find_edit(prog)), ("at", 0)] + tail
    s += [("at", 1324), ("generic", 1), ("block", 64), ("generic", 0), ("at", 0)] + tail
    s += [("shards", 3, n) for n in D_SHARDS] + [("at", 0)] + tail
    return s


def script_D_rates(prog):
    tail = [("block", 300), ("block", 1024), ("sync",)]
    s = [("block", 1024), ("block", 276), ("at", 1300)]
    for fs in (48000, 44100):
        s += [("reset", fs), ("at", 0), ("sync",)] + tail
    return s


def script_E(prog, chunk=4096):
    """one-frame calls on FIR chains"""
    R = prog.R
    s = []
    blocks_to(s, R - 2, chunk)
    s += [("at", R - 2), ("frames", 5), ("at", 3), ("block", 97), ("at", 100), ("frames", 5), ("block", 300), ("sync",)]
    return s


# ---- fir_tile's window ring in the scripts: program DEEP behind RING_PREFIX, whole blocks of 1024 frames -------------------------
RING_PREFIX = [("opt", "fir_rows", 4), ("opt", "fir_lean", 1)]


def script_A_ring(prog):
    """script A, every 1024-frame block of it a ring launch: checkpoints and forks at ring positions 0, 1, 1025, R - 1, R, R + 1, R + T - 1"""
    return RING_PREFIX + script_A(prog, 1024)


def script_B_ring(prog, pokes):
    """script B: uploads at used positions between ring launches, pokes at both ends of the 4097-tap line"""
    return RING_PREFIX + script_B(prog, pokes, 1024)


def script_D_ring(prog):
    return RING_PREFIX + script_D(prog)


def script_E_ring(prog):
    """script E, and a ring block behind the last one-frame calls: they lie between ring launches"""
    return RING_PREFIX + script_E(prog, 1024) + [("block", 1024), ("sync",)]


# (fir_impl, fir_rows, fir_lean) per block: the ring on both sides of every other kernel -- fir_mfma, fir_stream, fir_flow, fir_tile with
# two row tiles, fir_plain
N_TABLE = [(1, 4, 1), (2, 0, -1), (1, 4, 1), (3, 4, 0), (1, 4, 1), (4, 0, 0), (1, 4, 1), (1, 2, 1), (1, 4, 1), (0, 0, -1), (1, 4, 1)]
N_BLOCKS = [1024, 700, 513, 1024, 600]


def script_N(prog, wrapped):
    """the ring kernel taking turns with every other FIR kernel; `wrapped`: the first other kernel's block crosses the float ring's end"""
    R = prog.R
    s = list(RING_PREFIX)
    if wrapped:
        blocks_to(s, R - 150 - N_BLOCKS[0], 1024)
    for j, (impl, rows, lean) in enumerate(N_TABLE):
        s += [("opt", "fir_impl", impl), ("opt", "biquad_impl", (j + 1) % 2), ("opt", "fir_rows", rows), ("opt", "fir_lean", lean)]
        if j == 1:
            s += [("at", R - 150 if wrapped else 1024)]
        if j == 4:
            s += [("load", "c")]                        # between a fir_stream block and a ring block
        s += [("block", N_BLOCKS[j % 5])]
        if j == 0:
            s += [("save", "c")]
        if j % 2:
            s += [("sync",)]
    s += [("sync",)]
    return s


F_BLOCKS = [64, 1024, 256, 1, 700, 1024, 1024, 300]
F_SHARED = [1, 0, 1, 0]
F_FIR_IMPL = [1, 1, 1, 0, 1]


def script_F(prog):
    """shared path and back"""
    s = []
    for j, n in enumerate(F_BLOCKS):
        shared, impl = F_SHARED[j % 4], F_FIR_IMPL[j % 5]
        s += [("opt", "fir_shared", shared), ("opt", "fir_impl", impl), ("block", n),
              ("expect", "fir_shared_chains", len(prog.banked) if shared and impl == 1 else 0)]
        if j == 0:
            s += [("shards", 2, 256), ("at", 0)]        # (the plans are made again here: the blocks behind it wrap the ring)
        if j == 2:
            s += [("save", "c")]
        if j == 4:
            s += [("load", "c")]
    assert sum(F_BLOCKS[1:]) > prog.R
    s += [("at", sum(F_BLOCKS[1:]) - prog.R), ("sync",)]
    return s


def script_G(prog):
    """lane plans"""
    s = []
    for j, n in enumerate([300, 1, 700, 257, 2]):
        s += [("opt", "lane_hw", (j + 1) % 2), ("block", n)]
        if j == 1:
            s += [("save", "c"), ("frames", 3)]
        if j == 2:
            s += [("shards", 3, 100)]
    s += [("sync",), ("fork", "c")]
    return s


def script_H(prog):
    """fixed point"""
    s = []
    for j, n in enumerate([1, 7, 1024, 100, 33]):
        s += [("opt", "biquad_impl", (j + 1) % 2), ("block", n)]
        if j == 1:
            s += [("save", "c")]
        if j == 2:
            s += [("generic", 1), ("block", 64), ("generic", 0)]
        if j == 3:
            s += [("shards", 2, 100)]
    s += [("sync",), ("fork", "c")]
    return s


def _cases():
    out = {}

    def add(letter, name, fmts, make, *args):
        for fmt in fmts:
            out[f"{letter}-{name}-f{fmt}" + "".join(f"-{a}" for a in args if isinstance(a, str))] = (name, fmt, make, tuple(a for a in args if not isinstance(a, str)))

    add("A", "TIGHT", (4, 6), script_A)
    add("A", "MIXED", (4, 6), script_A)
    add("A", "LONG", (6,), script_A)
    for name in ("TIGHT", "MIXED"):
        add("B", name, (4,), script_B, False)
        add("B", name, (6,), script_B, True)
    add("C", "MIXED", (4, 6), script_C, False, "inside")
    add("C", "MIXED", (4, 6), script_C, True, "wrapped")
    add("C", "TIGHT", (6,), script_C, False, "inside")
    add("C", "TIGHT", (6,), script_C, True, "wrapped")
    add("D", "MIXED", (4, 6), script_D)
    add("D", "RATES", (6,), script_D_rates)
    add("E", "TIGHT", (4, 6), script_E)
    add("E", "LANE", (3, 5), script_E)
    add("E", "MIXED", (6,), script_E)
    add("F", "BANK", (6,), script_F)
    add("G", "LANE", (3, 5), script_G)
    add("H", "FIXED", (2,), script_H)
    add("A", "DEEP", (4, 6), script_A_ring)
    add("B", "DEEP", (4,), script_B_ring, False)
    add("B", "DEEP", (6,), script_B_ring, True)
    add("D", "DEEP", (4, 6), script_D_ring)
    add("E", "DEEP", (4, 6), script_E_ring)
    add("N", "DEEP", (4, 6), script_N, False, "inside")
    add("N", "DEEP", (4, 6), script_N, True, "wrapped")
    return out


CASES = _cases()
_inputs = {}


def case(case_id):
    """(program, script, input) of a case; made once"""
    if case_id not in _inputs:
        name, fmt, make, args = CASES[case_id]
        prog = program(name, fmt)
        script = make(prog, *args)
        # (the DEEP cases came later: they count on from the others, whose inputs stay what they were)
        order = sorted(c for c in CASES if "-DEEP-" not in c) + sorted(c for c in CASES if "-DEEP-" in c)
        seed = 1000 + order.index(case_id)
        _inputs[case_id] = (prog, script, pb.lcg_input(script_frames(script), prog.C, fmt in (5, 6), seed=seed))
    return _inputs[case_id]

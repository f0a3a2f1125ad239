"""The cases that take fir_tile's window ring (four row tiles, lean boundary, neither BIG nor SPLIT) through every
route that launches it, as data that imports without a GPU: programs, block lengths, options, and for every FIR launch of every block
what fir_choice / fir_hand_choice are asked -- tests/test_fir_ring_reach.py asks them (a device cannot say which variant ran),
tests/test_gpu_fir_ring_routes.py runs the cases against the oracle bit for bit, tests/test_fir_ring_model.py takes its tap counts
from here.  The ring cases of tests/state_scripts.py (program DEEP) are listed here too, launch by launch.

A launch, for the reach test: dict(frames, n, cascades, plan_taps, impl, rows, lean, hand, ring) -- `ring`: the block is meant for the
ring kernel; False: it is meant as another kernel between ring launches."""
from __future__ import annotations

import numpy as np

from avdsp_amd import progbuilder as pb

FMTS = (6, 4)
RING_OPTS = dict(fir_impl=1, fir_rows=4, fir_lean=1)
FIRST_WRAP, SECOND_WRAP = 1345, 2753        # the tap counts from which a lane's column pointer wraps once / twice

# (sections, taps): four chains to a workgroup, the last workgroup short; two FIR-only chains beside cascaded ones, so that
# all_cascaded is false and the plan still has an overlap mode
BASE = [(2, 4096), (1, 1345), (0, 2753), (1, 380), (3, 4097), (2, 1409), (0, 1900), (2, 65), (1, 3000)]
TEN = BASE + [(1, 1407)]                    # three shards of 4 / 3 / 3 chains


def chains_program(fmt, spec, stores=1, gap=1):
    """one chain per (sections, taps): LOAD_GAIN(IO nout + c) -> [BIQUADS] -> FIR (its own impulse) -> SAT0DB -> `stores` STOREs,
    `gap` IOs apart: chain c stores IOs gap * stores * c .. + stores - 1.  -> (program, nout)"""
    C = len(spec)
    nout = gap * stores * C
    pw = pb.ProgramWriter(fmt, pb.F48000, pb.F48000, capacity=64 + sum(T + 64 + 16 * S + 8 * stores for S, T in spec))
    pw.core()
    for c, (S, T) in enumerate(spec):
        pw.param()
        bank = pw.biquad_bank(pb.synth_sections(c, S, pb.F48000, pb.F48000)) if S else None
        imp = pw.fir_impulses([pb.lcg_taps_all(1, T, channel_base=c)[0]])
        pw.load_gain_fixed(nout + c, 1.0)
        if bank is not None:
            pw.biquads(bank, S)
        pw.fir(imp, T)
        pw.sat0db()
        for k in range(stores):
            pw.store(gap * stores * c + k)
    return pw.end_of_code(), nout


def cut(blocks):
    return list(zip(np.cumsum([0] + list(blocks[:-1])).tolist(), blocks))


def plan_facts(spec):
    """(FIR chains, cascades in front of FIRs, FIR chains x the longest FIR) as launch_fir hands them to fir_choice"""
    n = sum(1 for _, T in spec if T)
    return n, any(S for S, _ in spec), n * max(T for _, T in spec)


def launches_of(spec, blocks, opts, ring_blocks, n=None):
    """one plain FIR launch per block (every block here is one launch: at most 1024 frames)"""
    nf, casc, pt = plan_facts(spec)
    assert all(b <= 1024 for b in blocks)
    return [dict(frames=b, n=nf if n is None else n, cascades=casc, plan_taps=pt, impl=opts.get("fir_impl", 1), rows=opts.get("fir_rows", 0),
                 lean=opts.get("fir_lean", -1), hand=False, ring=k in ring_blocks) for k, b in enumerate(blocks)]


# ---------------------------------------------------------------------------------------------------------------------------------
# a. blocks in flight: device-resident blocks enqueued back to back on one stream, no host synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------
FLIGHT_BLOCKS = [1024, 600, 1024, 513, 1024, 333, 1024, 1024, 700, 100, 1024, 1024, 1024]
FLIGHT_RING = {k for k, b in enumerate(FLIGHT_BLOCKS) if b not in (333, 100)}       # 333 and 100: another kernel between ring launches
assert sum(FLIGHT_BLOCKS) > 8192 + 2048                                            # the float ring wraps under the window

# name -> options on top of RING_OPTS.  The first seven are tests/dev/gpu_overlap_sweep.ARR without its one "fir_lean" 0 entry (its
# "fir_lean" 1 entry is "behind" here, where every entry has the lean boundary).
# "staged": what "fir_ahead_now" must read behind a ring block; "path": the route's (tests/route_driver.py) with the streams apart
FLIGHT = {
    "event":            dict(opts=dict(overlap=1, ready_words=0, ring_wait=1)),
    "behind":           dict(opts=dict(overlap=1, ready_words=2, ring_wait=1)),
    "behind-nowait":    dict(opts=dict(overlap=1, ready_words=2, ring_wait=0)),
    "words":            dict(opts=dict(overlap=1, ready_words=1, ring_wait=1)),
    "own-stream":       dict(opts=dict(overlap=2, ready_words=0, ring_wait=1)),
    "flow":             dict(opts=dict(overlap=1, ready_words=2, ring_wait=1, fir_impl=4), ring=False),
    "by-plan":          dict(opts=dict(overlap=1, ready_words=-1, ring_wait=1)),
    "ahead":            dict(opts=dict(overlap=1, fir_ahead=1, ring_wait=1), staged=1),
    "ahead-nowait":     dict(opts=dict(overlap=1, fir_ahead=1, ready_words=2, ring_wait=0), staged=1),
    "ahead-launch2":    dict(opts=dict(overlap=1, fir_ahead=1, fir_launch=2), staged=1),            # (a staged launch has no launch mode: fir_launch is not read)
    "direct":           dict(opts=dict(overlap=1, fir_ahead=0, ready_words=-1)),
    "direct-launch1":   dict(opts=dict(overlap=1, fir_ahead=0, fir_launch=1, ready_words=2)),
    "direct-launch2":   dict(opts=dict(overlap=1, fir_ahead=0, fir_launch=2, ready_words=2)),
    "words-launch2":    dict(opts=dict(overlap=1, fir_ahead=0, fir_launch=2, ready_words=1, ring_wait=0)),
    "event-launch1":    dict(opts=dict(overlap=1, fir_ahead=0, fir_launch=1, ready_words=0)),
    # what the route refuses (tests/test_launch_route.py): the combination runs, on the path the route gives it instead
    "ahead-refused-overlap2": dict(opts=dict(overlap=2, fir_ahead=1, ready_words=2), staged=0,
                                   refused="overlap 2 has the FIRs on a stream of the library's own (own_fir): never a candidate for staging"),
    "ahead-refused-flow":     dict(opts=dict(overlap=1, fir_ahead=1, fir_impl=4), staged=0, ring=False,
                                   refused="only fir_tile is staged: fir_flow makes its operand ring on the launch's stream"),
    "launch2-unread-overlap2": dict(opts=dict(overlap=2, fir_launch=2, ready_words=1), staged=0,
                                    refused="fir_launch is the direct path's: under overlap 2 (own_fir) the launch mode stays 0"),
}
for _name, _a in FLIGHT.items():
    _a.setdefault("staged", 0)
    _a.setdefault("ring", True)
    _a["opts"] = {**RING_OPTS, **_a["opts"]}
# one arrangement per format on the odd samples
FLIGHT_STRESS = {6: "behind", 4: "ahead-nowait"}
# every global option a flight case may have set, and what it goes back to
FLIGHT_DEFAULTS = dict(overlap=0, ready_words=-1, ring_wait=1, fir_ahead=-1, fir_launch=-1, fir_impl=1, fir_rows=0, fir_lean=-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. one output block for every call (the staged contract)
# ---------------------------------------------------------------------------------------------------------------------------------
STAGED_BLOCKS = [1024, 1024, 1024, 600, 513]
STAGED = {                                  # name -> (formats, chains, stores, gap)
    "base": (FMTS, BASE, 1, 1),
    "two_stores": ((6,), BASE[:5], 2, 1),   # ten columns in a row, not a multiple of 16 bytes: the tiles leave the plain way
    "gapped": ((6,), BASE[4:], 1, 2),       # every other column, the ones between belong to nobody: the plain way too
}

# ---------------------------------------------------------------------------------------------------------------------------------
# c. shards
# ---------------------------------------------------------------------------------------------------------------------------------
SHARD_WORLD = 3
SHARD_BLOCKS = [1024, 600, 1024, 513]       # each as SHARD_WORLD calls
SHARD_WHOLE = 1024                          # then one whole block on the oracle's state


def shard_range(total, world, rank):
    q, r = divmod(total, world)
    return rank * q + min(rank, r), q + (1 if rank < r else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. memory-word trees
# ---------------------------------------------------------------------------------------------------------------------------------
TREE_BLOCKS = [1024, 600, 1024, 1024]
TREE_OPTIONS = ("mem_fir", "chain_mem", "fir_tail", "chain_delay", "chain_finish")


def tree_items():
    """tests/firtree_programs.py items of one core: a trunk of 2 sections + 4096 taps with three branches (sections only; a FIR alone of
    2753 taps, fed from the ring mem_stage writes; a handed one of 1345 taps with a DELAY and SAT0DB_TPDF_GAIN), a FIR-less trunk whose
    two branches are FIRs alone of 1409 and 4097 taps, and an ordinary handed chain of 4096 taps"""
    from tests import firtree_programs as tp
    return [tp.trunk("a", 2, 4096, 0.5),
            tp.branch("a", nsec=2, taps=0),
            tp.branch("a", nsec=0, taps=2753),
            tp.branch("a", nsec=1, taps=1345, slot="A", form="fixed", us=1000, finish="tpdf_gain", gain=0.93),
            tp.trunk("b", 2, 0, 0.6),
            tp.branch("b", nsec=0, taps=1409),
            tp.branch("b", nsec=0, taps=4097, finish="none"),
            tp.plain(nsec=1, taps=4096, slot="B", form="fixed", us=300, finish="tpdf")]


TREE_RING_FED = 2                           # item index of the ring-fed 2753-tap branch, TREE_HANDED of the ordinary handed chain
TREE_HANDED = 7
# the tree core's three FIR launches per block: (what, chains, hand)
TREE_LAUNCHES = [("the trunks' FIR", 1, False), ("the branches' plain FIRs", 3, False), ("the handed FIRs", 2, True)]
TREE_TAPS = [4096, 2753, 1345, 1409, 4097, 4096]


# ---------------------------------------------------------------------------------------------------------------------------------
# the launches of every case, for the reach test
# ---------------------------------------------------------------------------------------------------------------------------------
def script_launches(case_id):
    """a tests/state_scripts.py case launch by launch: the options as its "opt" steps leave them, blocks cut into launches of 1024
    frames.  `ring` is what the script is written for: a launch of more than 512 frames while the script's own steps -- all but its
    first two, the prefix a careless edit would drop -- have not asked for another kernel; RING_LAUNCHES below holds each case to a
    literal count of them"""
    from tests import state_scripts as ss
    prog, script, _ = ss.case(case_id)
    nf, casc, pt = plan_facts(prog.chains)
    cur = dict(fir_impl=1, fir_rows=0, fir_lean=-1)
    said = dict(RING_OPTS)
    out, generic = [], 0
    for i, st in enumerate(script):
        if st[0] == "opt" and st[1] in cur:
            cur[st[1]] = st[2]
            if i >= 2:
                said[st[1]] = st[2]
        elif st[0] == "generic":
            generic = st[1]
        elif st[0] in ("block", "shards") and not generic:
            frames = st[1] if st[0] == "block" else st[2]
            ns = [nf] if st[0] == "block" else [shard_range(prog.C, st[1], r)[1] for r in range(st[1])]
            for n in ns:
                left = frames
                while left > 0:
                    f = min(1024, left)
                    out.append(dict(frames=f, n=n, cascades=casc, plan_taps=pt, impl=cur["fir_impl"], rows=cur["fir_rows"], lean=cur["fir_lean"],
                                    hand=False, ring=f > 512 and said == RING_OPTS, step=i))
                    left -= f
    return out


def tree_launches():
    out = []
    for b in TREE_BLOCKS:
        for what, n, hand in TREE_LAUNCHES:
            # (a handed launch is lean by rule: fir_hand_choice is not given "fir_lean")
            out.append(dict(frames=b, n=n, cascades=True, plan_taps=len(TREE_TAPS) * max(TREE_TAPS), impl=1, rows=4, lean=1, hand=hand, ring=True, what=what))
    return out


def handed_launches():
    """tests/test_gpu_fir_window_ring.py::test_handed_chains sets "fir_rows" 4 and leaves the boundary to the rule"""
    return [dict(frames=b, n=5, cascades=True, plan_taps=5 * 4097, impl=1, rows=4, lean=-1, hand=True, ring=True) for b in (1024, 600, 1024, 1024)]


def reach_cases():
    """name -> dict(launches, taps, wraps): `wraps` is what the case's name or docstring promises (0, 1 or 2)"""
    out = {}
    for name, a in FLIGHT.items():
        out[f"flight-{name}"] = dict(launches=launches_of(BASE, FLIGHT_BLOCKS, a["opts"], FLIGHT_RING if a["ring"] else set()), taps=[t for _, t in BASE],
                                     wraps=2, some_other=a["ring"], no_ring=not a["ring"])      # (fir_flow's arrangements: ARR's, for comparison)
    for name, (fmts, spec, stores, gap) in STAGED.items():
        for ahead in (1, 0):
            out[f"staged-{name}-ahead{ahead}"] = dict(launches=launches_of(spec, STAGED_BLOCKS, RING_OPTS, set(range(len(STAGED_BLOCKS)))),
                                                      taps=[t for _, t in spec], wraps=2)
    for rank in range(SHARD_WORLD):
        lo, m = shard_range(len(TEN), SHARD_WORLD, rank)
        out[f"shard-{rank}of{SHARD_WORLD}"] = dict(launches=launches_of(TEN, SHARD_BLOCKS, RING_OPTS, set(range(len(SHARD_BLOCKS))), n=m),
                                                   taps=[t for _, t in TEN[lo:lo + m]], wraps=2)
    out["shard-whole"] = dict(launches=launches_of(TEN, [SHARD_WHOLE], RING_OPTS, {0}), taps=[t for _, t in TEN], wraps=2)
    out["tree"] = dict(launches=tree_launches(), taps=TREE_TAPS, wraps=2)
    out["window-ring-handed"] = dict(launches=handed_launches(), taps=[4096, 1345, 2753, 380, 4097], wraps=2)
    from tests import state_scripts as ss
    for cid in sorted(ss.CASES):
        if ss.CASES[cid][0] == "DEEP":
            out[f"script-{cid}"] = dict(launches=script_launches(cid), taps=[t for _, t in ss.DEEP_CHAINS], wraps=2,
                                        ring_launches=RING_LAUNCHES[cid], some_other=cid[0] in "BCDN")
    return out


# ring launches per DEEP script case, counted by hand from the scripts (tests/state_scripts.py): a block of `blocks_to(..., 1024)` is a
# ring launch when it is longer than 512 frames
RING_LAUNCHES = {
    # A: 1 | 1024 | 7166 = 6 x 1024 + 1022 | 1 | 1 | 4095 = 3 x 1024 + 1023 | up to 2R - 1200: 2896 = 2 x 1024 + 848 | 2500 = 1024 + 1024 + 452 | 100
    "A-DEEP-f4": 1 + 7 + 4 + 3 + 2, "A-DEEP-f6": 1 + 7 + 4 + 3 + 2,
    # B: 1, 1024 | to 4000: 2 x 1024 + 927 | load | 100, 1024 | 300 | (fir_impl 4: 300, 300) | to 2R + 200 = 16584 from 6049: 10 x 1024 + 295 | load | 100, 1024
    "B-DEEP-f4": 1 + 3 + 1 + 10 + 1, "B-DEEP-f6": 1 + 3 + 1 + 10 + 1,
    # D: 1024, 276 | 300, 1024 | 300, 1024 | (generic 64) 300, 1024 | shards 3 x (300, 1, 1024, 257): 3 ring | 300, 1024
    "D-DEEP-f4": 1 + 1 + 1 + 1 + 3 + 1, "D-DEEP-f6": 1 + 1 + 1 + 1 + 3 + 1,
    # E: to R - 2 = 8190: 7 x 1024 + 1022 | 5 frames | 97 | 5 frames | 300 | 1024
    "E-DEEP-f4": 8 + 1, "E-DEEP-f6": 8 + 1,
    # N: the table's six ring entries; wrapped: the run-up to R - 150 - 1024 = 7018 in front: 6 x 1024 + 874
    "N-DEEP-f4-inside": 6, "N-DEEP-f6-inside": 6, "N-DEEP-f4-wrapped": 13, "N-DEEP-f6-wrapped": 13,
}


def ring_tap_counts():
    """every tap count that runs through the ring kernel in tests/test_gpu_fir_window_ring.py, tests/test_gpu_fir_ring_routes.py and
    the DEEP scripts: what tests/test_fir_ring_model.py holds its mutations against"""
    window_ring = [1, 63, 64, 65, 1343, 1344, 1345, 1900, 1407, 1408, 1409, 2752, 2753, 4095, 4096, 4097, 380, 3000]
    from tests import state_scripts as ss
    return sorted(set(window_ring) | {t for _, t in TEN} | set(TREE_TAPS) | {t for _, t in ss.DEEP_CHAINS})

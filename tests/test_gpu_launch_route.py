"""The enqueuers of a block launch against the route they are handed: launch_all computes the facts of a call, asks
launch_gate / launch_route (avdsp_plan_layout.h) and enqueues what they say.  Two small programs, six calls of ragged lengths back
to back into three output blocks in turn (as bench.py does for "overlap" 2), under two dozen sets of the options that steer the
route; every block and the final state are held to the oracle word for word.

After each call the test reads what the library says it did ("ready_mode", "fir_ahead_now", "side_by_side", "fir_ahead_apart"),
asks tests/csrc/launch_route_driver.cpp -- the same pure function, built alone -- for the route of the call's facts and of the
probe results THIS process got, and holds the read-backs to its answer; so nothing depends on which hardware queues the runtime
dealt out.  The kernel timer samples FIR launch k of a program where k is a multiple of "profile_stride": the test counts.

Between them the sets take the back-to-back, direct, own-FIR and staged enqueuers, both copy kernels of the staged path (a window
as wide as the chains: ahead_copy_run; five words wider: ahead_copy_words), the three launch modes and the direct path's launch
that carries its kernel timer's stop event.  "cu_split" is not exercised here: its route is held by the rows of
tests/test_launch_route.py, its bits by test_gpu_ready_timeout.py's experiment.  Plans with memory words have their own enqueuer and
their own test (test_gpu_memtree.py)."""
import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests.route_driver import STAGED, ask, build_driver

BLOCKS = [1024, 333, 100, 1024, 100, 333]
SENT = 0x5EA1AB1E
SHAPES = {"f6": (6, 40, 8, 700), "f4": (4, 24, 4, 300)}          # test_gpu_fir_ahead.py's two
STEERING = ("overlap", "ready_words", "fir_launch", "fir_ahead", "ring_wait", "profile")


def S(overlap, ready_words=-1, fir_launch=-1, fir_ahead=-1, ring_wait=1, timer=0, wide=0):
    """an option set; timer: 0 off, else on with that "profile_stride"; wide: the output window's words beyond the chains'"""
    return dict(overlap=overlap, ready_words=ready_words, fir_launch=fir_launch, fir_ahead=fir_ahead, ring_wait=ring_wait, timer=timer, wide=wide)


SETS = [
    S(0),                                                      # back to back
    S(1), S(1, 0, 0), S(1, 1, 1), S(1, 2, 1), S(1, 2, 2), S(1, 1, 2), S(1, 2, 0, ring_wait=0), S(1, -1, 1, ring_wait=0),      # direct
    S(1, fir_launch=1, timer=1), S(1, fir_launch=1, timer=4), S(1, 2, timer=4), S(1, fir_launch=2, timer=1), S(1, 2, 1, fir_ahead=0),
    S(1, fir_ahead=1), S(1, fir_ahead=1, wide=5), S(1, 2, fir_ahead=1), S(1, fir_ahead=1, ring_wait=0), S(1, fir_ahead=1, timer=1),      # staged
    S(2), S(2, 1), S(2, 2), S(2, 2, ring_wait=0, timer=4), S(2, fir_ahead=1),                  # own-FIR
]


def set_id(s):
    return "overlap{overlap}_words{ready_words}_launch{fir_launch}_ahead{fir_ahead}_wait{ring_wait}_timer{timer}_wide{wide}".format(**s)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, why = build_driver(tmp_path_factory.mktemp("gpulaunchroute"))
    assert exe is not None, why
    return exe


@pytest.fixture
def _options_back():
    """options are process-wide: every case sets the ones it depends on, and leaves the process as it found it"""
    rt.lib().dspRuntimeRelease()
    found = [(key, rt.lib().dspRuntimeGetOption(key.encode())) for key in ("fir_impl", "biquad_impl", "fir_rows") + STEERING]
    yield
    rt.lib().dspRuntimeRelease()
    for key, v in found + [("profile_stride", 1)]:
        rt.Runtime.set_global_option(key, v)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


_REF = {}


def reference(name):
    """program, input, the oracle's output of every block and its final state -- computed once, shared, never written"""
    if name not in _REF:
        fmt, C, Sn, T = SHAPES[name]
        prog = pb.synth_program(fmt, C, Sn, T)
        x = pb.lcg_input(sum(BLOCKS), C, fmt == 6, seed=91)
        o = po.OracleProgram(fmt, prog)
        outs = [o.run_block(x[a:a + n], C, C) for a, n in cut(BLOCKS)]
        state = o.state.copy()
        for v in outs + [state, x, prog]:
            v.flags.writeable = False
        _REF[name] = (fmt, C, T, prog, x, outs, state)
    return _REF[name]


@pytest.mark.gpu
@pytest.mark.usefixtures("_options_back")
@pytest.mark.parametrize("opts", SETS, ids=set_id)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_enqueuers_follow_the_route(driver, name, opts):
    import torch
    fmt, C, T, prog, x, outs, state = reference(name)
    xd = [dm.to_device(x[a:a + n].copy()) for a, n in cut(BLOCKS)]
    torch.cuda.synchronize()                                 # the overlap modes' contract: inputs complete when the call is made
    r = rt.Runtime(fmt, prog)
    for key, v in (("fir_impl", 1), ("biquad_impl", 1), ("fir_rows", 0), ("profile_stride", max(opts["timer"], 1)), ("profile", int(opts["timer"] > 0))):
        r.set_option(key, v)
    for key in STEERING[:-1]:
        r.set_option(key, opts[key])
    width = C + opts["wide"]
    st = torch.cuda.current_stream().cuda_stream
    ys = [torch.empty((1024, width), dtype=torch.int32, device="cuda") for _ in range(3)]
    clones, said = [], []
    for k, n in enumerate(BLOCKS):
        y = ys[k % 3]
        y.fill_(SENT)
        r.run_block_device(xd[k].data_ptr(), C, C, y.data_ptr(), width, 0, n, st)
        got = {key: r.get_option(key) for key in ("ready_mode", "fir_ahead_now", "side_by_side", "fir_ahead_apart")}
        want = ask(driver, overlap=opts["overlap"], ready_words=opts["ready_words"], fir_launch=opts["fir_launch"], fir_ahead=opts["fir_ahead"],
                   nframes=n, out_stride=width, n_fir=C, max_taps=T, n_ahead_cols=C, timer_samples=opts["timer"] > 0 and k % opts["timer"] == 0,
                   ahead_apart=max(got["fir_ahead_apart"], 0), side_by_side=max(got["side_by_side"], 0))
        said.append((got, want))
        clones.append(y.clone())
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(said):
        what = f"{name}, {set_id(opts)}, call {k}: the library says {got}, the route is {want}"
        assert want["under"] == (opts["overlap"] != 0), what
        assert got["ready_mode"] == want["ready_mode"] and got["fir_ahead_now"] == (want["path"] == STAGED), what
        if want["under"]:
            assert got["side_by_side"] == want["side_by_side"], what
    for k, c in enumerate(clones):
        g, n = dm.to_host(c).view(np.uint32), BLOCKS[k]
        assert (g[:n, :C] == words(outs[k])).all(), f"{name}, {set_id(opts)}, block {k}: output differs from the oracle"
        assert (g[:n, C:] == SENT).all() and (g[n:] == SENT).all(), f"{name}, {set_id(opts)}, block {k}: a word outside the block was written"
    assert (r.sync_state() == state).all()
    assert r.get_option("ready_timeouts") == 0
    r.release()

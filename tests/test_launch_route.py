"""The route of a block launch (avdsp_amd/csrc/avdsp_plan_layout.h: launch_gate, launch_route), without a GPU.
tests/csrc/launch_route_driver.cpp is built against that header alone with AddressSanitizer and UBSan and run as a program of its
own; what it prints is compared with literal rows that follow from the branches launch_all has had all along: which of the four
paths a launch takes, how the FIR finds its cascades' block, what carries the events.  Rows are "chains x taps, frames"."""
import pytest

from tests.route_driver import BACK_TO_BACK, DIRECT, ON_CALLER, ON_FIR_FIRST, ON_FIR_TURN, OWN_FIR, STAGED, ask, build_driver


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    exe, why = build_driver(tmp_path_factory.mktemp("launchroute"))
    if exe is None:
        pytest.skip(why)
    return lambda **facts: ask(exe, **facts)


def pick(r, *names):
    return tuple(r[n] for n in names)


ROUTE = ("path", "ready_mode", "cascade_event", "write_through", "fir_waits_event", "ready_acquire", "fir_launch_mode", "rides")
BEHIND_DIRECT = (DIRECT, 2, 0, 0, 0, 0, 1, 1)             # a kernel behind the cascade publishes; the FIR's dispatch carries its event
EVENT_DIRECT = (DIRECT, 0, 1, 0, 1, 0, 1, 1)              # the FIR waits for the cascades' event


# ---------------------------------------------------------------- the staged path
def test_north_star_is_staged_where_its_streams_are_apart(route):
    r = route(ahead_apart=1)                               # 4096 x 4096, 1024
    assert pick(r, "under", "own_fir", "ahead_candidate") == (1, 0, 1)
    assert pick(r, *ROUTE) == (STAGED, 0, 1, 0, 1, 0, 0, 0)          # the event, whatever "ready_words" says; FIR on s_fir[blk & 1]
    assert r["side_by_side"] == 1                          # ahead_apart's copy: no side-by-side probe
    assert route(ahead_apart=1, side_by_side=0) == route(ahead_apart=1, side_by_side=1)
    assert route(ahead_apart=1, timer_samples=1) == r


def test_a_candidate_whose_streams_are_not_apart_goes_direct(route):
    r = route(ahead_apart=0, side_by_side=1)
    assert pick(r, "ahead_candidate", "probe_on", "side_by_side") == (1, ON_CALLER, 1)
    assert pick(r, *ROUTE) == BEHIND_DIRECT
    assert pick(route(ahead_apart=0, side_by_side=1, timer_samples=1), *ROUTE) == BEHIND_DIRECT[:-1] + (0,)      # the timer's events instead
    r = route(ahead_apart=0, side_by_side=0)
    assert pick(r, *ROUTE) == EVENT_DIRECT and r["side_by_side"] == 0


def test_fir_ahead_forced_and_off(route):
    r = route(fir_ahead=1, ahead_apart=0, side_by_side=1)
    assert pick(r, "ahead_candidate", "path", "ready_mode", "side_by_side") == (1, STAGED, 0, 0)
    assert pick(route(fir_ahead=1, n_fir=512, ahead_apart=1), "ahead_candidate", "path") == (1, STAGED)      # (forced: whatever the plan's size)
    r = route(fir_ahead=0, ahead_apart=1, side_by_side=1)
    assert r["ahead_candidate"] == 0 and pick(r, *ROUTE) == BEHIND_DIRECT


@pytest.mark.parametrize("n_fir, max_taps, nframes, candidate", [(2048, 4096, 256, 1), (2048, 4096, 255, 0), (1, 7999999, 1024, 0), (1, 8000000, 1024, 1)])
def test_fir_ahead_by_plan_boundaries(route, n_fir, max_taps, nframes, candidate):
    assert route(n_fir=n_fir, max_taps=max_taps, nframes=nframes, ahead_apart=1)["ahead_candidate"] == candidate


@pytest.mark.parametrize("fact", [dict(in_place=1), dict(out_stride=16385), dict(instances=2), dict(inst_n=2), dict(chain_inst=2),
                                  dict(n_sh_groups=1), dict(has_taps64=0), dict(n_ahead_cols=0), dict(fir_impl=4)],
                         ids=lambda f: next(iter(f)))
def test_what_rules_the_staged_path_out(route, fact):
    for forced in (-1, 1):
        r = route(fir_ahead=forced, ahead_apart=1, side_by_side=1, **fact)
        assert r["ahead_candidate"] == 0 and r["probe_on"] == ON_CALLER
        assert pick(r, *ROUTE) == BEHIND_DIRECT            # fir_flow takes mode 2 and the launch modes as fir_tile does
        assert r == route(fir_ahead=0, ahead_apart=1, side_by_side=1, **fact)
    assert route(out_stride=16384, ahead_apart=1)["path"] == STAGED          # (the cap itself: 1024 frames x 16384 words)


# ---------------------------------------------------------------- shards on the direct path
@pytest.mark.parametrize("n_fir, max_taps, nframes, mode", [(512, 4096, 1024, 2), (512, 4096, 768, 1), (512, 4096, 769, 2),
                                                             (1, 6000000, 1024, 2), (1, 6000001, 1024, 1)])
def test_launch_mode_by_plan(route, n_fir, max_taps, nframes, mode):
    r = route(n_fir=n_fir, max_taps=max_taps, nframes=nframes, ahead_apart=1, side_by_side=1)
    assert r["ahead_candidate"] == 0
    assert pick(r, *ROUTE) == (DIRECT, 0, 1, 0, 1, 0, mode, int(mode == 1))       # only mode 1 rides


def test_launch_mode_set(route):
    assert [pick(route(n_fir=512, fir_launch=m), "fir_launch_mode", "rides") for m in (0, 1, 2)] == [(0, 0), (1, 1), (2, 0)]
    assert pick(route(n_fir=512, fir_launch=1, timer_samples=1), "fir_launch_mode", "rides") == (1, 0)


@pytest.mark.parametrize("max_taps, mode", [(11999999, 0), (12000000, 2)])
def test_ready_words_default_boundary(route, max_taps, mode):
    r = route(n_fir=1, max_taps=max_taps, ahead_apart=0, side_by_side=1)
    assert pick(r, "ahead_candidate", "path", "ready_mode") == (1, DIRECT, mode)


# ---------------------------------------------------------------- the FIRs on a stream of the library's own
def test_overlap_2(route):
    r = route(overlap=2, ahead_apart=1, side_by_side=1)
    assert pick(r, "under", "own_fir", "ahead_candidate", "probe_on") == (1, 1, 0, ON_FIR_TURN)
    assert pick(r, *ROUTE) == (OWN_FIR, 0, 1, 0, 1, 0, 0, 0)                  # "ready_words" -1: the event
    assert pick(route(overlap=2, ready_words=2, side_by_side=1), *ROUTE) == (OWN_FIR, 2, 0, 0, 0, 1, 0, 0)
    assert pick(route(overlap=2, ready_words=1, side_by_side=1), *ROUTE) == (OWN_FIR, 1, 0, 1, 0, 1, 0, 0)
    assert pick(route(overlap=2, ready_words=2, side_by_side=0), *ROUTE) == (OWN_FIR, 0, 1, 0, 1, 0, 0, 0)
    assert route(overlap=2, fir_ahead=1, ahead_apart=1)["ahead_candidate"] == 0


def test_cu_split(route):
    for forced in (-1, 1):
        r = route(cu_split=16, fir_ahead=forced, ahead_apart=1, side_by_side=1)
        assert pick(r, "own_fir", "ahead_candidate", "probe_on") == (1, 0, ON_FIR_FIRST)
        assert pick(r, *ROUTE) == (OWN_FIR, 2, 0, 0, 0, 0, 0, 0)              # "overlap" 1's default of the ready words
    assert pick(route(cu_split=-16, ahead_apart=1), "own_fir", "ahead_candidate", "path") == (0, 1, STAGED)      # (only the cascades' stream is masked)


# ---------------------------------------------------------------- FIR chains without a cascade
def test_fir_only_chains_order_the_firs_of_two_streams(route):
    """a FIR alone appends its input inside its launch, and the next block's FIR reads it as history: where the FIRs of consecutive
    blocks take two streams in turn -- staged, "overlap" 2 -- each waits for the one before; one stream orders them by itself"""
    assert pick(route(n_fir_only=2, ahead_apart=1), "path", "fir_follows_fir") == (STAGED, 1)
    assert pick(route(n_fir_only=2, fir_ahead=1, n_fir=9, ahead_apart=0), "path", "fir_follows_fir") == (STAGED, 1)
    assert pick(route(n_fir_only=1, overlap=2, ready_words=2, side_by_side=1), "path", "fir_follows_fir") == (OWN_FIR, 1)
    assert pick(route(n_fir_only=1, cu_split=16, side_by_side=1), "path", "fir_follows_fir") == (OWN_FIR, 0)
    assert pick(route(n_fir_only=1, ahead_apart=0, side_by_side=1), "path", "fir_follows_fir") == (DIRECT, 0)
    assert pick(route(n_fir_only=1, overlap=0), "path", "fir_follows_fir") == (BACK_TO_BACK, 0)
    for facts in (dict(ahead_apart=1), dict(overlap=2, side_by_side=1), dict(fir_ahead=1)):
        assert route(**facts)["fir_follows_fir"] == 0           # every chain behind a cascade: FIR k + 1 needs nothing of FIR k


# ---------------------------------------------------------------- "ready_words" by implementation
def test_ready_words_by_implementation(route):
    assert pick(route(ready_words=1, side_by_side=1), "ready_mode", "write_through", "ready_acquire") == (1, 1, 1)
    assert route(ready_words=1, fir_impl=4, side_by_side=1)["ready_mode"] == 0        # only fir_tile takes mode 1
    assert route(ready_words=2, fir_impl=4, side_by_side=1)["ready_mode"] == 2
    for rw in (-1, 0, 1, 2):
        for fl in (-1, 0, 1, 2):
            r = route(fir_impl=3, ready_words=rw, fir_launch=fl, side_by_side=1)
            assert pick(r, *ROUTE) == (DIRECT, 0, 1, 0, 1, 0, 0, 0)
    assert route(ready_words=2, has_ready=0, side_by_side=1)["ready_mode"] == 0
    assert route(ready_words=2, has_timeouts=0, side_by_side=1)["ready_mode"] == 0
    assert route(ready_words=0, side_by_side=1)["ready_mode"] == 0


# ---------------------------------------------------------------- not under at all
@pytest.mark.parametrize("fact", [dict(overlap=0), dict(overlap_ok=0), dict(biquad_impl=0), dict(fir_impl=0)], ids=lambda f: next(iter(f)))
def test_back_to_back(route, fact):
    r = route(fir_ahead=1, ready_words=2, ahead_apart=1, side_by_side=1, **fact)
    assert pick(r, "under", "ahead_candidate") == (0, 0)
    assert pick(r, *ROUTE) == (BACK_TO_BACK, 0, 0, 0, 0, 0, 0, 0)

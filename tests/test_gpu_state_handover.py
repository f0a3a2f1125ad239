"""FIR rings and filter state handed over mid-stream, on the device against the oracle bit for bit: the scripts of
tests/state_scripts.py (its docstring names the steps; tests/test_state_scripts.py proves them oracle against oracle and checks the
ring positions they reach).  What lasts longer than one sequence of calls goes through a few small conversions --
ring_to_state / state_to_ring between the device's rings (read relative to the plan's write position) and the reference's delay
lines, ring_widen and the wide stores of ring_put / biquad_pipe / biquad_row for the operand ring that fir_stream and fir_flow
need, the plans dropped and made again with the position back at 0 -- and a kernel that is right inside a stream of blocks says
nothing about them.  After every step that yields samples the outputs are compared word for word, after every step that reads
state the whole state area.

    A  checkpoints at ring positions 0, 1, 1025, R - 1, R, R + 1, R + T - 1 and behind a 2500-frame block that crosses the ring's
       end; a second Runtime from every checkpoint repeats the ORACLE's next frames and state
    B  uploads at used positions (4000, and 200 in the third lap); Inf / NaN / subnormal words planted at both ends of a delay
       line, once with the operand ring in existence
    C  fir_impl, biquad_impl, fir_rows and fir_lean switched between blocks: the operand ring made from a used ring, and from one
       that has just wrapped, and kept up while the other kernels run
    D  plans made again mid-stream: upload_params with and without an edit, a hop through the interpreter, four sharded blocks,
       dspRuntimeReset at two rates
    E  one-frame calls across the ring's end
    F  the shared-impulse path and fir_tile taking turns on the same rings
    G  format 3 / 5 lane plans, H the int64 cascades: the same hand-overs where there is no ring
    N  fir_tile's window ring (four row tiles, lean boundary) taking turns with fir_mfma, fir_stream, fir_flow, two row tiles and
       fir_plain, a save behind the first block, a load between a fir_stream block and a ring block

Program DEEP (FIRs of 1345, 2753, 4096 and 4097 taps: the ring kernel's column pointer wraps once and twice) runs A, B, D and E with
"fir_rows" 4 and "fir_lean" 1 forced and 1024-frame blocks, so that the ring kernel stands on both sides of every hand-over
(tests/test_fir_ring_reach.py asks fir_choice whether it does).

"fir_split" (a tolerance, not bits), "overlap" and "ready_words" (blocks in flight: tests/test_gpu_sweeps.py) are not switched here."""
import pytest

from avdsp_amd import runtime as rt
from tests import state_scripts as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release():
    yield
    L = rt.lib()
    for key, v in ((b"fir_impl", 1), (b"biquad_impl", 1), (b"fir_rows", 0), (b"fir_lean", -1), (b"fir_shared", 1), (b"lane_hw", 1), (b"generic", 0)):
        L.dspRuntimeSetOption(key, v)
    L.dspRuntimeSetShard(0, 1)
    L.dspRuntimeRelease()


def cases(letter):
    return [c for c in sorted(ss.CASES) if c.startswith(letter + "-")]


def run(case_id):
    prog, script, x = ss.case(case_id)
    ss.play(script, prog.fmt, prog, x, device=True)


@pytest.mark.parametrize("case_id", cases("A"))
def test_checkpoints_at_every_phase_of_the_ring(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("B"))
def test_upload_at_a_used_position(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("C"))
def test_kernel_switches_between_blocks(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("D"))
def test_plans_made_again_mid_stream(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("E"))
def test_one_frame_calls_on_fir_chains(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("F"))
def test_shared_path_and_back(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("G"))
def test_lane_plans(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("H"))
def test_fixed_point(case_id):
    run(case_id)


@pytest.mark.parametrize("case_id", cases("N"))
def test_window_ring_between_the_other_kernels(case_id):
    run(case_id)

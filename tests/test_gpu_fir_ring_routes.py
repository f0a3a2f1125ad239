"""fir_tile's window ring (four row tiles, lean boundary) on every route that launches it, against the oracle bit for
bit.  tests/test_gpu_fir_window_ring.py holds the kernel's arithmetic to the oracle one call after another; what surrounds the
kernel differs by route, and only these cases see it: when the float ring is written relative to the prologue's 22-column fetch
and the later six-column ones (blocks in flight: "overlap", "ready_words", "ring_wait" 0, "fir_launch", staged "fir_ahead" launches),
who wrote the ring (a cascade, fir_append_input, mem_stage), which position a plan starts from and which chains a launch holds
(shards), whether a workgroup's tiles leave together or the plain way (store shapes), which variant ran the block before.

Every case forces "fir_rows" 4 and "fir_lean" 1 (handed launches are lean by rule) and keeps its interesting blocks above 512
frames; tests/test_fir_ring_reach.py asks fir_choice, without a GPU, whether each block then takes the ring kernel -- the cases are
data in tests/fir_ring_cases.py.  Every reference is computed once, shared between the parametrisations and never written."""
import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import fir_ring_cases as rc
from tests.fuzz_programs import stress_input

pytestmark = pytest.mark.gpu

SENT = 0x5EA1AB1E                                    # what unused columns and rows of an output block hold
SLEEP_CYCLES = 5_000_000                             # torch.cuda._sleep: a few milliseconds, far longer than a FIR of these sizes
INF, NINF, NAN, BIGEXP, SUB, NSUB = 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F812345, 0x00000012, 0x80000400
HEAD = 12                                            # program words of the header


@pytest.fixture(autouse=True)
def _options_back():
    """options are process-wide: every case sets what it depends on, and leaves the process as the library ships"""
    rt.lib().dspRuntimeRelease()
    yield
    rt.lib().dspRuntimeRelease()
    for key, v in rc.FLIGHT_DEFAULTS.items():
        rt.Runtime.set_global_option(key, v)
    for key in rc.TREE_OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.Runtime.set_global_option("biquad_impl", 1)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frozen(*arrays):
    for v in arrays:
        v.flags.writeable = False


def differ(got, want, what):
    g, w = words(got), words(want)
    if (g == w).all():
        return
    bad = np.nonzero((g != w).any(axis=0))[0]
    first = int(np.argmax((g != w).any(axis=1)))
    raise AssertionError(f"{what}: columns {bad[:12].tolist()} differ from the oracle, first at frame {first} ({np.count_nonzero(g != w)} words)")


def chain_reference(key, fmt, spec, blocks, x, stores=1, gap=1):
    """program, the oracle's output of every block, its state after every block"""
    if key not in _REF:
        prog, nout = rc.chains_program(fmt, spec, stores, gap)
        o = po.OracleProgram(fmt, prog)
        outs, states = [], []
        for a, n in rc.cut(blocks):
            outs.append(o.run_block(x[a:a + n], nout, nout))
            states.append(o.state.copy())
        frozen(prog, x, *outs, *states)
        _REF[key] = (prog, nout, x, outs, states)
    return _REF[key]


_REF = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# a. blocks in flight
# ---------------------------------------------------------------------------------------------------------------------------------
def flight_input(fmt, stress):
    n, C = sum(rc.FLIGHT_BLOCKS), len(rc.BASE)
    if not stress:
        return pb.lcg_input(n, C, fmt == 6, seed=60 + fmt)
    x = stress_input(np.random.default_rng(4200 + fmt), n, C, fmt == 6)
    if fmt == 6:
        # Inf and NaN where their reach stays finite -- the FIR-only chains -- and, late, in a cascaded one: a tile that met one is
        # summed again from the float ring (exact_tile) while the cascades of later blocks write it
        xv = x.view(np.uint32)
        for f, c, w in ((700, 2, INF), (2100, 6, NAN), (2101, 6, NINF), (5000, 2, BIGEXP), (5001, 2, NAN), (7900, 6, INF), (9500, 2, NINF),
                        (9900, 3, INF), (10200, 6, NAN)):
            xv[f, c] = w
    return x


def flight_reference(fmt, stress):
    key = ("flight", fmt, stress)
    if key not in _REF:
        chain_reference(key, fmt, rc.BASE, rc.FLIGHT_BLOCKS, flight_input(fmt, stress))
    return _REF[key]


FLIGHT_WIDTH = 12                                    # nine chains in a window of twelve words: two workgroups' tiles leave together


def run_flight(fmt, name, stress):
    import torch
    a = rc.FLIGHT[name]
    prog, nout, x, outs, states = flight_reference(fmt, stress)
    C = len(rc.BASE)
    r = rt.Runtime(fmt, prog)
    for k, v in a["opts"].items():
        r.set_option(k, v)
    r.set_option("biquad_impl", 1)
    xd = [dm.to_device(np.ascontiguousarray(x[p:p + n])) for p, n in rc.cut(rc.FLIGHT_BLOCKS)]
    yd = [torch.zeros((n, FLIGHT_WIDTH), dtype=xd[0].dtype, device="cuda") for n in rc.FLIGHT_BLOCKS]
    torch.cuda.synchronize()                                 # the overlap mode's contract: inputs complete when the call is made
    st = torch.cuda.current_stream().cuda_stream
    now = []
    for k, n in enumerate(rc.FLIGHT_BLOCKS):                 # back to back, no host synchronisation
        r.run_block_device(xd[k].data_ptr(), C, nout, yd[k].data_ptr(), FLIGHT_WIDTH, 0, n, st)
        now.append(r.get_option("fir_ahead_now"))
    torch.cuda.synchronize()
    ring = [k for k in range(len(rc.FLIGHT_BLOCKS)) if k in rc.FLIGHT_RING]
    assert [now[k] for k in ring] == [a["staged"]] * len(ring), f"{name}: fir_ahead_now behind the ring blocks reads {now}"
    for k, y in enumerate(yd):
        got = dm.to_host(y)
        differ(got[:, :nout], outs[k], f"{name}, format {fmt}, block {k} of {rc.FLIGHT_BLOCKS[k]} frames")
        assert not words(got[:, nout:]).any(), f"{name}, block {k}: a column outside the chains' was written"
    assert (r.sync_state() == states[-1]).all(), f"{name}, format {fmt}: the state differs from the oracle's"
    assert r.get_option("ready_timeouts") == 0
    r.release()


@pytest.mark.parametrize("fmt", rc.FMTS)
@pytest.mark.parametrize("name", sorted(rc.FLIGHT))
def test_blocks_in_flight(name, fmt):
    """thirteen device-resident blocks enqueued back to back: the float ring wraps under the window while the next blocks' cascades
    write it; 333 and 100 frames take another kernel between ring launches.  Every block's output, the final state, no bounded wait
    ran out, and "fir_ahead_now" says the path the arrangement is listed with (a refused combination: the path the route gives it)"""
    run_flight(fmt, name, False)


@pytest.mark.parametrize("fmt", rc.FMTS)
def test_blocks_in_flight_on_odd_samples(fmt):
    """zeros, full scale, subnormals -- and in format 6 Inf and NaN: exact_tile reads the float ring while later blocks are in flight"""
    run_flight(fmt, rc.FLIGHT_STRESS[fmt], True)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. one output block for every call
# ---------------------------------------------------------------------------------------------------------------------------------
def staged_reference(name, fmt):
    key = ("staged", name, fmt)
    if key not in _REF:
        _, spec, stores, gap = rc.STAGED[name]
        x = pb.lcg_input(sum(rc.STAGED_BLOCKS), len(spec), fmt == 6, seed=77 + len(name))
        chain_reference(key, fmt, spec, rc.STAGED_BLOCKS, x, stores, gap)
    return _REF[key]


@pytest.mark.parametrize("ahead", [1, 0])
@pytest.mark.parametrize("name, fmt", [(n, f) for n, v in rc.STAGED.items() for f in v[0]])
def test_one_output_block_serves_every_call(name, fmt, ahead):
    """"overlap" 1's contract (tests/test_gpu_fir_ahead.py): ONE output block for all five calls, sentinels refilled in stream order in
    front of every call, cloned behind a spin of a few milliseconds -- a FIR that wrote the caller's block early would put block
    k + 1 into clone k.  The base program's tiles leave together (a window of twelve words); two stores per chain and gapped columns
    send them the plain way, and the columns of nobody keep their sentinels"""
    import torch
    _, spec, stores, gap = rc.STAGED[name]
    prog, nout, x, outs, states = staged_reference(name, fmt)
    C = len(spec)
    width = 12 if name == "base" else nout
    stored = np.zeros(width, bool)
    stored[[gap * stores * c + k for c in range(C) for k in range(stores)]] = True
    r = rt.Runtime(fmt, prog)
    for k, v in dict(rc.RING_OPTS, biquad_impl=1, ready_words=-1, overlap=1, fir_ahead=ahead).items():
        r.set_option(k, v)
    assert r.get_option("fir_ahead_now") == 0
    xd = [dm.to_device(x[p:p + n].copy()) for p, n in rc.cut(rc.STAGED_BLOCKS)]
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((1024, width), dtype=torch.int32, device="cuda")
    clones = []
    for k, n in enumerate(rc.STAGED_BLOCKS):
        y.fill_(SENT)
        r.run_block_device(xd[k].data_ptr(), C, nout, y.data_ptr(), width, 0, n, st)
        assert r.get_option("fir_ahead_now") == ahead, f"call {k}"
        torch.cuda._sleep(SLEEP_CYCLES)
        clones.append(y.clone())
    torch.cuda.synchronize()
    for k, c in enumerate(clones):
        got, n = dm.to_host(c).view(np.uint32), rc.STAGED_BLOCKS[k]
        what = f"{name}, format {fmt}, fir_ahead {ahead}, block {k}"
        differ(got[:n, :nout][:, stored[:nout]], words(outs[k])[:, stored[:nout]], what)
        assert (got[:n, ~stored] == SENT).all(), f"{what}: a column of nobody's was written"
        assert (got[n:] == SENT).all(), f"{what}: a frame behind the block was written"
    assert (r.sync_state() == states[-1]).all()
    assert r.get_option("ready_timeouts") == 0
    r.release()


# ---------------------------------------------------------------------------------------------------------------------------------
# c. shards
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", rc.FMTS)
def test_three_shards(fmt):
    """ten chains as shards of 4 / 3 / 3: two launches start at a chain that is no multiple of four and store to unaligned columns.
    Four blocks, each as three calls behind set_shard(rank, 3) over that shard's columns, assembled and compared with the oracle's
    whole block; then the whole program again, on the oracle's state"""
    C, W = len(rc.TEN), rc.SHARD_WORLD
    blocks = rc.SHARD_BLOCKS + [rc.SHARD_WHOLE]
    x = pb.lcg_input(sum(blocks), C, fmt == 6, seed=90 + fmt)
    prog, nout = rc.chains_program(fmt, rc.TEN)
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    for k, v in rc.RING_OPTS.items():
        r.set_option(k, v)
    for k, (p, n) in enumerate(rc.cut(blocks)[:-1]):
        want = o.run_block(x[p:p + n], C, C)
        got = np.zeros((n, C), dtype=x.dtype)
        for rank in range(W):
            r.set_shard(rank, W)
            info = r.shard_info()
            lo, m = info["first_chain"], info["nchains"]
            assert (lo, m) == rc.shard_range(C, W, rank)
            got[:, lo:lo + m] = r.run_block(np.ascontiguousarray(x[p:p + n, lo:lo + m]), m, C + lo, lo)
        differ(got, want, f"format {fmt}, block {k} of {n} frames in {W} shards")
    r.set_shard(0, 1)
    assert (r.sync_state() == o.state).all(), "the state behind the sharded blocks differs from the oracle's"
    r.state[:] = o.state
    r.upload_state()
    p, n = rc.cut(blocks)[-1]
    differ(r.run_block(x[p:p + n], C, C), o.run_block(x[p:p + n], C, C), f"format {fmt}, the whole block behind the shards")
    assert (r.sync_state() == o.state).all()
    r.release()


# ---------------------------------------------------------------------------------------------------------------------------------
# d. memory-word trees
# ---------------------------------------------------------------------------------------------------------------------------------
def tree_program(fmt, odd=False):
    from tests import firtree_programs as tp
    items = rc.tree_items()
    if odd:
        # the samples reach the rings as they are placed: trunk "b" a plain LOAD without sections (its word is the input sample, its
        # branches' rings are fed with it), the handed chain a FIR alone behind a LOAD
        items[4] = tp.trunk("b", 0, 0, None)
        items[rc.TREE_HANDED] = tp.plain(nsec=0, taps=4096, slot="B", form="fixed", us=300, finish="tpdf", load_gain=None)
    c = tp.core(items, calc=0)
    prog, nin, nout, wd = tp.program(fmt, [c])
    return c, prog, nin, nout


def run_tree(fmt, c, prog, nout, x, blocks, what):
    from tests import firtree_programs as tp
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=24)
    for key in rc.TREE_OPTIONS:
        r.set_option(key, 1)
    for k, v in rc.RING_OPTS.items():
        r.set_option(k, v)
    # what the program holds: every item a chain; one trunk with a FIR, four branches with one, one of them handed; two handed FIR
    # chains in all (the branch and the ordinary chain), both with a delay; two trees, five branches
    assert r.core_info(0)["chains"] == len(c["items"]) == 8, r.last_error()
    assert r.mem_fir_info(0) == tp.fir_counts(c) == (1, 4, 1)
    assert r.fir_tail_info(0) == tp.tail_counts(c) == (2, 2)
    assert r.mem_info(0) == tp.mem_counts(c)
    assert r.core_info(0)["max_taps"] == 4097
    total = int(prog[1])
    for k, (p, n) in enumerate(rc.cut(blocks)):
        want = o.run_block(x[p:p + n], nout, tp.IN)
        got = r.run_block(x[p:p + n], nout, tp.IN)
        w = f"{what}, block {k} of {n} frames"
        differ(got, want, w)
        bad = np.nonzero(r.sync_state() != o.state)[0]
        assert bad.size == 0, f"{w}: {bad.size} words of the state area differ, first {bad[:6].tolist()}"
        bad = np.nonzero(r.buf[HEAD:total] != o.buf[HEAD:total])[0]
        assert bad.size == 0, f"{w}: {bad.size} program words (the memory words among them) differ, first {bad[:6].tolist()}"
    r.release()


@pytest.mark.parametrize("fmt", rc.FMTS)
def test_memory_word_trees(fmt):
    """the trunks' FIR launch (4096 taps), the plain launch of three branches that are a FIR alone -- their float rings written by
    mem_stage, not by a cascade -- and the handed launch (a 1345-tap branch with a DELAY and SAT0DB_TPDF_GAIN, an ordinary 4096-tap
    chain): three ring launches per block; outputs, state and memory words after every block"""
    c, prog, nin, nout = tree_program(fmt)
    assert nin == 3
    x = pb.lcg_input(sum(rc.TREE_BLOCKS), nin, fmt == 6, seed=50 + fmt)
    run_tree(fmt, c, prog, nout, x, rc.TREE_BLOCKS, f"format {fmt}")


def test_memory_word_trees_odd_samples():
    """format 6.  Column D of a tile at frame p holds frames p - 3 + 64 (16 - D) + row (tests/test_gpu_fir_window_ring.py): subnormals
    under the tile at frame 3072 and Inf / NaN under the one at 6144, in columns the prologue stages (D = 3, 20), in columns staged at
    a later boundary (30, 50) and in the mirrored column (0, 22, 44) -- of the handed 4096-tap chain and of the ring-fed 4097- and
    1409-tap branches.  The first Inf lies at frame 3970: the tile at 3072 sums finite samples but for its last frames"""
    blocks = [1024] * 7
    c, prog, nin, nout = tree_program(6, odd=True)
    n = sum(blocks)
    x = pb.lcg_input(n, nin, True, seed=31).copy()
    xv = x.view(np.uint32)

    def col(p, D, rows):
        return [p - 3 + 64 * (16 - D) + r for r in rows]

    for p, kinds in ((3072, (SUB, NSUB)), (6144, (INF, NAN, BIGEXP, NINF, SUB, NSUB))):
        prologue = col(p, 3, (0, 31, 63)) + col(p, 20, (1, 62))
        later = col(p, 30, (0, 40, 63)) + col(p, 50, (5, 63))
        mirrored = col(p, 0, (0, 1, 2)) + col(p, 22, (0, 33, 63)) + col(p, 44, (7, 63))
        for ch, shift in ((1, 0), (2, 1)):               # input 1: trunk "b" (the ring-fed branches), input 2: the handed chain
            for i, f in enumerate(prologue + later + mirrored):
                assert 0 <= f < n
                xv[f, ch] = kinds[(i + shift) % len(kinds)]
    assert min(col(6144, 50, (5,))) == 3970
    run_tree(6, c, prog, nout, x, blocks, "format 6, odd samples")


def test_signalling_nan_behind_a_plain_load():
    """format 6, what the odd samples above found: a FIR alone behind a plain LOAD keeps (float)(double)sample, and the reference's
    conversion has quieted a signalling NaN on the way -- dspMulFloatDouble reads another mantissa from 0x7FC12345 than from
    0x7F812345.  A LOAD and a LOAD_GAIN chain, plain launches of the ring kernel, outputs and the delay lines in the state"""
    from tests import firtree_programs as tp
    c = tp.core([tp.plain(nsec=0, taps=1345, finish="none", load_gain=None), tp.plain(nsec=0, taps=380, finish="sat", load_gain=1.0)])
    prog, nin, nout, _ = tp.program(6, [c])
    blocks = [1024, 600]
    x = pb.lcg_input(sum(blocks), nin, True, seed=7).copy()
    xv = x.view(np.uint32)
    for f, w in ((5, BIGEXP), (700, 0xFF800001), (1023, 0x7FBFFFFF), (1024, BIGEXP), (1500, 0xFFA00000)):
        xv[f, :] = w
    o = po.OracleProgram(6, prog, fs=48000, random=1, dither=24)
    r = rt.Runtime(6, prog, fs=48000, random=1, dither=24)
    for k, v in rc.RING_OPTS.items():
        r.set_option(k, v)
    assert r.core_info(0)["chains"] == 2, r.last_error()
    for k, (p, n) in enumerate(rc.cut(blocks)):
        differ(r.run_block(x[p:p + n], nout, tp.IN), o.run_block(x[p:p + n], nout, tp.IN), f"block {k}")
        assert (r.sync_state() == o.state).all(), f"block {k}: the state (the delay lines among it) differs from the oracle's"
    r.release()

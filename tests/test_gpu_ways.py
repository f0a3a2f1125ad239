"""Two-way COPYXY / SWAPXY forks and runs of GAIN / NEGX on the chain kernels ("chain_ways" 1): a fork's ways as two
chains of the cascades, the FIR and chain_tail; the runs in chain_tail's OPS form.  Every case is held to the oracle bit for bit after
each block -- the whole output block over a sentinel, the whole state area and the program words behind the header; each first asserts
through ways_info() and core_info() that its chains are lowered.  The sizes are the smallest that reach each seam: 2, 16, 17 and 34
ways in a core (a 16-lane row and its neighbour), 0, 1, 16 and 17 sections in a way (no cascade, a row, a piece boundary), blocks of
1, 2, 64, 65, 1024 and 1029 frames (one frame, a wave, a second launch)."""
import os

import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import ways_programs as wp
from tests.fuzz_programs import stress_input
from tests.lowered_programs import sentinel

pytestmark = pytest.mark.gpu
IN = wp.IN
HEAD = 12                                            # program words of the header (its checksum covers them alone)
BLOCKS = [1, 2, 64, 65, 1024, 1029]
SHORT = [65, 2, 1029]
SECS = [0, 1, 16, 17]
OPTIONS = ("chain_ways", "chain_finish", "chain_delay", "fir_tail", "chain_mem", "mem_fir", "shard_trees")
# (gains that are no powers of two: in format 2 a GAIN multiplies by the raw Q4.28 word, and 0.5 would shift every stored bit out)
OPS = [[("gain", 0.7)], ["neg"], [("gain", -1.3), "neg"], ["neg", ("gain", 1.0)], [("gain", 0.9), "neg", ("gain", -0.6), "neg"], [("gain", 0.0)]]
US = [20, 63, 1000, 25000]                           # lines of 0 (bypass), 3, 47 and 1199 samples: none, fewer than a block's, more than a block's


@pytest.fixture(autouse=True)
def _options_back():
    yield
    for key in OPTIONS:
        rt.Runtime.set_global_option(key, 0)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    g, w = words(got), words(want)
    bad = np.nonzero((g != w).any(axis=0))[0]
    assert bad.size == 0, (f"{what}: outputs {bad[:8].tolist()} differ, first frame "
                           f"{np.nonzero(g[:, bad[0]] != w[:, bad[0]])[0][:3].tolist()}: "
                           f"{g[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()} for {w[:, bad[0]][g[:, bad[0]] != w[:, bad[0]]][:2].tolist()}")


def same_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:6].tolist()}"


def cut(blocks):
    return list(zip(np.cumsum([0] + blocks[:-1]).tolist(), blocks))


def the_input(fmt, frames, nin, seed):
    """full-scale and beyond, zeros, tiny values: the int64 model's products wrap (tests/fuzz_programs.py)"""
    return stress_input(np.random.default_rng(seed), frames, nin, fmt in (5, 6))


def ways_runtime(fmt, prog, dither=24, ways=1):
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=dither)
    assert r.rc >= 0
    for key in OPTIONS[1:6]:
        r.set_option(key, 1)
    r.set_option("chain_ways", ways)                          # (unknown to the code before this option existed: every test here fails there)
    return r


def lowered(r, cores):
    """every core's chains are on the chain kernels: each way counted"""
    for k, c in enumerate(cores):
        info, chains = wp.counts(c)
        assert r.core_info(k)["chains"] == chains, r.last_error()
        assert r.ways_info(k) == info, r.last_error()


def compare_block(r, o, got, want, total, what):
    same(got, want, what)
    same_words(r.sync_state(), o.state, what + ", state area")
    same_words(r.buf[HEAD:total], o.buf[HEAD:total], what + ", program words")


def play(fmt, cores, blocks=BLOCKS, run="run_block", seed=7, dither=24, prog=None):
    """the program block by block against the oracle; -> (runtime, oracle, input, outputs) for the tests that go on"""
    if prog is None:
        prog, nin, nout, _ = wp.program(fmt, cores)
    else:
        prog, nin, nout = prog
    x = the_input(fmt, sum(blocks), nin, seed)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
    r = ways_runtime(fmt, prog, dither)
    lowered(r, cores)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        got = getattr(r, run)(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        compare_block(r, o, got, want, total, f"format {fmt}, {run}, block {k} of {b} frames")
    return r, o, x, nout


def plain_forks(nways, k=0):
    """nways ways: forks (an ordinary chain last when the count is odd), sections 0, 1, 16, 17 mixed over the ways, LOAD and LOAD_GAIN heads,
    SAT0DB or nothing in front of one or two STOREs"""
    def w(j):
        return wp.way(nsec=SECS[(j + k) % 4], finish=("sat", "none")[(j // 4) % 2], stores=2 if j % 5 == 3 else 1)
    items = [wp.fork(wp.head(None if j % 3 == 0 else 0.4 + 0.01 * j), w(2 * j), w(2 * j + 1)) for j in range(nways // 2)]
    if nways % 2:
        items.append(wp.chain(nsec=SECS[(nways + k) % 4], load_gain=0.7))
    return items


@pytest.mark.parametrize("fmt", [2, 3, 4, 5, 6])
def test_plain_forks(fmt):
    """cores of 2, 16, 17 and 34 ways"""
    cores = [wp.core(plain_forks(n, k)) for k, n in enumerate((2, 16, 17, 34))]
    assert {w["nsec"] for c in cores for it in c["items"] for w in it["ways"]} == set(SECS)
    play(fmt, cores)[0].release()


def dressed_forks(fmt):
    """dressed finishes; a DELAY in slot A and in slot B, fixed and with a parameter, lines of 0, 3, 47 and 1199 samples; a FIR of 33 taps in
    one way (formats 4 and 6); a LOAD_MEM head; beside ordinary, delayed and tree chains"""
    fin = ["tpdf", "gain", "tpdf_gain", "sat", "none"]
    items = []
    for j in range(8):
        a = wp.way(nsec=SECS[j % 4], slot="AB"[j % 2], form=("fixed", "param")[(j // 2) % 2], us=US[j % 4], max_us=max(US[j % 4], 50), finish=fin[j % 5], gain=0.9 + 0.01 * j)
        b = wp.way(nsec=SECS[(j + 1) % 4], slot=(None, "A", "B")[j % 3], us=US[(j + 2) % 4], finish=fin[(j + 2) % 5], gain=0.8, stores=1 + j % 2)
        if a["slot"] == "B" and a["finish"] == "none":
            a["finish"] = "sat"                               # (slot B is behind a SAT0DB slot that holds an opcode)
        if b["slot"] == "B" and b["finish"] == "none":
            b["finish"] = "sat"
        items.append(wp.fork(wp.head(None if j % 2 else 0.6), a, b))
    if fmt != 2:
        items.append(wp.fork(wp.head(0.5), wp.way(nsec=1, taps=33, finish="sat"), wp.way(nsec=2, finish="tpdf")))
        items.append(wp.fork(wp.head(None), wp.way(nsec=0, finish="sat"), wp.way(nsec=0, taps=33, slot="A", us=63, finish="tpdf_gain")))
    items += [wp.trunk("a", 2), wp.fork(wp.head(key="a"), wp.way(nsec=1, finish="tpdf"), wp.way(nsec=0, slot="A", us=1000, finish="sat")),
              wp.chain(key="a", nsec=0), wp.trunk("b", 0, None), wp.fork(wp.head(key="b"), wp.way(nsec=0), wp.way(nsec=17, finish="gain")),
              wp.fork(wp.head(key="w"), wp.way(nsec=0, finish="none"), wp.way(nsec=1)),
              wp.chain(nsec=2), wp.chain(nsec=1, slot="A", us=1000, finish="tpdf"), wp.chain(nsec=0, finish="tpdf_gain")]
    return items


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_dressed_delayed_fir_and_tree_forks(fmt):
    c = wp.core(dressed_forks(fmt), calc=0)
    prog, nin, nout, wd = wp.program(fmt, [c])
    wp.set_word(prog, wd["w"], -0.37, fmt)                    # (a word nobody writes: a constant branch twice)
    r = play(fmt, [c], prog=(prog, nin, nout))[0]
    assert r.mem_info() == (2, 7, 2) and r.delay_info()[1] == wp.samples(25000) and r.fir_tail_info() == ((1, 1) if fmt != 2 else (0, 0))
    r.release()


def ops_items():
    """runs of 1, 2 and 4 (gains of 0, 1.0 and negative ones among them): behind 0, 1, 16 and 17 sections, with and without a delay and a
    dressed finish, in the ways of forks, on branches without sections; ordinary chains beside them"""
    fin = ["sat", "tpdf", "none", "tpdf_gain", "gain"]
    items = []
    for j in range(12):
        slot = (None, "A", "B")[j % 3]
        f = fin[j % 5] if not (slot == "B" and fin[j % 5] == "none") else "sat"
        items.append(wp.chain(nsec=SECS[j % 4], ops=OPS[j % 6], slot=slot, form=("fixed", "param")[(j // 3) % 2], us=US[(j + 1) % 4], max_us=max(US[(j + 1) % 4], 50),
                              finish=f, gain=0.95, load_gain=None if j % 2 else 0.8, stores=1 + (j % 4 == 3)))
    items += [wp.fork(wp.head(0.8), wp.way(nsec=2, finish="tpdf", slot="B", us=1000), wp.way(nsec=2, ops=[("gain", 0.7)], finish="tpdf_gain")),
              wp.fork(wp.head(None), wp.way(nsec=0, ops=OPS[4]), wp.way(nsec=16, ops=OPS[2], finish="none")),
              wp.trunk("a", 1), wp.chain(key="a", nsec=0, ops=OPS[4], finish="tpdf"), wp.chain(key="a", nsec=0), wp.chain(key="a", nsec=1, ops=["neg"]),
              wp.fork(wp.head(key="a"), wp.way(nsec=0, ops=[("gain", -0.5)]), wp.way(nsec=0, ops=OPS[1], slot="A", us=63)),
              wp.trunk("b", 0), wp.chain(key="b", nsec=0, ops=OPS[3], finish="none"),
              wp.chain(nsec=1), wp.chain(nsec=0), wp.chain(nsec=2, slot="A", us=63, finish="sat")]
    return items


@pytest.mark.parametrize("dither", [24, 16])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_ops_runs(fmt, dither):
    c = wp.core(ops_items(), calc=0)
    assert {len(w["ops"]) for it in c["items"] for w in it["ways"]} == {0, 1, 2, 4}
    r = play(fmt, [c], dither=dither)[0]
    assert r.ways_info() == (3, 20)
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_int64_wrap_is_reached(fmt):
    """full-scale samples through LOAD_GAIN 7.9, gains of 7.9 and -7.9: in format 2 the 64 x 32 product wraps"""
    c = wp.core([wp.chain(nsec=0, ops=[("gain", 7.9), ("gain", -7.9), "neg", ("gain", 7.9)], load_gain=7.9, finish="none"),
                 wp.chain(nsec=1, ops=[("gain", 7.9), ("gain", 7.9)], load_gain=7.9)])
    prog, nin, nout, _ = wp.program(fmt, [c])
    x = the_input(fmt, 64, nin, 3)
    if fmt == 2:                                              # the oracle's own product, without the wrap, leaves 63 bits
        big = int(np.abs(x.astype(np.int64)).max()) * int(7.9 * (1 << 28)) ** 4
        assert big >> 63
    play(fmt, [c], blocks=[64, 65])[0].release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_and_on_again_across_a_block(fmt):
    c = wp.core(ops_items(), calc=0)
    prog, nin, nout, _ = wp.program(fmt, [c])
    blocks = [65, 64, 2, 1029]
    x = the_input(fmt, sum(blocks), nin, 11)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = ways_runtime(fmt, prog)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        on = k != 1
        r.set_option("chain_ways", int(on))
        assert r.core_info()["chains"] == (wp.counts(c)[1] if on else 0) and r.ways_info() == (wp.counts(c)[0] if on else (0, 0))
        want = o.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        got = r.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        compare_block(r, o, got, want, total, f"format {fmt}, block {k}, chain_ways {int(on)}")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_run_block_all_and_two_cores(fmt):
    """a writer core and a reader core whose forks start from the writer's words; run_block_all arranges them"""
    c1 = wp.core([wp.trunk("l", 2), wp.trunk("r", 0, None), wp.fork(wp.head(0.5), wp.way(nsec=1, ops=["neg"]), wp.way(nsec=0))], calc=0)
    c2 = wp.core([wp.fork(wp.head(key="l"), wp.way(nsec=1, finish="tpdf"), wp.way(nsec=0, ops=[("gain", 0.5)], slot="A", us=1000)),
                  wp.fork(wp.head(key="r"), wp.way(nsec=0), wp.way(nsec=17, ops=OPS[4], finish="gain"))])
    play(fmt, [c1, c2], blocks=SHORT, run="run_block_all")[0].release()
    play(fmt, [c1, c2], blocks=SHORT, run="run_block")[0].release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_an_in_place_device_call(fmt):
    """one [frames][io] block in device memory as both windows: way B loads its input again behind way A's stores"""
    import torch
    c = wp.core(ops_items() + plain_forks(4), calc=0)
    prog, nin, nout, _ = wp.program(fmt, [c])
    W = IN + nin
    x = the_input(fmt, sum(SHORT), nin, 23)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = ways_runtime(fmt, prog)
    lowered(r, [c])
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(SHORT)):
        frame = sentinel(fmt, (b, W))
        frame[:, IN:IN + nin] = x[a:a + b]
        want = frame.copy()
        o.run_block(want, W, 0, 0, out=want)
        d = dm.to_device(frame)
        r.run_block_device(d.data_ptr(), W, 0, d.data_ptr(), W, 0, b, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        compare_block(r, o, dm.to_host(d), want, total, f"format {fmt}, in place, block {k} of {b} frames")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_an_edited_gain_reaches_the_next_block(fmt):
    c = wp.core([wp.chain(nsec=1, ops=[("gain", 0.5), "neg"]), wp.fork(wp.head(0.9), wp.way(nsec=0), wp.way(nsec=2, ops=[("gain", 0.25)], finish="tpdf_gain"))], calc=0)
    r, o, x, nout = play(fmt, [c], blocks=[65])
    prog2 = wp.program(fmt, [wp.core([wp.chain(nsec=1, ops=[("gain", -0.75), "neg"]), wp.fork(wp.head(0.9), wp.way(nsec=0), wp.way(nsec=2, ops=[("gain", 1.5)], finish="tpdf_gain"))], calc=0)])[0]
    at = wp.gain_words(prog2)
    assert len(at) == 2 and all(o.buf[w] != prog2[w] for w in at)
    for w in at:                                              # the edit goes into both program copies
        o.buf[w] = prog2[w]
        r.buf[w] = prog2[w]
    r.upload_params()
    xb = the_input(fmt, 64, x.shape[1], 5)
    want = o.run_block(xb, nout, IN, out=sentinel(fmt, (64, nout)))
    got = r.run_block(xb, nout, IN, out=sentinel(fmt, (64, nout)))
    compare_block(r, o, got, want, int(prog2[1]), f"format {fmt}, behind the edit")


@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_shard_over_a_block(fmt, rank):
    """rank of 3 for the second block: its ways' columns alone, then the whole program again from the oracle's state"""
    items = plain_forks(6) + [wp.chain(nsec=1, ops=OPS[4], slot="A", us=63), wp.fork(wp.head(0.5), wp.way(nsec=1, ops=["neg"]), wp.way(nsec=0, slot="B", us=1000))]
    c = wp.core(items)
    prog, nin, nout, _ = wp.program(fmt, [c])
    stores = [w["stores"] for it in items for w in it["ways"]]
    first = np.cumsum([0] + stores).tolist()
    x = the_input(fmt, sum(SHORT), nin, 31)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = ways_runtime(fmt, prog)
    lowered(r, [c])
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(SHORT)):
        want = o.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        if k == 1:
            r.set_shard(rank, 3)
            s = r.shard_info()
            assert s["total_chains"] == len(stores) == 9 and s["nchains"] == 3
            mine = range(s["first_chain"], s["first_chain"] + s["nchains"])
            cols = {col for ch in mine for col in range(first[ch], first[ch + 1])}
            other = [col for col in range(nout) if col not in cols]
            want[:, other] = sentinel(fmt, (b, len(other)))
        got = r.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        same(got, want, f"format {fmt}, rank {rank}, block {k}")
        if k == 1:                                            # a shard moves its chains' state alone: the rest comes from the oracle
            st = r.sync_state()
            moved = st != before
            assert (st[moved] == o.state[moved]).all(), "a shard's state words are the oracle's"
            r.set_shard(0, 1)
            r.state[:] = o.state
            r.upload_state()
        else:
            same_words(r.sync_state(), o.state, f"format {fmt}, block {k}, state area")
            same_words(r.buf[HEAD:total], o.buf[HEAD:total], f"format {fmt}, block {k}, program words")
        before = r.sync_state().copy()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_checkpoint_into_a_fresh_runtime(fmt):
    c = wp.core(ops_items(), calc=0)
    r, o, x, nout = play(fmt, [c], blocks=[65, 1029])
    total = int(o.buf[1])
    state, now = r.sync_state().copy(), r.buf[:total].copy()
    r.release()
    r2 = ways_runtime(fmt, now)
    r2.state[:] = state
    r2.upload_state()
    lowered(r2, [c])
    keep = o.state.copy()                                     # the oracle: reset (the generator starts again, as the fresh runtime's), its state put back
    assert o.reset(48000, 1, 24) >= 0
    o.state[:] = keep
    for k, b in enumerate((64, 1029)):
        xb = the_input(fmt, b, x.shape[1], 40 + k)
        want = o.run_block(xb, nout, IN, out=sentinel(fmt, (b, nout)))
        got = r2.run_block(xb, nout, IN, out=sentinel(fmt, (b, nout)))
        compare_block(r2, o, got, want, total, f"format {fmt}, behind the checkpoint, block {k}")


def test_crossoverLV6_second_core_on_the_chain_kernels():
    """tests/golden/crossoverLV6.bin with "chain_finish" and "chain_ways": its second core is LOAD_GAIN, COPYXY, BIQUADS, SAT0DB_TPDF, STORE,
    SWAPXY, BIQUADS, SAT0DB_TPDF, STORE (crossoverLV6.c:54-62) -- one fork; its first core has a SUBYX and a GAIN in front of the banks and
    stays with the interpreter"""
    prog = np.fromfile(os.path.join(os.path.dirname(__file__), "golden", "crossoverLV6.bin"), dtype=np.uint32)
    o = po.OracleProgram(2, prog, fs=48000, random=9, dither=24)
    r = rt.Runtime(2, prog, fs=48000, random=9, dither=24)
    r.set_option("chain_finish", 1)
    r.set_option("chain_ways", 1)
    assert len(r.cores) == 2
    assert r.core_info(1)["chains"] == 2 and r.ways_info(1) == (1, 0) and r.finish_info(1) == (2, 0), r.last_error()
    assert r.core_info(0)["chains"] == 0 and r.ways_info(0) == (0, 0) and "is not lowered to the HIP path" in r.last_error()
    r.set_option("profile", 1)
    try:
        total = int(prog[1])
        for k, (a, b) in enumerate(cut(SHORT)):
            x = the_input(2, b, 8, 50 + k)
            want = o.run_block(x, 8, 16, 24, scratch_len=40)     # inputs IO 16..23, outputs IO 24..31 (tests/test_gpu_edge.py's C host)
            r.kernel_time(0)
            got = r.run_block_all(x, 8, 16, 24)
            assert r.kernel_time(0)[1] >= 1                      # (the cascades' timer: core 1 ran on biquad kernels)
            compare_block(r, o, got, want, total, f"crossoverLV6, block {k}")
    finally:
        r.set_option("profile", 0)

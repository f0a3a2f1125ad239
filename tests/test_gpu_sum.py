"""Sum heads on the chain kernels ("chain_sum" 1): LOAD_MEM, (LOAD_MEM, ADDXY | SUBXY)+ as a tree of its own in
mem_stage's SUM form, and behind it whatever a branch may be.  Every case is held to the oracle bit for bit after each block -- the
whole output block over a sentinel, the whole state area and the program words behind the header; each first asserts through
sum_info(), mem_info(), ways_info() and core_info() that its chains are lowered.  The sizes are the smallest that reach each seam:
buses of 2, 3 and 8 words, operand trunks of 0, 1, 16 and 17 sections, heads of 0, 1 and 17, 15 to 17 sum trees behind 3 word trees
(mem_stage's tile of 16), blocks of 1, 2, 63, 64, 65, 1024 and 1029 frames (the stage's 64-frame workgroups, a second launch)."""
import os

import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests import sum_programs as sp
from tests.fuzz_programs import stress_input
from tests.golden import make_sum_goldens as mg
from tests.golden_recipes import GOLDEN_DIR
from tests.lowered_programs import sentinel

pytestmark = pytest.mark.gpu
IN = sp.IN
HEAD = 12                                            # program words of the header (its checksum covers them alone)
BLOCKS = [1, 2, 63, 64, 65, 1024, 1029]
SHORT = [65, 2, 1029]
OPTIONS = ("chain_sum", "chain_finish", "chain_delay", "fir_tail", "chain_mem", "mem_fir", "chain_ways", "shard_trees")
US = [20, 63, 1000]                                  # lines of 0 (bypass), 3 and 47 samples
MIXED = ["ADDXY", "SUBXY", "SUBXY", "ADDXY", "SUBXY", "ADDXY", "ADDXY"]


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
    """full-scale and beyond, zeros, tiny values: the int64 model's sums wrap (tests/fuzz_programs.py)"""
    return stress_input(np.random.default_rng(seed), frames, nin, fmt in (5, 6))


def sum_runtime(fmt, prog, dither=24, sum_=1):
    r = rt.Runtime(fmt, prog, fs=48000, random=1, dither=dither)
    assert r.rc >= 0
    for key in OPTIONS[1:7]:
        r.set_option(key, 1)
    r.set_option("chain_sum", sum_)                           # (unknown to the code before this option existed: every test here fails there)
    return r


def lowered(r, cores):
    """every core's chains are on the chain kernels: each head one chain and one branch"""
    for k, c in enumerate(cores):
        sums, ways, mem, chains = sp.counts(c)
        assert r.core_info(k)["chains"] == chains, r.last_error()
        assert r.sum_info(k) == sums and r.ways_info(k) == ways and r.mem_info(k)[:2] == mem, r.last_error()


def compare_block(r, o, got, want, total, what):
    same(got, want, what)
    same_words(r.sync_state(), o.state, what + ", state area")
    same_words(r.buf[HEAD:total], o.buf[HEAD:total], what + ", program words")


def constants(fmt, prog, wd, values):
    """the words nobody writes: {key: a value, or the 64 bits of one}"""
    for key, v in values.items():
        if isinstance(v, int):
            sp.set_word_bits(prog, wd[key], v, fmt)
        else:
            sp.set_word(prog, wd[key], v, fmt)


def play(fmt, cores, blocks=BLOCKS, run="run_block", seed=7, dither=24, prog=None, values=None, check=lowered):
    """the program block by block against the oracle; -> (runtime, oracle, input, outputs) for the tests that go on"""
    if prog is None:
        prog, nin, nout, wd = sp.program(fmt, cores)
        prog = prog.copy()
        constants(fmt, prog, wd, values if values is not None else {k: -0.37 for k in ("w",) if k in wd})
    else:
        prog, nin, nout = prog
    x = the_input(fmt, sum(blocks), nin, seed)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=dither)
    r = sum_runtime(fmt, prog, dither)
    check(r, cores)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        want = o.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        got = getattr(r, run)(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        compare_block(r, o, got, want, total, f"format {fmt}, {run}, block {k} of {b} frames")
    return r, o, x, nout


def trunks():
    """operand trunks: a LOAD_GAIN and a LOAD without sections, then 1, 16 and 17 sections; "w" is a word nobody writes"""
    return [sp.trunk("a", 0, 0.8), sp.trunk("b", 0, None), sp.trunk("c", 1, 0.6), sp.trunk("d", 16, None), sp.trunk("e", 17, 0.7)]


def bus_items():
    """2, 3 and 8 words; ADDXY, SUBXY and mixed; one word twice; heads of 0, 1 and 17 sections; a head without sections stored plain (with
    and without SAT0DB, twice) and dressed -- the stage's own stores"""
    return trunks() + [
        sp.bus(["a", "b"], ["ADDXY"], nsec=0, finish="none"),
        sp.bus(["c", "d"], ["SUBXY"], nsec=0, finish="sat", stores=2),
        sp.bus(["e", "a", "w"], ["SUBXY", "ADDXY"], nsec=0, finish="tpdf_gain", gain=0.9),
        sp.bus(["c", "c"], ["SUBXY"], nsec=0, finish="tpdf"),
        sp.bus(["a", "b", "c", "d", "e", "w", "a", "c"], MIXED, nsec=1),
        sp.bus(["w", "e", "d", "c", "b", "a", "w", "w"], ["ADDXY"] * 7, nsec=17, finish="gain"),
        sp.bus(["d", "w"], ["ADDXY"], nsec=1, finish="none"),
        sp.bus(["b", "a", "e"], ["SUBXY", "SUBXY"], nsec=17, finish="tpdf"),
        sp.chain(key="c", nsec=1), sp.chain(key="a", nsec=0), sp.chain(nsec=2)]


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_buses_of_2_3_and_8_words(fmt):
    c = sp.core(bus_items(), calc=0)
    r = play(fmt, [c])[0]
    assert r.sum_info() == (8, 30) and r.mem_info() == (5, 10, 0)
    r.release()


def delayed_items():
    """a DELAY in slot A and in slot B, fixed and with a parameter, lines of 0, 3 and 47 samples, behind heads of 0 and 1 sections; "n" is NaN
    and "i" +Inf in the float models: a slot-A line keeps to_sp of the sum"""
    items = trunks()[:3]
    for j in range(6):
        slot = "AB"[j % 2]
        items.append(sp.bus([["a", "b"], ["c", "n"], ["i", "a", "c"]][j % 3], [["ADDXY"], ["SUBXY"], ["SUBXY", "ADDXY"]][j % 3], nsec=j // 3, slot=slot,
                            form=("fixed", "param")[(j // 2) % 2], us=US[j % 3], max_us=max(US[j % 3], 50), finish=("sat", "tpdf", "none")[j % 3] if slot == "A" else ("sat", "tpdf_gain")[j % 2]))
    items.append(sp.bus(["n", "n2"], ["ADDXY"], nsec=0, slot="A", us=63, finish="none"))
    return items


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_delay_lines_behind_the_head(fmt):
    c = sp.core(delayed_items(), calc=0)
    values = {"n": 0.25, "n2": -0.125, "i": 0.5} if fmt == 2 else {"n": mg.NAN_A, "n2": mg.NAN_B, "i": mg.PINF}
    r = play(fmt, [c], values=values)[0]
    assert r.delay_info() == (7, sp.wp.samples(1000))
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_gain_negx_runs_and_a_lone_fir_behind_the_head(fmt):
    items = trunks()[:3] + [sp.bus(["a", "c"], ["ADDXY"], nsec=0, way_ops=[("gain", 0.7), "neg"]),
                            sp.bus(["b", "w", "c"], ["SUBXY", "ADDXY"], nsec=1, way_ops=["neg", ("gain", -1.3)], slot="A", us=63, finish="tpdf"),
                            sp.bus(["c", "a"], ["SUBXY"], nsec=0, way_ops=[("gain", 0.9)], finish="tpdf_gain")]
    if fmt != 2:
        items += [sp.bus(["a", "b"], ["SUBXY"], nsec=0, taps=33), sp.bus(["c", "w"], ["ADDXY"], nsec=0, taps=33, slot="A", us=63, finish="tpdf")]
    r = play(fmt, [sp.core(items, calc=0)], blocks=SHORT + [64])[0]
    assert r.mem_fir_info() == ((0, 2, 1) if fmt != 2 else (0, 0, 0))
    r.release()


@pytest.mark.parametrize("fmt", [4, 6])
def test_a_fir_trunk_as_an_operand(fmt):
    """"mem_fir": a trunk whose FIR's HAND launch fills the row a term reads"""
    items = [sp.raw([("load", 0.5), ("biquads", 1), ("fir", 33), ("store_mem", "f")]), sp.raw([("load", None), ("fir", 16), ("store_mem", "g")]), sp.trunk("a", 0),
             sp.bus(["f", "a"], ["ADDXY"], nsec=0), sp.bus(["g", "f", "g"], ["SUBXY", "ADDXY"], nsec=1, finish="tpdf")]

    def check(r, cores):
        assert r.sum_info() == (2, 5) and r.mem_info() == (3, 2, 0) and r.mem_fir_info()[0] == 2 and r.core_info()["chains"] == 5, r.last_error()
    play(fmt, [sp.core(items, calc=0)], blocks=SHORT + [64], check=check)[0].release()


@pytest.mark.parametrize("n", [15, 16, 17])
@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_sum_trees_across_the_tile_seam(fmt, n):
    """3 word trees (two trunks and a constant branch), then n buses: mem_stage's tile of 16 trees closes inside the sum trees"""
    items = [sp.trunk("a", 1, 0.8), sp.trunk("b", 0, None), sp.chain(key="a", nsec=1), sp.chain(key="w", nsec=0)]
    for k in range(n):
        items.append(sp.bus([("a", "b", "w")[(k + j) % 3] for j in range(2 + k % 3)], MIXED[k % 4:k % 4 + 1 + k % 3], nsec=(0, 1)[k % 2], finish=("sat", "none", "tpdf")[k % 3]))
    r = play(fmt, [sp.core(items, calc=0)], blocks=SHORT)[0]
    assert r.sum_info()[0] == n
    r.release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_int64_wrap_is_reached(fmt):
    """full-scale samples through LOAD_GAIN 7.9, summed eight times over: in format 2 the 64-bit sum wraps"""
    items = [sp.trunk("a", 0, 7.9), sp.trunk("b", 0, -7.9), sp.bus(["a"] * 8, ["ADDXY"] * 7, nsec=0, finish="none"), sp.bus(["a", "b", "a", "b"], ["SUBXY"] * 3, nsec=1),
             sp.bus(["b", "a"], ["SUBXY"], nsec=0, finish="sat")]
    c = sp.core(items)
    prog, nin, nout, _ = sp.program(fmt, [c])
    x = the_input(fmt, 129, nin, 3)
    if fmt == 2:
        assert (int(np.abs(x.astype(np.int64)).max()) * int(7.9 * (1 << 28)) * 8) >> 63
    play(fmt, [c], blocks=[64, 65], seed=3)[0].release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_the_goldens_program_against_the_oracle_and_the_reference(fmt):
    """tests/golden/sum_f*.npz: lfe_core() and the constant cases -- +Inf and -Inf, a NaN on either side, both NaN -- in its blocks of 64,
    cores outer in blocks; the outputs are the compiled reference's too"""
    g = np.load(os.path.join(GOLDEN_DIR, f"sum_f{fmt}.npz"))
    prog, x, nout = g["prog"].copy(), g["x"], int(g["meta"][6])
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = sum_runtime(fmt, prog)
    lowered(r, mg.cores(fmt))
    total, outs = int(prog[1]), []
    for k, a in enumerate(range(0, len(x), 64)):
        b = min(64, len(x) - a)
        want = o.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        outs.append(r.run_block_all(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout))))
        compare_block(r, o, outs[-1], want, total, f"format {fmt}, the goldens' program, block {k}")
    same(np.concatenate(outs), g["out"], f"format {fmt}, against the compiled reference")
    same_words(r.sync_state(), g["state"], "the reference's state area")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_option_off_and_on_again_across_a_block(fmt):
    c = sp.core(bus_items() + delayed_items()[3:6], calc=0)
    prog, nin, nout, wd = sp.program(fmt, [c])
    prog = prog.copy()
    constants(fmt, prog, wd, {"w": -0.37, "n": 0.25, "i": 0.5})
    blocks = [65, 64, 2, 1029]
    x = the_input(fmt, sum(blocks), nin, 11)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = sum_runtime(fmt, prog)
    total = int(prog[1])
    for k, (a, b) in enumerate(cut(blocks)):
        on = k != 1
        r.set_option("chain_sum", int(on))
        assert r.core_info()["chains"] == (sp.counts(c)[3] if on else 0) and r.sum_info() == (sp.counts(c)[0] if on else (0, 0))
        want = o.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        got = r.run_block(x[a:a + b], nout, IN, out=sentinel(fmt, (b, nout)))
        compare_block(r, o, got, want, total, f"format {fmt}, block {k}, chain_sum {int(on)}")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_run_block_all_and_two_cores(fmt):
    """a writer core and a reader core whose buses read the writer's words as constants: the words the first core's launch left"""
    c1 = sp.core([sp.trunk("l", 2, 0.8), sp.trunk("r", 0, None), sp.bus(["l", "r"], ["ADDXY"], nsec=1)], calc=0)
    c2 = sp.core([sp.bus(["l", "r"], ["SUBXY"], nsec=1, finish="tpdf"), sp.bus(["r", "l", "w"], ["ADDXY", "ADDXY"], nsec=0, slot="A", us=1000),
                  sp.trunk("m", 1), sp.bus(["m", "l"], ["SUBXY"], nsec=0, finish="none")])
    play(fmt, [c1, c2], blocks=SHORT, run="run_block_all")[0].release()
    play(fmt, [c1, c2], blocks=SHORT, run="run_block")[0].release()


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_an_in_place_device_call(fmt):
    """one [frames][io] block in device memory as both windows: a term reads its trunk's sample behind the first phase's stores"""
    import torch
    c = sp.core(bus_items() + delayed_items()[3:6], calc=0)
    prog, nin, nout, wd = sp.program(fmt, [c])
    prog = prog.copy()
    constants(fmt, prog, wd, {"w": -0.37, "n": 0.25, "i": 0.5})
    W = IN + nin
    x = the_input(fmt, sum(SHORT), nin, 23)
    o = po.OracleProgram(fmt, prog, fs=48000, random=1, dither=24)
    r = sum_runtime(fmt, prog)
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
def test_an_uploaded_constant_term_reaches_the_next_block(fmt):
    c = sp.core([sp.trunk("a", 1), sp.bus(["a", "w"], ["ADDXY"], nsec=0, finish="none"), sp.bus(["w", "v", "a"], ["SUBXY", "ADDXY"], nsec=1)], calc=0)
    prog, nin, nout, wd = sp.program(fmt, [c])
    prog = prog.copy()
    constants(fmt, prog, wd, {"w": -0.37, "v": 0.11})
    r, o, x, nout = play(fmt, [c], blocks=[65], prog=(prog, nin, nout))
    for buf in (o.buf, r.buf):                                # the edit goes into both program copies
        sp.set_word(buf, wd["w"], 0.29, fmt)
        sp.set_word(buf, wd["v"], -0.05, fmt)
    r.upload_params()
    xb = the_input(fmt, 64, x.shape[1], 5)
    want = o.run_block(xb, nout, IN, out=sentinel(fmt, (64, nout)))
    got = r.run_block(xb, nout, IN, out=sentinel(fmt, (64, nout)))
    compare_block(r, o, got, want, int(prog[1]), f"format {fmt}, behind the edit")


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_a_checkpoint_into_a_fresh_runtime(fmt):
    c = sp.core(bus_items() + delayed_items()[3:6], calc=0)
    prog, nin, nout, wd = sp.program(fmt, [c])
    prog = prog.copy()
    constants(fmt, prog, wd, {"w": -0.37, "n": 0.25, "i": 0.5})
    r, o, x, nout = play(fmt, [c], blocks=[65, 1029], prog=(prog, nin, nout))
    total = int(o.buf[1])
    state, now = r.sync_state().copy(), r.buf[:total].copy()
    r.release()
    r2 = sum_runtime(fmt, now)
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


@pytest.mark.parametrize("fmt", [2, 4, 6])
def test_lfe_program_on_the_chain_kernels(fmt):
    """crossover2x2lfe.c's opcode sequence with all the options on: one head of two words, two forks, two trunks, no refusal"""
    prog, nin, nout, wd, c = sp.lfe_program(fmt)
    r = play(fmt, [c], prog=(prog, nin, nout), dither=24)[0]
    assert r.sum_info() == (1, 2) and r.ways_info()[0] == 2 and r.mem_info()[0] == 2 and r.core_info()["chains"] == 7, r.last_error()
    r.set_option("profile", 1)
    try:
        r.kernel_time(0)
        r.run_block(the_input(fmt, 64, nin, 9), nout, IN)
        assert r.kernel_time(0)[1] >= 1                        # (the cascades' timer: the core ran on biquad kernels)
    finally:
        r.set_option("profile", 0)
    r.release()

"""The headline configurations at FULL width against the compiled reference, and runtime-level channel sharding.

tests/golden/headline_*.npz + headline_manifest.json were produced by tests/golden/make_headline_goldens.py from
oracle/_ref (the reference runtime itself): every channel of BASELINE.json's configs 3, 4, 5 and of the north-star
program over several blocks -- SHA-256 of each block's output and of the final state area, per-channel and
per-frame sums (a mismatch is localised to a channel and a frame), first and last frames.  The bar is the reference's
bits: SHA equality in every format (the float models are bit-exact here, far inside north_star's 1e-6).

Sharding: dspRuntimeSetShard(rank, world) cuts any loaded chain program after lowering; the shards of
the UNSHARDED cfg5 program are run one after the other on this one GPU and their column slices, put side by side,
must be the unsharded reference result."""
import hashlib
import json
import os
import socket

import numpy as np
import pytest

from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from avdsp_amd import devmem as dm
from avdsp_amd import sharding as sh
from oracle import pyoracle as po
from tests.golden_recipes import GOLDEN_DIR

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN_DIR, "headline_manifest.json")) as _f:
    HEADLINE = json.load(_f)["cases"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(autouse=True)
def _release():
    yield
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def check_pins(name, out, state):
    """the whole [frames][C] output and the final state area against the reference's pins"""
    case = HEADLINE[name]
    g = np.load(os.path.join(GOLDEN_DIR, f"headline_{name}.npz"))
    C, B = case["channels"], case["block"]
    w = words(out)
    col = w.sum(axis=0, dtype=np.uint64).astype(np.uint32)
    row = w.sum(axis=1, dtype=np.uint64).astype(np.uint32)
    bad_c = np.nonzero(col != g["col_sum"])[0]
    bad_r = np.nonzero(row != g["row_sum"])[0]
    assert bad_c.size == 0 and bad_r.size == 0, \
        f"{name}: {bad_c.size} of {C} channels differ from the reference (first {bad_c[:8].tolist()}), first frame {bad_r[:1].tolist()}"
    assert (words(out[:2]) == words(g["head"])).all() and (words(out[-2:]) == words(g["tail"])).all()
    for k, want in enumerate(case["block_sha"]):
        assert sha(out[k * B:(k + 1) * B]) == want, f"{name}: block {k} differs from the reference"
    assert sha(out) == case["out_sha"]
    per = case["state_words_per_channel"]
    scol = state.reshape(C, per).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    bad_s = np.nonzero(scol != g["state_col"])[0]
    assert bad_s.size == 0, f"{name}: state of {bad_s.size} channels differs from the reference (first {bad_s[:8].tolist()})"
    assert sha(state) == case["state_sha"]


def headline_program(case):
    return pb.synth_program(case["fmt"], case["channels"], case["sections"], case["taps"])


def headline_input(case):
    return pb.lcg_input(case["frames"], case["channels"], case["fmt"] in (5, 6), seed=case["seed"])


@pytest.mark.parametrize("name", ["cfg3_f2", "cfg3_f4", "cfg3_f6", "cfg4_f4", "cfg4_f6", "north_f6"])
def test_headline_config_every_channel_matches_the_reference(name):
    """cfg3 (4096 ch x 16 biquads, int64 / double), cfg4 (256 ch x 4096 taps), north star (4096 ch x (16 biquads +
    4096 taps), 5 blocks so the FIR history is full): all channels, block by block, outputs and state."""
    case = HEADLINE[name]
    C, B = case["channels"], case["block"]
    x = headline_input(case)
    assert sha(x) == case["in_sha"]
    r = rt.Runtime(case["fmt"], headline_program(case))
    assert r.rc > 0
    out = np.concatenate([r.run_block(x[b:b + B], C, C) for b in range(0, case["frames"], B)])
    check_pins(name, out, r.sync_state())


def run_sharded(r, x, world, C_out, nblocks, B, order=None):
    """every shard of the loaded program, one after the other on this GPU: returns the assembled [frames][C_out] output"""
    out = np.zeros((x.shape[0], C_out), dtype=x.dtype)
    in_base_full = C_out                                   # synthetic layout: inputs at IO C.., outputs at IO 0..
    for rank in (order or range(world)):
        r.set_shard(rank, world)
        info = r.shard_info()
        if info["nchains"] == 0:
            continue
        ilo, ihi, olo, ohi = info["in_io_min"], info["in_io_max"] + 1, info["out_io_min"], info["out_io_max"] + 1
        xs = np.ascontiguousarray(x[:, ilo - in_base_full:ihi - in_base_full])
        for k in range(nblocks):
            ys = r.run_block(xs[k * B:(k + 1) * B], ohi - olo, ilo, olo)
            out[k * B:(k + 1) * B, olo:ohi] = ys
    return out


def test_cfg5_unsharded_program_in_8_shards_matches_the_reference():
    """BASELINE config 5: 16384 ch x (8 biquads + 2048-tap FIR), block 1024, sharded 8 ways.  The UNSHARDED program is
    loaded once; dspRuntimeSetShard(rank, 8) selects 2048 chains at a time; the eight column slices side by side are the
    reference's unsharded output, and the state area after the last shard is the reference's final state."""
    case = HEADLINE["cfg5_f6"]
    C, B, world = case["channels"], case["block"], 8
    x = headline_input(case)
    assert sha(x) == case["in_sha"]
    r = rt.Runtime(6, headline_program(case))
    assert r.rc > 0
    r.set_shard(3, world)
    assert r.shard_info() == dict(total_chains=C, first_chain=3 * 2048, nchains=2048, in_io_min=C + 3 * 2048,
                                  in_io_max=C + 4 * 2048 - 1, out_io_min=3 * 2048, out_io_max=4 * 2048 - 1)
    out = run_sharded(r, x, world, C, case["frames"] // B, B, order=[5, 0, 7, 1, 2, 6, 3, 4])
    r.set_shard(0, 1)
    check_pins("cfg5_f6", out, r.sync_state())


def test_cfg5_one_shard_program_and_sampled_oracle():
    """one rank's view of cfg5 as bench.py runs it at 8 GPUs (2048 chains of the unsharded program), against the
    reference pins of exactly those columns and the oracle on sampled channels"""
    case = HEADLINE["cfg5_f6"]
    C, B, S, T = case["channels"], case["block"], case["sections"], case["taps"]
    g = np.load(os.path.join(GOLDEN_DIR, "headline_cfg5_f6.npz"))
    x = headline_input(case)
    r = rt.Runtime(6, headline_program(case))
    r.set_shard(6, 8)
    lo, hi = sh.shard_range(C, 8, 6)
    xs = np.ascontiguousarray(x[:, lo:hi])
    ys = np.concatenate([r.run_block(xs[b:b + B], hi - lo, C + lo, lo) for b in range(0, case["frames"], B)])
    col = words(ys).sum(axis=0, dtype=np.uint64).astype(np.uint32)
    assert (col == g["col_sum"][lo:hi]).all()
    taps = pb.lcg_taps_all(3, T, channel_base=lo + 100)
    for k, c in enumerate((lo + 100, lo + 101, lo + 102)):
        sub = pb.ProgramWriter(6, capacity=1 << 14)
        sub.core(); sub.param()
        bank = sub.biquad_bank(pb.synth_sections(c, S, pb.F48000, pb.F48000))
        imp = sub.fir_impulses([taps[k]])
        sub.load_gain_fixed(1, 1.0); sub.biquads(bank, S); sub.fir(imp, T); sub.sat0db(); sub.store(0)
        want = po.OracleProgram(6, sub.end_of_code()).run_block(np.ascontiguousarray(x[:, c:c + 1]), 1, 1)
        assert (words(ys[:, c - lo:c - lo + 1]) == words(want)).all(), f"channel {c}"


@pytest.mark.parametrize("fmt,world", [(6, 3), (2, 5), (4, 2)])
def test_a_reference_encoded_program_shards(fmt, world, manifest):
    """A .bin that progbuilder did not build: 8 ch x 8 biquads emitted by the REFERENCE ENCODER (tests/golden/refenc_*.npy,
    written by oracle/_ref/ref_encode) and the reference runtime's own outputs for it (golden bq_c8_s8_b256): cut into
    3 / 5 / 2 ragged shards after loading."""
    name = f"bq_c8_s8_b256_f{fmt}"
    case = next(c for c in manifest["cases"] if c["name"] == name)
    path = os.path.join(GOLDEN_DIR, f"refenc_f{fmt}_c8_s8_5_5.npy")
    prog = np.load(path) if os.path.exists(path) else None
    if prog is None:                                         # only formats 2 and 6 were kept as files: the float encoding is shared
        prog = np.load(os.path.join(GOLDEN_DIR, "refenc_f6_c8_s8_5_5.npy"))
    from tests.golden_recipes import make_input
    x = make_input(case["input"], fmt)
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    r = rt.Runtime(fmt, prog)
    out = run_sharded(r, x, world, 8, 1, 256)
    assert (words(out) == words(g["out"])).all()
    r.set_shard(0, 1)
    assert (r.sync_state() == g["state"]).all()


def irregular_program(fmt):
    """chains a host might write by hand: scattered IO numbers, two STOREs, a plain LOAD, different section counts, a FIR"""
    pw = pb.ProgramWriter(fmt, capacity=1 << 14)
    pw.core()
    spec = [(40, [3], 2, 0, True), (17, [9, 21], 0, 5, False), (33, [0], 5, 0, True), (18, [30], 1, 12, True),
            (50, [7], 3, 0, False), (41, [8, 2], 2, 31, True), (19, [11], 4, 0, True)]
    if fmt == 2:
        spec = [(i, o, s, 0, sat) for (i, o, s, t, sat) in spec]
    for k, (io_in, outs, nsec, ntaps, sat) in enumerate(spec):
        pw.param()
        bank = pw.biquad_bank(pb.synth_sections(k * 7, nsec, pb.F48000, pb.F48000)) if nsec else None
        imp = pw.fir_impulses([pb.lcg_taps(k, ntaps)]) if ntaps else None
        if k % 2:
            pw.load(io_in)
        else:
            pw.load_gain_fixed(io_in, 0.5 + 0.1 * k)
        if bank is not None:
            pw.biquads(bank, nsec)
        if imp is not None:
            pw.fir(imp, ntaps)
        if sat:
            pw.sat0db()
        for o in outs:
            pw.store(o)
    return pw.end_of_code(), spec


@pytest.mark.parametrize("fmt", [2, 4, 6])
@pytest.mark.parametrize("world", [2, 3, 7, 9])
def test_irregular_program_shards_vs_oracle(fmt, world):
    """IO numbers in no order, chains of different shapes, more ranks than chains (world 9 > 7 chains: two ranks idle):
    every rank passes only the IO window dspRuntimeShardInfo names; assembled == oracle on the unsharded program"""
    prog, spec = irregular_program(fmt)
    frames, span = 200, 64
    x = pb.lcg_input(frames, span, fmt == 6, seed=7)         # one input frame = IO 0..63, whatever the program loads
    o = po.OracleProgram(fmt, prog)
    want = o.run_block(x, span, 0, 0, scratch_len=span + 1)  # windows overlap on the oracle: inputs show through, fine
    r = rt.Runtime(fmt, prog)
    got = np.zeros((frames, span), dtype=x.dtype)
    seen = 0
    for rank in range(world):
        r.set_shard(rank, world)
        info = r.shard_info()
        seen += info["nchains"]
        if not info["nchains"]:
            assert info["total_chains"] == len(spec)
            r.run_block(x[:, :1], 1, 0, 1)                   # an idle rank's call is a no-op, not an error
            continue
        ilo, ihi, olo, ohi = info["in_io_min"], info["in_io_max"] + 1, info["out_io_min"], info["out_io_max"] + 1
        for b0, b1 in ((0, 37), (37, 200)):
            ys = r.run_block(np.ascontiguousarray(x[b0:b1, ilo:ihi]), ohi - olo, ilo, olo)
            lo, hi = sh.shard_range(len(spec), world, rank)
            for (_, outs, _, _, _) in spec[lo:hi]:
                for oo in outs:
                    got[b0:b1, oo] = ys[:, oo - olo]
    assert seen == len(spec)
    stored = sorted(oo for (_, outs, _, _, _) in spec for oo in outs)
    assert (words(got[:, stored]) == words(want[:, stored])).all()
    r.set_shard(0, 1)
    assert (r.sync_state() == o.state).all()


def _gloo_worker(rank, world, port, fmt, C, S, T, B, nblocks, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        prog = pb.synth_program(fmt, C, S, T)                # every rank loads the UNSHARDED program
        x = pb.lcg_input(B * nblocks, C, fmt == 6, seed=31)
        r = rt.Runtime(fmt, prog)
        r.set_option("device", 0)
        r.set_shard(rank, world)
        info = r.shard_info()
        lo, n = info["first_chain"], info["nchains"]
        xs = np.ascontiguousarray(x[:, info["in_io_min"] - C:info["in_io_max"] + 1 - C])
        y = np.concatenate([r.run_block(xs[k * B:(k + 1) * B], n, info["in_io_min"], info["out_io_min"]) for k in range(nblocks)])
        # block-boundary collectives only: gather the ragged slices, reduce the checksums
        widths = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(widths, torch.tensor([n], dtype=torch.int64))
        wmax = int(max(w.item() for w in widths))
        pad = np.zeros((y.shape[0], wmax), dtype=np.int32); pad[:, :n] = y.view(np.int32)
        parts = [torch.zeros((y.shape[0], wmax), dtype=torch.int32) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(pad))
        full = np.concatenate([p.numpy()[:, :int(w.item())] for p, w in zip(parts, widths)], axis=1)
        cks = torch.tensor([sh.block_checksum(y) % (1 << 62)], dtype=torch.int64)
        dist.all_reduce(cks, op=dist.ReduceOp.SUM)
        dist.barrier()
        if rank == 0:
            ref = po.OracleProgram(fmt, prog).run_block(x, C, C, block=B)
            q.put((bool((full.view(np.uint32) == ref.view(np.uint32)).all()),
                   int(cks.item()) == sum(sh.block_checksum(ref[:, a:b]) % (1 << 62)
                                          for a, b in (sh.shard_range(C, world, k) for k in range(world))),
                   (lo, n) == (0, sh.shard_range(C, world, 0)[1])))
        r.release()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,fmt,C,S,T", [(2, 6, 10, 3, 33), (2, 2, 7, 4, 0), (3, 6, 8, 2, 40)])
def test_world_n_ranks_hip_path_over_gloo(world, fmt, C, S, T):
    """The N > 1 path with the HIP kernels doing the work: `world` processes share this one GPU (RCCL refuses two ranks on
    one device, so the block-boundary collectives go over gloo), each loads the unsharded program and calls
    dspRuntimeSetShard(rank, world); rank 0 checks the gathered block against the oracle -- the checker only."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_gloo_worker, args=(k, world, port, fmt, C, S, T, 64, 3, q)) for k in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    same, cks_ok, range_ok = q.get(timeout=5)
    assert same and cks_ok and range_ok


@pytest.mark.parametrize("fir_impl", [1, 3])
@pytest.mark.parametrize("fmt,C,S,T", [(6, 600, 16, 700), (6, 40, 8, 4096), (4, 70, 24, 300), (6, 40, 40, 100)])
def test_overlap_mode_is_bit_identical(fmt, C, S, T, fir_impl):
    """dspRuntimeSetOption("overlap", 1): the cascade of block k+1 runs under the FIR of block k (on a side stream; the FIR stays on
    the caller's).  Six blocks are enqueued back to back without any host synchronisation -- with buffers of their own, and once
    more into ONE output buffer copied out on the caller's stream after every block; the result must be the oracle's, bit for
    bit, outputs and state -- and the same with the option off."""
    import torch
    B, nb = 1024, 6
    prog = pb.synth_program(fmt, C, S, T)
    x = pb.lcg_input(B * nb, C, fmt == 6, seed=5)
    o = po.OracleProgram(fmt, prog)
    want = o.run_block(x, C, C, block=B)
    # overlap 2: also the FIRs of consecutive blocks on two streams in turn.  ready_words 1: fir_tile finds its cascades' blocks through
    # the per-chain ready words, polled in the kernel, published by the cascade's waves; 2: set by a kernel behind the cascade (no
    # wait packet on the FIRs' stream: the library's choice where the FIR is the bound); 0: an event between the two queues;
    # ring_wait 0 / 1: the cascades' stream / the host waits for the FIR three blocks back
    for overlap, ready_words, ring_wait in ((2, 1, 1), (2, 0, 1), (1, 1, 1), (1, 0, 1), (1, 2, 1), (1, 2, 0), (2, 2, 1), (1, 0, 0), (1, -1, 1), (0, 1, 1)):
        r = rt.Runtime(fmt, prog)
        r.set_option("fir_impl", fir_impl)                    # fir_tile / fir_stream (the cascade then feeds the operand ring as well)
        r.set_option("overlap", overlap)
        r.set_option("ready_words", ready_words)
        r.set_option("ring_wait", ring_wait)
        assert r.get_option("overlap") == overlap and r.get_option("ready_words") == ready_words and r.get_option("ring_wait") == ring_wait
        xd = [dm.to_device(x[k * B:(k + 1) * B].copy()) for k in range(nb)]
        yd = [torch.zeros((B, C), dtype=xd[0].dtype, device="cuda") for _ in range(nb)]
        torch.cuda.synchronize()                             # the mode's contract: inputs complete when the call is made
        st = torch.cuda.current_stream().cuda_stream
        for k in range(nb):
            r.run_block_device(xd[k].data_ptr(), C, C, yd[k].data_ptr(), C, 0, B, st)
        torch.cuda.synchronize()
        got = np.concatenate([dm.to_host(y) for y in yd])
        assert (words(got) == words(want)).all(), f"overlap={overlap} ready_words={ready_words} ring_wait={ring_wait}"
        assert (r.sync_state() == o.state).all()
        assert r.get_option("ready_timeouts") == 0            # no wave ever gave up waiting for a ready word
        r.release()
        if overlap >= 2:                                      # (that mode's contract rules the next part out: an output block is not reused while in flight)
            continue
        # one output buffer for every block, copied out on the caller's stream right behind each call
        r = rt.Runtime(fmt, prog)
        r.set_option("fir_impl", fir_impl)
        r.set_option("overlap", overlap)
        r.set_option("ready_words", ready_words)
        r.set_option("ring_wait", ring_wait)
        y1 = torch.zeros((B, C), dtype=xd[0].dtype, device="cuda")
        outs = []
        for k in range(nb):
            r.run_block_device(xd[k].data_ptr(), C, C, y1.data_ptr(), C, 0, B, st)
            outs.append(y1.clone())                           # (on the current stream: ordered behind the block)
        torch.cuda.synchronize()
        got = np.concatenate([dm.to_host(y) for y in outs])
        assert (words(got) == words(want)).all(), f"overlap={overlap} ready_words={ready_words}, one output buffer"
        r.set_option("overlap", 0)
        r.set_option("ready_words", -1)
        r.set_option("ring_wait", 1)
        r.set_option("fir_impl", 1)
        r.release()


def _bench_ranks(world, extra=(), env_extra=None, workload="cfg3"):
    """bench.py as the driver launches it for N = world (torch.distributed.run, one fresh process per rank; the ranks share this
    box's one GPU, so the process group is gloo -- RCCL refuses two ranks on one device)"""
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AVDSP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "4", "--warmup", "1",
           "--settle", "0.05", "--workload", workload, "--no-cpu-baseline", "--full", *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)


def test_bench_verifies_every_rank_and_reports_the_gather_leg():
    """N = 2: before anything is timed every rank pushes the headline input through the same dspRuntimeBlockDevice path and compares
    ITS columns with the reference's pins; the JSON line says so (verified, verified_ranks), carries the per-rank step times, and --
    by default for N > 1 -- the timed block-boundary collectives beside the metric."""
    import json
    p = _bench_ranks(2)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and len(line["rank_ms_per_step"]) == 2
    assert line["verified"] and "cfg3_f6" in line["verified"] and "channels 0..2047" in line["verified"]
    assert line["verified_ranks"] == 2
    assert line["gather"]["all_gather_ms"] > 0 and line["gather"]["bytes_per_rank"] == 1024 * 2048 * 4
    assert line["config"]["channels_per_gpu"] == 2048 and line["scaling"] == "strong"


# The GPU boxes of this pool allow at most six processes on the card at once (more and the run is killed: "process guard"; five ranks
# under the test runner were counted as seven), the test runner itself being one of them: four ranks is the widest rehearsal that may
# run here.  AVDSP_REHEARSAL_WORLD=8 runs the same test at the 8-GPU node's rank count where no such limit applies (one rank per GPU
# there, or a box without the guard).
REHEARSAL_WORLD = int(os.environ.get("AVDSP_REHEARSAL_WORLD", "4"))


def test_bench_rehearsal_at_the_widest_world_this_box_allows():
    """The north-star program's N > 1 bench line at the widest world the box allows (4 ranks x 1024 chains; ragged shards -- 4096
    chains over 3 ranks -- are test_bench_ragged_shards'): every rank
    verifies its own columns against the reference's pins, all of them are counted, every rank's step time is listed and the
    gather leg reports what a rank hands over."""
    import json
    w = REHEARSAL_WORLD
    p = _bench_ranks(w, workload="north")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == w and line["ranks"] == w and len(line["rank_ms_per_step"]) == w
    assert line["verified_ranks"] == w and "north_f6" in line["verified"]
    cmax = -(-4096 // w)
    assert line["config"]["channels_per_gpu"] == cmax
    assert line["gather"]["bytes_per_rank"] == 1024 * cmax * 4 and line["gather"]["all_gather_ms"] > 0
    assert line["roofline"]["bound"] == "mfma" and line["value"] > 0


def test_bench_ragged_shards():
    """4096 chains over 3 ranks (1366 + 1365 + 1365): the pins are checked per rank on its own ragged range, the gather leg pads."""
    import json
    p = _bench_ranks(3, workload="cfg3")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["ranks"] == 3 and line["verified_ranks"] == 3 and line["config"]["channels_per_gpu"] == 1366
    assert line["gather"]["bytes_per_rank"] == 1024 * 1366 * 4


def test_bench_ranks_leave_together_when_one_rank_fails_its_check():
    """A rank whose columns differ from the pins must not exit alone (the others would sit in their next barrier until the
    launcher's timeout): every rank learns of it through an all_reduce(MIN) and all leave non-zero, no JSON line."""
    import time
    t0 = time.time()
    p = _bench_ranks(2, env_extra={"AVDSP_BENCH_FAIL_RANK": "1"})
    assert p.returncode != 0
    assert "VERIFICATION FAILED on rank 1" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert time.time() - t0 < 300


def _bench_line(p):
    import json
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _clean_env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "AVDSP_BENCH_CPU_JSON")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", **kw)
    return env


def test_bench_gpus_2_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher around it (round-4 review, Missing #2: that command used to run the whole program
    on one GPU and print n_gpus 1): the bare process times the CPU baseline without touching the GPU, starts two fresh rank processes
    itself and relays rank 0's line -- which says n_gpus 2 and carries a cpu_baseline like the N = 1 line does."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--settle", "0.05",
                        "--workload", "cfg3", "--cpu-budget", "1.5", "--full"], env=_clean_env(AVDSP_DIST_BACKEND="gloo"),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = _bench_line(p)
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and len(line["rank_ms_per_step"]) == 2
    assert line["verified_ranks"] == 2 and line["config"]["channels_per_gpu"] == 2048
    cpu = line["cpu_baseline"]
    assert cpu is not None and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["kind"] in ("reference", "port")
    assert line["collectives"]["backend"] == "gloo" and line["gather"]["all_gather_ms"] > 0


def test_every_collective_of_bench_runs_on_rccl_at_world_1():
    """The N > 1 legs of bench.py are rehearsed over gloo (RCCL refuses two ranks on one card), so until an 8-GPU node runs them the
    RCCL calls themselves had never executed.  World 1 under the launcher with --dist: init_process_group("nccl", device_id=...),
    the all_reduce(MIN / SUM) on slices of a DEVICE tensor, barrier, all_gather + all_reduce(MAX) of the times, the all_gather of the
    [B][C] output block and the all_reduce of its checksum, barrier, destroy -- every call the 8-GPU job makes, on RCCL, once."""
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--dist", "--steps", "4", "--warmup", "1",
           "--settle", "0.05", "--workload", "cfg3", "--cpu-budget", "1.0", "--full"]
    p = subprocess.run(cmd, env=_clean_env(), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _bench_line(p)
    assert line["collectives"]["backend"] == "nccl" and line["collectives"]["world"] == 1
    assert line["n_gpus"] == 1 and line["ranks"] == 1 and line["verified_ranks"] == 1
    assert line["gather"]["backend"] == "nccl" and line["gather"]["bytes_per_rank"] == 1024 * 4096 * 4
    assert line["gather"]["all_gather_ms"] > 0 and line["gather"]["checksum_all_reduce_ms"] > 0
    assert line["cpu_baseline"] is not None


def test_bench_block_sizes_push_the_same_pins_through():
    """--block B: the workload's frames in calls of B frames.  The pre-timing check pushes the reference's 5 x 1024 pinned frames
    through in calls of B (ragged at the end when B does not divide) and must find the same bits: 64, 256 and 4096 on the cascade."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for blk in (64, 256, 4096):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "1", "--settle", "0.05",
                            "--workload", "cfg3", "--block", str(blk), "--no-cpu-baseline", "--full"], env=_clean_env(),
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        line = _bench_line(p)
        assert line["config"]["block"] == blk and f"calls of {blk} frames" in line["verified"] and "SHA-256" in line["verified"]
    # ... and the north-star program (cascade + 4096-tap FIR) at the short blocks whose FIR launches regroup their waves (one tile of a
    # one-row-tile wave at 256 frames, four chains per two-row-tile workgroup at 512)
    for blk in (256, 512):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "1", "--settle", "0.05",
                            "--workload", "north", "--block", str(blk), "--no-cpu-baseline", "--full"], env=_clean_env(),
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        line = _bench_line(p)
        assert line["config"]["block"] == blk and "north_f6" in line["verified"] and "SHA-256" in line["verified"]


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain run (no --full) prints the headline line without the --full legs, and --dump-outputs writes the output block of its last
    timed step: the same bits whatever the time-based settle phase ran before the warm-up (the state goes back to the program's initial
    state after it), and on sampled channels the oracle's bits for the 200 re-settle, warm-up and timed steps of the same block from
    that state."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps, warmup = 3, 1
    dumps = []
    for k, settle in enumerate(("0.3", "0.05")):
        d = tmp_path / f"run{k}"
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--settle", settle,
                            "--workload", "north", "--dump-outputs", str(d)], env=_clean_env(), capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        line = _bench_line(p)
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "Msamples/s"
        assert line["cpu_baseline"] is None and line["verified"] is None and "roofline" not in line and "kernels_ms" not in line
        assert sorted(os.listdir(d)) == ["output.npy"]
        dumps.append(np.load(d / "output.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (1024, 4096)
    assert (words(dumps[0]) == words(dumps[1])).all(), "the dumped outputs depend on the settle phase"
    fmt, S, T, B = 6, 16, 4096, 1024
    x = pb.lcg_input(B, 4096, True, seed=12345)
    for c in (0, 1234, 4095):
        o = po.OracleProgram(fmt, pb.synth_program(fmt, 1, S, T, channel_base=c))
        xc = np.ascontiguousarray(x[:, c:c + 1])
        for _ in range(200 + warmup + steps):
            want = o.run_block(xc, 1, 1)
        assert (words(want[:, 0]) == words(dumps[0][:, c])).all(), f"channel {c} differs from the oracle"

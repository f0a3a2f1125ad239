"""The LOAD_MUX stage where its bookkeeping can go wrong: several mix groups in one launch, list lengths on both
sides of every seam of mux_tile's chunks and k-steps, row tails of its tiles, mux_tile against mux_plain on one group through the
shard cut, live edits of lists and gains, and the rest of the API in front of a mixer.  Every comparison is with the oracle, word for
word: the outputs of every block and dspRuntimeSyncState at the end (the opcodes' result words are part of it).  The programs are
tests/mux_recipes.py's; tests/test_mux_lowering.py checks their groups and runs the oracle over them without a GPU."""
import numpy as np
import pytest

from avdsp_amd import devmem as dm
from avdsp_amd import progbuilder as pb
from avdsp_amd import runtime as rt
from oracle import pyoracle as po
from tests.mux_recipes import (ROW_TAIL_GROUPS, SEAM_INPUTS, SEAM_LENGTHS, check_seam_lengths, list_seams, live_edit, mixer_input, mux_tables, row_tails,
                               several_groups, shard_group, small_mixer, stored_program, windows_program)

pytestmark = pytest.mark.gpu

DEFAULTS = (("generic", 0), ("overlap", 0), ("fir_impl", 1), ("biquad_impl", 1), ("fir_shared", 1))


@pytest.fixture(autouse=True)
def _release():
    for k, v in DEFAULTS:
        rt.lib().dspRuntimeSetOption(k.encode(), v)
    yield
    for k, v in DEFAULTS:
        rt.lib().dspRuntimeSetOption(k.encode(), v)
    rt.lib().dspRuntimeSetShard(0, 1)
    rt.lib().dspRuntimeRelease()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def chain_text(meta, c):
    ch = meta["chains"][c]
    return f"chain {c} (group {ch['group']}, list of {len(ch['ios'])}, {ch['tail']})"


def same(got, want, meta, what, first_io=0):
    """bit for bit; a difference is named by the chains that store the columns"""
    d = words(got) != words(want)
    if not d.any():
        return
    by_io = {io: c for c, ch in enumerate(meta["chains"]) for io in ch["out"]}
    cols = np.nonzero(d.any(axis=0))[0]
    named = []
    for col in cols[:6].tolist():
        c = by_io.get(first_io + col)
        frame = int(np.nonzero(d[:, col])[0][0])
        named.append(f"column {col} from frame {frame}: " + (chain_text(meta, c) if c is not None else "no chain stores it"))
    groups = sorted({meta["chains"][by_io[first_io + c]]["group"] for c in cols.tolist() if first_io + c in by_io})
    raise AssertionError(f"{what}: {cols.size} columns differ, groups {groups[:12]}; " + "; ".join(named))


def same_state(got, want, meta, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    if bad.size == 0:
        return
    owner = {}
    for c, ch in enumerate(meta["chains"]):
        if ch["result"] is not None:
            owner[ch["result"]] = owner[ch["result"] + 1] = c
    named = sorted({owner[w] for w in bad.tolist() if w in owner})
    raise AssertionError(f"{what}: state words {bad[:8].tolist()} differ from the oracle's; result words of "
                         + (", ".join(chain_text(meta, c) for c in named[:4]) if named else "no chain") + " among them")


def lcg(frames, ch, fmt, seed):
    return pb.lcg_input(frames, ch, fmt == 6, seed=seed)


def run_vs_oracle(fmt, prog, meta, x, blocks, all_cores=False, what=""):
    W = meta["width"]
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    assert r.rc == o.rc and r.rc > 0
    pos = 0
    for b in blocks:
        want = o.run_block(x[pos:pos + b], W, W)
        got = (r.run_block_all if all_cores else r.run_block)(x[pos:pos + b], W, W)
        same(got, want, meta, f"{what}format {fmt}, block at frame {pos} ({b} frames)")
        pos += b
    assert pos == len(x)
    same_state(r.sync_state(), o.state, meta, f"{what}format {fmt}")
    return r


# ---- 1. several groups in one launch ----------------------------------------------------------------------------------------------------

def several_groups_input(fmt):
    x = mixer_input(dict(kind="special", frames=257, channels=64, seed=77), fmt)
    two = np.zeros((2, 64), dtype=x.dtype)
    if fmt == 6:
        two.view(np.uint32)[0, :] = 0x80000000                               # a frame of -0, then one of +0
    return np.concatenate([x[:64], two, x[64:]])                            # (the last frame of the first block, and the one-frame block)


@pytest.mark.parametrize("fmt", [6, 4, 2])
def test_several_groups_in_one_launch(fmt):
    """three groups (one tile of 16 rows, one of 17, two tiles of 64 and 6 rows; lists of 3, 33 and 64 entries: kpad 4, 36, 64), their
    chains interleaved with each other, with 15 chains of one sequence, private lists and LOAD_GAIN chains (mux_plain)"""
    prog, meta = several_groups(fmt)
    r = rt.Runtime(fmt, prog)
    assert r.core_info()["chains"] == 123
    assert r.mux_info() == dict(mux_chains=121, groups=3, grouped_chains=103, longest_list=64)
    r.release()
    run_vs_oracle(fmt, prog, meta, several_groups_input(fmt), [65, 1, 63, 130])


def test_several_groups_through_every_core_at_once():
    prog, meta = several_groups(6)
    run_vs_oracle(6, prog, meta, several_groups_input(6), [65, 1, 63, 130], all_cores=True, what="dspRuntimeBlockAll, ")


# ---- 2. list lengths on the seams of mux_tile's chunks (32 positions) and k-steps (4) ---------------------------------------------------

def test_the_list_lengths_sit_on_the_seams():
    check_seam_lengths()                                                     # (host-only; tests/test_mux_lowering.py runs it too)


def seam_input(fmt):
    """Inf, NaN and a subnormal (INT_MIN, INT_MAX and 1) in the last frame of the 81-frame block -- frame 80, in the partial 16-frame
    tile of the second 64-frame workgroup -- and in the input that most lists name at their LAST position"""
    x = lcg(82, SEAM_INPUTS, fmt, 29).copy()
    ends = [(L - 1 + g) % SEAM_INPUTS for g, L in enumerate(SEAM_LENGTHS)]
    col = max(set(ends), key=ends.count)
    assert ends.count(col) >= 3
    vals = np.array([np.inf, np.nan, 1e-40, -np.inf], dtype=np.float32) if fmt == 6 else np.array([-2147483648, 2147483647, 1, -1], dtype=np.int32)
    others = [c for c in range(SEAM_INPUTS) if c != col]
    x[80, others[7]], x[80, others[20]], x[80, others[33]] = vals[0], vals[1], vals[2]
    x[11, col], x[46, col], x[63, col], x[64, col], x[80, col], x[81, col] = vals[0], vals[2], vals[1], vals[3], vals[2], vals[0]
    return x


@pytest.mark.parametrize("fmt", [6, 4])
def test_list_seams_on_mux_tile(fmt):
    prog, meta = list_seams(fmt)
    r = rt.Runtime(fmt, prog)
    assert r.mux_info() == dict(mux_chains=464, groups=29, grouped_chains=464, longest_list=129)
    r.release()
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    x, W, pos = seam_input(fmt), meta["width"], 0
    for b in (81, 1):
        want, got = o.run_block(x[pos:pos + b], W, W), r.run_block(x[pos:pos + b], W, W)
        d = (words(got) != words(want)).any(axis=0)
        lengths = sorted({len(meta["chains"][c]["ios"]) for c in np.nonzero(d)[0].tolist()})
        assert not lengths, f"format {fmt}, block at frame {pos}: lists of {lengths} entries differ"
        pos += b
    same_state(r.sync_state(), o.state, meta, f"format {fmt}")


# ---- 3. row tails of a tile -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [6, 4])
def test_row_tails_of_the_tiles(fmt):
    """groups of 16 .. 129 chains: last tiles of 1, 15, 16, 17, 31, 32, 33, 48, 49 and 63 rows, behind full ones from 65 chains on"""
    prog, meta = row_tails(fmt)
    r = rt.Runtime(fmt, prog)
    assert r.mux_info() == dict(mux_chains=sum(ROW_TAIL_GROUPS), groups=12, grouped_chains=sum(ROW_TAIL_GROUPS), longest_list=6)
    r.release()
    x = mixer_input(dict(kind="special", frames=79, channels=12, seed=31), fmt)
    run_vs_oracle(fmt, prog, meta, x, [64, 15])


# ---- 4. mux_tile against mux_plain on one group: the shard cut puts a rank's slice under the group minimum -------------------------------

@pytest.mark.parametrize("fmt", [6, 4])
@pytest.mark.parametrize("nchains,world,tiled", [(40, 3, (0, 0, 0)), (40, 2, (1, 1)), (47, 3, (1, 1, 0))])
def test_tile_against_plain_through_the_shard_cut(nchains, world, tiled, fmt):
    prog, meta = shard_group(fmt, nchains)
    O, I, B = meta["width"], meta["inputs"], 70
    assert O == nchains
    x = mixer_input(dict(kind="special", frames=2 * B, channels=I, seed=41), fmt)
    whole = rt.Runtime(fmt, prog)
    assert whole.mux_info() == dict(mux_chains=nchains, groups=1, grouped_chains=nchains, longest_list=12)
    want = np.concatenate([whole.run_block(x[k * B:(k + 1) * B], O, O) for k in range(2)])
    want_state = whole.sync_state().copy()
    whole.release()
    o = po.OracleProgram(fmt, prog)
    same(want, o.run_block(x, O, O, block=B), meta, f"format {fmt}, unsharded (mux_tile)")
    same_state(want_state, o.state, meta, f"format {fmt}, unsharded")
    r = rt.Runtime(fmt, prog)
    out = np.zeros_like(want)
    sizes = []
    for rank in range(world):
        r.set_shard(rank, world)
        s = r.shard_info()
        sizes.append(s["nchains"])
        info = r.mux_info()
        assert info["mux_chains"] == s["nchains"]
        assert info["groups"] == tiled[rank] and info["grouped_chains"] == tiled[rank] * s["nchains"], f"rank {rank} of {world}: {info}"
        lo, hi = s["out_io_min"], s["out_io_max"] + 1
        for k in range(2):
            out[k * B:(k + 1) * B, lo:hi] = r.run_block(x[k * B:(k + 1) * B], hi - lo, O, lo)
    assert sum(sizes) == nchains and [n >= 16 for n in sizes] == [bool(t) for t in tiled]
    same(out, want, meta, f"format {fmt}: {world} shards of {sizes} chains against the unsharded run")
    same_state(r.sync_state(), want_state, meta, f"format {fmt}: {world} shards")
    r.set_shard(0, 1)


# ---- 5. live edits ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [6, 2])
def test_live_edits(fmt):
    """dspRuntimeUploadParams drops the plans: the gains of the tiles are widened again, and the groups are formed again from the edited
    lists -- a chain that names another IO leaves its group, a group of 15 goes to mux_plain"""
    prog, meta = live_edit(fmt)
    W, I = meta["width"], meta["inputs"]
    tabs = mux_tables(prog)
    assert len(tabs) == 36 and [len(ch["ios"]) for ch in meta["chains"][:33]] == [7] * 17 + [5] * 16
    x = lcg(3 * 70, I, fmt, 51)
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    assert r.mux_info() == dict(mux_chains=36, groups=2, grouped_chains=33, longest_list=7)
    same(r.run_block(x[:70], W, W), o.run_block(x[:70], W, W), meta, f"format {fmt}, before the edits")

    def gain(v):
        return pb._qm32(v) if fmt == 2 else pb._f32_bits(v)

    def entry(chain, k):
        t = tabs[chain]
        assert int(prog[t]) == (pb.OP_LOAD_MUX << 16) | len(meta["chains"][chain]["ios"]) and int(prog[t + 1 + 2 * k]) == W + meta["chains"][chain]["ios"][k]
        return t + 1 + 2 * k
    edits = [(entry(0, 0) + 1, gain(0.7109375)),          # position 0 of the first grouped chain
             (entry(16, 6) + 1, gain(-1.25)),              # the last position of the 17th chain: the one row of the tile's second row tile
             (entry(32, 4) + 1, gain(0.3330078)),          # the last position of the last chain of the second tile
             (entry(5, 3), W + 5),                         # chain 5 names another IO: it leaves the group of 17
             (entry(20, 1), W + 3)]                        # chain 20 too: 15 chains are left, no group
    for at, v in edits:
        r.buf[at] = o.buf[at] = np.uint32(v)
    r.upload_params()
    assert r.mux_info() == dict(mux_chains=36, groups=1, grouped_chains=16, longest_list=7)
    for k in (1, 2):
        same(r.run_block(x[70 * k:70 * (k + 1)], W, W), o.run_block(x[70 * k:70 * (k + 1)], W, W), meta, f"format {fmt}, block {k} after the edits")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}, after the edits")


# ---- 6. the rest of the API in front of a small mixer -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [6, 2])
def test_reset_to_another_rate(fmt):
    prog, meta = small_mixer(fmt, fmin=pb.F44100, fmax=pb.F96000)
    W = meta["width"]
    x = lcg(90, 5, fmt, 61)
    o = po.OracleProgram(fmt, prog, fs=44100)
    r = rt.Runtime(fmt, prog, fs=44100)
    same(r.run_block(x, W, W), o.run_block(x, W, W), meta, f"format {fmt}, 44.1 kHz")
    assert r.reset(96000) == 0 and o.reset(96000) == 0
    assert r.mux_info()["groups"] == 1
    same(r.run_block(x, W, W), o.run_block(x, W, W), meta, f"format {fmt}, 96 kHz after dspRuntimeReset")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}, 96 kHz")


@pytest.mark.parametrize("fmt", [6, 2])
def test_checkpoint_and_restore(fmt):
    prog, meta = small_mixer(fmt)
    W = meta["width"]
    x = lcg(150, 5, fmt, 62)
    o = po.OracleProgram(fmt, prog)
    want = o.run_block(x, W, W, block=50)
    r = rt.Runtime(fmt, prog)
    same(r.run_block(x[:50], W, W), want[:50], meta, "first block")
    saved = r.sync_state().copy()
    rest = r.run_block(x[50:], W, W, block=50)
    same(rest, want[50:], meta, "the run that goes on")
    end = r.sync_state().copy()
    r.release()
    r2 = rt.Runtime(fmt, prog)
    r2.state[:] = saved
    r2.upload_state()
    same(r2.run_block(x[50:], W, W, block=50), rest, meta, "the run from the checkpoint")
    same_state(r2.sync_state(), end, meta, "from the checkpoint")
    same_state(end, o.state, meta, "the run that goes on")


@pytest.mark.parametrize("fmt", [6, 4, 2])
def test_single_frames_then_a_block(fmt):
    """dspRuntime_N: both windows are the caller's samples[] array, over the span of the IOs that the LISTS name and the chains store"""
    prog, meta = small_mixer(fmt)
    W = meta["width"]
    x = lcg(40 + 33, 5, fmt, 63)
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    for n in range(40):
        frame_o = np.zeros(W + 5, dtype=rt.sample_dtype(fmt))
        frame_o[W:] = x[n]
        frame_d = frame_o.copy()
        po.lib().oracle_run(o.ctx, o.cores[0], o.data_ptr, frame_o.ctypes.data)
        assert r.run_frame(frame_d) == 0
        same(frame_d[None, :], frame_o[None, :], meta, f"format {fmt}, frame {n}")
        if n < 5:
            same_state(r.sync_state(), o.state, meta, f"format {fmt}, after frame {n}")
    same(r.run_block(x[40:], W, W), o.run_block(x[40:], W, W), meta, f"format {fmt}, the block behind the frames")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}")


def test_overlap_modes_change_nothing():
    """a plan with LOAD_MUX chains ignores "overlap": FIRs behind the heads, the same bits in modes 0, 1 and 2"""
    prog, meta = small_mixer(6, fir=True)
    W = meta["width"]
    x = lcg(300, 5, 6, 64)
    o = po.OracleProgram(6, prog)
    want = o.run_block(x, W, W, block=100)
    for mode in (0, 1, 2):
        r = rt.Runtime(6, prog)
        r.set_option("overlap", mode)
        assert r.core_info()["max_taps"] == 19
        same(r.run_block(x, W, W, block=100), want, meta, f'"overlap" {mode}')
        same_state(r.sync_state(), o.state, meta, f'"overlap" {mode}')
        r.set_option("overlap", 0)
        r.release()


@pytest.mark.parametrize("fmt", [6, 2])
def test_queued_blocks(fmt):
    prog, meta = small_mixer(fmt)
    W, B, depth = meta["width"], 256, 2
    x = lcg(4 * B, 5, fmt, 65)
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    xin = [np.ascontiguousarray(x[k * B:(k + 1) * B]) for k in range(4)]
    out = [np.zeros((B, W), dtype=x.dtype) for _ in range(4)]
    for k in range(4):
        assert 1 <= r.submit_block(xin[k], out[k], W, 0) <= 4
        assert r.wait_blocks(depth - 1) <= depth - 1
    assert r.wait_blocks(0) == 0
    for k in range(4):
        same(out[k], o.run_block(xin[k], W, W), meta, f"format {fmt}, queued block {k}")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}")
    r.set_option("host_pin", 0)


def _pack(samples32, pcm):
    """int32 s.31 words -> packed little-endian PCM bytes, dropping the low bits the format lacks"""
    u = samples32.astype(np.int32).view(np.uint32).reshape(-1)
    if pcm == rt.PCM_S16:
        return (u >> 16).astype("<u2").view(np.uint8)
    b = np.empty((u.size, 3), dtype=np.uint8)
    b[:, 0] = (u >> 8) & 0xFF; b[:, 1] = (u >> 16) & 0xFF; b[:, 2] = (u >> 24) & 0xFF
    return b.reshape(-1)


def _unpack_like_the_plugin(raw, pcm):
    if pcm == rt.PCM_S16:
        return raw.view("<i2").astype(np.int32) << 16
    b = raw.reshape(-1, 3).astype(np.uint32)
    return ((b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)).view(np.int32)


@pytest.mark.parametrize("pcm", [rt.PCM_S16, rt.PCM_S24_3LE], ids=["S16", "S24_3LE"])
@pytest.mark.parametrize("fmt", [4, 2])
def test_packed_pcm_into_a_mixer(fmt, pcm):
    prog, meta = small_mixer(fmt)
    W, B = meta["width"], 77
    x = pb.lcg_input(B, 5, False, seed=66)
    raw = _pack(x, pcm)
    xq = _unpack_like_the_plugin(raw, pcm).reshape(B, 5)
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    same(r.run_block_pcm(pcm, raw, B, 5, W, W), o.run_block(xq, W, W), meta, f"format {fmt}, pcm {pcm}")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}, pcm {pcm}")


@pytest.mark.parametrize("fmt", [4, 2])
def test_the_plugins_tag_on_an_output_of_the_stage(fmt):
    """linux/avdsp_plugin.c:133-137 on a core whose first output the stage stores itself, with 24-bit stores (mux_emit's store mask)"""
    prog, meta = small_mixer(fmt)
    assert meta["chains"][0]["tail"] == "stored" and meta["chains"][0]["out"] == [0]
    W = meta["width"]
    x = pb.lcg_input(100, 5, False, seed=67)
    o = po.OracleProgram(fmt, prog, fs=48000, random=3, dither=24)
    r = rt.Runtime(fmt, prog, fs=48000, random=3, dither=24)
    f = getattr(r.L, f"dspRuntimeBlock_{fmt}")
    prev = 0
    for b0, b1 in ((0, 37), (37, 38), (38, 100)):
        want = np.zeros((b1 - b0, W), dtype=np.int32)
        got = np.zeros((b1 - b0, W), dtype=np.int32)
        o.L.oracle_run_block(o.ctx, o.cores[0], o.data_ptr, x[b0:b1].ctypes.data, 5, W, want.ctypes.data, W, 0, b1 - b0, W + 6)
        assert (want & 0xFF).max() == 0                                                 # 24-bit stores
        assert b1 - b0 < 8 or (want[:, 0] & 0xFF00).any()                               # (and bits for the tag to replace)
        for n in range(b1 - b0):                                                        # the plugin's lines, frame by frame
            new = int(want[n, 0]) & -65536
            want[n, 0] = np.int32(new | (prev & 0xFF00))
            prev = ((new >> 8) + 0x100) & 0xFFFFFFFF
            prev = prev - (1 << 32) if prev & 0x80000000 else prev
        assert f(r.cores[0], r.rundata, x[b0:b1].ctypes.data, 5, W, got.ctypes.data, W, 0, b1 - b0) == 0
        if b0 == 0:
            assert rt.lib().dspRuntimeTagOutputReset(0) == 0
        r.tag_output(got, 0)
        same(got, want, meta, f"format {fmt}, frames {b0} .. {b1}")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}")


@pytest.mark.parametrize("fmt", [6, 2])
def test_a_block_of_2051_frames(fmt):
    """cut at 1024 frames inside the call: the stage stores its chains into the caller's block at the cut's offset"""
    prog, meta = small_mixer(fmt)
    W = meta["width"]
    x = lcg(2051, 5, fmt, 68)
    run_vs_oracle(fmt, prog, meta, x, [2051])


def test_a_block_of_2051_frames_in_place():
    import torch
    prog, meta = small_mixer(6)
    W, B = meta["width"], 2051
    x = lcg(B, 5, 6, 69)
    o = po.OracleProgram(6, prog)
    want = o.run_block(x, W, W)
    r = rt.Runtime(6, prog)
    frame = np.zeros((B, W), dtype=np.float32)
    frame[:, :5] = x                                                         # input IO W + j lies in column j, where output j goes
    d = dm.to_device(frame)
    r.run_block_device(d.data_ptr(), W, W, d.data_ptr(), W, 0, B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same(dm.to_host(d), want, meta, "2051 frames in place")
    same_state(r.sync_state(), o.state, meta, "2051 frames in place")


# ---- 7. windows with offsets and spare columns ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [6, 4, 2])
def test_windows_with_offsets_and_spare_columns(fmt):
    """the input window begins two IOs below the smallest list IO, the output window at IO 3 (the chains store IO 5 ..), both strides
    four wider than the IOs in use; what no chain stores keeps the caller's words, with mux_tile (a group of 16) and mux_plain"""
    prog, meta = windows_program(fmt)
    W = meta["width"]
    lo = min(min(ch["ios"]) for ch in meta["chains"])
    hi = max(max(ch["ios"]) for ch in meta["chains"])
    assert (lo, hi) == (10, 16)
    in_base, in_stride = W + lo - 2, (hi - lo + 1) + 2 + 4
    out_base, out_stride = 3, (W - 3) + 4
    assert out_base + out_stride <= in_base                                  # (the oracle keeps one frame for both windows)
    x = lcg(83, in_stride, fmt, 71)                                          # (the columns outside the lists hold samples too)
    sentinel = np.full((83, out_stride), 0x5A5A5A5A, dtype=np.uint32).view(rt.sample_dtype(fmt))
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    assert r.mux_info() == dict(mux_chains=21, groups=1, grouped_chains=16, longest_list=4)
    stored = sorted(io - out_base for ch in meta["chains"] for io in ch["out"])
    kept = [c for c in range(out_stride) if c not in stored]
    assert kept == [0, 1] + list(range(out_stride - 4, out_stride))
    pos = 0
    for b in (66, 1, 16):
        want = o.run_block(x[pos:pos + b], out_stride, in_base, out_base, out=sentinel[pos:pos + b].copy())
        got = r.run_block(x[pos:pos + b], out_stride, in_base, out_base, out=sentinel[pos:pos + b].copy())
        assert (words(got)[:, kept] == 0x5A5A5A5A).all(), f"format {fmt}: a column that no chain stores was written"
        assert (words(got)[:, stored] != 0x5A5A5A5A).any(axis=0).all()
        same(got, want, meta, f"format {fmt}, block at frame {pos}", first_io=out_base)
        pos += b
    same_state(r.sync_state(), o.state, meta, f"format {fmt}")


# ---- 8. a one-frame block call in place -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [6, 2])
def test_one_frame_in_place(fmt):
    """143 chains that the stage stores itself (format 6: three workgroups of mux_tile and mux_plain; format 2: three waves of
    mux_plain), one frame, input IO W + j in the column where output j goes: the stage reads a copy of the frame.  (Without the
    copy, a wave that stores columns 0 .. 5 before another has read them changes that one's sums; whether it happens is timing.)"""
    import torch
    prog, meta = stored_program(fmt)
    W, I = meta["width"], meta["inputs"]
    assert W == 143 and all(ch["tail"].startswith("stored") for ch in meta["chains"])
    x = lcg(6, I, fmt, 81)
    o = po.OracleProgram(fmt, prog)
    r = rt.Runtime(fmt, prog)
    for n in range(6):
        want = o.run_block(x[n:n + 1], W, W)
        frame = np.zeros((1, W), dtype=rt.sample_dtype(fmt))
        frame[0, :I] = x[n]
        d = dm.to_device(frame)
        r.run_block_device(d.data_ptr(), W, W, d.data_ptr(), W, 0, 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same(dm.to_host(d), want, meta, f"format {fmt}, frame {n} in place")
    same_state(r.sync_state(), o.state, meta, f"format {fmt}")

"""A model of the READS of fir_tile's window ring (avdsp_amd/csrc/avdsp_kernels.hip, `RING`: four row tiles, lean boundary; DESIGN.md
4.2) -- a transcription of the kernel's integer arithmetic into plain Python and nothing else: the chunking (Sall, nch, ck),
ring_fetch_all / ring_store_all, ring_fetch / ring_store with both branches and the guard write, wcg's start, ring_down in front of
step 14, win_off<4>, slast and the EDGE 1 / EDGE 2 rules for which MFMAs are issued.  No sample is multiplied: the model tracks which
FRAME (relative to the tile's F0) every LDS cell of the window image holds, and says for every issued MFMA which frame each lane's
window operand came from.  The picture it is held to: lane (a, k) = (lane & 15, lane >> 4) of k-step s, m = -64 + 4 s,
multiplies x[F0 + 64 a - (m + k)].

It is a model of the reads, not a run of a wrong kernel: a mutation here is the same slip made in this transcription
(tests/test_fir_ring_model.py), and what it shows is which tap counts would put a wrong sample under a real tap."""
from __future__ import annotations

import numpy as np

NR, ROW, CKMAX = 64, 23, 96                  # TileGeom<4>: rows of the tile, doubles per window row, k-steps per chunk
RL, NC = ROW - 1, CKMAX // 16                # the ring's columns 1 .. RL (0: the guard); the columns a chunk adds at most
R = 4
UNSET = -(1 << 40)                           # a cell nothing was written to (or an address outside the image)

LANE = np.arange(64)
I16, K = LANE & 15, LANE >> 4


def win_off(j):
    """win_off<4>(j): doubles from the lane's column pointer to its operand of step j of a group"""
    return ((NR - (4 * j) % NR) % NR) * ROW - (4 * j + NR - 1) // NR + (64 // NR - 1)


WOFF = np.array([win_off(j) for j in range(16)])
STEP = np.arange(16)
WOFF_AHEAD = WOFF[(STEP + 2) & 15]           # a k-step reads the operands of the step two ahead
ROWTILE = np.arange(4)
FIRST = 4 * (3 - ROWTILE)                    # the first k-step of the launch at which row tile r has a tap

# the mutations of tests/test_fir_ring_model.py: name -> what differs.  Every key is read by name below.
MUTATIONS = {
    "ring_down wraps one column short": dict(down_to=RL - 1),
    "ring_down wraps one column late": dict(down_at=0),
    "the guard is not rewritten when column 22 is": dict(no_guard=True),
    "pc0 one too high": dict(pc0=+1),
    "pc0 one too low": dict(pc0=-1),
    "Dhi one too high in ring_fetch": dict(dhi_fetch=+1),
    "Dhi one too low in ring_fetch": dict(dhi_fetch=-1),
    "Dhi one too high in ring_store": dict(dhi_store=+1),
    "Dhi one too low in ring_store": dict(dhi_store=-1),
    "five columns staged instead of six": dict(nc=NC - 1),
    "the prologue stages 21 columns, the newest missing": dict(prologue=RL - 1),
    "the prologue stages 21 columns, the oldest missing": dict(prologue=RL - 1, prologue_from=RL - 2),
    "the pointer steps in front of step 13": dict(step_at=13),
    "the pointer steps in front of step 15": dict(step_at=15),
}


def chunking(T):
    """(Sall, nch, ck, slast) as the kernel computes them (SPLIT off: Sb = 0, S = Sall)"""
    Sall = (((T + NR + 3) >> 2) + 15) & ~15
    nch = max(1, (Sall + CKMAX - 1) // CKMAX)
    ck = max(16, (((Sall + nch - 1) // nch) + 15) & ~15)
    return Sall, nch, ck, (T - 1 + NR) >> 2


class Image:
    """the wave's window image: cell (row, physical column) at row * ROW + column, the frame it holds"""

    def __init__(self, mut):
        self.m = mut
        self.cells = np.full(NR * ROW, UNSET, dtype=np.int64)

    def put(self, col, frames):
        """win_put(wrow_lds, col, ...): every lane writes its row's cell of that column (lane = row)"""
        if frames is not None:
            self.cells[LANE * ROW + col] = frames

    def load(self, addr):
        ok = (addr >= 0) & (addr < NR * ROW)
        return np.where(ok, self.cells[np.where(ok, addr, 0)], UNSET)

    # ---- the prologue
    def fetch_all(self):
        n, top = self.m.get("prologue", RL), self.m.get("prologue_from", RL - 1)
        b0 = -3 + 64 * (16 - top) + LANE
        return [b0 + 64 * t if t < n else None for t in range(RL)]       # wpro[t]; None: a register never loaded

    def store_all(self, wpro):
        n, shift = self.m.get("prologue", RL), (RL - 1) - self.m.get("prologue_from", RL - 1)
        for t in range(n):
            self.put(1 + t + shift, wpro[t])
        self.put(0, wpro[RL - 1])

    # ---- a later chunk's boundary
    def fetch(self, s0, ckc):
        Dhi = (s0 >> 4) + (ckc >> 4) + 15 + self.m.get("dhi_fetch", 0)
        b0 = -3 + 64 * (16 - Dhi) + LANE
        n = self.m.get("nc", NC)
        return [b0 + 64 * t if t < n else None for t in range(NC)]       # wreg[t]

    def store(self, s0, ckc, wreg):
        Dhi = (s0 >> 4) + (ckc >> 4) + 15 + self.m.get("dhi_store", 0)
        pc0 = RL - Dhi % RL + self.m.get("pc0", 0)
        n = self.m.get("nc", NC)
        if pc0 + n <= RL:
            for t in range(n):
                self.put(pc0 + t, wreg[t])
        else:
            for tl in range(n):
                if RL - pc0 == tl:                                       # wreg[tl] is physical column RL
                    for t in range(n):
                        self.put(RL - tl + t if t <= tl else t - tl, wreg[t])
                    if not self.m.get("no_guard"):
                        self.put(0, wreg[tl])


_cache = {}


def groups(T, mut=None):
    """groups_of(Sall, slast): the reads depend on the tap count through these two alone (the last call's answer is kept: T and T + 1
    mostly share them)"""
    Sall, _, _, slast = chunking(T)
    key = (Sall, slast, tuple(sorted((mut or {}).items())))
    if _cache.get("key") != key:
        _cache["key"], _cache["groups"] = key, groups_of(T, mut)
    return _cache["groups"]


def groups_of(T, mut=None):
    """the wave's groups of 16 k-steps, in order: (sg, frames, issued) -- sg the group's first k-step, frames[j][lane] the frame the
    lane's window operand of step sg + j came from (UNSET: from a cell never written), issued[j][r] whether row tile r's MFMA of that
    step is issued; both cut at the step an EDGE 2 group ends at"""
    mut = mut or {}
    Sall, nch, ck, slast = chunking(T)
    img = Image(mut)
    step_at, down_at, down_to = mut.get("step_at", 14), mut.get("down_at", 1), mut.get("down_to", RL)
    wcol1 = (3 - K) * ROW + 1                                  # the lane's row, physical column 1
    wcg = wcol1 + (RL - 16 + I16)

    def ring_down(p):
        return np.where(p == wcol1 - 1 + down_at, wcol1 - 1 + down_to, p - 1)

    out = []
    pending = img.fetch_all()
    for s0 in range(0, Sall, ck):
        ckc = min(ck, Sall - s0)
        if s0 == 0:
            img.store_all(pending)
        else:
            img.store(s0, ckc, pending)
        if s0 + ckc < Sall:
            pending = img.fetch(s0 + ckc, min(ck, Sall - s0 - ckc))
        carry = np.stack((wcg + WOFF[0], wcg + WOFF[1]))       # chunk_begin
        gfull = min(ckc // 16, ((slast - 4 * (R - 1) - 15 - s0) >> 4) + 1)
        for g in range(ckc // 16):
            sg = s0 + 16 * g
            edge = 1 if (g == 0 and s0 == 0 and gfull > 0) else 0 if g < gfull else 2
            n = 16 if edge != 2 else min(16, max(0, slast - sg + 1))
            down = ring_down(wcg)
            # step t reads for step t + 2: reads[t][lane]
            reads = np.where(STEP[:, None] < step_at, wcg[None, :], down[None, :]) + WOFF_AHEAD[:, None]
            addr = np.concatenate((carry, reads[:14]))[:n]
            frames = img.load(addr)
            s = sg + STEP[:n, None]
            if edge == 0:
                issued = np.ones((n, R), dtype=bool)
            elif edge == 1:
                issued = STEP[:n, None] >= FIRST[None, :]
            else:
                issued = (s - FIRST[None, :] >= 0) & (s - FIRST[None, :] <= slast - 4 * ROWTILE[None, :] - FIRST[None, :])
            out.append((sg, frames, issued))
            if n == 16:
                carry = reads[14:]
            if n > step_at:
                wcg = down
    return out


def wave(T, mut=None):
    """the groups in one piece: (s[N], frames[N][lane], issued[N][r]) over the N k-steps the wave runs"""
    g = groups(T, mut)
    if "wave" not in _cache or _cache["wave"][0] is not g:
        _cache["wave"] = (g, np.concatenate([sg + STEP[:len(f)] for sg, f, _ in g]), np.concatenate([f for _, f, _ in g]), np.concatenate([i for _, _, i in g]))
    return _cache["wave"][1:]


def picture(s):
    """frames[n][lane] of the k-steps s[n] as the picture has them: 64 a - (m + k), m = -64 + 4 s"""
    return 64 * I16[None, :] - (-NR + 4 * s[:, None] + K[None, :])


def real(T, s):
    """real[n][r][k]: row tile r's MFMA at k-step s[n] meets a tap 0 .. T-1 in the lanes of k: their taps are h[m + k + 16 r + i],
    i = 0 .. 15"""
    lo = -NR + 4 * s[:, None, None] + ROWTILE[None, None, :] + 16 * ROWTILE[None, :, None]
    return (lo + 15 >= 0) & (lo <= T - 1)


def mfmas(T, mut=None):
    """every issued MFMA: (k-step, row tile, the 64 lanes' operand frames)"""
    s, frames, issued = wave(T, mut)
    for n in range(len(s)):
        for r in range(R):
            if issued[n, r]:
                yield int(s[n]), r, frames[n]


def wrong_reads(T, mut=None):
    """(issued MFMAs, lanes of them whose operand is not the picture's, those of these that meet a real tap)"""
    s, frames, issued = wave(T, mut)
    bad = frames != picture(s)                                                 # [n][lane]
    hit = bad[:, None, :] & issued[:, :, None]                                 # [n][r][lane]
    return int(issued.sum()), int(hit.sum()), int((hit & real(T, s)[:, :, K]).sum())


def sees(T, mut):
    return wrong_reads(T, mut)[2] > 0

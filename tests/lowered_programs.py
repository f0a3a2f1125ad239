"""Random programs over the whole grammar that the host lowers to the chain kernels with the seven opt-in options on -- "chain_finish",
"chain_delay", "fir_tail", "mux_tail", "chain_mem", "chain_copy", "mem_fir"  -- and what the host's report calls
have to say of each core.  Test infrastructure, importable without a GPU: tests/test_lowered_programs.py holds it to the host,
tests/dev/gpu_lowered_sweep.py plays the programs on the device against the oracle, tests/golden/make_lowered_goldens.py pins the oracle to
the compiled reference on some of them.

random_lowered_program(seed, fmt) -> (program words, input stride from IO IN, output stride from IO 0, description).  The words are built
by tests/firtree_programs.program() from the item builders of the feature modules (trunk, branch, plain, copies; LOAD_MUX lists drawn by
tests/mux_recipes.mixer_lists); words and description come from one draw, and the same (seed, fmt) always gives the same words.

A program has 1 to 4 cores, each of one class:

    plain   LOAD | LOAD_GAIN, [BIQUADS], [FIR], [DELAY A], [SAT0DB | dressed finish | nothing], [DELAY B], STORE+ ; both delay forms; a
            fir_shared group (16 or more chains of one impulse bank) with one or two handed chains of that bank beside it; repeated
            stores (the chain left without a STORE has a DSP_DELAY); LOAD_STORE lists in front of the TPDF_CALC, between chains, at the end
    mux     as plain, some heads LOAD_MUX (a mix group of one IO sequence, private lists of 1 to 20 entries); no memory words
    tree    STORE_MEM trunks with and without sections and a FIR; branches without a FIR, with sections and a FIR, a FIR alone (ring
            feeds), handed endings; branches of a word the core only reads (an earlier core's, or nobody's); ordinary chains beside; lists
    pairs   LOAD_STORE pairs alone: forwarding, a dead pair, a self-copy

Core 0 may begin with TPDF_CALC(0).  Format 2 has no FIR; formats 3 and 5 get plain SAT0DB chains, lists and pairs cores only.  Every core
holds something that only the options lower, so that none of them is lowered with the options off.  Sizes come from the kernels' edges:
CHAINS chains a core, SECS sections, TAPS taps (rarely 1030, in a small core), lines of US microseconds; a parameter delay may ask for 0
(a bypass) or for more than its line holds (clamped).

Not produced, because the host refuses it: overlapping lines or a line inside a FIR history (the encoder lays them out apart), a pair that
feeds a chain or copies a chain's output, a TPDF_CALC of another width, memory words beside LOAD_MUX heads.  Not produced, because the
reference leaves it undefined (tests/fuzz_programs.py): a DSP_FIR in format 2, gains and list lengths that could carry a float
accumulator to Inf."""
from __future__ import annotations

import numpy as np

from avdsp_amd import progbuilder as pb
from tests import copy_programs as cp
from tests import delay_programs as dp
from tests import firtree_programs as tp
from tests import mux_recipes as mr
from tests.finish_programs import FINISHES, OP_SAT0DB_GAIN, OP_SAT0DB_TPDF_GAIN, OP_TPDF_CALC, words_of

IN = tp.IN
IN_STRIDE = 288                                      # inputs IO IN .. IN + 287: the chains' loads from 0 up, LOAD_MUX entries below SPARE, self-copies from SPARE on
SPARE = 280
OPTIONS = ("chain_finish", "chain_delay", "fir_tail", "mux_tail", "chain_mem", "chain_copy", "mem_fir")
CHAINS = [1, 2, 15, 16, 17, 37, 66]                  # the 16-lane rows, a wave, a stage tile closed by a tree's columns
SECS = [0, 1, 2, 16, 17, 40]
TAPS = [1, 7, 15, 16, 17, 63, 97, 300]
US = [63, 21, 150, 1000, 2100, 7000]                 # lines of 3, 1, 7, 47, 100 and 336 samples at 48 kHz
MAX_CHAINS, MAX_TAPS = 150, 26000                    # per program: what the oracle gets through in a moment
OP_LOAD_STORE, OP_LOAD_MEM, OP_STORE_MEM, OP_DELAY, OP_CORE = 38, 39, 40, 47, 3

FORMS = ("dressed finish", "delay A", "delay B", "parameter-form delay", "plain FIR chain", "handed FIR chain", "fir_shared group",
         "LOAD_MUX head", "trunk", "FIR trunk", "plain branch", "sections + FIR branch", "ring-fed branch", "branch of an unwritten word",
         "live copy pair", "dropped store", "head TPDF_CALC")
TREE_FORMS = ("trunk", "FIR trunk", "plain branch", "sections + FIR branch", "ring-fed branch", "branch of an unwritten word")
# what one core may not hold together (no memory words beside LOAD_MUX heads; 4.2l: the chains of a core with a tree are
# not offered to fir_shared); every other pair of forms is lowered side by side
EXCLUDED = {frozenset((a, b)) for a in ("LOAD_MUX head", "fir_shared group") for b in TREE_FORMS}
ALLOWED_PAIRS = [(a, b) for i, a in enumerate(FORMS) for b in FORMS[i + 1:] if frozenset((a, b)) not in EXCLUDED]


# ---- the draw -------------------------------------------------------------------------------------------------------------------------------
class _Draw:
    def __init__(self, seed, fmt):
        self.r = np.random.default_rng(77000 + 10 * seed + (2 if fmt == 2 else 3 if fmt in (3, 5) else 6))
        self.fmt = fmt
        self.lane = fmt in (3, 5)
        self.fir = fmt != 2
        self.taps_left = MAX_TAPS
        self.next_out = 0
        self.next_bank = 0
        self.next_spare = SPARE
        self.trunk_keys = []                         # of earlier cores

    def pick(self, seq, p=None):
        return seq[int(self.r.choice(len(seq), p=p))]

    def chance(self, p):
        return bool(self.r.random() < p)

    def out(self):
        self.next_out += 1
        return self.next_out - 1

    def taps(self, few=False, p=0.45):
        if not self.fir or not self.chance(p):
            return 0
        t = 1030 if few and self.chance(0.25) else self.pick(TAPS)
        if t > self.taps_left:
            t = self.pick([1, 7, 15])
        self.taps_left -= t
        return t

    def tail(self, few=False, taps=None):
        """what stands behind a chain's load"""
        r = self.r
        kw = dict(nsec=self.pick(SECS, [0.3, 0.2, 0.2, 0.1, 0.1, 0.1]), taps=self.taps(few) if taps is None else taps,
                  load_gain=None if self.chance(0.3) else float(np.float32(r.uniform(0.2, 0.9))), stores=2 if self.chance(0.2) else 1)
        if self.lane:
            kw.update(slot=None, finish="sat")
            return kw
        slot = self.pick([None, "A", "B"], [0.5, 0.25, 0.25])
        form, us = self.pick(["fixed", "param"]), self.pick(US)
        max_us = 2 * us + 50
        if form == "param":
            v = r.random()
            if v < 0.2:
                us, max_us = 0, 2100                 # a bypass
            elif v < 0.4:
                max_us = max(us // 2, 21)            # more than the line holds: clamped
        kw.update(slot=slot, form=form, us=us, max_us=max_us, finish=self.pick(["sat", "none", "tpdf", "gain", "tpdf_gain"]),
                  gain=float(np.float32(r.uniform(0.5, 1.2))))
        return kw

    def lists(self, n_lists):
        """LOAD_STORE lists: sources among the inputs, destinations where no chain stores; with forwarding, a dead pair and a self-copy"""
        out = []
        for _ in range(n_lists):
            n = self.pick([1, 2, 5, 17], [0.3, 0.3, 0.3, 0.1])
            pairs = [(IN + int(self.r.integers(0, IN_STRIDE)), self.out()) for _ in range(n)]
            if n >= 2 and self.chance(0.6):
                pairs.append((pairs[0][1], self.out()))                      # forwarding: reads the first pair's destination
            if n >= 2 and self.chance(0.6):
                pairs.append((IN + int(self.r.integers(0, IN_STRIDE)), pairs[1][1]))      # a second writer: the first pair of that IO is dead
            if self.chance(0.4) and self.next_spare < IN_STRIDE:
                pairs.append((IN + self.next_spare, IN + self.next_spare))  # a self-copy, of an input no chain reads
                self.next_spare += 1
            out.append(cp.copies(pairs))
        return out

    def sprinkle(self, items, core):
        """0 to 3 lists in the legal positions: in front of the TPDF_CALC, between chains (behind a trunk's STORE_MEM too), at the end"""
        for lst in self.lists(self.pick([0, 1, 2, 3], [0.45, 0.3, 0.15, 0.1])):
            where = self.pick(["head", "between", "end"])
            if where == "head":
                core["head"].append(lst)
            elif where == "end":
                items.append(lst)
            else:
                items.insert(int(self.r.integers(0, len(items) + 1)), lst)

    def repeated_stores(self, chains):
        """two chains store one IO: the earlier STORE is dead; where that leaves the earlier chain without one it has a DSP_DELAY"""
        if self.lane or len(chains) < 2 or not self.chance(0.4):
            return
        i, j = sorted(int(v) for v in self.r.choice(len(chains), 2, replace=False))
        a, b = chains[i], chains[j]
        if a["bank"] is not None:                                            # (a chain of the shared bank stays what it is)
            return
        if a["slot"] is None:
            a.update(slot=self.pick(["A", "B"]), form="fixed", us=self.pick(US[:4]))
            a["max_us"] = 2 * a["us"] + 50
        b["store_to"] = [a["store_to"][-1]] + b["store_to"][:3]
        a["dropped"] = True

    def stores(self, chains):
        for c in chains:
            if c["kind"] != "trunk":
                c["store_to"] = [self.out() for _ in range(c["stores"])]

    # ---- the classes ----
    def plain_core(self, n, mux=False):
        few = n <= 2
        chains = [tp.plain(**self.tail(few)) for _ in range(n)]
        if self.fmt in (4, 6) and n >= 16 and self.chance(0.55):
            g = 16 if n <= 17 else int(self.r.integers(16, min(n - 2, 24) + 1))
            t = self.pick([7, 16, 17, 63, 97])
            bank, self.next_bank = self.next_bank, self.next_bank + 1
            self.taps_left -= t * g
            for c in chains[:g]:                                             # the group: plain FIR chains of one bank
                c.update(taps=t, bank=bank, slot=None, finish=self.pick(["sat", "none"]), nsec=self.pick([0, 1, 2, 17], [0.4, 0.25, 0.25, 0.1]))
            for c in chains[g:g + self.pick([1, 2])]:                        # handed chains of the same bank beside it
                c.update(taps=t, bank=bank)
                if c["slot"] is None and c["finish"] not in FINISHES:
                    c.update(finish=self.pick(list(FINISHES)))
            chains = [chains[int(k)] for k in self.r.permutation(n)]
        if mux:
            self.mux_heads(chains)
        self.stores(chains)
        self.repeated_stores(chains)
        return chains

    def mux_heads(self, chains):
        """LOAD_MUX heads: one IO sequence for a run of chains (a mix group from 16 on), private lists, some LOAD / LOAD_GAIN heads left"""
        n = len(chains)
        seed = int(self.r.integers(1, 1 << 30))
        shared = n if n < 16 else self.pick([16, 17, n])
        shared = max(1, shared - (1 if n in (2, 15) else 0))
        entries = self.pick([1, 2, 3, 6, 20])
        base = int(self.r.integers(0, SPARE - 24))
        group = mr.mixer_lists(dict(outputs=shared, inputs=max(entries, 2), entries=entries, lists=self.pick(["shared", "shuffled"]), seed=seed))
        order = [int(k) for k in self.r.permutation(n)]
        for k, lst in zip(order[:shared], group):
            chains[k]["mux"] = [(base + io, g) for io, g in lst]
        for k in order[shared:]:
            if self.chance(0.7):
                e = self.pick([1, 2, 5, 8, 20])
                lst = mr.mixer_lists(dict(outputs=1, inputs=24, entries=e, lists="private", seed=seed + k + 1))[0]
                chains[k]["mux"] = [(base + io, g) for io, g in lst]

    def tree_core(self, n):
        items, late, count, trees = [], [], 0, 0
        me = len(self.trunk_keys)

        def a_branch(key):
            kind = self.pick(["plain", "sections+fir", "feed", "handed"]) if self.fir else "plain"
            kw = self.tail()
            if kind == "plain":
                kw["taps"] = 0
            else:
                if not kw["taps"]:
                    kw["taps"] = self.taps(p=1.0)
                kw["nsec"] = self.pick([1, 2, 17]) if kind == "sections+fir" else 0 if kind == "feed" else kw["nsec"]
                if kind == "handed" and kw["slot"] is None and kw["finish"] not in FINISHES:
                    kw["finish"] = self.pick(list(FINISHES))
                if kind != "handed":
                    kw.update(slot=None, finish=self.pick(["sat", "none"]))
            return tp.branch(key, **kw)

        mine = []
        while count < n:
            left, v = n - count, self.r.random()
            if v < 0.2 and trees:
                items.append(tp.plain(**self.tail()))
                count += 1
            elif v < 0.35 or (left == 1 and self.chance(0.5)):
                key = self.pick(self.trunk_keys) if self.trunk_keys and self.chance(0.8) else f"w{me}_{count}"
                items.append(a_branch(key))
                count += 1
            else:
                key = f"t{me}_{trees}"
                trees += 1
                mine.append(key)
                items.append(tp.trunk(key, self.pick(SECS, [0.3, 0.2, 0.2, 0.1, 0.1, 0.1]), self.taps(p=0.5),
                                      None if self.chance(0.3) else float(np.float32(self.r.uniform(0.2, 0.9)))))
                items += late
                late = []
                count += 1
                fan = min(left - 1, self.pick([0, 1, 2, 3, 4, 17], [0.1, 0.25, 0.25, 0.2, 0.15, 0.05]))
                for _ in range(fan):
                    (late if self.chance(0.25) else items).append(a_branch(key))
                count += fan
        items += late
        chains = [it for it in items]
        self.stores(chains)
        self.repeated_stores([c for c in chains if c["kind"] != "trunk"])
        self.trunk_keys += mine
        return items

    def pairs_core(self):
        lists = []
        while not lists or not cp.resolve([p for lst in lists for p in lst["pairs"]]):
            lists = self.lists(self.pick([1, 2]))
        return lists


def _depends_on_the_options(core):
    return bool(core["head"]) or core["calc"] is not None or any(
        it["kind"] in ("copies", "trunk", "branch") or it.get("dropped") or it["slot"] is not None or it["finish"] in FINISHES for it in core["items"])


def draw_cores(seed, fmt):
    d = _Draw(seed, fmt)
    cores, total = [], 0
    for k in range(int(d.r.integers(1, 5))):
        if d.lane:
            cls = d.pick(["plain", "pairs"], [0.8, 0.2])
        else:
            cls = d.pick(["plain", "mux", "tree", "pairs"], [0.3, 0.25, 0.35, 0.1])
        n = d.pick(CHAINS)
        if total + n > MAX_CHAINS:
            n = d.pick([1, 2, 15])
        core = tp.core([], calc=0 if k == 0 and not d.lane and cls != "pairs" and d.chance(0.6) else None)
        core["cls"] = cls
        if cls == "pairs":
            core["items"] = d.pairs_core()
        else:
            total += n
            core["items"] = d.tree_core(n) if cls == "tree" else d.plain_core(n, mux=cls == "mux")
            d.sprinkle(core["items"], core)
            if not _depends_on_the_options(core):
                core["items"] += d.lists(1)
        cores.append(core)
    assert d.next_out + 2 <= IN, "the outputs stay below the first input"
    return cores, d.next_out + 2                      # (two columns nobody writes: they keep the player's sentinel)


# ---- the description ------------------------------------------------------------------------------------------------------------------------
def chains_of(core):
    return [it for it in core["items"] if it["kind"] != "copies"]


def all_pairs(core):
    return [p for it in core["head"] + core["items"] if it["kind"] == "copies" for p in it["pairs"]]


def shared_groups(core):
    """the groups fir_shared takes: 16 or more plain FIR chains of one bank, in a core without memory words"""
    ch = chains_of(core)
    if any(c["kind"] != "plain" for c in ch):
        return []
    n = {}
    for c in ch:
        if c["bank"] is not None and tp.has_fir(c) and not tp.is_handed(c):
            n[c["bank"]] = n.get(c["bank"], 0) + 1
    return [v for v in n.values() if v >= 16]


def chain_forms(it, core, written_before):
    """the forms of FORMS that one chain is"""
    f = []
    if it["kind"] == "trunk":
        return ["trunk"] + (["FIR trunk"] if tp.has_fir(it) else [])
    if it["finish"] in FINISHES:
        f.append("dressed finish")
    if it["slot"]:
        f.append("delay " + it["slot"])
        if it["form"] == "param":
            f.append("parameter-form delay")
    if it["kind"] == "plain" and tp.has_fir(it):
        f.append("handed FIR chain" if tp.is_handed(it) else "plain FIR chain")
    if it.get("mux"):
        f.append("LOAD_MUX head")
    if it["kind"] == "branch":
        f.append("plain branch" if not tp.has_fir(it) else "sections + FIR branch" if it["nsec"] else "ring-fed branch")
        if it["key"] not in {c["key"] for c in chains_of(core) if c["kind"] == "trunk"}:
            f.append("branch of an unwritten word")
    if it.get("dropped"):
        f.append("dropped store")
    return f


def describe(cores, fmt, fs=48000):
    """per core: its class, the forms it holds, the form of every chain, and what the host's report calls say of it with every option on"""
    out, written = [], set()
    for core in cores:
        ch = chains_of(core)
        per_chain = [chain_forms(it, core, written) for it in ch]
        forms = {f for fs_ in per_chain for f in fs_}
        pairs = all_pairs(core)
        live = cp.resolve(pairs)
        if live:
            forms.add("live copy pair")
        if core["calc"] is not None:
            forms.add("head TPDF_CALC")
        groups = shared_groups(core)
        if groups:
            forms.add("fir_shared group")
        own = {c["key"] for c in ch if c["kind"] == "trunk"}
        reads_earlier = any(c["kind"] == "branch" and c["key"] in written and c["key"] not in own for c in ch)
        delayed = [c for c in ch if c["kind"] != "trunk" and c["slot"]]
        dressed = [c for c in ch if c["kind"] != "trunk" and c["finish"] in FINISHES]
        has_mux = any(c.get("mux") for c in ch)
        stage = [c for c in ch if c.get("mux") and not c["nsec"] and not tp.has_fir(c) and (c["slot"] or c["finish"] in FINISHES)]
        mem = dict(items=ch)
        info = dict(chains=len(ch), copy=(len(pairs), len(live)), finish=(len(dressed), int(core["calc"] is not None)),
                    delay=(len(delayed), max([dp.samples(c["us"], fs, c["max_us"] if c["form"] == "param" else None) for c in delayed] + [0])),
                    fir_tail=tp.tail_counts(mem), mux_tail=(len(dressed), len(delayed), len(stage)) if has_mux else (0, 0, 0),
                    mem=tp.mem_counts(mem), mem_fir=tp.fir_counts(mem),
                    fir_group=dict(groups=len(groups), grouped_chains=sum(groups), largest_group=max(groups + [0])))
        out.append(dict(cls=core["cls"], chains=len(ch), forms=forms, chain_forms=per_chain, info=info, reads_an_earlier_cores_word=reads_earlier,
                        stores=[list(c.get("store_to") or ()) for c in ch], live=live, trees=len(own), has_fir=any(tp.has_fir(c) for c in ch)))
        written |= own
    return out


_CACHE = {}


def random_lowered_program(seed, fmt):
    """-> (program words, input stride from IO IN, output stride from IO 0, description).  The description: dict(seed, fmt, cores -- see
    describe() --, words: {key: index of the memory word}, item lists as drawn under "drawn")"""
    key = (seed, 2 if fmt == 2 else 6 if fmt in (4, 6) else 3)
    if key not in _CACHE:
        cores, out_stride = draw_cores(seed, fmt)
        prog, nin, _, words = tp.program(fmt, cores, capacity=1 << 22, lines_last=True)
        assert nin <= SPARE
        for k, (name, w) in enumerate(sorted(words.items())):                # the words nobody writes start from values of their own
            if name.startswith("w"):
                tp.set_word(prog, w, (0.31 - 0.07 * (k % 7)) * (-1) ** k, 2 if fmt == 2 else 6)
        prog.flags.writeable = False
        _CACHE[key] = (prog, out_stride, cores, words)
    prog, out_stride, cores, words = _CACHE[key]
    return prog.copy(), IN_STRIDE, out_stride, dict(seed=seed, fmt=fmt, cores=describe(cores, fmt), words=dict(words), drawn=cores)


# ---- where things are in the words (for the player's edits and its messages) -------------------------------------------------------------------
def gain_bits(fmt, v):
    """a gain as the encoding holds it: Q4.28 in format 2, a float else"""
    return int(round(v * (1 << 28))) & 0xFFFFFFFF if fmt == 2 else int(np.float32(v).view(np.uint32))


def editable_words(prog):
    """the words a live edit may write: LOAD_GAIN gains, finish gains, the microsecond words of parameter delays, LOAD_MUX gains"""
    rel = lambda at, k: at + int(np.int32(prog[at + k]))      # noqa: E731
    return dict(load_gain=sorted({rel(at, 2) for at in words_of(prog, pb.OP_LOAD_GAIN)}),
                finish_gain=sorted({rel(at, 1) for op in (OP_SAT0DB_GAIN, OP_SAT0DB_TPDF_GAIN) for at in words_of(prog, op)}),
                delay_us=sorted(set(dp.us_words(prog))),
                mux_gain=sorted({t + 2 + 2 * k for t in mr.mux_tables(prog) for k in range(int(prog[t]) & 0xFFFF)}))


def state_owners(prog, nfreq=2):
    """[(first data offset, core, chain of the core or -1, what)] sorted by offset: the state words the opcodes of every chain own"""
    out, core, chain, pos = [], -1, -1, 0
    while True:
        skip, op = int(prog[pos]) & 0xFFFF, int(prog[pos]) >> 16
        if skip == 0:
            break
        a = [int(np.int32(v)) for v in prog[pos + 1:pos + skip]]
        if op == OP_CORE:
            core, chain = core + 1, -1
        elif op in (pb.OP_LOAD, pb.OP_LOAD_GAIN, OP_LOAD_MEM):
            chain += 1
        elif op == pb.OP_LOAD_MUX:
            chain += 1
            out.append((a[1], core, chain, "LOAD_MUX result"))
        elif op == pb.OP_BIQUADS:
            out.append((a[0], core, chain, "biquad state"))
        elif op == pb.OP_FIR:
            out.append((a[nfreq], core, chain, "FIR history"))
        elif op == OP_DELAY:
            out.append((a[1], core, chain, "delay line"))
        elif op == OP_TPDF_CALC:
            out.append((a[1], core, -1, "TPDF_CALC result"))
        pos += skip
    return sorted(out)


def owner_of_state(owners, desc, offset):
    """text: whose state word `offset` is"""
    mine = [o for o in owners if o[0] <= offset]
    if not mine:
        return "no opcode's"
    _, core, chain, what = mine[-1]
    forms = desc["cores"][core]["chain_forms"][chain] if chain >= 0 else []
    return f"{what} of core {core} ({desc['cores'][core]['cls']}) chain {chain} [{', '.join(forms) or 'plain chain'}]"


def owner_of_column(desc, io):
    """text: which chain or pair stores output IO `io` (the last core that does)"""
    for k in range(len(desc["cores"]) - 1, -1, -1):
        c = desc["cores"][k]
        for n, st in enumerate(c["stores"]):
            if io in st:
                return f"core {k} ({c['cls']}) chain {n} [{', '.join(c['chain_forms'][n]) or 'plain chain'}]"
        if io in c["live"]:
            return f"core {k} ({c['cls']}) live pair from IO {c['live'][io]}"
    return "nobody's (the sentinel)"


# ---- scripts and the player ------------------------------------------------------------------------------------------------------------------
BLOCKS = [1, 2, 7, 64, 100, 333, 1024, 1029]         # a lane, under a wave, a wave, ragged, a launch, more than one launch
MAX_FRAMES = 2000
HEAD = 12                                            # program words of the header (its checksum covers them alone)
EVENTS = ("none", "other_call", "in_place", "toggle", "impl", "params", "checkpoint", "reset", "shard")
IMPLS = [("biquad_impl", 0, 1), ("fir_impl", 0, 1), ("fir_rows", 1, 0), ("fir_rows", 2, 0), ("fir_rows", 4, 0)]      # (key, value, default)
SHARD_WORLD = 3

# The committed slice: the seeds tests/test_gpu_lowered_sweep.py plays on the device and tests/test_lowered_programs.py holds to the host,
# per format.  Chosen (greedily, among seeds 0 .. 199) so that every pair of ALLOWED_PAIRS stands in one core somewhere, every form in
# a core of 16, of 17 and of 37 chains, and every event of EVENTS is drawn; 2, 10 and 12 in format 6 are the seeds that found the
# subnormal x words of biquad_pipe's state.  PINNED: the seeds tests/golden/lowered_f*.npz pin to the compiled reference.
SLICE = {2: [11, 5, 22, 56, 59, 0, 3, 6], 4: [5, 64, 75, 96, 124, 97, 102, 2], 6: [5, 64, 75, 96, 124, 36, 61, 2, 10, 12], 3: [0, 1, 2, 3], 5: [0, 1, 2, 3]}
PINNED = {2: [11, 5, 22, 56, 0, 3], 4: [5, 64, 75, 96, 124, 2], 6: [5, 64, 75, 96, 124, 2]}
GPU_CASES = ([(f"f{fmt}-{k // 3}", fmt, SLICE[fmt][k:k + 3]) for fmt in (2, 4, 6) for k in range(0, len(SLICE[fmt]), 3)]
             + [("lanes", None, [(fmt, s) for fmt in (3, 5) for s in SLICE[fmt]])])


def slice_runs():
    """every (seed, format) of the slice"""
    return [(seed, fmt) for fmt in sorted(SLICE) for seed in SLICE[fmt]]


def shardable(desc):
    """set_shard is for programs without memory words, lists and repeated stores (DESIGN.md 4.2j, 4.2k refuse them under a shard)"""
    return all(c["cls"] in ("plain", "mux") and c["info"]["copy"] == (0, 0) and "dropped store" not in c["forms"] for c in desc["cores"])


def script(seed, fmt):
    """the drawn run of a seed: dict(fs, random, dither, input, call, blocks, events) -- events[k] stands in front of block k (none in front
    of block 0), each a tuple whose first entry is one of EVENTS"""
    prog, _, _, desc = random_lowered_program(seed, fmt)
    rng = np.random.default_rng(91000 + 10 * seed + fmt)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]      # noqa: E731
    s = dict(fs=pick([48000, 44100, 48000]), random=pick([1, 12345]), dither=pick([24, 16, 31]), input=pick(["lcg", "stress"]),
             call=pick(["run_block", "run_block_all"]), blocks=[], events=[("none",)])
    left = MAX_FRAMES
    for _ in range(int(rng.integers(3, 7))):
        fit = [b for b in BLOCKS if b <= left]
        s["blocks"].append(pick(fit))
        left -= s["blocks"][-1]
    words = editable_words(prog)
    kinds = [k for k in EVENTS if (k != "shard" or shardable(desc))]
    for _ in s["blocks"][1:]:
        k = pick(kinds)
        if k == "toggle":
            ev = (k, pick(list(OPTIONS)))
        elif k == "impl":
            ev = (k,) + pick(IMPLS)
        elif k == "params":
            what = pick(sorted(w for w in words if words[w]) or [None])
            if what is None:
                ev = ("none",)
            else:
                at = pick(words[what])
                v = (pick([0, 21, 1000, 60000]) if what == "delay_us" else
                     gain_bits(fmt, float(rng.uniform(-0.45, 0.45) if what == "mux_gain" else rng.uniform(0.2, 1.1))))
                ev = (k, what, int(at), int(v))
        elif k == "checkpoint":
            ev = (k, pick([1, 777]))
        elif k == "reset":
            ev = (k, pick([44100, 48000]), pick([1, 4242]))
        elif k == "shard":
            ev = (k, int(rng.integers(0, SHARD_WORLD)))
        else:
            ev = (k,)
        s["events"].append(ev)
    return s


def sentinel(fmt, shape):
    out = np.empty(shape, dtype=np.float32 if fmt in (5, 6) else np.int32)
    out.view(np.uint32)[...] = 0x7FC0BEEF if fmt in (5, 6) else 0x5A5A1234
    return out


def script_input(seed, fmt, s):
    from tests.fuzz_programs import stress_input
    n = sum(s["blocks"])
    if s["input"] == "stress":
        return stress_input(np.random.default_rng(5000 + seed), n, IN_STRIDE, fmt in (5, 6))
    return pb.lcg_input(n, IN_STRIDE, fmt in (5, 6), seed=100 + seed)


class _OracleUnit:
    """a second oracle behind the player's device interface (play(device=False)): it takes the player's other route at a checkpoint -- a
    FRESH oracle given the saved state -- where the first oracle is reset and given its state back"""
    def __init__(self, fmt, prog, fs, random, dither):
        from oracle import pyoracle as po
        self.po, self.fmt = po, fmt
        self.o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
        self.rc, self.buf = self.o.rc, self.o.buf

    state = property(lambda self: self.o.state)

    def run(self, call, x, out):
        return self.o.run_block(x, out.shape[1], IN, out=out)

    def run_in_place(self, frame):
        return self.o.run_block(frame, frame.shape[1], 0, 0, out=frame)

    def sync_state(self):
        return self.o.state

    def set_option(self, key, value): pass
    def upload_params(self): pass
    def upload_state(self): pass
    def release(self): pass
    def shard(self, rank, world): pass

    def reset(self, fs, random, dither):
        return self.o.reset(fs, random, dither)

    def fresh(self, words, state, fs, random, dither):
        u = _OracleUnit(self.fmt, words, fs, random, dither)
        u.state[:] = state
        return u


class _DeviceUnit:
    def __init__(self, fmt, prog, fs, random, dither):
        from avdsp_amd import runtime as rt
        self.rt, self.fmt = rt, fmt
        self.r = rt.Runtime(fmt, prog, fs=fs, random=random, dither=dither)
        self.rc, self.buf = self.r.rc, self.r.buf
        for key in OPTIONS:
            self.r.set_option(key, 1)

    state = property(lambda self: self.r.state)

    def run(self, call, x, out):
        return getattr(self.r, call)(x, out.shape[1], IN, out=out)

    def run_in_place(self, frame):
        import torch
        from avdsp_amd import devmem as dm
        d = dm.to_device(frame)
        for k in range(len(self.r.cores)):                                   # cores outer, as the oracle's host loop
            self.r.run_block_device(d.data_ptr(), frame.shape[1], 0, d.data_ptr(), frame.shape[1], 0, frame.shape[0],
                                    torch.cuda.current_stream().cuda_stream, core_index=k)
        torch.cuda.synchronize()
        return dm.to_host(d)

    def sync_state(self):
        return self.r.sync_state()

    def set_option(self, key, value):
        self.r.set_option(key, value)

    def upload_params(self):
        self.r.upload_params()

    def upload_state(self):
        self.r.upload_state()

    def release(self):
        self.r.release()

    def shard(self, rank, world):
        self.r.set_shard(rank, world)

    def reset(self, fs, random, dither):
        return self.r.reset(fs, random, dither)

    def fresh(self, words, state, fs, random, dither):
        u = _DeviceUnit(self.fmt, words, fs, random, dither)
        u.state[:] = state
        u.upload_state()
        return u


def shard_range(total, world, rank):
    q, r = divmod(total, world)
    return rank * q + min(rank, r), q + (1 if rank < r else 0)


def play(seed, fmt, device=True, trace=None):
    """One seed: the program in one unit (an rt.Runtime with the seven options on; device=False: a second oracle) against one
    po.OracleProgram, block by block through the seed's script.  After every block the whole output block (written over a sentinel), the
    whole state area and the program words [HEAD, totalLength) are compared word for word.  -> [] or [the first mismatch, described].
    trace (a list): gets (event, frames, the oracle's outputs, state) per block"""
    from oracle import pyoracle as po
    prog, in_stride, out_stride, desc = random_lowered_program(seed, fmt)
    s = script(seed, fmt)
    x = script_input(seed, fmt, s)
    total = int(prog[1])
    owners = state_owners(prog)
    fs, random, dither = s["fs"], s["random"], s["dither"]
    o = po.OracleProgram(fmt, prog, fs=fs, random=random, dither=dither)
    u = (_DeviceUnit if device else _OracleUnit)(fmt, prog, fs, random, dither)
    assert o.rc >= 0 and u.rc == o.rc
    W = IN + in_stride
    pos, bad = 0, []
    try:
        for k, (n, ev) in enumerate(zip(s["blocks"], s["events"])):
            what = f"seed {seed} format {fmt} block {k} of {n} frames behind event {ev}"
            call, restore, cols, in_place = s["call"], None, None, False
            if ev[0] == "other_call":
                call = "run_block_all" if call == "run_block" else "run_block"
            elif ev[0] == "in_place":
                in_place = True
            elif ev[0] == "toggle":                           # the core replans onto the interpreter and, behind the block, back
                u.set_option(ev[1], 0)
                restore = (ev[1], 1)
            elif ev[0] == "impl":
                u.set_option(ev[1], ev[2])
                restore = (ev[1], ev[3])
            elif ev[0] == "params":                           # the edit goes into both program copies
                o.buf[ev[2]] = ev[3]
                u.buf[ev[2]] = ev[3]
                u.upload_params()
            elif ev[0] == "checkpoint":                       # the unit: a fresh one given the synced state; the oracle: reset, its state put back
                state, now = u.sync_state().copy(), u.buf[:total].copy()
                old, u = u, u.fresh(now, state, fs, ev[1], dither)
                old.release()
                keep = o.state.copy()
                assert o.reset(fs, ev[1], dither) >= 0
                o.state[:] = keep
                random = ev[1]
            elif ev[0] == "reset":
                fs, random = ev[1], ev[2]
                assert o.reset(fs, random, dither) >= 0 and u.reset(fs, random, dither) >= 0
            elif ev[0] == "shard":
                u.shard(ev[1], SHARD_WORLD)
                cols, mine = set(), set()
                for ci, c in enumerate(desc["cores"]):
                    lo, m = shard_range(c["chains"], SHARD_WORLD, ev[1])
                    for ch in range(lo, lo + m):
                        cols.update(c["stores"][ch])
                        mine.add((ci, ch))
            xb = x[pos:pos + n]
            if in_place:
                frame = sentinel(fmt, (n, W))
                frame[:, IN:] = xb
                want = frame.copy()
                o.run_block(want, W, 0, 0, out=want)
                got = u.run_in_place(frame)
            else:
                want = o.run_block(xb, out_stride, IN, out=sentinel(fmt, (n, out_stride)))
                got = u.run(call, xb, sentinel(fmt, (n, out_stride)))
            if cols is not None:                              # a shard stores its chains' columns alone
                other = [c for c in range(out_stride) if c not in cols]
                want[:, other] = sentinel(fmt, (n, len(other)))
                if not device:                                # (the second oracle knows no shards)
                    got[:, other] = sentinel(fmt, (n, len(other)))
            g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
            st, pw = u.sync_state(), u.buf[HEAD:total]
            if trace is not None:
                trace.append((ev, n, want.copy(), o.state.copy()))
            if (g != w).any():
                ch = int(np.nonzero((g != w).any(axis=0))[0][0])
                fr = int(np.nonzero(g[:, ch] != w[:, ch])[0][0])
                io = ch if in_place else ch
                bad.append(f"{what}: outputs differ, first in channel {ch} at frame {fr} ({int(g[fr, ch]):#010x} for {int(w[fr, ch]):#010x}; "
                           f"{np.count_nonzero((g != w).any(axis=0))} channels): {owner_of_column(desc, io)}")
                break
            diff = st != o.state
            if cols is not None:                              # ... and moves its chains' state alone
                own = np.zeros(len(diff), dtype=bool)
                edges = [a for a, *_ in owners] + [len(diff)]
                for (a, ci, ch, _), b in zip(owners, edges[1:]):
                    if ch < 0 or (ci, ch) in mine:
                        own[a:b] = True
                diff &= own
            if diff.any():
                at = int(np.nonzero(diff)[0][0])
                bad.append(f"{what}: state differs in {int(diff.sum())} words, first at data offset {at} ({int(st[at]):#010x} for {int(o.state[at]):#010x}): "
                           f"{owner_of_state(owners, desc, at)}")
                break
            if cols is None and (pw != o.buf[HEAD:total]).any():
                at = HEAD + int(np.nonzero(pw != o.buf[HEAD:total])[0][0])
                mem = [key for key, wd in desc["words"].items() if wd <= at < wd + 2]
                bad.append(f"{what}: program words differ, first at word {at} ({int(u.buf[at]):#010x} for {int(o.buf[at]):#010x})"
                           + (f": memory word {mem[0]}" if mem else ""))
                break
            if cols is not None:                              # the whole program again, from the oracle's state
                u.shard(0, 1)
                u.state[:] = o.state
                u.upload_state()
            if restore:
                u.set_option(*restore)
            pos += n
    finally:
        try:
            if device:
                u.shard(0, 1)
                for key in OPTIONS:
                    u.set_option(key, 0)
                for key, _, default in IMPLS:
                    u.set_option(key, default)
        finally:
            u.release()
    return bad

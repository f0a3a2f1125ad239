/*
 * avdsp_plan_layout.h -- the host-side tables of a chain plan, computed from an avdsp_plan_desc, and the choice of the FIR kernel
 * of a launch.  Plain C++17: no HIP header, no HIP call, nothing of the device -- avdsp_kernels.hip includes it, and so does the
 * stand-alone driver of tests/test_plan_layout.py, which runs every check below (they are what keeps a kernel from following a
 * word index out of the mirror) without a GPU.
 *
 * avdsp_hip_prog_add_plan runs the stages in this order; each returns its tables, or an error text for set_err:
 *     check_heads      section words, load modes, what LOAD_MUX chains refuse, the mirror words [lo, hi) that hold their lists
 *     mux_records      (plans with LOAD_MUX chains) the stage's records from the chains and those words, which the caller downloads; which chains the
 *                      stage stores, finishes or hands over itself ("mux_tail")
 *     copy_list        ("chain_copy") the live DSP_LOAD_STORE pairs against each other and against every IO the chains load and store; sorted by destination
 *     mem_trees        (plans with trunks or AVDSP_LOAD_MEM branches, "chain_mem") the trees, their hand-over rows, the columns of the branch block, mem_stage's tiles;
 *                      ("mem_fir") the trunks with a FIR and the stage's ring feeds
 *     check_chains     section ranges, IOs, FIR words, dressed finishes, delay lines, the IO spans, max_taps, the `fir`, `fir_hand`, `pass` and `tail` lists
 *     cascade_groups   launch groups by section count (dressed and delayed chains apart), pieces of long cascades, biquad_row's records, the merged row table
 *     shared_fir_layout, mux_tiles, and the scalars (fir_groups_per_chunk, ring_length, taps64_pitch, stores_whole_window, overlap_ok)
 */
#ifndef AVDSP_PLAN_LAYOUT_H_
#define AVDSP_PLAN_LAYOUT_H_

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "avdsp_hip.h"

namespace avdsp_layout {

constexpr int kFirChunk = 1024;      /* frames per launch: 4 MFMA tiles of 256 frames */
constexpr int kRingAhead = 3;        /* launches of frames a FIR ring holds beside the longest history ("overlap": cascade k waits for FIR k - 3) */
constexpr int kNG = 2;
constexpr int kMaxGpc = 56;          /* 896 tap positions per chunk: <= 27 KB of LDS, 5 workgroups per CU, no spills */
constexpr int kTapsLead = 64;        /* zeros in front of a chain's taps in the f64 copy */
constexpr int kTapsTail = 384;       /* zeros behind them (the last k-steps and the operand prefetch read on) */
/* Pieces of a long cascade: what travels between two sections is a 32-bit word -- (int)(acc >> 28), or the bits of (float)acc -- and
 * between two PIECES the same word goes through a scratch column: kLoadRaw takes a sample word as the first section's input as it is,
 * kStoreRaw (in the chain record's `sat`) stores the last section's result word as it is.  Device-side only; the host's descriptors
 * never hold them (check_heads refuses the load mode). */
constexpr int kLoadRaw = 2, kStoreRaw = 2;
/* "mem_fir" (DESIGN.md 4.2l): the load mode of a branch that is a FIR alone.  mem_stage has put the chain's input into its ring (the FEED
 * form); no FIR kernel and no fir_feed may append it a second time (they append for records with 0 sections: the device record of such a
 * chain says -1, dev_records in avdsp_kernels.hip).  Never in the host's descriptors, as kLoadRaw */
constexpr int kLoadFed = 5;
constexpr int kPieceMax = 16;        /* sections per piece: a cascade of more is cut into pieces that are each one biquad_row launch */
constexpr int kMuxRows = 64;         /* chains per mux_tile workgroup */

/* what biquad_row needs of a chain and of a section, one record per row slot / per lane of a launch group */
struct RowRec { int cid, in_io, out_io, flags; unsigned gain_bits; int pad[3]; };      /* flags: load_mode | sat << 8 | to_ring << 9 | raw << 10 | n_out << 16; pad[0]: the row's section count
                                                                                            (a launch with BiquadArgs::nsec 0 holds rows of several counts, four-row waves of one
                                                                                            count each; cid -1: a row that only fills its wave) */
struct LaneRec { int coef_word, state_word; };                                          /* -1: the lane holds no section */
/* a column group of fir_shared: chains ids[first .. first + n) (n <= 16) of group `group` (its taps row) */
struct SharedTile { int group, first, n, taps; };
struct MuxRec {                      /* one per chain of a plan that holds LOAD_MUX chains */
    int list_word, count;            /* first (IO, gain) pair in the mirror and the number of pairs; count 0: a LOAD / LOAD_GAIN chain
                                        beside them -- its sample word of IO `list_word` is copied into its column as it is */
    int result_word;                 /* the opcode's 8-byte result word in the mirror */
    int col;                         /* scratch column; -1: no filter behind the head, the stage stores the chain itself -- or ("mux_tail", the TAIL forms
                                        of the stage) finishes it, or hands its accumulator to chain_tail (ChainTables::hand_row) */
    int sat, n_out, out_io[AVDSP_MAX_STORES];
};
/* up to 64 chains of one mix group (lists of one IO sequence): four row tiles of mux_tile's workgroup */
struct MuxTile {
    int id0, nrec;                   /* its chains: ids[id0 .. id0 + nrec) */
    int count, kpad;                 /* list length, and that padded to a multiple of 4 (the pitch of the gains rows) */
    int list_word;                   /* the list that names the group's IO sequence (its first chain's) */
    long long g64;                   /* the gains as doubles, mulop(gain): [nrec][kpad] from here, zeros behind `count` */
};

/* "chain_mem" (DESIGN.md 4.2j): a tree is one memory word, the trunk that writes it (or none: the word is constant through a launch)
 * and the branches that read it.  mem_stage takes the accumulator of every frame from `src` and fans it out */
constexpr int kMemFrames = 64;       /* frames per mem_stage workgroup */
constexpr int kMemTileTrees = 16;    /* trees per mem_stage workgroup at most ... */
constexpr int kMemTileCols = 64;     /* ... and a tile is closed once it holds this many columns (one tree may bring more) */
enum { kMemSrcRow = 0, kMemSrcSample = 1, kMemSrcWord = 2, kMemSrcSum = 3 };
struct MemTree {
    int word;                        /* the first of the two mirror words */
    int src;                         /* kMemSrcRow: the trunk's hand-over row; kMemSrcSample: a trunk without sections, load_stage of its sample;
                                        kMemSrcWord: no trunk in this plan, the word as the mirror holds it when the launch starts;
                                        kMemSrcSum ("chain_sum"): a sum tree -- no word (0), no trunk, the accumulator formed from its MemTerms */
    int trunk;                       /* the trunk's chain, -1: none */
    int row;                         /* kMemSrcRow: the row read.  Else: a row the stage FILLS for chain_tail (branches without sections but with a
                                        delay line), -1: no such branch */
    int in_io, load_mode; unsigned gain_bits;      /* kMemSrcSample: the trunk's head */
    int col0, ncol;                  /* scratch columns of its branches with sections: [col0, col0 + ncol), in branch order */
    int first_own, n_own;            /* MemOwn records of the branches the stage finishes and stores itself */
};
struct MemOwn { int tree, cid, sat, finish; unsigned gain_bits; int n_out, out_io[AVDSP_MAX_STORES]; };
struct MemTile { int tree0, ntree, col0, ncol; };
/* "mem_fir" (DESIGN.md 4.2l): a branch with a FIR and no sections has no column -- mem_stage's FEED form puts the word the FIR takes of
 * every frame's accumulator into the chain's ring.  The feeds tree by tree: those of tree k are mem_feed[mem_feed_start[k] ..
 * mem_feed_start[k + 1]) (a table beside MemTree, whose layout the stage without feeds keeps) */
struct MemFeed { int tree, cid; };
/* "chain_sum" (DESIGN.md 4.2o): a sum head is a tree of its own (kMemSrcSum), behind all word trees; its one branch is the head's chain.
 * Its terms in program order: those of tree k are mem_terms[mem_sum_start[k] .. mem_sum_start[k + 1]) (again a table beside MemTree).
 * A term takes the accumulator exactly as a LOAD_MEM of its word would see it in that frame: kMemSrcRow, the hand-over row of the
 * word's trunk (sections or a FIR); kMemSrcSample, load_stage of the trunk's own sample (no sections -- never a row the stage itself
 * fills in the same launch); kMemSrcWord, the mirror's word when the launch starts (no chain of the core writes it).  op: 0 for the
 * first term, then AVDSP_SUM_ADD (newest + running) or AVDSP_SUM_SUB (newest - running) */
struct MemTerm { int src, row, word, in_io, load_mode; unsigned gain_bits; int op; };

/* "chain_copy" (DESIGN.md 4.2k): one live pair of the core's DSP_LOAD_STORE lists -- out[frame][dst] = in[frame][src], the raw word */
struct CopyPair { int src, dst; };
constexpr int kCopyIoLimit = 65536;  /* IO numbers of a pair: [0, kCopyIoLimit) */

inline std::string text(const char *fmt, ...)
{
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    return b;
}

inline int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

/* words every index of the plan must lie inside: the mirror, or all its copies (chain instances) */
inline long long mirror_words(const avdsp_plan_desc *d, int total_words) { return d->instances > 1 ? (long long)AVDSP_INSTANCE_STRIDE(total_words) * d->instances : total_words; }

/* ---- the chains ---- */
struct ChainTables {
    std::vector<avdsp_chain> chains;     /* the host's records; in a plan with LOAD_MUX chains every chain reads column i of the stage's
                                            scratch block -- a chain with a filter the word the stage has formed (kLoadRaw), a LOAD /
                                            LOAD_GAIN chain beside them its sample word, copied there */
    std::vector<int> coef, state;        /* per section: the word of b0 and of the six state words */
    bool has_mux = false;
    int mux_lo = 0x7FFFFFFF, mux_hi = 0; /* the mirror words that hold the lists */
    std::vector<MuxRec> mux_recs;
    std::vector<char> mux_stored;        /* chains the mux stage stores itself (no filter behind the head, no delay line) */
    int n_mux_stored = 0;
    /* "mux_tail" (DESIGN.md 4.2i): LOAD_MUX chains without a filter whose accumulator the stage hands to chain_tail (a delay line behind
     * the head; they are not stored by the stage), and those it finishes itself with a dressed finish (they are, and count above).  A plan
     * with either launches the TAIL forms of mux_tile and mux_plain, every other plan the stage as it was */
    std::vector<char> mux_handed;
    int n_mux_handed = 0, n_mux_finished = 0;
    bool mux_tail_forms() const { return n_mux_handed + n_mux_finished > 0; }
    std::vector<int> hand_row;           /* per chain: its row of the hand-over block (the chains of `tail` with a cascade, a FIR or a stage hand-over), else -1 */
    int n_hand_rows = 0;
    int io_in_min = 0x7FFFFFFF, io_in_max = -1, io_out_min = 0x7FFFFFFF, io_out_max = -1, max_taps = 0;
    std::vector<int> fir, pass;          /* chains with a FIR; chains with neither sections nor FIR */
    std::vector<int> pass_dressed;       /* ... of the latter, those with a dressed finish (they are not in `pass`) */
    int n_dressed = 0;                   /* chains with a dressed finish */
    std::vector<int> tail;               /* chains with a DSP_DELAY ("chain_delay"), the handed FIR chains and ("chain_ways") chains with way operations: chain_tail finishes and stores them (they are in neither pass list) */
    int n_way_ops = 0;                   /* "chain_ways": of those, the chains with way operations -- a plan with one launches chain_tail's OPS form */
    /* "fir_tail": the handed FIR chains -- a FIR, and a dressed finish and / or a delay behind it.  Their FIR launch (a HAND form) leaves
     * the accumulators in the hand-over block for chain_tail.  `fir` holds every chain with a FIR, they among them (rings, taps, history);
     * `fir_plain` those that store themselves */
    std::vector<int> fir_hand, fir_plain;
    /* "mem_fir" (DESIGN.md 4.2l): the trunks with a FIR.  They are in `fir` (ring, taps, history) and in neither list above: their launch,
     * a HAND form in front of mem_stage, leaves the sums in the trunks' rows, which the stage reads as it reads a cascade's */
    std::vector<int> fir_trunk;
    /* "chain_mem" (DESIGN.md 4.2j), made by mem_trees: the trees, the columns of the branch block, the branches the stage stores itself.
     * A branch with sections is a kLoadRaw chain of its column (phase 2: its cascade reads the branch block, not the caller's samples);
     * trunks and ordinary chains stay on the caller's block (phase 1) */
    bool has_mem = false;
    std::vector<char> mem_kind;          /* per chain: 0 ordinary, 1 trunk, 2 branch */
    std::vector<char> mem_stored;        /* branches without sections and without a delay line: the stage finishes and stores them */
    std::vector<int> mem_row;            /* per chain: the hand-over row mem_trees gave it (a trunk with sections: its own; a branch without
                                            sections but with a delay line: its tree's), else -1 */
    std::vector<MemTree> mem_tree_list;
    std::vector<MemOwn> mem_own;
    std::vector<MemTile> mem_tiles;
    std::vector<int> mem_col_tree;       /* per column of the branch block: its tree */
    int n_mem_cols = 0, n_mem_trunks = 0, n_mem_branches = 0, n_mem_constant = 0;
    std::vector<MemFeed> mem_feed;       /* "mem_fir": the branches that are a FIR alone, tree by tree ... */
    std::vector<int> mem_feed_start;     /* ... [trees + 1]: where each tree's begin (made when there is a feed) */
    std::vector<MemTerm> mem_terms;      /* "chain_sum": the terms of the sum trees, tree by tree ... */
    std::vector<int> mem_sum_start;      /* ... [trees + 1]: where each tree's begin (made when there is a sum tree) */
    int n_mem_sums = 0;                  /* sum trees: a plan with one launches mem_stage's SUM form */
    /* "chain_copy" (DESIGN.md 4.2k), made by copy_list: the live pairs, sorted by destination (consecutive lanes of copy_pairs store
     * consecutive words where the IOs are).  They count in the IO spans and in stores_whole_window */
    std::vector<CopyPair> copy;
};

inline std::string check_heads(const avdsp_plan_desc *d, long long buf_words, ChainTables &t)
{
    t.chains.assign(d->chains, d->chains + d->nchains);
    t.coef.assign(d->sec_coef_word, d->sec_coef_word + d->nsections);
    t.state.assign(d->sec_state_word, d->sec_state_word + d->nsections);
    t.mux_stored.assign(d->nchains, 0);
    t.mux_handed.assign(d->nchains, 0);
    t.mem_kind.assign(d->nchains, 0); t.mem_stored.assign(d->nchains, 0); t.mem_row.assign(d->nchains, -1);
    for (int i = 0; i < d->nsections; i++)
        if (t.coef[i] < 0 || t.coef[i] + 5 > buf_words || t.state[i] < 0 || t.state[i] + 6 > buf_words || (t.state[i] & 1))
            return text("section %d addresses words outside the loaded buffer", i);
    for (int i = 0; i < d->nchains; i++) {
        const int m = t.chains[i].load_mode;
        const bool mem = d->chain_mem && (m == AVDSP_LOAD_MEM || (t.chains[i].mem_store && (m == AVDSP_LOAD_PLAIN || m == AVDSP_LOAD_GAIN)));
        if (m != AVDSP_LOAD_PLAIN && m != AVDSP_LOAD_GAIN && m != AVDSP_LOAD_MUX && !mem) return text("chain %d: load mode %d", i, m);
        if (t.chains[i].mem_store && !mem) return text("chain %d: a memory word has no kernel here", i);
        if (t.chains[i].sum_n && !mem) return text("chain %d: a sum head that is no branch", i);
        t.has_mux = t.has_mux || m == AVDSP_LOAD_MUX;
        t.has_mem = t.has_mem || mem;
    }
    if (t.has_mem) {
        if (d->format != 2 && d->format != 4 && d->format != 6) return text("memory words have no kernels in format %d", d->format);
        if (d->instances > 1) return "memory words have no chain instances";
        if (t.has_mux) return "memory words beside LOAD_MUX chains have no kernels";
    }
    if (!t.has_mux) return "";
    if (d->format == 3 || d->format == 5) return text("LOAD_MUX chains have no kernels in format %d", d->format);
    if (d->instances > 1) return "LOAD_MUX chains have no chain instances";
    for (int i = 0; i < d->nchains; i++) {
        const avdsp_chain &c = t.chains[i];
        if (c.load_mode != AVDSP_LOAD_MUX) continue;
        if (c.mux_count < 1 || c.mux_count > 32767 || c.mux_word < 0 || (long long)c.mux_word + 2ll * c.mux_count > buf_words ||
            c.mux_result_word < 0 || (long long)c.mux_result_word + 2 > buf_words)
            return text("chain %d: LOAD_MUX list or result word outside the loaded buffer", i);
        t.mux_lo = std::min(t.mux_lo, c.mux_word); t.mux_hi = std::max(t.mux_hi, c.mux_word + 2 * c.mux_count);
    }
    return "";
}

/* `words`: the mirror's words [mux_lo, mux_hi) */
inline std::string mux_records(const std::vector<int> &words, ChainTables &t)
{
    const int n = (int)t.chains.size();
    t.mux_recs.resize(n);
    for (int i = 0; i < n; i++) {
        avdsp_chain &c = t.chains[i];
        MuxRec r{};
        r.sat = c.sat; r.n_out = c.n_out;
        for (int k = 0; k < AVDSP_MAX_STORES; k++) r.out_io[k] = c.out_io[k];
        if (c.load_mode == AVDSP_LOAD_MUX) {
            for (int k = 0; k < c.mux_count; k++) {
                const int io = words[(size_t)(c.mux_word - t.mux_lo) + 2 * k];
                if (io < 0) return text("chain %d: LOAD_MUX entry %d names IO %d", i, k, io);
                t.io_in_min = std::min(t.io_in_min, io); t.io_in_max = std::max(t.io_in_max, io);
            }
            r.list_word = c.mux_word; r.count = c.mux_count; r.result_word = c.mux_result_word;
            r.col = (c.nsec || c.fir_taps) ? i : -1;
            if (r.col < 0 && c.delay_slot) { t.mux_handed[i] = 1; t.n_mux_handed++; }      /* ("mux_tail": chain_tail stores it, from its hand-over row) */
            else if (r.col < 0) { t.mux_stored[i] = 1; t.n_mux_stored++; t.n_mux_finished += c.finish != 0; }
            c.load_mode = kLoadRaw;
        } else {
            if (c.in_io < 0) return text("chain %d: bad IO", i);
            t.io_in_min = std::min(t.io_in_min, c.in_io); t.io_in_max = std::max(t.io_in_max, c.in_io);
            r.list_word = c.in_io; r.count = 0; r.col = i;
        }
        c.in_io = i;
        t.mux_recs[i] = r;
    }
    return "";
}

/* "chain_copy" (DESIGN.md 4.2k), behind check_heads and in front of the stages that rewrite the chains' heads: the host has resolved
 * the lists (forwarding, the last writer, self-copies); here the finished plan is held to what copy_pairs relies on, whoever made it.
 * Every source is read from the caller's input block and every destination written to its output block while the chains run, so: the
 * destinations pairwise distinct, no destination an IO a chain loads (`words`: the mirror's words [mux_lo, mux_hi), the LOAD_MUX
 * lists) or stores, no source a destination or an IO a chain stores.  The pairs sorted by destination */
inline std::string copy_list(const avdsp_plan_desc *d, const std::vector<int> &words, ChainTables &t)
{
    if (d->ncopy < 0 || (d->ncopy > 0 && (!d->copy_src || !d->copy_dst))) return "bad LOAD_STORE pair list";
    if (d->ncopy && !d->chain_copy) return "LOAD_STORE pairs have no kernel here";
    if (!d->ncopy) return "";
    if (d->instances > 1) return "LOAD_STORE pairs have no chain instances";
    std::vector<char> stored(kCopyIoLimit, 0), loaded(kCopyIoLimit, 0), dst(kCopyIoLimit, 0);
    auto mark = [](std::vector<char> &v, int io) { if (io >= 0 && io < kCopyIoLimit) v[(size_t)io] = 1; };
    for (const avdsp_chain &c : t.chains) {
        for (int k = 0; k < c.n_out && k < AVDSP_MAX_STORES; k++) mark(stored, c.out_io[k]);
        if (c.load_mode == AVDSP_LOAD_MUX)
            for (int k = 0; k < c.mux_count; k++) mark(loaded, words[(size_t)(c.mux_word - t.mux_lo) + 2 * k]);
        else if (c.load_mode != AVDSP_LOAD_MEM) mark(loaded, c.in_io);
    }
    t.copy.resize((size_t)d->ncopy);
    for (int i = 0; i < d->ncopy; i++) {
        const CopyPair p{d->copy_src[i], d->copy_dst[i]};
        if (p.src < 0 || p.src >= kCopyIoLimit || p.dst < 0 || p.dst >= kCopyIoLimit) return text("pair %d: IO %d -> %d outside [0,%d)", i, p.src, p.dst, kCopyIoLimit);
        if (dst[(size_t)p.dst]) return text("pair %d: IO %d is the destination of two pairs", i, p.dst);
        if (loaded[(size_t)p.dst] || stored[(size_t)p.dst]) return text("pair %d: its destination IO %d is loaded or stored by a chain", i, p.dst);
        if (stored[(size_t)p.src]) return text("pair %d: its source IO %d is stored by a chain", i, p.src);
        dst[(size_t)p.dst] = 1;
        t.copy[(size_t)i] = p;
    }
    for (int i = 0; i < d->ncopy; i++)
        if (dst[(size_t)t.copy[(size_t)i].src]) return text("pair %d: its source IO %d is the destination of a pair", i, t.copy[(size_t)i].src);
    std::sort(t.copy.begin(), t.copy.end(), [](const CopyPair &a, const CopyPair &b) { return a.dst < b.dst; });
    for (const CopyPair &p : t.copy) {
        t.io_in_min = std::min(t.io_in_min, p.src); t.io_in_max = std::max(t.io_in_max, p.src);
        t.io_out_min = std::min(t.io_out_min, p.dst); t.io_out_max = std::max(t.io_out_max, p.dst);
    }
    return "";
}

/* "chain_mem" (DESIGN.md 4.2j), behind check_heads in a plan with trunks or branches: the trees in program order (those with a trunk
 * first, then the words nobody here writes), every word index against the buffer, the hand-over rows the stage reads or fills, the
 * columns of the branch block -- consecutive within a tree -- and mem_stage's tiles.  A branch with sections becomes a kLoadRaw chain of
 * its column, as the chains of a LOAD_MUX plan do */
inline std::string mem_trees(const avdsp_plan_desc *d, long long buf_words, ChainTables &t)
{
    const int n = (int)t.chains.size();
    auto word_ok = [&](int w) { return w >= 1 && (long long)w + 2 <= buf_words; };
    auto find_tree = [&](int w, int *exact) {
        *exact = -1;
        for (size_t k = 0; k < t.mem_tree_list.size(); k++) {
            /* ("chain_sum": a sum tree has no word -- its 0 would collide with word 1's overlap test) */
            if (t.mem_tree_list[k].src == kMemSrcSum) continue;
            const int o = t.mem_tree_list[k].word;
            if (o == w) *exact = (int)k; else if (o == w - 1 || o == w + 1) return false;
        }
        return true;
    };
    std::vector<int> tree_of(n, -1);
    /* ("mem_fir": formats 4 and 6 -- the int64 model has no FIR) */
    const bool mem_fir = d->mem_fir && (d->format == 4 || d->format == 6);
    for (int i = 0; i < n && !mem_fir; i++) if (t.chains[i].fir_taps) return text("chain %d: a FIR beside memory words has no kernel", i);
    for (int i = 0; i < n; i++) {
        const avdsp_chain &c = t.chains[i];
        if (!c.mem_store) continue;
        if (c.sum_n) return text("chain %d: a sum head that is a trunk", i);
        if (c.load_mode == AVDSP_LOAD_MEM || c.n_out || c.sat || c.finish || c.delay_slot || c.ways_n || (c.fir_taps && !mem_fir) || c.in_io < 0) return text("chain %d: not a trunk", i);
        if (!word_ok(c.mem_word)) return text("chain %d: memory word outside the loaded buffer", i);
        int exact;
        if (!find_tree(c.mem_word, &exact)) return text("chain %d: its memory word overlaps another", i);
        if (exact >= 0) return text("chain %d: a second trunk of memory word %d", i, c.mem_word);
        MemTree tr{};
        /* (a trunk with a FIR, "mem_fir": its FIR's HAND launch fills the row -- the cascade in front, if any, feeds the ring) */
        tr.word = c.mem_word; tr.trunk = i; tr.src = c.nsec || c.fir_taps ? kMemSrcRow : kMemSrcSample;
        tr.row = c.nsec || c.fir_taps ? t.n_hand_rows++ : -1;
        if (c.fir_taps) t.fir_trunk.push_back(i);
        tr.in_io = c.in_io; tr.load_mode = c.load_mode; tr.gain_bits = c.gain_bits;
        t.mem_kind[i] = 1; t.mem_row[i] = tr.row; t.n_mem_trunks++;
        t.mem_tree_list.push_back(tr);
    }
    for (int i = 0; i < n; i++) {
        const avdsp_chain &c = t.chains[i];
        if (c.load_mode != AVDSP_LOAD_MEM) continue;
        if (c.sum_n < 0 || c.sum_n > AVDSP_MAX_SUM_TERMS - 1) return text("chain %d: %d sum terms", i, c.sum_n);
        for (int q = 0; q < c.sum_n; q++)
            if (c.sum_op[q] != AVDSP_SUM_ADD && c.sum_op[q] != AVDSP_SUM_SUB) return text("chain %d: sum operation %d", i, c.sum_op[q]);
        if (c.sum_n && !d->chain_sum) return text("chain %d: a sum head has no kernel here", i);
        if (c.mem_store || (c.fir_taps && !mem_fir) || (c.n_out < 1 && !(d->chain_copy && c.delay_slot))) return text("chain %d: not a branch", i);
        if (!word_ok(c.mem_word)) return text("chain %d: memory word outside the loaded buffer", i);
        if (c.sum_n) continue;                               /* (below, behind all word trees) */
        int exact;
        if (!find_tree(c.mem_word, &exact)) return text("chain %d: its memory word overlaps another", i);
        if (exact >= 0 && t.mem_tree_list[exact].trunk > i) return text("chain %d: a branch in front of its trunk", i);
        if (exact < 0) {
            MemTree tr{};
            tr.word = c.mem_word; tr.trunk = -1; tr.src = kMemSrcWord; tr.row = -1;
            exact = (int)t.mem_tree_list.size();
            t.mem_tree_list.push_back(tr);
        }
        tree_of[i] = exact; t.mem_kind[i] = 2; t.n_mem_branches++;
        t.n_mem_constant += t.mem_tree_list[exact].trunk < 0;
    }
    /* ("chain_sum") the sum heads: a tree each, behind all word trees, and its terms -- the head's own word first -- each from where a
     * LOAD_MEM of that word takes it.  A word with a trunk must have it in front of the head */
    const size_t n_word_trees = t.mem_tree_list.size();
    for (int i = 0; i < n; i++) {
        const avdsp_chain &c = t.chains[i];
        if (c.load_mode != AVDSP_LOAD_MEM || !c.sum_n) continue;
        if (t.mem_sum_start.empty()) t.mem_sum_start.assign(n_word_trees, 0);
        t.mem_sum_start.push_back((int)t.mem_terms.size());
        for (int q = 0; q <= c.sum_n; q++) {
            const int w = q ? c.sum_word[q - 1] : c.mem_word;
            if (!word_ok(w)) return text("chain %d: memory word of a sum term outside the loaded buffer", i);
            int exact;
            if (!find_tree(w, &exact)) return text("chain %d: the memory word of a sum term overlaps another", i);
            MemTerm m{};
            m.src = kMemSrcWord; m.row = -1; m.word = w; m.op = q ? c.sum_op[q - 1] : 0;
            if (exact >= 0 && t.mem_tree_list[exact].trunk >= 0) {
                const MemTree &o = t.mem_tree_list[exact];
                if (o.trunk > i) return text("chain %d: a sum term in front of its trunk", i);
                m.src = o.src; m.row = o.src == kMemSrcRow ? o.row : -1; m.in_io = o.in_io; m.load_mode = o.load_mode; m.gain_bits = o.gain_bits;
            }
            t.mem_terms.push_back(m);
        }
        MemTree tr{};
        tr.word = 0; tr.trunk = -1; tr.src = kMemSrcSum; tr.row = -1;
        tree_of[i] = (int)t.mem_tree_list.size(); t.mem_kind[i] = 2; t.n_mem_branches++; t.n_mem_sums++;
        t.mem_tree_list.push_back(tr);
    }
    if (t.n_mem_sums) t.mem_sum_start.push_back((int)t.mem_terms.size());
    /* the branches tree by tree: columns, the stage's own stores, the rows it fills */
    std::vector<std::vector<int>> members(t.mem_tree_list.size());
    for (int i = 0; i < n; i++) if (tree_of[i] >= 0) members[tree_of[i]].push_back(i);
    for (size_t k = 0; k < t.mem_tree_list.size(); k++) {
        MemTree &tr = t.mem_tree_list[k];
        tr.col0 = t.n_mem_cols; tr.first_own = (int)t.mem_own.size();
        t.mem_feed_start.push_back((int)t.mem_feed.size());
        for (int i : members[k]) {
            avdsp_chain &c = t.chains[i];
            c.load_mode = kLoadRaw; c.in_io = 0;
            if (c.nsec) { c.in_io = t.n_mem_cols++; t.mem_col_tree.push_back((int)k); }
            /* ("mem_fir": a FIR alone -- no column, no record of the stage's own, no row of the tree's: the stage feeds its ring, its FIR
             * stores it or hands it over like any FIR chain's) */
            else if (c.fir_taps) { c.load_mode = kLoadFed; t.mem_feed.push_back(MemFeed{(int)k, i}); }
            /* ("chain_ways": a branch with way operations is chain_tail's like a delayed one -- the stage fills its tree's row, and does not finish it) */
            else if (c.delay_slot || c.ways_n) { if (tr.row < 0) tr.row = t.n_hand_rows++; t.mem_row[i] = tr.row; }
            else {
                MemOwn o{};
                o.tree = (int)k; o.cid = i; o.sat = c.sat; o.finish = c.finish; o.gain_bits = c.finish_gain_bits; o.n_out = c.n_out;
                for (int q = 0; q < AVDSP_MAX_STORES; q++) o.out_io[q] = c.out_io[q];
                t.mem_own.push_back(o); t.mem_stored[i] = 1;
            }
        }
        tr.ncol = t.n_mem_cols - tr.col0; tr.n_own = (int)t.mem_own.size() - tr.first_own;
        if (t.mem_tiles.empty() || t.mem_tiles.back().ntree == kMemTileTrees || t.mem_tiles.back().ncol >= kMemTileCols)
            t.mem_tiles.push_back(MemTile{(int)k, 0, tr.col0, 0});
        t.mem_tiles.back().ntree++; t.mem_tiles.back().ncol += tr.ncol;
    }
    t.mem_feed_start.push_back((int)t.mem_feed.size());
    if (t.mem_feed.empty()) t.mem_feed_start.clear();
    return "";
}

inline std::string check_chains(const avdsp_plan_desc *d, long long buf_words, ChainTables &t)
{
    const bool fir_tail = d->fir_tail && (d->format == 4 || d->format == 6);
    const bool mux_refused = t.has_mux && !d->mux_tail;   /* ("mux_tail": dressed finishes, delay lines and a head TPDF_CALC in a plan with LOAD_MUX chains) */
    t.hand_row.assign(d->nchains, -1);
    for (int i = 0; i < d->nchains; i++) {
        const avdsp_chain &c = t.chains[i];
        if (c.sec_base < 0 || c.nsec < 0 || c.sec_base + c.nsec > d->nsections) return text("chain %d: bad section range", i);
        /* ("chain_copy": a chain whose every STORE a later chain repeats keeps none -- only where chain_tail finishes it, for its line) */
        const bool storeless = t.mem_kind[i] == 1 || (d->chain_copy && c.delay_slot && d->instances <= 1);
        if ((c.n_out < 1 && !storeless) || c.n_out > AVDSP_MAX_STORES || c.in_io < 0) return text("chain %d: bad IO", i);
        if (!t.has_mux && t.mem_kind[i] != 2) { t.io_in_min = std::min(t.io_in_min, c.in_io); t.io_in_max = std::max(t.io_in_max, c.in_io); }
        for (int k = 0; k < c.n_out; k++) {
            if (c.out_io[k] < 0) return text("chain %d: bad IO", i);
            t.io_out_min = std::min(t.io_out_min, c.out_io[k]); t.io_out_max = std::max(t.io_out_max, c.out_io[k]);
        }
        if (c.fir_taps) {
            if (d->format == 2) return text("chain %d: FIR has no int64 definition", i);
            if (c.fir_coef_word < 0 || c.fir_coef_word + c.fir_taps > buf_words ||
                c.fir_state_word < 0 || c.fir_state_word + c.fir_taps > buf_words)
                return text("chain %d: FIR addresses words outside the loaded buffer", i);
            t.fir.push_back(i);
            t.max_taps = std::max(t.max_taps, c.fir_taps);
        }
        /* (a trunk, "chain_mem": its cascade -- "mem_fir": or its FIR, which is in `fir` and in mem_trees' `fir_trunk` -- hands over to
         * mem_stage, nothing else follows) */
        if (t.mem_kind[i] == 1) { t.hand_row[i] = t.mem_row[i]; continue; }
        if (c.finish) {
            /* a dressed finish (avdsp_chain::finish): the chain kernels of formats 2, 4 and 6, no FIR in front (but under "fir_tail"), no LOAD_MUX plan (but under "mux_tail"), no instances */
            if (c.finish < AVDSP_FINISH_TPDF || c.finish > AVDSP_FINISH_TPDF_GAIN || c.sat != 1) return text("chain %d: finish %d", i, c.finish);
            if ((d->format != 2 && d->format != 4 && d->format != 6) || (c.fir_taps && !fir_tail) || mux_refused || d->instances > 1)
                return text("chain %d: a dressed finish has no kernel here", i);
            t.n_dressed++;
        }
        if (c.delay_slot) {
            /* one DSP_DELAY (avdsp_chain::delay_slot): chain_tail of formats 2, 4 and 6, no FIR (but under "fir_tail"), no LOAD_MUX plan (but under "mux_tail"), no instances; the line
             * -- its index word and the samples of the longest delay it can be asked for -- and the parameter word inside the buffer */
            if ((c.delay_slot != AVDSP_DELAY_A && c.delay_slot != AVDSP_DELAY_B) || (c.delay_slot == AVDSP_DELAY_B && c.sat != 1))
                return text("chain %d: delay slot %d", i, c.delay_slot);
            if ((d->format != 2 && d->format != 4 && d->format != 6) || (c.fir_taps && !fir_tail) || mux_refused || d->instances > 1)
                return text("chain %d: a delay line has no kernel here", i);
            const long long nline = c.delay_us_word ? (long long)c.delay_max : (long long)(((unsigned long long)(unsigned)c.delay_max * d->delay_line_factor) >> 32);
            if (c.delay_max < 0 || c.delay_word < 0 || (long long)c.delay_word + 1 + nline > buf_words || c.delay_us_word < 0 || c.delay_us_word >= buf_words)
                return text("chain %d: delay line outside the loaded buffer", i);
        }
        if (c.ways_n) {
            /* way operations (avdsp_chain::ways_n, "chain_ways"): chain_tail's OPS form of formats 2, 4 and 6; no FIR, no LOAD_MUX plan, no instances */
            if (c.ways_n < 0 || c.ways_n > AVDSP_MAX_WAY_OPS) return text("chain %d: %d way operations", i, c.ways_n);
            for (int k = 0; k < c.ways_n; k++)
                if (c.ways_op[k] != AVDSP_WAY_GAIN && c.ways_op[k] != AVDSP_WAY_NEG) return text("chain %d: way operation %d", i, c.ways_op[k]);
            if (!d->chain_ways || (d->format != 2 && d->format != 4 && d->format != 6) || c.fir_taps || t.has_mux || d->instances > 1)
                return text("chain %d: way operations have no kernel here", i);
            t.n_way_ops++;
        }
        const bool handed = c.fir_taps && (c.finish || c.delay_slot);
        if (handed) t.fir_hand.push_back(i); else if (c.fir_taps) t.fir_plain.push_back(i);
        /* ("chain_ways": a chain with way operations is a tail chain exactly as a delayed one is -- without a DSP_DELAY it gets the record of a
         * line of 0 samples, as a handed FIR chain without one) */
        if (c.delay_slot || handed || c.ways_n) {
            t.tail.push_back(i);
            if (c.nsec || c.fir_taps || t.mux_handed[i]) t.hand_row[i] = t.n_hand_rows++;
            else if (t.mem_row[i] >= 0) t.hand_row[i] = t.mem_row[i];      /* (a branch without sections: its tree's row, shared with its siblings) */
            continue;
        }
        if (!c.nsec && !c.fir_taps && !t.mux_stored[i] && !t.mem_stored[i]) (c.finish ? t.pass_dressed : t.pass).push_back(i);
    }
    if (d->tpdf_calc) {
        if ((d->format != 2 && d->format != 4 && d->format != 6) || mux_refused || d->instances > 1) return "a head TPDF_CALC has no kernel here";
        if (d->tpdf_calc_result_word < 0 || (long long)d->tpdf_calc_result_word + 2 > buf_words) return "TPDF_CALC result word outside the loaded buffer";
    }
    return "";
}

/* ---- the cascades ---- */
/* one launch: the chains of one section count, or one piece of them */
struct GroupLayout {
    int P = 0, nsec = 0, n = 0;          /* lanes per chain, sections, chains */
    bool all_fir = false;                /* every chain of the group feeds a FIR (its cascade writes the ring) */
    bool raw_out = false;                /* a piece but the last: it stores its last section's result word as it is */
    bool hand = false;                   /* (with wide) its chains have a delay line: the launch hands every frame's accumulator to chain_tail
                                            instead of finishing it (biquad_pipe's HAND form) */
    int phase = 0;                       /* "chain_mem": 1: branches, launched behind mem_stage with the branch block as their input; 0: everything else */
    bool wide = false;                   /* its chains have a dressed finish or a delay line: the launch keeps the last section's whole accumulator per frame
                                            (biquad_pipe's WIDE form; no biquad_row records).  Of a long cascade only the last piece is */
    std::vector<int> ids;                /* the chains' records in `dev_chains` */
    std::vector<RowRec> rows; std::vector<LaneRec> lanes;      /* biquad_row's records (P == 16), sections right-aligned in the row */
    std::vector<GroupLayout> pieces;     /* a cascade of more than kPieceMax sections: launched one after the other; piece k hands the
                                            word between its last section and piece k + 1's first through column j (the chain's place
                                            in the group) of a scratch block */
};
struct CascadeLayout {
    std::vector<avdsp_chain> dev_chains; /* what the kernels see: the host's records + the pieces of long cascades behind them */
    std::vector<GroupLayout> groups;     /* by section count, in first-seen order */
    /* the rows of ALL the 16-lane groups in one table -- runs of one section count, each filled up to whole waves (four rows) with
     * empty rows, the table to whole workgroups (16) -- for ONE biquad_row launch instead of one per section count.  Only made when
     * there are two such groups or more. */
    std::vector<RowRec> all_rows; std::vector<LaneRec> all_lanes;
    bool rows_all_fir = true; int n_row_groups = 0;
};

/* biquad_row's records of the chains `ids` (records of `chains`), all of one section count */
inline void row_records(int format, const std::vector<avdsp_chain> &chains, const ChainTables &t, GroupLayout &g)
{
    g.rows.resize(g.ids.size());
    g.lanes.assign(g.ids.size() * 16, LaneRec{-1, -1});
    for (size_t j = 0; j < g.ids.size(); j++) {
        const avdsp_chain &c = chains[g.ids[j]];
        /* bit 8: SAT0DB in front of the store -- in the int64 kernel "the stored word is acc >> 28", which is also what a piece
         * hands on (bit 10 then takes the dither mask off); in the double kernels a piece's word is the float as it is: no bit 8 */
        const bool raw = c.sat == kStoreRaw;
        const bool sat = raw ? format == 2 : c.sat != 0;
        g.rows[j] = RowRec{g.ids[j], c.in_io, c.out_io[0], (c.load_mode & 0xFF) | (sat ? 1 << 8 : 0) | (c.fir_taps ? 1 << 9 : 0) | (raw ? 1 << 10 : 0) | (c.n_out << 16),
                           c.gain_bits, {c.nsec, 0, 0}};
        for (int q = 0; q < c.nsec; q++) g.lanes[j * 16 + (16 - c.nsec) + q] = LaneRec{t.coef[c.sec_base + q], t.state[c.sec_base + q]};
    }
}

inline CascadeLayout cascade_groups(int format, const ChainTables &t)
{
    CascadeLayout L;
    L.dev_chains = t.chains;
    for (int i = 0; i < (int)t.chains.size(); i++) {
        const int nsec = t.chains[i].nsec;
        if (!nsec) continue;
        /* dressed chains: launch groups of their own, next to the others; delayed chains (dressed or not): again groups of their own.
         * Not the cascade of a handed FIR chain ("fir_tail"): delay and finish stand behind its FIR, the cascade feeds the ring like any */
        const bool fir = t.chains[i].fir_taps != 0;
        /* ("chain_mem": a trunk hands over like a delayed chain -- "mem_fir": unless a FIR stands behind its cascade, which then feeds
         * the ring like any; branches are groups of their own, of the second phase) */
        const int kind = t.has_mem ? t.mem_kind[i] : 0, phase = kind == 2 ? 1 : 0;
        const bool hand = !fir && (t.chains[i].delay_slot != 0 || t.chains[i].ways_n != 0 || kind == 1), wide = hand || (!fir && t.chains[i].finish != 0);
        auto it = std::find_if(L.groups.begin(), L.groups.end(), [&](const GroupLayout &g) { return g.nsec == nsec && g.wide == wide && g.hand == hand && g.phase == phase; });
        if (it == L.groups.end()) { L.groups.emplace_back(); it = L.groups.end() - 1; it->nsec = nsec; it->wide = wide; it->hand = hand; it->phase = phase; }
        it->ids.push_back(i);
    }
    for (GroupLayout &g : L.groups) {
        g.n = (int)g.ids.size();
        /* lanes per chain: the next power of two -- but a 16-lane row per chain while the chip has SIMDs to spare (<= 1024 waves): its
         * step is shorter (one input batch per 16 steps, no mid-row section-0 lanes) and idle lanes cost nothing there */
        g.P = g.nsec > 64 ? 128 : pow2ceil(g.nsec);
        if (g.P < 16 && (long long)g.n * 16 <= 65536) g.P = 16;
        if (g.wide && g.P < 16) g.P = 16;                /* (dressed chains: the WIDE form exists for 16-lane rows only) */
        g.all_fir = true;
        for (int id : g.ids) g.all_fir = g.all_fir && t.chains[id].fir_taps != 0;
        if (g.nsec > kPieceMax) {
            /* A cascade of more than 16 sections runs as pieces of equal length (+- 1), each a biquad_row launch, one after the other:
             * a 16-lane row per chain wastes no lanes on lengths like 17 or 33, and a cascade of more than 64 sections fits no wave at
             * all.  The pieces but the last are chain records of their own behind the host's (no FIR, no SAT0DB, one raw
             * store into the scratch column); the last piece is the chain's own record with its input moved to the scratch column (its
             * ring, stores and ready word are the chain's). */
            const int np = (g.nsec + kPieceMax - 1) / kPieceMax, base = g.nsec / np, extra = g.nsec % np;
            int at = 0;
            for (int k = 0; k < np; k++) {
                GroupLayout pg;
                pg.nsec = base + (k < extra ? 1 : 0); pg.P = 16; pg.n = g.n; pg.phase = g.phase;
                pg.all_fir = k + 1 == np && g.all_fir; pg.raw_out = k + 1 < np;
                pg.wide = k + 1 == np && g.wide; pg.hand = k + 1 == np && g.hand;
                pg.ids.resize(g.n);
                for (int j = 0; j < g.n; j++) {
                    const avdsp_chain &c = t.chains[g.ids[j]];
                    avdsp_chain pc = c;
                    pc.sec_base = c.sec_base + at; pc.nsec = pg.nsec;
                    if (k > 0) { pc.in_io = j; pc.load_mode = kLoadRaw; }
                    if (k + 1 < np) {
                        pc.fir_taps = 0; pc.sat = kStoreRaw; pc.n_out = 1; pc.out_io[0] = j; pc.finish = 0; pc.delay_slot = 0; pc.ways_n = 0;
                        pg.ids[j] = (int)L.dev_chains.size(); L.dev_chains.push_back(pc);
                    } else { pg.ids[j] = g.ids[j]; L.dev_chains[g.ids[j]] = pc; }
                }
                if (!pg.wide) row_records(format, L.dev_chains, t, pg);
                g.pieces.push_back(std::move(pg));
                at += base + (k < extra ? 1 : 0);
            }
        } else if (g.P == 16 && !g.wide) {
            row_records(format, t.chains, t, g);
            if (t.has_mem) continue;                         /* ("chain_mem": two phases with two input blocks -- no table of all rows) */
            /* ... and the same rows in the table of all lengths: this run, filled up to whole waves.  (An empty row is a copy of a real
             * one with no chain behind it: every lane of a wave FETCHES, section or not -- its input column must be one the block has;
             * nothing of it is stored) */
            L.all_rows.insert(L.all_rows.end(), g.rows.begin(), g.rows.end());
            L.all_lanes.insert(L.all_lanes.end(), g.lanes.begin(), g.lanes.end());
            RowRec empty = g.rows[0]; empty.cid = -1;
            while (L.all_rows.size() % 4) { L.all_rows.push_back(empty); L.all_lanes.insert(L.all_lanes.end(), 16, LaneRec{-1, -1}); }
            L.n_row_groups++;
            L.rows_all_fir = L.rows_all_fir && g.all_fir;
        }
    }
    if (L.n_row_groups >= 2) {
        RowRec empty = L.all_rows.back(); empty.cid = -1;
        while (L.all_rows.size() % 16) { L.all_rows.push_back(empty); L.all_lanes.insert(L.all_lanes.end(), 16, LaneRec{-1, -1}); }
    } else { L.all_rows.clear(); L.all_lanes.clear(); }
    return L;
}

/* ---- fir_shared: the host's groups of chains on one impulse bank -- a taps row per group, column groups of <= 16 chains ---- */
struct SharedLayout {
    std::string err;
    std::vector<int> ids;                /* the grouped chains, group by group */
    std::vector<int> feed;               /* ... those without a cascade in front (fir_feed appends their input) */
    std::vector<int> rest;               /* the FIR chains in no group: fir_tile beside fir_shared */
    std::vector<int> reps;               /* per group: the chain whose taps are the group's */
    std::vector<SharedTile> tiles;
};
inline SharedLayout shared_fir_layout(const avdsp_plan_desc *d, const ChainTables &t)
{
    SharedLayout S;
    /* ("mem_fir": the chains of a plan with memory words are in no group -- the host offers none) */
    if (t.has_mem && !t.fir.empty() && d->fir_ngroups > 0) { S.err = "FIR groups beside memory words have no kernel"; return S; }
    if (t.fir.empty() || !(d->fir_ngroups > 0 && d->fir_group_start && d->fir_group_chains && d->instances <= 1 && (d->format == 4 || d->format == 6))) return S;
    std::vector<char> in_group(d->nchains, 0);
    for (int g = 0; g < d->fir_ngroups; g++) {
        const int b = d->fir_group_start[g], e = d->fir_group_start[g + 1];
        if (b < 0 || e < b || e - b < AVDSP_FIR_GROUP_MIN) { S.err = text("FIR group %d: %d chains", g, e - b); return S; }
        const int c0 = d->fir_group_chains[b];
        for (int j = b; j < e; j++) {
            const int ci = d->fir_group_chains[j];
            if (ci < 0 || ci >= d->nchains || in_group[ci] || !t.chains[ci].fir_taps || t.chains[ci].finish || t.chains[ci].delay_slot || t.chains[ci].fir_taps != t.chains[c0].fir_taps ||
                t.chains[ci].fir_coef_word != t.chains[c0].fir_coef_word) { S.err = text("FIR group %d: chain %d is not one of its bank", g, ci); return S; }
            in_group[ci] = 1;
            if (!t.chains[ci].nsec) S.feed.push_back(ci);
        }
        const int gi = (int)S.reps.size();
        S.reps.push_back(c0);
        for (int j = b; j < e; j += 16)
            S.tiles.push_back(SharedTile{gi, (int)S.ids.size() + (j - b), std::min(16, e - j), t.chains[c0].fir_taps});
        S.ids.insert(S.ids.end(), d->fir_group_chains + b, d->fir_group_chains + e);
    }
    for (int ci : t.fir_plain) if (!in_group[ci]) S.rest.push_back(ci);
    return S;
}

/* ---- mix groups -> mux_tile's blocks of up to kMuxRows chains (formats 4 and 6); every other chain -> mux_plain ---- */
struct MuxLayout {
    std::string err;
    std::vector<int> tile_ids, plain, kpads;     /* the tiles' chains (kpads: each one's padded list length); the chains mux_plain takes */
    std::vector<MuxTile> tiles;
    std::vector<long long> rows;                 /* per tiled chain: where its gains row starts */
    long long g64_len = 0;                       /* doubles of all gains rows */
};
inline MuxLayout mux_tiles(const avdsp_plan_desc *d, const ChainTables &t)
{
    MuxLayout M;
    std::vector<char> tiled(d->nchains, 0);
    if (d->format != 2 && d->mux_ngroups > 0 && d->mux_group_start && d->mux_group_chains)
        for (int g = 0; g < d->mux_ngroups; g++) {
            const int b = d->mux_group_start[g], e = d->mux_group_start[g + 1];
            if (b < 0 || e < b || e - b < AVDSP_MUX_GROUP_MIN) { M.err = text("mix group %d: %d chains", g, e - b); return M; }
            const int c0 = d->mux_group_chains[b];
            if (c0 < 0 || c0 >= d->nchains || t.mux_recs[c0].count < 1) { M.err = text("mix group %d: chain %d has no list", g, c0); return M; }
            const int count = t.mux_recs[c0].count, kpad = (count + 3) & ~3;
            for (int j = b; j < e; j++) {
                const int ci = d->mux_group_chains[j];
                /* (the kernel reads the IO numbers from the first chain's list: the host has compared the sequences) */
                if (ci < 0 || ci >= d->nchains || tiled[ci] || t.mux_recs[ci].count != count) { M.err = text("mix group %d: chain %d is not one of its lists", g, ci); return M; }
                tiled[ci] = 1;
                if ((j - b) % kMuxRows == 0) M.tiles.push_back(MuxTile{(int)M.tile_ids.size(), std::min(kMuxRows, e - j), count, kpad, t.mux_recs[c0].list_word, M.g64_len});
                M.tile_ids.push_back(ci); M.rows.push_back(M.g64_len); M.kpads.push_back(kpad);
                M.g64_len += kpad;
            }
        }
    for (int i = 0; i < d->nchains; i++) if (!tiled[i]) M.plain.push_back(i);
    return M;
}

/* ---- scalars ---- */
/* fir_mfma: groups of 16 tap positions per LDS chunk */
inline int fir_groups_per_chunk(int max_taps)
{
    const int G = (max_taps + 15 + 15) >> 4;
    const int nc = (G + kMaxGpc - 1) / kMaxGpc;
    const int gpc = (G + nc - 1) / nc;
    return std::min((gpc + kNG - 1) / kNG * kNG, kMaxGpc);
}
/* floats of a chain's FIR history ring: the longest history, kRingAhead launches of frames (under "overlap" the cascade appends block
 * k + 1 while the FIR still reads block k's window) and a chunk */
inline int ring_length(int max_taps) { return pow2ceil(max_taps + kRingAhead * kFirChunk + 16 * fir_groups_per_chunk(max_taps) + 16 * (kNG + 4) + 64); }
/* doubles of a chain's row in the f64 copy of the taps */
constexpr int taps64_pitch(int max_taps) { return (kTapsLead + max_taps + kTapsTail + 1) & ~1; }
/* every IO of [io_out_min, io_out_max] is stored by some chain or is the destination of a live pair ("chain_copy": they are in the
 * span, so they are in the count) (check_independent, host: no IO is stored twice) */
inline bool stores_whole_window(const ChainTables &t)
{
    long long nout = (long long)t.copy.size();
    for (const avdsp_chain &c : t.chains) nout += c.n_out;
    return t.io_out_max >= t.io_out_min && nout == (long long)t.io_out_max - t.io_out_min + 1;
}
/* every cascade of the plan feeds a FIR: its launches may run under the previous block's FIR.  (Not behind a mux stage: the cascades
 * follow it on the caller's stream.) */
inline bool overlap_ok(const ChainTables &t)
{
    bool any = false;
    if (t.has_mem) return false;                         /* ("chain_mem": trunks, the stage and the branches follow each other on the caller's stream) */
    if (!t.fir_hand.empty()) return false;               /* (a handed FIR chain: its tail follows its FIR on the caller's stream, the plan runs back to back) */
    for (const avdsp_chain &c : t.chains) { if (c.nsec && !c.fir_taps) return false; any = any || c.nsec; }
    return any && !t.fir.empty() && !t.has_mux;
}

/* ---- "fir_ahead": FIR launches of consecutive blocks in flight together, their output through a staging block ---- */
/* the output columns the plain FIR chains of a plan store, in ascending order: what the copy behind a staged FIR launch moves, and nothing
 * else (passthrough chains, other cores and padding are never touched in the caller's block).  `run`: they are one run of consecutive IOs */
struct AheadColumns { std::vector<int> cols; bool run = false; };
inline AheadColumns ahead_columns(const ChainTables &t)
{
    AheadColumns A;
    for (int i : t.fir) {                                /* (a plan with handed FIR chains has no overlap mode: every FIR chain here is a plain one) */
        const avdsp_chain &c = t.chains[i];
        for (int k = 0; k < c.n_out; k++) A.cols.push_back(c.out_io[k]);
    }
    std::sort(A.cols.begin(), A.cols.end());
    A.cols.erase(std::unique(A.cols.begin(), A.cols.end()), A.cols.end());
    A.run = !A.cols.empty() && (size_t)(A.cols.back() - A.cols.front()) + 1 == A.cols.size();
    return A;
}
/* Whether an overlapped launch takes the staged path when "fir_ahead" leaves it to the plan (-1).  It pays where a launch is more than
 * a chip of waves at a time, so that the next launch's first workgroups fill the SIMDs the last ones of this launch leave: plans of
 * `kAheadPlanTaps` taps in all (FIR chains x the longest FIR) or more -- the north star (4096 x 4096) and a 2048-chain half of it, not
 * the shards (512 x 4096, 2048 x 2048), whose cascades are the clock and lose under overlapped FIRs (0.087 -> 0.097 ms) -- and blocks of
 * `kAheadMinFrames` frames or more: measured at 1024, 512 and 256 frames (0.498 -> 0.488, 0.261 -> 0.252, 0.139 -> 0.133 ms per step,
 * profiles/fir_ahead.md); shorter blocks have not been measured and stay on the direct path. */
constexpr long long kAheadPlanTaps = 8000000ll;
constexpr int kAheadMinFrames = 256;
inline bool fir_ahead_by_plan(long long n_fir, int max_taps, int frames) { return n_fir * max_taps >= kAheadPlanTaps && frames >= kAheadMinFrames; }
/* words of one staging block: a launch's frames in the caller's window geometry; 0: over the cap (64 MB a block), the call takes the direct path */
constexpr long long kAheadStageCapWords = 16ll << 20;
inline long long ahead_stage_words(int out_stride) { const long long w = (long long)kFirChunk * out_stride; return out_stride > 0 && w <= kAheadStageCapWords ? w : 0; }

/* fir_impl's values, and fir_shared, which launch_all takes for the grouped chains of a plan (shared_path) */
enum FirFamily { kFirPlain = 0, kFirTile = 1, kFirMfma = 2, kFirStream = 3, kFirFlow = 4, kFirShared = 5 };

/* ---- the route of a block launch: what launch_all (avdsp_kernels.hip) enqueues, decided here and nowhere else ---- */
/* everything the decision reads */
struct LaunchFacts {
    int overlap, cu_split, fir_ahead, ready_words, fir_launch;                  /* the options of those names */
    int fir_impl, biquad_impl, nframes, out_stride; bool in_place;              /* the call */
    bool overlap_ok; int n_fir, max_taps, n_ahead_cols, instances, n_sh_groups; /* the plan ... */
    bool has_taps64, has_ready;                                                 /* ... its per-chain f64 taps, its ready words */
    int inst_n, chain_inst; bool has_timeouts;                                  /* the program; its time-out words */
    bool timer_samples;                                                         /* this launch's FIR kernel timer is sampled */
    int n_fir_only;                                                             /* the plan's FIR chains without a cascade in front: they append their input inside the FIR launch */
};
enum LaunchPath { kBackToBack = 0, kDirect = 1, kOwnFir = 2, kStaged = 3 };
enum ProbeOn { kProbeCaller = 0, kProbeFirTurn = 1, kProbeFirFirst = 2 };       /* the caller's stream, s_fir[blk & 1], s_fir[0] */
struct LaunchGate { bool under, own_fir, ahead_candidate; int probe_on; };
struct LaunchRoute {
    int path, ready_mode;
    bool cascade_event, write_through, fir_waits_event, ready_acquire;
    int fir_launch_mode;                                  /* (the direct path's; 0 elsewhere) */
    bool rides;
    int side_by_side;                                     /* what the program remembers of the probes: a staged launch's is its ahead_apart */
    bool fir_follows_fir;                                 /* this block's FIR waits for the previous block's: see launch_route */
};

/* "ready_words" by the plan (-1).  Mode 2 takes the wait packet off the FIRs' stream (a FIR follows the previous one like any kernel of a
 * queue): 4096 chains 0.5025 -> 0.4980 ms per step.  Where the cascades are the bound that packet's ~9 us are bubbles they live on: 2048
 * chains 0.2594 -> 0.2686, 512 chains 0.0864 -> 0.0933 (one box) -- so by default only where a launch is more than one round of waves:
 * plans of `kReadyBehindTaps` taps in all or more.  (fir_choice's kLeanPlanTaps is the same figure and the same two plans either side of
 * it, but another experiment -- the chunk boundary, not the wait packet: two names, so that measuring one again does not move the other.) */
constexpr long long kReadyBehindTaps = 12000000ll;
constexpr long long kLeanPlanTaps = 12000000ll;         /* fir_tile's lean chunk boundary by the plan: the measurements are in fir_choice */
/* "fir_launch" by the plan (-1): mode 2 (a start and a stop event on the dispatch) where the cascade of the next blocks is what the step
 * waits for -- plans of at most `kPairLaunchTaps` taps in all: 512 chains 0.0971 -> 0.0868 ms, 1024 chains 0.1559 -> 0.1464, cfg5's
 * 2048-chain shard 0.1575 -> 0.1477; on the long launches it only costs (0.5078 -> 0.5202) -- and blocks of more than `kPairLaunchFrames`
 * frames (round 5, tools/shard_blocks_ab.sh: mode 2's empty microseconds only pay where the cascades are the clock, and that takes a block
 * long enough for them to be -- shards of 512 / 1024 chains, mode 2 against mode 1: 86.9 / 90.8 and 146.5 / 148.6 us at 1024 frames, but
 * 150.4 / 138.0 at 768, 91.2 / 78.1 and 57.6 / 51.6 at 512, 58.1 / 47.9 and 56.6 / 45.4 at 256); else mode 1. */
constexpr long long kPairLaunchTaps = 6000000ll;
constexpr int kPairLaunchFrames = 768;

/* Phase 1, before any probe.  `ahead_candidate`: the staged path ("fir_ahead") is eligible, legal and either forced or
 * wanted by the plan; only then are its four streams probed (ahead_streams_apart).  Not eligible, and the call takes another path as
 * ever: chain instances, "overlap" 2 (its own contract), "cu_split"; a plan with impulse groups (the shared-impulse path's plans: their
 * per-chain taps may still have to be made, by a kernel on the launch's stream -- ensure_private_taps -- which nothing orders in front of
 * the OTHER stream's FIR), a fir_impl other than fir_tile's (fir_stream and fir_flow make their operand ring the same way:
 * ensure_operand_ring): whatever a staged launch reads exists since the plan was built.  Not legal: an in-place call (the next call's
 * cascade reads its input at once, from the stream of the cascades), a window over the staging cap.  (Plans with handed FIR chains or a
 * mux stage have no overlap at all: overlap_ok.) */
inline LaunchGate launch_gate(const LaunchFacts &f)
{
    LaunchGate g{};
    g.under = f.overlap && f.overlap_ok && f.biquad_impl && f.fir_impl;
    g.own_fir = f.overlap >= 2 || f.cu_split > 0;       /* the FIRs on a stream of the library's own */
    const bool eligible = g.under && f.fir_ahead != 0 && !g.own_fir && f.n_ahead_cols > 0 && f.instances <= 1 && f.inst_n <= 1 && f.chain_inst <= 1 &&
                          f.fir_impl == kFirTile && f.n_sh_groups == 0 && f.has_taps64;
    const bool legal = ahead_stage_words(f.out_stride) > 0 && !f.in_place;
    g.ahead_candidate = eligible && legal && (f.fir_ahead == 1 || fir_ahead_by_plan(f.n_fir, f.max_taps, f.nframes));
    g.probe_on = f.overlap >= 2 ? kProbeFirTurn : f.cu_split > 0 ? kProbeFirFirst : kProbeCaller;
    return g;
}

/* Phase 2, after the probes: `ahead_apart` is ahead_streams_apart's answer (asked and read for a candidate only), `side_by_side`
 * probe_side_by_side's on g.probe_on (asked and read where the launch is not staged: launch_staged says so in between). */
inline bool launch_staged(const LaunchFacts &f, const LaunchGate &g, int ahead_apart) { return g.ahead_candidate && (f.fir_ahead == 1 || ahead_apart); }      /* (by the plan: only where it can gain) */
inline LaunchRoute launch_route(const LaunchFacts &f, const LaunchGate &g, int ahead_apart, int side_by_side)
{
    LaunchRoute r{};
    if (!g.under) return r;                               /* kBackToBack: cascades and FIRs on the caller's stream, nothing else applies */
    const bool staged = launch_staged(f, g, ahead_apart);
    r.side_by_side = staged ? ahead_apart : side_by_side;
    const bool tile_or_flow = f.fir_impl == kFirTile || f.fir_impl == kFirFlow;
    /* fir_tile finds its cascades' blocks through the ready words; the other FIR kernels wait for the cascades' event */
    const bool can_words = tile_or_flow && f.has_ready && f.has_timeouts && r.side_by_side;
    /* (kReadyBehindTaps; not with "overlap" 2: two FIRs in flight, the later one's waves would sit on their SIMDs looking at words of a
     * cascade that both of them starve -- 0.496 -> 0.547 ms; nor with a staged launch, for the same reason: the event, whatever
     * "ready_words" says) */
    const int rw = staged ? 0 : f.ready_words >= 0 ? f.ready_words : (f.overlap == 1 && (long long)f.n_fir * f.max_taps >= kReadyBehindTaps ? 2 : 0);
    const bool behind = rw == 2 && can_words;                                       /* a kernel behind the cascade publishes */
    const bool words = (rw == 1 && f.fir_impl == kFirTile && can_words) || behind;      /* the FIR looks at the words: no event wait on its stream */
    r.path = staged ? kStaged : g.own_fir ? kOwnFir : kDirect;
    r.ready_mode = behind ? 2 : words ? 1 : 0;
    r.cascade_event = !words;
    r.write_through = words && !behind;                   /* the cascade's own waves publish: write-through ring stores */
    r.fir_waits_event = !words;
    r.ready_acquire = words && (!behind || f.overlap >= 2);
    if (r.path == kDirect) {
        r.fir_launch_mode = !tile_or_flow ? 0 : f.fir_launch >= 0 ? f.fir_launch
                          : ((long long)f.n_fir * f.max_taps <= kPairLaunchTaps && f.nframes > kPairLaunchFrames) ? 2 : 1;
        /* (a launch whose kernel timer is sampled carries the timer's events instead; its event is then recorded behind it) */
        r.rides = r.fir_launch_mode == 1 && !f.timer_samples;
    }
    /* The staged path and "overlap" 2 put the FIRs of consecutive blocks on two streams in turn: FIR k + 1 needs nothing of FIR k -- as
     * long as every FIR chain has a cascade in front, whose stream appends the blocks in order.  A FIR alone appends its block's input
     * inside its own launch (fir_append_input), and FIR k + 1 reads that as history: with such a chain in the plan the FIR's stream
     * waits for the previous block's FIR (found by tests/test_gpu_fir_ring_routes.py: launches of three workgroups do start side by
     * side, and block k + 1 was summed over a ring block k had not reached yet).  One stream -- the direct path, "cu_split" -- orders
     * them by itself. */
    r.fir_follows_fir = f.n_fir_only > 0 && (r.path == kStaged || (r.path == kOwnFir && f.overlap >= 2));
    return r;
}

/* ---- which FIR kernel a launch takes ---- */
struct FirChoice { int family, R; bool BIG, SPLIT, LEAN; bool HAND = false; };       /* R: row tiles per wave (fir_mfma: its NG); the flags are fir_tile's / fir_flow's, else false;
                                                                                         HAND: the launch of a plan's handed FIR chains (fir_hand_choice) */
inline bool operator==(const FirChoice &a, const FirChoice &b) { return a.family == b.family && a.R == b.R && a.BIG == b.BIG && a.SPLIT == b.SPLIT && a.LEAN == b.LEAN && a.HAND == b.HAND; }
struct FirOptions { int fir_rows, fir_split, fir_lean; };         /* the options of those names: 0 = by the rules below, 0 = off, -1 = by the plan */

/* Row tiles per wave by cost.  The chip holds 2048 of these waves at a time, a wave of R row tiles lasts R units, and a launch is over
 * when its LAST round of waves is -- 3000 chains at four row tiles were 1.46 rounds, i.e. two: 480 us, as long as 4096 chains.  So: the R
 * with the fewest units, rounds(R) x R / efficiency(R) (0.90 / 0.84 / 0.79 of the matrix pipe at 4 / 2 / 1 row tiles).
 * `tile_frames`: the frames one row tile covers per wave (fir_tile 256; fir_shared 64, `waves_per_unit` 4 waves per column group).
 * A tile of twice the block would multiply zeros: such an R is out, whoever chose it. */
inline int fir_rows_for(int fir_rows, long long units, int waves_per_unit, int frames, int tile_frames)
{
    int rows = fir_rows;
    if (rows != 1 && rows != 2 && rows != 4) {
        double best = 1e30;
        rows = 1;
        for (int r : {4, 2, 1}) {
            if (r > 1 && tile_frames / 2 * r >= frames) continue;
            const long long waves = units * waves_per_unit * ((frames + tile_frames * r - 1) / (tile_frames * r));
            const double cost = (double)((waves + 2047) / 2048) * r / (r == 4 ? 0.90 : r == 2 ? 0.84 : 0.79);
            if (cost < best - 1e-9) { best = cost; rows = r; }
        }
    }
    while (rows > 1 && tile_frames / 2 * rows >= frames) rows >>= 1;
    return rows;
}

/* fir_shared over a plan's `ntiles` column groups.  Format 4 stops at two row tiles: with four, store_word_f4's epilogue takes the
 * kernel to 256 VGPRs and spills -- that variant does not exist. */
inline FirChoice fir_shared_choice(int format, int ntiles, int frames, int fir_rows)
{
    const int rows = fir_rows_for(fir_rows, ntiles, 4, frames, 64);
    return FirChoice{kFirShared, format == 4 ? std::min(rows, 2) : rows, false, false, false};
}

/* a launch of `n` chains over `frames` frames with fir_impl `impl`; `cascades`: the plan has cascades in front of its FIRs;
 * `plan_taps`: the plan's FIR chains x its longest FIR */
inline FirChoice fir_choice(int impl, long long n, int frames, const FirOptions &o, bool cascades, long long plan_taps)
{
    const bool rows_set = o.fir_rows == 1 || o.fir_rows == 2 || o.fir_rows == 4;
    const long long waves1 = n * ((frames + 255) / 256);         /* waves of one row tile */
    auto halved = [&](int rows) { while (rows > 1 && 128 * rows >= frames) rows >>= 1; return rows; };
    switch (impl) {
    case kFirFlow: {
        const int rows = halved(rows_set ? o.fir_rows : n >= 2048 ? 4 : n >= 1024 ? 2 : 1);
        /* at most a wave per SIMD: long chunks, two window images */
        return FirChoice{kFirFlow, rows, rows == 1 && waves1 <= 1024 && o.fir_rows != 1, false, false};
    }
    case kFirStream:      /* row tiles per wave: as many as leave every SIMD a wave (1024) */
        return FirChoice{kFirStream, halved(rows_set ? o.fir_rows : waves1 >= 4 * 1024 ? 4 : waves1 >= 2 * 1024 ? 2 : 1), false, false, false};
    case kFirTile: {
        const int rows = fir_rows_for(o.fir_rows, n, 1, frames, 256);
        /* the lean chunk boundary (fir_tile, LEAN) where it was measured to win (tools/fir_boundary_lab.sh, one box, long / lean):
         * plans without cascades in front (256 chains x 4096 taps: 40.9 -> 39.4 us per step) and launches of more than one round of
         * waves (4096 chains: 0.511 -> 0.506 ms; kLeanPlanTaps).  In between, the next blocks' cascades run beside the FIR and live on the long
         * boundary's bubbles: 2048 chains 0.259 -> 0.269 ms, 1024 chains 0.147 -> 0.154, 512 chains 0.0876 -> 0.0966. */
        const bool lean = o.fir_lean >= 0 ? o.fir_lean != 0 : (!cascades || plan_taps >= kLeanPlanTaps);
        /* one row tile and at most a wave per SIMD (1024): chunks twice as long (BIG) -- nothing hides a boundary there -- or, with
         * "fir_split" (opt-in, not the reference's summation order), two waves per tile instead */
        const bool few = rows == 1 && waves1 <= 1024;
        const bool split = few && o.fir_split;
        return FirChoice{kFirTile, rows, few && !split && o.fir_rows != 1, split, lean};
    }
    case kFirPlain: return FirChoice{kFirPlain, 1, false, false, false};
    default:              /* fir_mfma.  Few workgroups per CU: the deeper operand sets */
        return FirChoice{kFirMfma, n <= 2 * 256 ? 2 : 1, false, false, false};
    }
}

/* the launch of a plan's handed FIR chains ("fir_tail"): fir_plain with fir_impl 0, else fir_tile -- never split (the hand-over keeps the
 * reference's summation order), always the lean boundary (no cascade runs beside it: such a plan has no overlap) */
inline FirChoice fir_hand_choice(int impl, long long n, int frames, int fir_rows, bool cascades, long long plan_taps)
{
    FirChoice c = fir_choice(impl == kFirPlain ? kFirPlain : kFirTile, n, frames, FirOptions{fir_rows, 0, 1}, cascades, plan_taps);
    c.HAND = true;
    return c;
}

}  // namespace avdsp_layout

#endif

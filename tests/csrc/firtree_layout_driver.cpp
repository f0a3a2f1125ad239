/* tests/test_firtree_layout.py: what "mem_fir"  adds to the tables of avdsp_plan_layout.h -- a FIR in a trunk or a
 * branch: mem_trees' rows, fir_trunk and ring feeds, check_chains' fir / fir_plain / fir_hand lists and rows, cascade_groups' phases and
 * forms -- built against the header alone, with AddressSanitizer and UBSan, run as a program of its own.  argv[1] names a scenario; what
 * is printed is one JSON object. */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

struct Desc {
    int fmt = 6, total = 16384, instances = 0, chain_mem = 1, mem_fir = 1, fir_tail = 1, next = 1000;
    std::vector<avdsp_chain> chains;
    std::vector<int> coef, state, g_start, g_chains;
    int add(int nsec, int mode = AVDSP_LOAD_PLAIN)
    {
        avdsp_chain c;
        memset(&c, 0, sizeof c);
        const int i = (int)chains.size();
        c.in_io = 64 + i; c.load_mode = mode; c.nsec = nsec; c.sec_base = (int)coef.size(); c.n_out = 1; c.out_io[0] = i;
        for (int k = 0; k < nsec; k++) { coef.push_back(next); state.push_back(next + 6); next += 12; }
        chains.push_back(c);
        return i;
    }
    int trunk(int word, int nsec, int mode = AVDSP_LOAD_GAIN) { const int i = add(nsec, mode); chains[i].n_out = 0; chains[i].mem_word = word; chains[i].mem_store = 1; return i; }
    int branch(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_MEM); chains[i].in_io = 0; chains[i].mem_word = word; return i; }
    int fir(int i, int taps, int coef_word = 5000, int state_word = -1) { chains[i].fir_taps = taps; chains[i].fir_coef_word = coef_word; chains[i].fir_state_word = state_word < 0 ? 6000 + 40 * i : state_word; return i; }
    void delay(int i, int slot) { chains[i].delay_slot = slot; chains[i].delay_word = 3000 + 40 * i; chains[i].delay_max = 30; chains[i].delay_us_word = 20 + i; if (slot == AVDSP_DELAY_B) chains[i].sat = 1; }
    void dress(int i) { chains[i].sat = 1; chains[i].finish = AVDSP_FINISH_TPDF_GAIN; }
};

static void ints(const char *name, const std::vector<int> &v, bool last = false)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%d", i ? ", " : "", v[i]);
    printf("]%s", last ? "" : ", ");
}

static int run(Desc &D)
{
    avdsp_plan_desc d;
    memset(&d, 0, sizeof d);
    d.format = D.fmt; d.nchains = (int)D.chains.size(); d.chains = D.chains.data();
    d.nsections = (int)D.coef.size(); d.sec_coef_word = D.coef.data(); d.sec_state_word = D.state.data();
    d.store_mask = -1; d.instances = D.instances; d.chain_mem = D.chain_mem; d.mem_fir = D.mem_fir; d.fir_tail = D.fir_tail;
    if (!D.g_start.empty()) { d.fir_ngroups = (int)D.g_start.size() - 1; d.fir_group_start = D.g_start.data(); d.fir_group_chains = D.g_chains.data(); }
    const long long buf_words = mirror_words(&d, D.total);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    if (e.empty() && t.has_mem) e = mem_trees(&d, buf_words, t);
    if (e.empty()) e = check_chains(&d, buf_words, t);
    if (e.empty()) e = shared_fir_layout(&d, t).err;
    if (!e.empty()) { printf("{\"error\": \"%s\"}\n", e.c_str()); return 0; }
    const CascadeLayout L = cascade_groups(d.format, t);
    const SharedLayout S = shared_fir_layout(&d, t);
    printf("{\"has_mem\": %d, \"rows\": %d, \"cols\": %d, \"overlap_ok\": %d, \"all_rows\": %d, \"dev_chains\": %d, \"max_taps\": %d, \"shared\": %d, \"counts\": [%d, %d, %d], ",
           t.has_mem ? 1 : 0, t.n_hand_rows, t.n_mem_cols, overlap_ok(t) ? 1 : 0, (int)L.all_rows.size(), (int)L.dev_chains.size(), t.max_taps, (int)S.reps.size(),
           t.n_mem_trunks, t.n_mem_branches, t.n_mem_constant);
    printf("\"trees\": [");
    for (size_t k = 0; k < t.mem_tree_list.size(); k++) {
        const MemTree &m = t.mem_tree_list[k];
        printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", k ? ", " : "", m.word, m.src, m.trunk, m.row, m.col0, m.ncol, m.first_own, m.n_own);
    }
    printf("], \"tiles\": [");
    for (size_t k = 0; k < t.mem_tiles.size(); k++)
        printf("%s[%d, %d, %d, %d]", k ? ", " : "", t.mem_tiles[k].tree0, t.mem_tiles[k].ntree, t.mem_tiles[k].col0, t.mem_tiles[k].ncol);
    printf("], \"feeds\": [");
    for (size_t k = 0; k < t.mem_feed.size(); k++) printf("%s[%d, %d]", k ? ", " : "", t.mem_feed[k].tree, t.mem_feed[k].cid);
    printf("], \"groups\": [");
    for (size_t k = 0; k < L.groups.size(); k++) {
        const GroupLayout &g = L.groups[k];
        printf("%s{\"nsec\": %d, \"phase\": %d, \"wide\": %d, \"hand\": %d, \"all_fir\": %d, \"pieces\": %d, ", k ? ", " : "", g.nsec, g.phase, g.wide ? 1 : 0, g.hand ? 1 : 0,
               g.all_fir ? 1 : 0, (int)g.pieces.size());
        std::vector<int> to_ring;                            /* per row of biquad_row's records: bit 9, the cascade writes the chain's ring */
        for (const RowRec &r : g.rows) to_ring.push_back(r.flags >> 9 & 1);
        if (!g.pieces.empty()) for (const RowRec &r : g.pieces.back().rows) to_ring.push_back(r.flags >> 9 & 1);
        ints("to_ring", to_ring);
        ints("ids", g.ids, true);
        printf("}");
    }
    printf("], ");
    std::vector<int> own, mode, in_io, kind, stored;
    for (const MemOwn &o : t.mem_own) own.push_back(o.cid);
    for (size_t i = 0; i < t.chains.size(); i++) { mode.push_back(t.chains[i].load_mode); in_io.push_back(t.chains[i].in_io); kind.push_back(t.mem_kind[i]); stored.push_back(t.mem_stored[i]); }
    /* every index a kernel follows lies inside what the plan allocates: rows, columns, feeds' trees and chains */
    int bad = 0;
    for (const MemFeed &f : t.mem_feed) bad += f.tree < 0 || f.tree >= (int)t.mem_tree_list.size() || f.cid < 0 || f.cid >= d.nchains || !t.chains[f.cid].fir_taps;
    if (!t.mem_feed.empty()) {
        bad += t.mem_feed_start.size() != t.mem_tree_list.size() + 1 || t.mem_feed_start.front() != 0 || t.mem_feed_start.back() != (int)t.mem_feed.size();
        for (size_t k = 0; k + 1 < t.mem_feed_start.size(); k++) {
            bad += t.mem_feed_start[k] > t.mem_feed_start[k + 1];
            for (int q = t.mem_feed_start[k]; q < t.mem_feed_start[k + 1]; q++) bad += t.mem_feed[q].tree != (int)k;
        }
    }
    for (int r : t.hand_row) bad += r >= t.n_hand_rows;
    for (const MemTree &m : t.mem_tree_list) bad += m.row >= t.n_hand_rows || m.col0 + m.ncol > t.n_mem_cols;
    for (int i : t.fir) bad += i < 0 || i >= d.nchains || t.chains[i].fir_coef_word + t.chains[i].fir_taps > buf_words || t.chains[i].fir_state_word + t.chains[i].fir_taps > buf_words;
    ints("own", own); ints("col_tree", t.mem_col_tree); ints("load_mode", mode); ints("in_io", in_io); ints("kind", kind); ints("stored", stored);
    ints("feed_start", t.mem_feed_start); ints("fir", t.fir); ints("fir_trunk", t.fir_trunk); ints("fir_plain", t.fir_plain); ints("fir_hand", t.fir_hand);
    ints("hand_row", t.hand_row); ints("tail", t.tail); ints("pass", t.pass); ints("pass_dressed", t.pass_dressed);
    printf("\"bad_indices\": %d, \"io_in\": [%d, %d], \"io_out\": [%d, %d]}\n", bad, t.io_in_min, t.io_in_max, t.io_out_min, t.io_out_max);
    return 0;
}

int main(int argc, char **argv)
{
    std::string s = argc > 1 ? argv[1] : "";
    Desc D;
    /* "<scenario>_off": the same descriptor with mem_fir 0 */
    const bool off = s.size() > 4 && s.compare(s.size() - 4, 4, "_off") == 0;
    if (off) { s.resize(s.size() - 4); D.mem_fir = 0; }
    if (s == "tree") {
        D.fir(D.trunk(100, 2), 31);                          /* 0: tree 0 -- cascade to the ring, the FIR fills row 0 */
        D.fir(D.add(1), 63);                                 /* 1: an ordinary plain FIR chain between */
        D.fir(D.branch(100, 1), 63);                         /* 2: column 0, a phase-1 cascade that feeds the ring; plain */
        D.chains[D.fir(D.branch(100, 0), 63)].sat = 1;       /* 3: a FIR alone: the stage feeds its ring; plain */
        D.branch(100, 3);                                    /* 4: no FIR: column 1 */
        D.fir(D.trunk(104, 0, AVDSP_LOAD_PLAIN), 7);         /* 5: tree 1 -- a trunk that is a FIR alone: row 1 */
        D.delay(D.fir(D.branch(104, 0), 255), AVDSP_DELAY_A);/* 6: fed by the stage, handed: row 4 */
        D.dress(D.fir(D.branch(104, 17), 700));              /* 7: column 2, two pieces, handed: row 5 */
        D.fir(D.branch(200, 0), 1500);                       /* 8: tree 3 (behind the trees with a trunk), a word nobody writes; fed by the stage */
        D.delay(D.branch(200, 0), AVDSP_DELAY_B);            /* 9: no FIR: chain_tail from a row the stage fills: row 3 */
        D.delay(D.fir(D.add(2), 63), AVDSP_DELAY_B);         /* 10: an ordinary handed FIR chain: row 6 */
        D.trunk(106, 2);                                     /* 11: tree 2 -- a trunk without FIR: WIDE + HAND, row 2 (the trunks' rows come first) */
        D.chains[D.branch(106, 0)].sat = 1;                  /* 12: the stage stores it */
    } else if (s == "feeds") {
        /* 17 trees, one more than a tile; tree 3 has 5 FIR-only branches, tree 16 has 17; tree 5 has 70 columns (it closes its tile) */
        for (int k = 0; k < 17; k++) D.trunk(100 + 2 * k, 1);
        for (int j = 0; j < 5; j++) D.fir(D.branch(106, 0), 63);
        for (int j = 0; j < 70; j++) D.branch(110, 1);
        for (int j = 0; j < 17; j++) D.fir(D.branch(132, 0), 63);
    } else if (s == "plain") {
        D.add(1); D.fir(D.add(2), 63); D.add(1); D.add(0); D.add(17); D.fir(D.add(0), 31);
        D.delay(2, AVDSP_DELAY_A);
    } else if (s == "memtree") {                             /* a "chain_mem" plan without a FIR */
        D.trunk(100, 2); D.add(1); D.branch(100, 3); D.chains[D.branch(100, 0)].sat = 1; D.delay(D.branch(100, 0), AVDSP_DELAY_A);
        D.trunk(104, 0, AVDSP_LOAD_PLAIN); D.delay(D.branch(104, 0), AVDSP_DELAY_B); D.branch(200, 17);
    }
    else if (s == "trunk_fir") { D.fir(D.trunk(100, 1), 8); }
    else if (s == "branch_fir") { D.fir(D.branch(100, 0), 8); }
    else if (s == "beside") { D.trunk(100, 1); D.fir(D.add(0), 8); }
    else if (s == "format2") { D.fmt = 2; D.fir(D.trunk(100, 1), 8); }
    else if (s == "no_fir_tail") { D.fir_tail = 0; D.trunk(100, 1); D.delay(D.fir(D.branch(100, 0), 8), AVDSP_DELAY_A); }
    else if (s == "no_fir_tail_dressed") { D.fir_tail = 0; D.trunk(100, 1); D.dress(D.fir(D.branch(100, 0), 8)); }
    else if (s == "trunk_taps_high") { D.fir(D.trunk(100, 1), 8, D.total - 7); }
    else if (s == "trunk_history_high") { D.fir(D.trunk(100, 1), 8, 5000, D.total - 7); }
    else if (s == "trunk_history_last") { D.fir(D.trunk(100, 1), 8, 5000, D.total - 8); }
    else if (s == "branch_taps_high") { D.trunk(100, 1); D.fir(D.branch(100, 0), 8, D.total - 7); }
    else if (s == "branch_history_negative") { D.trunk(100, 1); D.fir(D.branch(100, 0), 8, 5000, 0); D.chains[1].fir_state_word = -1; }
    else if (s == "trunk_stored") { const int i = D.fir(D.trunk(100, 1), 8); D.chains[i].n_out = 1; }
    else if (s == "trunk_delayed") { D.delay(D.fir(D.trunk(100, 1), 8), AVDSP_DELAY_A); }
    else if (s == "groups") {                                /* a hand-made descriptor that offers a tree core's chains to fir_shared */
        D.trunk(100, 1);
        for (int j = 0; j < 16; j++) { D.fir(D.branch(100, 0), 64); D.g_chains.push_back(1 + j); }
        D.g_start = {0, 16};
    }
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    return run(D);
}

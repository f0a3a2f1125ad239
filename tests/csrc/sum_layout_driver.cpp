/* tests/test_sum_layout.py: what avdsp_plan_layout.h (check_heads, mem_trees, check_chains, cascade_groups) makes of a plan with sum
 * heads ("chain_sum") -- built against the header alone, with AddressSanitizer and UBSan, run as a program of its own.
 * argv[1] names a scenario; what is printed is one JSON object. */
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

struct Desc {
    int fmt = 6, total = 8192, chain_mem = 1, chain_sum = 1, chain_ways = 1, mem_fir = 0, next = 1000;
    std::vector<avdsp_chain> chains;
    std::vector<int> coef, state;
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
    int trunk(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_GAIN); chains[i].n_out = 0; chains[i].mem_word = word; chains[i].mem_store = 1; chains[i].gain_bits = 0x3F000000u + (unsigned)i; return i; }
    int branch(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_MEM); chains[i].in_io = 0; chains[i].mem_word = word; return i; }
    /* a sum head: LOAD_MEM words[0], then (LOAD_MEM words[k], ADDXY | SUBXY alternating from ADDXY) */
    int bus(std::initializer_list<int> words, int nsec)
    {
        const int i = branch(*words.begin(), nsec);
        int k = 0;
        for (auto w = words.begin() + 1; w != words.end(); ++w, ++k)
            if (k < AVDSP_MAX_SUM_TERMS - 1) { chains[i].sum_word[k] = *w; chains[i].sum_op[k] = k % 2 ? AVDSP_SUM_SUB : AVDSP_SUM_ADD; }
        chains[i].sum_n = k;
        return i;
    }
    int delay(int i, int slot) { chains[i].delay_slot = slot; chains[i].delay_word = 6000 + 40 * i; chains[i].delay_max = 30; chains[i].delay_us_word = 20 + i; if (slot == AVDSP_DELAY_B) chains[i].sat = 1; return i; }
    int ops(int i) { chains[i].ways_n = 1; chains[i].ways_op[0] = AVDSP_WAY_NEG; return i; }
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
    d.store_mask = -1; d.chain_mem = D.chain_mem; d.chain_ways = D.chain_ways; d.chain_sum = D.chain_sum; d.mem_fir = D.mem_fir;
    d.delay_line_factor = 206158430u;                        /* 48 kHz */
    const long long buf_words = mirror_words(&d, D.total);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    if (e.empty() && t.has_mem) e = mem_trees(&d, buf_words, t);
    if (e.empty()) e = check_chains(&d, buf_words, t);
    if (!e.empty()) { printf("{\"error\": \"%s\"}\n", e.c_str()); return 0; }
    const CascadeLayout L = cascade_groups(d.format, t);
    printf("{\"rows\": %d, \"sums\": %d, \"cols\": %d, \"branches\": %d, \"constant\": %d, \"dev_chains\": %d, ", t.n_hand_rows, t.n_mem_sums, t.n_mem_cols, t.n_mem_branches,
           t.n_mem_constant, (int)L.dev_chains.size());
    printf("\"trees\": [");
    for (size_t k = 0; k < t.mem_tree_list.size(); k++) {
        const MemTree &m = t.mem_tree_list[k];
        printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", k ? ", " : "", m.word, m.src, m.trunk, m.row, m.col0, m.ncol, m.first_own, m.n_own);
    }
    printf("], \"terms\": [");
    for (size_t k = 0; k < t.mem_terms.size(); k++) {
        const MemTerm &m = t.mem_terms[k];
        printf("%s[%d, %d, %d, %d, %d, %u, %d]", k ? ", " : "", m.src, m.row, m.word, m.in_io, m.load_mode, m.gain_bits, m.op);
    }
    printf("], \"tiles\": [");
    for (size_t k = 0; k < t.mem_tiles.size(); k++) {
        const MemTile &m = t.mem_tiles[k];
        printf("%s[%d, %d, %d, %d]", k ? ", " : "", m.tree0, m.ntree, m.col0, m.ncol);
    }
    printf("], \"groups\": [");
    for (size_t k = 0; k < L.groups.size(); k++) {
        const GroupLayout &g = L.groups[k];
        printf("%s{\"nsec\": %d, \"phase\": %d, \"wide\": %d, \"hand\": %d, ", k ? ", " : "", g.nsec, g.phase, g.wide ? 1 : 0, g.hand ? 1 : 0);
        ints("ids", g.ids, true);
        printf("}");
    }
    printf("], ");
    std::vector<int> own, stored, kind, load, in_io, feed;
    for (const MemOwn &o : t.mem_own) own.push_back(o.cid);
    for (const MemFeed &f : t.mem_feed) feed.push_back(f.cid);
    for (size_t i = 0; i < t.chains.size(); i++) { stored.push_back(t.mem_stored[i]); kind.push_back(t.mem_kind[i]); load.push_back(t.chains[i].load_mode); in_io.push_back(t.chains[i].in_io); }
    ints("sum_start", t.mem_sum_start); ints("col_tree", t.mem_col_tree); ints("feed", feed); ints("feed_start", t.mem_feed_start);
    ints("own", own); ints("stored", stored); ints("kind", kind); ints("load", load); ints("in_io", in_io); ints("mem_row", t.mem_row);
    ints("hand_row", t.hand_row); ints("tail", t.tail); ints("pass", t.pass); ints("fir", t.fir);
    printf("\"io_in\": [%d, %d], \"io_out\": [%d, %d]}\n", t.io_in_min, t.io_in_max, t.io_out_min, t.io_out_max);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    Desc D;
    if (s == "sum" || s == "sum_off" || s == "sum_format2" || s == "sum_format4") {
        D.trunk(100, 2);                                     /* 0: tree 0, row 0 */
        D.trunk(104, 0);                                     /* 1: tree 1, a trunk without sections */
        D.branch(100, 1);                                    /* 2: a branch of tree 0: column 0 */
        D.branch(108, 0);                                    /* 3: a word nobody writes: tree 2, stored by the stage */
        D.bus({100, 104, 108}, 2);                           /* 4: a term of each kind, sections: tree 3, column 1 */
        D.bus({108, 108}, 0);                                /* 5: one word twice, no sections: tree 4, the stage's own store */
        D.delay(D.bus({104, 112}, 0), AVDSP_DELAY_A);        /* 6: a delay line: tree 5, the stage fills row 1; word 112 has no tree */
        D.ops(D.bus({100, 104}, 0));                         /* 7: way operations: tree 6, row 2 */
        D.add(1);                                            /* 8: ordinary */
        D.delay(D.bus({104, 100}, 1), AVDSP_DELAY_B);        /* 9: sections and a delay: tree 7, column 2, row 3 of its own cascade */
        if (s == "sum_off") D.chain_sum = 0;
        if (s == "sum_format2") D.fmt = 2;
        if (s == "sum_format4") D.fmt = 4;
    } else if (s == "feed") {
        D.mem_fir = 1;
        D.trunk(100, 1);
        const int i = D.bus({100, 104}, 0);                  /* a lone FIR behind the head: a MemFeed of its sum tree */
        D.chains[i].fir_taps = 8; D.chains[i].fir_coef_word = 200; D.chains[i].fir_state_word = 300;
    } else if (s == "seam15" || s == "seam16" || s == "seam17") {
        /* 3 word trees, then 15, 16 or 17 sum trees of one column each: across the tile of 16 trees */
        D.trunk(100, 1); D.trunk(104, 0); D.branch(100, 1); D.branch(104, 0); D.branch(108, 1);
        const int n = s == "seam15" ? 15 : s == "seam16" ? 16 : 17;
        for (int k = 0; k < n; k++) D.bus({k % 2 ? 104 : 100, 108, 100}, k % 3 ? 1 : 0);
    } else if (s == "plain" || s == "plain_off") {
        /* no sum head anywhere: the tables of the plan with the flag on and off */
        D.add(1); D.add(0); D.trunk(100, 2); D.branch(100, 1); D.delay(D.branch(100, 0), AVDSP_DELAY_B); D.chains[D.branch(100, 0)].sat = 1;
        D.trunk(104, 0); D.ops(D.branch(104, 0)); D.branch(108, 17);
        if (s == "plain_off") D.chain_sum = 0;
    } else if (s == "eight") { D.bus({100, 100, 100, 100, 100, 100, 100, 100}, 0); D.chains[0].sum_n = 8; }
    else if (s == "negative") { D.bus({100, 104}, 0); D.chains[0].sum_n = -1; }
    else if (s == "bad_op") { D.bus({100, 104, 108}, 0); D.chains[0].sum_op[1] = 3; }
    else if (s == "word_outside") { D.bus({100, D.total - 1}, 0); }
    else if (s == "word_zero") { D.bus({100, 0}, 0); }
    else if (s == "head_outside") { D.bus({D.total - 1, 100}, 0); }
    else if (s == "overlap") { D.trunk(100, 1); D.bus({100, 101}, 0); }
    else if (s == "before_trunk") { D.trunk(100, 1); D.bus({100, 104}, 0); D.trunk(104, 1); }
    else if (s == "sum_trunk") { const int i = D.trunk(100, 1); D.chains[i].sum_n = 1; D.chains[i].sum_word[0] = 104; D.chains[i].sum_op[0] = AVDSP_SUM_ADD; D.branch(100, 0); }
    else if (s == "sum_trunk_load_mem") { const int i = D.bus({100, 104}, 1); D.chains[i].mem_store = 1; D.chains[i].n_out = 0; }
    else if (s == "no_branch") { const int i = D.add(1); D.chains[i].sum_n = 1; D.chains[i].sum_word[0] = 104; D.chains[i].sum_op[0] = AVDSP_SUM_ADD; D.trunk(100, 1); D.branch(100, 0); }
    else if (s == "format3") { D.fmt = 3; D.bus({100, 104}, 0); }
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    return run(D);
}

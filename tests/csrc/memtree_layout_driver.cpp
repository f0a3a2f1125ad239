/* tests/test_memtree_layout.py: the "chain_mem" stage of avdsp_plan_layout.h (mem_trees) and what check_heads, check_chains,
 * cascade_groups and overlap_ok make of a plan with trunks and branches -- built against the header alone, with AddressSanitizer and
 * UBSan, run as a program of its own.  argv[1] names a scenario; what is printed is one JSON object. */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

struct Desc {
    int fmt = 6, total = 4096, instances = 0, chain_mem = 1, next = 1000;
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
    int trunk(int word, int nsec, int mode = AVDSP_LOAD_GAIN) { const int i = add(nsec, mode); chains[i].n_out = 0; chains[i].mem_word = word; chains[i].mem_store = 1; return i; }
    int branch(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_MEM); chains[i].in_io = 0; chains[i].mem_word = word; return i; }
    void delay(int i, int slot) { chains[i].delay_slot = slot; chains[i].delay_word = 3000 + 40 * i; chains[i].delay_max = 30; chains[i].delay_us_word = 20 + i; if (slot == AVDSP_DELAY_B) chains[i].sat = 1; }
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
    d.store_mask = -1; d.instances = D.instances; d.chain_mem = D.chain_mem;
    const long long buf_words = mirror_words(&d, D.total);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    if (e.empty() && t.has_mem) e = mem_trees(&d, buf_words, t);
    if (e.empty()) e = check_chains(&d, buf_words, t);
    if (!e.empty()) { printf("{\"error\": \"%s\"}\n", e.c_str()); return 0; }
    const CascadeLayout L = cascade_groups(d.format, t);
    printf("{\"has_mem\": %d, \"rows\": %d, \"cols\": %d, \"overlap_ok\": %d, \"all_rows\": %d, \"dev_chains\": %d, \"counts\": [%d, %d, %d], ",
           t.has_mem ? 1 : 0, t.n_hand_rows, t.n_mem_cols, overlap_ok(t) ? 1 : 0, (int)L.all_rows.size(), (int)L.dev_chains.size(),
           t.n_mem_trunks, t.n_mem_branches, t.n_mem_constant);
    printf("\"trees\": [");
    for (size_t k = 0; k < t.mem_tree_list.size(); k++) {
        const MemTree &m = t.mem_tree_list[k];
        printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", k ? ", " : "", m.word, m.src, m.trunk, m.row, m.col0, m.ncol, m.first_own, m.n_own);
    }
    printf("], \"tiles\": [");
    for (size_t k = 0; k < t.mem_tiles.size(); k++)
        printf("%s[%d, %d, %d, %d]", k ? ", " : "", t.mem_tiles[k].tree0, t.mem_tiles[k].ntree, t.mem_tiles[k].col0, t.mem_tiles[k].ncol);
    printf("], \"groups\": [");
    for (size_t k = 0; k < L.groups.size(); k++) {
        const GroupLayout &g = L.groups[k];
        printf("%s{\"nsec\": %d, \"phase\": %d, \"wide\": %d, \"hand\": %d, \"pieces\": %d, ", k ? ", " : "", g.nsec, g.phase, g.wide ? 1 : 0, g.hand ? 1 : 0, (int)g.pieces.size());
        bool same_phase = true;
        for (const GroupLayout &p : g.pieces) same_phase = same_phase && p.phase == g.phase;
        printf("\"pieces_in_phase\": %d, ", same_phase ? 1 : 0);
        ints("ids", g.ids, true);
        printf("}");
    }
    printf("], ");
    std::vector<int> own, mode, in_io, kind, stored;
    for (const MemOwn &o : t.mem_own) own.push_back(o.cid);
    for (size_t i = 0; i < t.chains.size(); i++) { mode.push_back(t.chains[i].load_mode); in_io.push_back(t.chains[i].in_io); kind.push_back(t.mem_kind[i]); stored.push_back(t.mem_stored[i]); }
    ints("own", own); ints("col_tree", t.mem_col_tree); ints("load_mode", mode); ints("in_io", in_io); ints("kind", kind); ints("stored", stored);
    ints("hand_row", t.hand_row); ints("tail", t.tail); ints("pass", t.pass); ints("pass_dressed", t.pass_dressed);
    printf("\"io_in\": [%d, %d], \"io_out\": [%d, %d]}\n", t.io_in_min, t.io_in_max, t.io_out_min, t.io_out_max);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    Desc D;
    if (s == "tree" || s == "tree_off") {
        D.trunk(100, 2);                                     /* 0: tree 0, row 0 */
        D.add(1);                                            /* 1: an ordinary chain between */
        D.branch(100, 3);                                    /* 2: column 0 */
        D.chains[D.branch(100, 0)].sat = 1;                  /* 3: the stage stores it */
        D.delay(D.branch(100, 0), AVDSP_DELAY_A);            /* 4: chain_tail, from the trunk's row */
        D.trunk(104, 0, AVDSP_LOAD_PLAIN);                   /* 5: tree 1, the stage loads the sample */
        D.delay(D.branch(104, 0), AVDSP_DELAY_B);            /* 6: chain_tail, from a row the stage fills */
        D.branch(200, 17);                                   /* 7: tree 2, a word nobody writes; two pieces */
        { const int i = D.branch(200, 0); D.chains[i].sat = 1; D.chains[i].finish = AVDSP_FINISH_TPDF_GAIN; }      /* 8: the stage finishes it */
        D.delay(D.branch(100, 1), AVDSP_DELAY_A);            /* 9: tree 0 again, not adjacent: column 1, a row of its own */
        D.add(1);                                            /* 10 */
        D.add(0);                                            /* 11: passthrough */
        if (s == "tree_off") D.chain_mem = 0;
    } else if (s == "plain" || s == "plain_off") {
        D.add(1); D.add(2); D.add(1); D.add(0); D.add(17); D.add(3);
        D.chains[1].sat = 1; D.chains[1].finish = AVDSP_FINISH_TPDF;
        D.delay(2, AVDSP_DELAY_A);
        if (s == "plain_off") D.chain_mem = 0;
    } else if (s == "tiles") {
        for (int k = 0; k < 40; k++) { D.trunk(100 + 2 * k, 1); D.branch(100 + 2 * k, 1); }
        D.trunk(400, 1);
        for (int k = 0; k < 70; k++) D.branch(400, 1);
        D.trunk(402, 0); D.branch(402, 2);
    } else if (s == "trunk_off") { D.trunk(100, 1); D.chain_mem = 0; }
    else if (s == "branch_off") { D.add(1); D.branch(100, 1); D.chain_mem = 0; }
    else if (s == "word_high") { D.trunk(D.total - 1, 1); }
    else if (s == "word_last") { D.trunk(D.total - 2, 1); }
    else if (s == "word_zero") { D.trunk(0, 1); }
    else if (s == "branch_high") { D.branch(D.total - 1, 1); }
    else if (s == "branch_negative") { D.branch(-5, 0); }
    else if (s == "format3") { D.fmt = 3; D.trunk(100, 1); }
    else if (s == "instances") { D.instances = 2; D.trunk(100, 1); }
    else if (s == "mux") { D.trunk(100, 1); const int i = D.add(0, AVDSP_LOAD_MUX); D.chains[i].mux_word = 200; D.chains[i].mux_count = 1; D.chains[i].mux_result_word = 300; }
    else if (s == "two_trunks") { D.trunk(100, 1); D.trunk(100, 0); }
    else if (s == "overlap") { D.trunk(100, 1); D.branch(101, 0); }
    else if (s == "lag") { D.branch(100, 1); D.trunk(100, 1); }
    else if (s == "fir") { D.trunk(100, 1); const int i = D.add(0); D.chains[i].fir_taps = 8; D.chains[i].fir_coef_word = 200; D.chains[i].fir_state_word = 300; }
    else if (s == "stored_trunk") { const int i = D.trunk(100, 1); D.chains[i].n_out = 1; }
    else if (s == "trunk_from_mem") { const int i = D.trunk(100, 1); D.chains[i].load_mode = AVDSP_LOAD_MEM; }
    else if (s == "branch_fir") { const int i = D.branch(100, 0); D.chains[i].fir_taps = 8; D.chains[i].fir_coef_word = 200; D.chains[i].fir_state_word = 300; }
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    return run(D);
}

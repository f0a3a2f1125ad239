/* tests/test_ways_layout.py: what avdsp_plan_layout.h (check_heads, mem_trees, check_chains, cascade_groups) makes of a plan whose chains
 * have way operations ("chain_ways") -- built against the header alone, with AddressSanitizer and UBSan, run as a
 * program of its own.  argv[1] names a scenario; what is printed is one JSON object. */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

struct Desc {
    int fmt = 6, total = 8192, instances = 0, chain_mem = 1, chain_ways = 1, next = 1000;
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
    int trunk(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_GAIN); chains[i].n_out = 0; chains[i].mem_word = word; chains[i].mem_store = 1; return i; }
    int branch(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_MEM); chains[i].in_io = 0; chains[i].mem_word = word; return i; }
    int delay(int i, int slot) { chains[i].delay_slot = slot; chains[i].delay_word = 6000 + 40 * i; chains[i].delay_max = 30; chains[i].delay_us_word = 20 + i; if (slot == AVDSP_DELAY_B) chains[i].sat = 1; return i; }
    int ops(int i, int n)
    {
        chains[i].ways_n = n;
        for (int k = 0; k < n && k < AVDSP_MAX_WAY_OPS; k++) { chains[i].ways_op[k] = k % 2 ? AVDSP_WAY_NEG : AVDSP_WAY_GAIN; chains[i].ways_gain_bits[k] = 0x3F000000u; }
        return i;
    }
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
    d.store_mask = -1; d.instances = D.instances; d.chain_mem = D.chain_mem; d.chain_ways = D.chain_ways;
    d.delay_line_factor = 206158430u;                        /* 48 kHz */
    const long long buf_words = mirror_words(&d, D.total);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    if (e.empty() && t.has_mux) { std::vector<int> w((size_t)(t.mux_hi - t.mux_lo), 64); e = mux_records(w, t); }
    if (e.empty() && t.has_mem) e = mem_trees(&d, buf_words, t);
    if (e.empty()) e = check_chains(&d, buf_words, t);
    if (!e.empty()) { printf("{\"error\": \"%s\"}\n", e.c_str()); return 0; }
    const CascadeLayout L = cascade_groups(d.format, t);
    printf("{\"rows\": %d, \"way_ops\": %d, \"dev_chains\": %d, \"all_rows\": %d, \"overlap_ok\": %d, ", t.n_hand_rows, t.n_way_ops, (int)L.dev_chains.size(),
           (int)L.all_rows.size(), overlap_ok(t) ? 1 : 0);
    printf("\"trees\": [");
    for (size_t k = 0; k < t.mem_tree_list.size(); k++) {
        const MemTree &m = t.mem_tree_list[k];
        printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", k ? ", " : "", m.word, m.src, m.trunk, m.row, m.col0, m.ncol, m.first_own, m.n_own);
    }
    printf("], \"groups\": [");
    for (size_t k = 0; k < L.groups.size(); k++) {
        const GroupLayout &g = L.groups[k];
        printf("%s{\"nsec\": %d, \"phase\": %d, \"wide\": %d, \"hand\": %d, \"P\": %d, ", k ? ", " : "", g.nsec, g.phase, g.wide ? 1 : 0, g.hand ? 1 : 0, g.P);
        std::vector<int> pw, ph, pn, pops;
        for (const GroupLayout &p : g.pieces) {
            pw.push_back(p.wide); ph.push_back(p.hand); pn.push_back(p.nsec);
            for (int id : p.ids) pops.push_back(L.dev_chains[(size_t)id].ways_n);
        }
        ints("piece_nsec", pn); ints("piece_wide", pw); ints("piece_hand", ph); ints("piece_ways_n", pops);
        printf("\"rows\": %d, ", (int)g.rows.size());
        ints("ids", g.ids, true);
        printf("}");
    }
    printf("], ");
    std::vector<int> own, stored, kind;
    for (const MemOwn &o : t.mem_own) own.push_back(o.cid);
    for (size_t i = 0; i < t.chains.size(); i++) { stored.push_back(t.mem_stored[i]); kind.push_back(t.mem_kind[i]); }
    ints("own", own); ints("stored", stored); ints("kind", kind); ints("mem_row", t.mem_row);
    ints("hand_row", t.hand_row); ints("tail", t.tail); ints("pass", t.pass); ints("pass_dressed", t.pass_dressed); ints("fir", t.fir);
    printf("\"dressed\": %d, \"io_in\": [%d, %d], \"io_out\": [%d, %d]}\n", t.n_dressed, t.io_in_min, t.io_in_max, t.io_out_min, t.io_out_max);
    return 0;
}

static void dress(Desc &D, int i) { D.chains[i].sat = 1; D.chains[i].finish = AVDSP_FINISH_TPDF_GAIN; D.chains[i].finish_gain_bits = 0x3F000000u; }

int main(int argc, char **argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    Desc D;
    if (s == "ways" || s == "ways_off" || s == "ways_format2" || s == "ways_format4") {
        D.add(2);                                            /* 0: ordinary */
        D.ops(D.add(2), 1);                                  /* 1: way operations behind two sections: row 0 */
        D.ops(D.add(0), 4);                                  /* 2: ... behind the head: chain_tail loads the sample */
        D.delay(D.add(1), AVDSP_DELAY_A);                    /* 3: a delayed chain: row 1 */
        D.delay(D.ops(D.add(17), 2), AVDSP_DELAY_B);         /* 4: both, two pieces: row 2 */
        D.add(0);                                            /* 5: a passthrough */
        dress(D, D.ops(D.add(0), 1));                        /* 6: a dressed finish behind the operations: chain_tail's, not passthrough's */
        D.trunk(100, 1);                                     /* 7: tree 0, row 3 */
        D.ops(D.branch(100, 0), 2);                          /* 8: a branch without sections: the trunk's row */
        D.chains[D.branch(100, 0)].sat = 1;                  /* 9: ... and one the stage finishes itself */
        D.trunk(104, 0);                                     /* 10: tree 1, no row of its own */
        D.ops(D.branch(104, 0), 1);                          /* 11: the stage fills row 4 for it */
        D.ops(D.branch(104, 2), 1);                          /* 12: a branch with sections: column 0, row 5 of its own cascade */
        dress(D, D.add(2));                                  /* 13: a dressed chain without operations: WIDE, not HAND */
        if (s == "ways_off") D.chain_ways = 0;
        if (s == "ways_format2") D.fmt = 2;
        if (s == "ways_format4") D.fmt = 4;
    } else if (s == "plain" || s == "plain_off") {
        /* no way operations anywhere: the tables of the plan with the flag on and off */
        D.add(1); D.add(2); D.add(1); D.add(0); D.add(17); D.add(3);
        dress(D, 1);
        D.delay(2, AVDSP_DELAY_A);
        D.trunk(100, 2); D.branch(100, 1); D.delay(D.branch(100, 0), AVDSP_DELAY_B); D.chains[D.branch(100, 0)].sat = 1;
        if (s == "plain_off") D.chain_ways = 0;
    } else if (s == "format3") { D.fmt = 3; D.ops(D.add(1), 1); }
    else if (s == "format5") { D.fmt = 5; D.ops(D.add(0), 1); }
    else if (s == "instances") { D.instances = 2; D.ops(D.add(1), 1); }
    else if (s == "fir") { const int i = D.ops(D.add(1), 1); D.chains[i].fir_taps = 8; D.chains[i].fir_coef_word = 200; D.chains[i].fir_state_word = 300; }
    else if (s == "mux") { D.ops(D.add(1), 1); const int i = D.add(0, AVDSP_LOAD_MUX); D.chains[i].mux_word = 200; D.chains[i].mux_count = 1; D.chains[i].mux_result_word = 300; }
    else if (s == "five") { D.ops(D.add(1), 5); }
    else if (s == "negative") { D.ops(D.add(1), 1); D.chains[0].ways_n = -1; }
    else if (s == "bad_op") { D.ops(D.add(1), 2); D.chains[0].ways_op[1] = 3; }
    else if (s == "trunk") { D.ops(D.trunk(100, 1), 1); D.branch(100, 0); }
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    return run(D);
}

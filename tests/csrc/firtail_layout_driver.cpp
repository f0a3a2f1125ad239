/* Stand-alone driver of tests/test_firtail_lowering.py: what avdsp_amd/csrc/avdsp_plan_layout.h makes of handed FIR chains ("fir_tail",
 * DESIGN.md 4.2h) -- check_chains' lists, cascade_groups' launch groups, shared_fir_layout, overlap_ok, fir_hand_choice.  No HIP.
 *
 *   firtail_layout_driver layout format fir_tail grouped  nchains x (nsec taps finish delay_slot sat bank)
 *       chains get their words in order (a section 12 words, a FIR its taps -- or those of chain `bank`, -1: its own -- and a history,
 *       a delay line 1 + 100 words and one to keep the next section even); grouped 1: the chains with taps and neither finish nor delay are offered as one FIR group.
 *       Prints one JSON object, or {"error": text}.
 *   firtail_layout_driver choice impl n frames fir_rows
 */
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

static void ints(const char *name, const std::vector<int> &v, bool last = false)
{
    std::cout << '"' << name << "\": [";
    for (size_t i = 0; i < v.size(); i++) std::cout << (i ? ", " : "") << v[i];
    std::cout << (last ? "]" : "], ");
}

static void group_json(const GroupLayout &g)
{
    std::cout << "{\"nsec\": " << g.nsec << ", \"n\": " << g.n << ", \"P\": " << g.P << ", \"wide\": " << g.wide << ", \"hand\": " << g.hand << ", \"all_fir\": " << g.all_fir
              << ", \"nrows\": " << g.rows.size() << ", ";
    ints("ids", g.ids);
    std::cout << "\"pieces\": [";
    for (size_t i = 0; i < g.pieces.size(); i++) { if (i) std::cout << ", "; group_json(g.pieces[i]); }
    std::cout << "]}";
}

int main(int argc, char **argv)
{
    if (argc >= 6 && !strcmp(argv[1], "choice")) {
        const FirChoice c = fir_hand_choice(atoi(argv[2]), atoll(argv[3]), atoi(argv[4]), atoi(argv[5]), true, 0);
        std::cout << "{\"family\": " << c.family << ", \"R\": " << c.R << ", \"BIG\": " << c.BIG << ", \"SPLIT\": " << c.SPLIT << ", \"LEAN\": " << c.LEAN << ", \"HAND\": " << c.HAND << "}\n";
        return 0;
    }
    if (argc < 5 || strcmp(argv[1], "layout") || (argc - 5) % 6) return 2;
    const int format = atoi(argv[2]), fir_tail = atoi(argv[3]), grouped = atoi(argv[4]), n = (argc - 5) / 6;
    std::vector<avdsp_chain> chains(n);
    std::vector<int> coef, state, members;
    int w = 16;
    for (int i = 0; i < n; i++) {
        char **a = argv + 5 + 6 * i;
        avdsp_chain c;
        memset(&c, 0, sizeof c);
        c.in_io = 1000 + i; c.n_out = 1; c.out_io[0] = i;
        c.nsec = atoi(a[0]); c.sec_base = (int)coef.size();
        for (int q = 0; q < c.nsec; q++) { coef.push_back(w); state.push_back(w + 6); w += 12; }
        c.fir_taps = atoi(a[1]);
        const int bank = atoi(a[5]);
        if (c.fir_taps) {
            if (bank >= 0) c.fir_coef_word = chains[bank].fir_coef_word; else { c.fir_coef_word = w; w += c.fir_taps; }
            c.fir_state_word = w; w += c.fir_taps;
        }
        c.finish = atoi(a[2]); c.delay_slot = atoi(a[3]); c.sat = atoi(a[4]);
        if (c.delay_slot) { c.delay_word = w; c.delay_max = 100; c.delay_us_word = 8; w += 102; }
        if (grouped && c.fir_taps && !c.finish && !c.delay_slot) members.push_back(i);
        chains[i] = c;
    }
    std::vector<int> start{0, (int)members.size()};
    avdsp_plan_desc d;
    memset(&d, 0, sizeof d);
    d.format = format; d.nchains = n; d.chains = chains.data();
    d.nsections = (int)coef.size(); d.sec_coef_word = coef.data(); d.sec_state_word = state.data();
    d.fir_tail = fir_tail;
    if (grouped) { d.fir_ngroups = 1; d.fir_group_start = start.data(); d.fir_group_chains = members.data(); }
    ChainTables t;
    std::string e = check_heads(&d, w, t);
    if (e.empty()) e = check_chains(&d, w, t);
    if (!e.empty()) { std::cout << "{\"error\": \"" << e << "\"}\n"; return 0; }
    const CascadeLayout L = cascade_groups(format, t);
    const SharedLayout S = shared_fir_layout(&d, t);
    if (!S.err.empty()) { std::cout << "{\"error\": \"" << S.err << "\"}\n"; return 0; }
    std::cout << "{";
    ints("fir", t.fir); ints("fir_hand", t.fir_hand); ints("fir_plain", t.fir_plain); ints("tail", t.tail); ints("pass", t.pass); ints("pass_dressed", t.pass_dressed);
    ints("shared_ids", S.ids); ints("shared_rest", S.rest);
    std::vector<int> merged;
    for (const RowRec &r : L.all_rows) merged.push_back(r.cid);
    ints("merged_rows", merged);
    std::cout << "\"n_dressed\": " << t.n_dressed << ", \"max_taps\": " << t.max_taps << ", \"overlap_ok\": " << overlap_ok(t) << ", \"dev_chains\": " << L.dev_chains.size() << ", \"groups\": [";
    for (size_t i = 0; i < L.groups.size(); i++) { if (i) std::cout << ", "; group_json(L.groups[i]); }
    std::cout << "]}\n";
    return 0;
}

/* Stand-alone driver of tests/test_muxtail_lowering.py: what avdsp_amd/csrc/avdsp_plan_layout.h makes of dressed and delayed chains in a
 * plan with LOAD_MUX chains ("mux_tail") -- mux_records' columns and the chains the stage stores, finishes or hands over,
 * check_chains' lists and hand-over rows, cascade_groups' launch groups, mux_tiles, and whether the stage takes its TAIL forms.  No HIP.
 *
 *   muxtail_layout_driver format mux_tail fir_tail tpdf_calc  nchains x (head nsec taps finish delay_slot sat)
 *       head 0: LOAD, 1: LOAD_GAIN, 2: LOAD_MUX on the list all such chains share (3 entries; 16 of them or more are offered as one mix
 *       group), 3: LOAD_MUX on a list of its own (2 entries).  Chains get their words in order (a list its pairs and a result word, a
 *       section 12 words, a FIR taps and history, a delay line 1 + 100 words).  Prints one JSON object, or {"error": text}.
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

int main(int argc, char **argv)
{
    if (argc < 6 || (argc - 5) % 6) return 2;
    const int format = atoi(argv[1]), n = (argc - 5) / 6;
    std::vector<avdsp_chain> chains(n);
    std::vector<int> coef, state, members, mirror(16, 0);
    auto word = [&](int v) { mirror.push_back(v); return (int)mirror.size() - 1; };
    for (int i = 0; i < n; i++) {
        char **a = argv + 5 + 6 * i;
        avdsp_chain c;
        memset(&c, 0, sizeof c);
        const int head = atoi(a[0]);
        c.in_io = 1000 + i; c.n_out = 1; c.out_io[0] = i;
        c.load_mode = head == 1 ? AVDSP_LOAD_GAIN : head >= 2 ? AVDSP_LOAD_MUX : AVDSP_LOAD_PLAIN;
        if (head >= 2) {
            c.mux_count = head == 2 ? 3 : 2;
            c.mux_word = (int)mirror.size();
            for (int k = 0; k < c.mux_count; k++) { word(head == 2 ? 1000 + k : 1010 + i + k); word(0x3F000000); }
            if (mirror.size() & 1) word(0);
            c.mux_result_word = word(0); word(0);
            c.in_io = head == 2 ? 1000 : 1010 + i;
            if (head == 2) members.push_back(i);
        }
        c.nsec = atoi(a[1]); c.sec_base = (int)coef.size();
        for (int q = 0; q < c.nsec; q++) { coef.push_back((int)mirror.size()); state.push_back((int)mirror.size() + 6); mirror.resize(mirror.size() + 12, 0); }
        c.fir_taps = atoi(a[2]);
        if (c.fir_taps) { c.fir_coef_word = (int)mirror.size(); c.fir_state_word = c.fir_coef_word + c.fir_taps; mirror.resize(mirror.size() + 2 * (size_t)c.fir_taps, 0); }
        c.finish = atoi(a[3]); c.delay_slot = atoi(a[4]); c.sat = atoi(a[5]);
        if (c.delay_slot) { c.delay_word = (int)mirror.size(); c.delay_max = 100; c.delay_us_word = 8; mirror.resize(mirror.size() + 102, 0); }
        chains[i] = c;
    }
    const bool grouped = (int)members.size() >= AVDSP_MUX_GROUP_MIN;
    std::vector<int> start{0, (int)members.size()};
    avdsp_plan_desc d;
    memset(&d, 0, sizeof d);
    d.format = format; d.nchains = n; d.chains = chains.data();
    d.nsections = (int)coef.size(); d.sec_coef_word = coef.data(); d.sec_state_word = state.data();
    d.mux_tail = atoi(argv[2]); d.fir_tail = atoi(argv[3]); d.tpdf_calc = atoi(argv[4]); d.tpdf_calc_result_word = 10;
    if (grouped) { d.mux_ngroups = 1; d.mux_group_start = start.data(); d.mux_group_chains = members.data(); }
    const long long w = (long long)mirror.size();
    ChainTables t;
    std::string e = check_heads(&d, w, t);
    if (e.empty() && t.has_mux) e = mux_records(std::vector<int>(mirror.begin() + t.mux_lo, mirror.begin() + t.mux_hi), t);
    if (e.empty()) e = check_chains(&d, w, t);
    if (!e.empty()) { std::cout << "{\"error\": \"" << e << "\"}\n"; return 0; }
    const CascadeLayout L = cascade_groups(format, t);
    const MuxLayout M = t.has_mux ? mux_tiles(&d, t) : MuxLayout{};
    if (!M.err.empty()) { std::cout << "{\"error\": \"" << M.err << "\"}\n"; return 0; }
    std::vector<int> col, count, load_mode, in_io, stored(t.mux_stored.begin(), t.mux_stored.end()), handed(t.mux_handed.begin(), t.mux_handed.end());
    for (const MuxRec &r : t.mux_recs) { col.push_back(r.col); count.push_back(r.count); }
    for (const avdsp_chain &c : t.chains) { load_mode.push_back(c.load_mode); in_io.push_back(c.in_io); }
    std::cout << "{";
    ints("col", col); ints("count", count); ints("load_mode", load_mode); ints("in_io", in_io); ints("mux_stored", stored); ints("mux_handed", handed);
    ints("hand_row", t.hand_row); ints("tail", t.tail); ints("pass", t.pass); ints("pass_dressed", t.pass_dressed); ints("fir_hand", t.fir_hand);
    ints("tile_ids", M.tile_ids); ints("plain", M.plain);
    std::cout << "\"groups\": [";
    for (size_t i = 0; i < L.groups.size(); i++) {
        const GroupLayout &g = L.groups[i];
        std::cout << (i ? ", " : "") << "{\"nsec\": " << g.nsec << ", \"wide\": " << g.wide << ", \"hand\": " << g.hand << ", ";
        ints("ids", g.ids, true);
        std::cout << "}";
    }
    std::cout << "], \"n_mux_stored\": " << t.n_mux_stored << ", \"n_mux_finished\": " << t.n_mux_finished << ", \"n_mux_handed\": " << t.n_mux_handed
              << ", \"n_hand_rows\": " << t.n_hand_rows << ", \"n_dressed\": " << t.n_dressed << ", \"tail_forms\": " << t.mux_tail_forms()
              << ", \"ntiles\": " << M.tiles.size() << ", \"overlap_ok\": " << overlap_ok(t) << "}\n";
    return 0;
}

/* Stand-alone driver of tests/test_plan_layout.py: avdsp_amd/csrc/avdsp_plan_layout.h alone, no HIP, built with
 * -fsanitize=address,undefined.
 *
 *   plan_layout_driver layout FILE     the stages of plan building in avdsp_hip_prog_add_plan's order over the plan description in
 *                                      FILE, the layout as one JSON object on stdout -- or {"error": text} and nothing else
 *   plan_layout_driver choice impl n frames fir_rows fir_split fir_lean cascades plan_taps
 *   plan_layout_driver hand impl n frames fir_rows cascades plan_taps        fir_hand_choice: the launch of a plan's handed FIR chains
 *   plan_layout_driver shared format ntiles frames fir_rows
 *   plan_layout_driver ring max_taps
 *
 * FILE, integers separated by white space:
 *   format total_words instances nsections nchains nfirgroups nmuxgroups nmirror
 *   nsections x (coef_word state_word)
 *   nchains x (in_io load_mode gain_bits nsec sec_base fir_taps fir_coef_word fir_state_word sat n_out out_io[4] mux_word mux_count mux_result_word)
 *   nfirgroups x (n, n chain ids), nmuxgroups x (n, n chain ids)
 *   nmirror x (word index, value): the mirror's words that are not 0 (the LOAD_MUX lists)
 *   optionally: ndressed, ndressed x (chain id, finish): the chains with a dressed finish (AVDSP_FINISH_*)
 */
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

template <typename T, typename F>
static void arr(const char *name, const std::vector<T> &v, F one, bool last = false)
{
    std::cout << '"' << name << "\": [";
    for (size_t i = 0; i < v.size(); i++) { if (i) std::cout << ", "; one(v[i]); }
    std::cout << (last ? "]" : "], ");
}
static void ints(const char *name, const std::vector<int> &v, bool last = false) { arr(name, v, [](int x) { std::cout << x; }, last); }

static void group_json(const GroupLayout &g)
{
    std::cout << "{\"P\": " << g.P << ", \"nsec\": " << g.nsec << ", \"n\": " << g.n << ", \"all_fir\": " << g.all_fir << ", \"raw_out\": " << g.raw_out << ", \"wide\": " << g.wide << ", ";
    ints("ids", g.ids);
    arr("rows", g.rows, [](const RowRec &r) { std::cout << '[' << r.cid << ", " << r.in_io << ", " << r.out_io << ", " << r.flags << ", " << r.gain_bits << ", " << r.pad[0] << ']'; });
    arr("lanes", g.lanes, [](const LaneRec &l) { std::cout << '[' << l.coef_word << ", " << l.state_word << ']'; });
    arr("pieces", g.pieces, group_json, true);
    std::cout << '}';
}

static int fail(const std::string &e)
{
    std::cout << "{\"error\": \"" << e << "\"}\n";
    return 0;
}

static int layout(const char *path)
{
    std::ifstream in(path);
    int format, total_words, instances, nsections, nchains, nfg, nmg, nmirror;
    in >> format >> total_words >> instances >> nsections >> nchains >> nfg >> nmg >> nmirror;
    std::vector<int> coef(nsections), state(nsections);
    for (int i = 0; i < nsections; i++) in >> coef[i] >> state[i];
    std::vector<avdsp_chain> chains(nchains);
    for (auto &c : chains) {
        in >> c.in_io >> c.load_mode >> c.gain_bits >> c.nsec >> c.sec_base >> c.fir_taps >> c.fir_coef_word >> c.fir_state_word >> c.sat >> c.n_out;
        for (int &o : c.out_io) in >> o;
        in >> c.mux_word >> c.mux_count >> c.mux_result_word;
    }
    std::vector<int> gstart[2] = {{0}, {0}}, gchains[2];
    for (int k = 0; k < 2; k++)
        for (int g = 0; g < (k ? nmg : nfg); g++) {
            int n; in >> n;
            for (int j = 0; j < n; j++) { int c; in >> c; gchains[k].push_back(c); }
            gstart[k].push_back((int)gchains[k].size());
        }
    std::vector<int> mirror((size_t)total_words, 0);
    for (int i = 0; i < nmirror; i++) { int w, v; in >> w >> v; mirror.at((size_t)w) = v; }
    if (!in) { std::cerr << "bad plan file\n"; return 2; }
    int ndressed = 0;
    if (in >> ndressed)
        for (int i = 0; i < ndressed; i++) {
            int c, f;
            if (!(in >> c >> f)) { std::cerr << "bad plan file\n"; return 2; }
            chains.at((size_t)c).finish = f;
        }

    avdsp_plan_desc d{};
    d.format = format; d.nchains = nchains; d.chains = chains.data(); d.nsections = nsections;
    d.sec_coef_word = coef.data(); d.sec_state_word = state.data(); d.store_mask = -1; d.instances = instances;
    d.fir_ngroups = nfg; d.fir_group_start = gstart[0].data(); d.fir_group_chains = gchains[0].data();
    d.mux_ngroups = nmg; d.mux_group_start = gstart[1].data(); d.mux_group_chains = gchains[1].data();

    const long long buf_words = mirror_words(&d, total_words);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    if (!e.empty()) return fail(e);
    if (t.has_mux) {
        const std::vector<int> words(mirror.begin() + t.mux_lo, mirror.begin() + t.mux_hi);      /* (what add_plan downloads) */
        if (!(e = mux_records(words, t)).empty()) return fail(e);
    }
    if (!(e = check_chains(&d, buf_words, t)).empty()) return fail(e);
    const CascadeLayout L = cascade_groups(format, t);
    const SharedLayout S = shared_fir_layout(&d, t);
    if (!S.err.empty()) return fail(S.err);
    const MuxLayout M = t.has_mux ? mux_tiles(&d, t) : MuxLayout{};
    if (!M.err.empty()) return fail(M.err);

    std::cout << "{\"has_mux\": " << t.has_mux << ", \"n_mux_stored\": " << t.n_mux_stored << ", \"max_taps\": " << t.max_taps
              << ", \"io\": [" << t.io_in_min << ", " << t.io_in_max << ", " << t.io_out_min << ", " << t.io_out_max << "], ";
    ints("fir", t.fir); ints("pass", t.pass);
    arr("dev_chains", L.dev_chains, [](const avdsp_chain &c) {
        std::cout << "{\"in_io\": " << c.in_io << ", \"load_mode\": " << c.load_mode << ", \"nsec\": " << c.nsec << ", \"sec_base\": " << c.sec_base << ", \"fir_taps\": " << c.fir_taps
                  << ", \"sat\": " << c.sat << ", \"n_out\": " << c.n_out << ", \"out_io\": " << c.out_io[0] << '}'; });
    arr("groups", L.groups, group_json);
    GroupLayout merged;
    merged.rows = L.all_rows; merged.lanes = L.all_lanes; merged.n = (int)L.all_rows.size(); merged.all_fir = L.rows_all_fir;
    std::cout << "\"merged\": "; group_json(merged); std::cout << ", ";
    std::cout << "\"shared\": {";
    ints("ids", S.ids); ints("feed", S.feed); ints("rest", S.rest); ints("reps", S.reps);
    arr("tiles", S.tiles, [](const SharedTile &x) { std::cout << '[' << x.group << ", " << x.first << ", " << x.n << ", " << x.taps << ']'; }, true);
    std::cout << "}, \"mux\": {";
    arr("recs", t.mux_recs, [](const MuxRec &r) { std::cout << '[' << r.list_word << ", " << r.count << ", " << r.result_word << ", " << r.col << ']'; });
    ints("tile_ids", M.tile_ids); ints("plain", M.plain); ints("kpads", M.kpads);
    arr("rows", M.rows, [](long long x) { std::cout << x; });
    arr("tiles", M.tiles, [](const MuxTile &x) { std::cout << '[' << x.id0 << ", " << x.nrec << ", " << x.count << ", " << x.kpad << ", " << x.list_word << ", " << x.g64 << ']'; });
    std::cout << "\"g64_len\": " << M.g64_len << "}, ";
    std::cout << "\"stores_whole_window\": " << stores_whole_window(t) << ", \"overlap_ok\": " << overlap_ok(t) << "}\n";
    return 0;
}

int main(int argc, char **argv)
{
    auto num = [&](int i) { return atoll(argv[i]); };
    if (argc == 3 && !strcmp(argv[1], "layout")) return layout(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "ring")) {
        std::cout << ring_length((int)num(2)) << ' ' << fir_groups_per_chunk((int)num(2)) << ' ' << taps64_pitch((int)num(2)) << '\n';
        return 0;
    }
    FirChoice c;
    if (argc == 10 && !strcmp(argv[1], "choice"))
        c = fir_choice((int)num(2), num(3), (int)num(4), FirOptions{(int)num(5), (int)num(6), (int)num(7)}, num(8) != 0, num(9));
    else if (argc == 8 && !strcmp(argv[1], "hand"))
        c = fir_hand_choice((int)num(2), num(3), (int)num(4), (int)num(5), num(6) != 0, num(7));
    else if (argc == 6 && !strcmp(argv[1], "shared"))
        c = fir_shared_choice((int)num(2), (int)num(3), (int)num(4), (int)num(5));
    else { std::cerr << "usage: see the head of plan_layout_driver.cpp\n"; return 2; }
    std::cout << c.family << ' ' << c.R << ' ' << c.BIG << ' ' << c.SPLIT << ' ' << c.LEAN;
    if (c.HAND) std::cout << " HAND";
    std::cout << '\n';
    return 0;
}

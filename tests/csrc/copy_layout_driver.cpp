/* tests/test_copy_layout.py: the "chain_copy" stage of avdsp_plan_layout.h (copy_list) and what check_chains, cascade_groups,
 * stores_whole_window and overlap_ok make of a plan with LOAD_STORE pairs -- built against the header alone, with AddressSanitizer and
 * UBSan, run as a program of its own.  argv[1] names a scenario; what is printed is one JSON object. */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

struct Desc {
    int fmt = 6, total = 4096, instances = 0, chain_copy = 1, next = 1000;
    std::vector<avdsp_chain> chains;
    std::vector<int> coef, state, src, dst;
    std::vector<int> mux_words;                          /* the mirror's words of the LOAD_MUX lists, from word 2000 */
    int add(int nsec, int in_io, int out_io, int mode = AVDSP_LOAD_PLAIN)
    {
        avdsp_chain c;
        memset(&c, 0, sizeof c);
        const int i = (int)chains.size();
        c.in_io = in_io; c.load_mode = mode; c.nsec = nsec; c.sec_base = (int)coef.size(); c.n_out = 1; c.out_io[0] = out_io; c.sat = 1;
        for (int k = 0; k < nsec; k++) { coef.push_back(next); state.push_back(next + 6); next += 12; }
        chains.push_back(c);
        return i;
    }
    int mux(int nsec, int out_io, std::vector<int> ios)
    {
        const int i = add(nsec, ios[0], out_io, AVDSP_LOAD_MUX);
        chains[i].mux_word = 2000 + (int)mux_words.size(); chains[i].mux_count = (int)ios.size(); chains[i].mux_result_word = 3000 + 2 * i;
        for (int io : ios) { mux_words.push_back(io); mux_words.push_back(0x3F000000); }
        return i;
    }
    void pair(int a, int b) { src.push_back(a); dst.push_back(b); }
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
    d.store_mask = -1; d.instances = D.instances; d.chain_copy = D.chain_copy;
    d.ncopy = (int)D.src.size(); d.copy_src = D.src.data(); d.copy_dst = D.dst.data();
    const long long buf_words = mirror_words(&d, D.total);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    std::vector<int> words;
    if (e.empty() && t.has_mux) words.assign(D.mux_words.begin() + (t.mux_lo - 2000), D.mux_words.begin() + (t.mux_hi - 2000));
    if (e.empty()) e = copy_list(&d, words, t);
    if (e.empty() && t.has_mux) e = mux_records(words, t);
    if (e.empty()) e = check_chains(&d, buf_words, t);
    if (!e.empty()) { printf("{\"error\": \"%s\"}\n", e.c_str()); return 0; }
    const CascadeLayout L = cascade_groups(d.format, t);
    const AheadColumns A = ahead_columns(t);
    printf("{\"whole\": %d, \"overlap_ok\": %d, \"all_rows\": %d, \"dev_chains\": %d, ", stores_whole_window(t) ? 1 : 0, overlap_ok(t) ? 1 : 0,
           (int)L.all_rows.size(), (int)L.dev_chains.size());
    std::vector<int> s, ds, groups;
    for (const CopyPair &p : t.copy) { s.push_back(p.src); ds.push_back(p.dst); }
    for (const GroupLayout &g : L.groups) { groups.push_back(g.nsec); groups.push_back(g.n); groups.push_back(g.P); }
    ints("src", s); ints("dst", ds); ints("groups", groups); ints("pass", t.pass); ints("tail", t.tail); ints("ahead", A.cols);
    ints("io_in", {t.io_in_min, t.io_in_max}); ints("io_out", {t.io_out_min, t.io_out_max}, true);
    printf("}\n");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    Desc D;
    /* three chains: IO 64 -> 0 (2 sections), 65 -> 1 (2 sections), 66 -> 2 (none) */
    auto three = [&]() { D.add(2, 64, 0); D.add(2, 65, 1); D.add(0, 66, 2); };
    if (s == "sort") {                                   /* pairs out of order, sources shared with each other and with a chain's input */
        three();
        D.pair(70, 9); D.pair(64, 5); D.pair(70, 3); D.pair(71, 12); D.pair(90, 4);
    } else if (s == "alone") {                           /* no chain at all */
        D.pair(8, 3); D.pair(9, 1); D.pair(8, 2);
    } else if (s == "plain" || s == "plain_off") {       /* no pairs: the flag changes nothing */
        three();
        D.chain_copy = s == "plain";
    } else if (s == "whole") {                           /* chains store 0, 1, 2; pairs fill 3 and 4: the window [0, 4] is whole */
        three();
        D.pair(70, 4); D.pair(71, 3);
    } else if (s == "hole") {                            /* ... a pair at 5 leaves 3 and 4 untouched */
        three();
        D.pair(70, 5);
    } else if (s == "whole_chains") {                    /* no pairs: whole as ever */
        three();
    } else if (s == "mux_ok") {                          /* a destination beside a LOAD_MUX list's IOs */
        D.mux(1, 0, {64, 65, 66}); D.add(1, 67, 1);
        D.pair(64, 9); D.pair(80, 8);
    } else if (s == "flag_off") {
        three(); D.pair(70, 9); D.chain_copy = 0;
    } else if (s == "instances") {
        three(); D.pair(70, 9); D.instances = 2;
    } else if (s == "src_high") {
        three(); D.pair(65536, 9);
    } else if (s == "src_negative") {
        three(); D.pair(-1, 9);
    } else if (s == "dst_high") {
        three(); D.pair(70, 65536);
    } else if (s == "dst_negative") {
        three(); D.pair(70, -3);
    } else if (s == "dst_twice") {
        three(); D.pair(70, 9); D.pair(71, 9);
    } else if (s == "dst_loaded") {
        three(); D.pair(70, 65);
    } else if (s == "dst_stored") {
        three(); D.pair(70, 1);
    } else if (s == "dst_mux_entry") {
        D.mux(1, 0, {64, 65, 66}); D.add(1, 67, 1);
        D.pair(80, 66);
    } else if (s == "src_stored") {
        three(); D.pair(2, 9);
    } else if (s == "src_is_dst") {
        three(); D.pair(70, 9); D.pair(9, 10);
    } else if (s == "storeless_delay" || s == "storeless_off" || s == "storeless_plain") {
        /* chain 1 keeps no STORE (a later chain stores its IOs again): legal with the flag where chain_tail finishes the chain */
        three();
        D.chains[1].n_out = 0; D.chains[1].out_io[0] = 0;
        if (s != "storeless_plain") { D.chains[1].delay_slot = AVDSP_DELAY_A; D.chains[1].delay_word = 3000; D.chains[1].delay_max = 30; D.chains[1].delay_us_word = 20; }
        D.chain_copy = s != "storeless_off";
    } else if (s == "null_list") {
        three(); D.pair(70, 9);
        avdsp_plan_desc d;
        memset(&d, 0, sizeof d);
        d.format = 6; d.nchains = 0; d.chain_copy = 1; d.ncopy = 1;
        ChainTables t;
        std::string e = check_heads(&d, 4096, t);
        if (e.empty()) e = copy_list(&d, {}, t);
        printf("{\"error\": \"%s\"}\n", e.c_str());
        return 0;
    } else {
        fprintf(stderr, "unknown scenario %s\n", s.c_str());
        return 2;
    }
    return run(D);
}

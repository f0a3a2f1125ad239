/* tests/test_shard_trees_layout.py: a core of memory-word trees cut at tree boundaries ("shard_trees"), without a GPU.  For
 * a scenario (argv[1]) -- the shapes of tests/shard_tree_programs.py as chain descriptors -- and every world of 2, 3 and 8 the driver cuts
 * the core with avdsp_shard_cut.h as the host does, lays out the plan of every rank's slice with avdsp_plan_layout.h (the slice in its
 * own numbering: chains + lo, the section tables from the slice's first section on) and checks every row, column, tree, chain and word
 * index the kernels would follow against what the plan allocates, and that no branch of a slice became a branch of a constant word
 * while its trunk exists in the core.  Built with AddressSanitizer and UBSan, run as a program of its own; prints one JSON object. */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "avdsp_plan_layout.h"
#include "avdsp_shard_cut.h"

using namespace avdsp_layout;

struct Core {
    int fmt = 6, total = 1 << 16, next = 1000;
    std::vector<avdsp_chain> chains;
    std::vector<int> coef, state;
    int add(int nsec, int mode = AVDSP_LOAD_GAIN)
    {
        avdsp_chain c;
        memset(&c, 0, sizeof c);
        const int i = (int)chains.size();
        c.in_io = 512 + i; c.load_mode = mode; c.nsec = nsec; c.sec_base = (int)coef.size(); c.n_out = 1; c.out_io[0] = i; c.sat = 1;
        for (int k = 0; k < nsec; k++) { coef.push_back(next); state.push_back(next + 6); next += 12; }
        chains.push_back(c);
        return i;
    }
    int trunk(int word, int nsec) { const int i = add(nsec); chains[i].n_out = 0; chains[i].sat = 0; chains[i].mem_word = word; chains[i].mem_store = 1; return i; }
    int branch(int word, int nsec) { const int i = add(nsec, AVDSP_LOAD_MEM); chains[i].in_io = 0; chains[i].mem_word = word; return i; }
    int fir(int i, int taps) { chains[i].fir_taps = taps; chains[i].fir_coef_word = 20000 + 64 * i; chains[i].fir_state_word = 40000 + 64 * i; return i; }
    int way(int i) { chains[i].delay_slot = AVDSP_DELAY_A; chains[i].delay_word = 50000 + 64 * i; chains[i].delay_max = 48; chains[i].finish = AVDSP_FINISH_TPDF_GAIN; return i; }
};

static void trees_of_1_3(Core &C, int trees, int late)
{
    int held = -1;
    for (int t = 0; t < trees; t++) {
        C.trunk(100 + 2 * t, t % 3 == 0 ? 2 : t % 3 == 1 ? 0 : 1);
        if (held >= 0) { C.branch(held, 2); held = -1; }
        for (int j = 0; j < 3; j++) { if (t == late && j == 2) held = 100 + 2 * t; else C.branch(100 + 2 * t, j); }
    }
}

static void of_length(Core &C, int n)
{
    int t = 0;
    while ((int)C.chains.size() + 4 <= n - 1) {
        if (t == 2) C.branch(90, 0);
        C.trunk(100 + 2 * t, t % 3);
        for (int j = 0; j < 3; j++) C.branch(100 + 2 * t, (t + j) % 3);
        t++;
    }
    while ((int)C.chains.size() < n) C.add(1 + (int)C.chains.size() % 3);
}

static bool build(Core &C, const std::string &s)
{
    if (s == "crossover") {
        for (int t = 0; t < 5; t++) {
            if (t) { C.add(1 + (2 * t) % 3); C.add(1 + (2 * t + 1) % 3); }
            C.trunk(100 + 2 * t, 2);
            for (int j = 0; j < 3; j++) C.way(C.branch(100 + 2 * t, 2));
        }
    } else if (s == "late_branch") trees_of_1_3(C, 5, 1);
    else if (s == "late17") trees_of_1_3(C, 17, 5);
    else if (s == "interleaved") {
        C.trunk(100, 2); C.trunk(102, 1);
        for (int j = 0; j < 3; j++) { C.branch(100, j % 2); C.branch(102, 1 + j % 2); }
    } else if (s == "constant_alone") C.branch(90, 1);
    else if (s == "chains17") of_length(C, 17);
    else if (s == "chains37") of_length(C, 37);
    else if (s == "mem_fir") {
        for (int t = 0; t < 4; t++) { C.fir(C.trunk(100 + 2 * t, 2), 37); C.branch(100 + 2 * t, 1); C.branch(100 + 2 * t, 2); }
        for (int t = 0; t < 3; t++) { C.trunk(120 + 2 * t, 1); for (int j = 0; j < 3; j++) C.fir(C.branch(120 + 2 * t, 0), 20); }
    } else return false;
    return true;
}

/* the layout of chains [lo, hi) as the host hands them over; returns the number of bad indices, -1: the layout refused the slice */
static int slice_layout(const Core &C, int lo, int hi, int *misclassified, int *constant, std::string *err)
{
    std::vector<avdsp_chain> ch(C.chains.begin() + lo, C.chains.begin() + hi);
    const int sec0 = C.chains[lo].sec_base, sec1 = hi < (int)C.chains.size() ? C.chains[hi].sec_base : (int)C.coef.size();
    for (avdsp_chain &c : ch) c.sec_base -= sec0;
    avdsp_plan_desc d;
    memset(&d, 0, sizeof d);
    d.format = C.fmt; d.nchains = hi - lo; d.chains = ch.data();
    d.nsections = sec1 - sec0; d.sec_coef_word = C.coef.data() + sec0; d.sec_state_word = C.state.data() + sec0;
    d.store_mask = -1; d.chain_mem = 1; d.mem_fir = 1; d.fir_tail = 1; d.delay_line_factor = 206158430u;       /* 48 kHz */
    const long long buf_words = mirror_words(&d, C.total);
    ChainTables t;
    std::string e = check_heads(&d, buf_words, t);
    if (e.empty() && t.has_mem) e = mem_trees(&d, buf_words, t);
    if (e.empty()) e = check_chains(&d, buf_words, t);
    if (e.empty()) e = shared_fir_layout(&d, t).err;
    if (!e.empty()) { *err = e; return -1; }
    const CascadeLayout L = cascade_groups(d.format, t);
    const int n = d.nchains, ntree = (int)t.mem_tree_list.size();
    int bad = 0;
    for (int k = 0; k < ntree; k++) {
        const MemTree &m = t.mem_tree_list[k];
        bad += m.word < 1 || m.word + 2 > buf_words || m.trunk >= n || m.row >= t.n_hand_rows || m.col0 < 0 || m.ncol < 0 || m.col0 + m.ncol > t.n_mem_cols;
        bad += m.first_own < 0 || m.n_own < 0 || m.first_own + m.n_own > (int)t.mem_own.size();
        bad += m.src == kMemSrcRow && (m.trunk < 0 || m.row < 0);
        bad += m.src != kMemSrcWord && (m.trunk < 0 || !t.chains[m.trunk].mem_store || t.chains[m.trunk].mem_word != m.word);
        if (m.src == kMemSrcWord) {
            (*constant)++;
            for (const avdsp_chain &c : C.chains) *misclassified += c.mem_store && c.mem_word == m.word;
        }
    }
    for (const MemOwn &o : t.mem_own) bad += o.tree < 0 || o.tree >= ntree || o.cid < 0 || o.cid >= n || o.n_out < 0 || o.n_out > AVDSP_MAX_STORES;
    for (int c : t.mem_col_tree) bad += c < 0 || c >= ntree;
    bad += (int)t.mem_col_tree.size() != t.n_mem_cols;
    int trees_seen = 0, cols_seen = 0;
    for (const MemTile &m : t.mem_tiles) {
        bad += m.tree0 != trees_seen || m.ntree < 1 || m.ntree > kMemTileTrees || m.col0 != cols_seen || m.ncol < 0;
        trees_seen += m.ntree; cols_seen += m.ncol;
    }
    bad += trees_seen != ntree || cols_seen != t.n_mem_cols;
    for (const MemFeed &f : t.mem_feed) bad += f.tree < 0 || f.tree >= ntree || f.cid < 0 || f.cid >= n || !t.chains[f.cid].fir_taps;
    if (!t.mem_feed.empty()) bad += (int)t.mem_feed_start.size() != ntree + 1 || t.mem_feed_start.front() != 0 || t.mem_feed_start.back() != (int)t.mem_feed.size();
    for (int r : t.hand_row) bad += r >= t.n_hand_rows;
    for (int r : t.mem_row) bad += r >= t.n_hand_rows;
    for (int i = 0; i < n; i++) {
        const avdsp_chain &c = t.chains[i];
        bad += c.sec_base < 0 || c.sec_base + c.nsec > d.nsections;
        if (t.mem_kind[i] == 2 && c.nsec) bad += c.load_mode != kLoadRaw || c.in_io < 0 || c.in_io >= t.n_mem_cols;
        if (c.fir_taps) bad += c.fir_coef_word < 0 || c.fir_coef_word + c.fir_taps > buf_words || c.fir_state_word < 0 || c.fir_state_word + c.fir_taps > buf_words;
    }
    for (int i : t.fir) bad += i < 0 || i >= n;
    for (int i : t.fir_trunk) bad += i < 0 || i >= n || t.mem_kind[i] != 1;
    for (int i : t.tail) bad += i < 0 || i >= n;
    for (const GroupLayout &g : L.groups) for (int id : g.ids) bad += id < 0 || id >= (int)L.dev_chains.size();
    for (int s : t.coef) bad += s < 0 || s + 5 > buf_words;
    for (int s : t.state) bad += s < 0 || s + 6 > buf_words;
    return bad;
}

int main(int argc, char **argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    Core C;
    if (!build(C, s)) { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const int n = (int)C.chains.size();
    /* the tree of every chain, as avdsp_host.c's tree_of_chains() */
    std::vector<int> tree_of(n);
    for (int i = 0; i < n; i++) {
        tree_of[i] = i;
        if (!C.chains[i].mem_word || C.chains[i].mem_store) continue;
        for (int j = 0; j < n; j++) if (C.chains[j].mem_store && C.chains[j].mem_word == C.chains[i].mem_word) { tree_of[i] = j; break; }
    }
    printf("{\"chains\": %d, \"tree_of\": [", n);
    for (int i = 0; i < n; i++) printf("%s%d", i ? ", " : "", tree_of[i]);
    printf("], \"worlds\": {");
    const int worlds[3] = {2, 3, 8};
    int bad = 0, misclassified = 0, slices = 0, refused = 0;
    std::string err;
    for (int wi = 0; wi < 3; wi++) {
        const int world = worlds[wi];
        std::vector<int> bounds(world + 1), scratch(2 * n + 1);
        avdsp_tree_shard_bounds(tree_of.data(), n, world, bounds.data(), scratch.data());
        printf("%s\"%d\": {\"bounds\": [", wi ? ", " : "", world);
        for (int k = 0; k <= world; k++) printf("%s%d", k ? ", " : "", bounds[k]);
        printf("], \"constant\": [");
        for (int k = 0; k < world; k++) {
            int constant = 0;
            if (bounds[k + 1] > bounds[k]) {
                const int b = slice_layout(C, bounds[k], bounds[k + 1], &misclassified, &constant, &err);
                if (b < 0) refused++; else bad += b;
                slices++;
            }
            printf("%s%d", k ? ", " : "", constant);
        }
        printf("]}");
    }
    printf("}, \"slices\": %d, \"refused\": %d, \"error\": \"%s\", \"bad_indices\": %d, \"misclassified\": %d}\n", slices, refused, err.c_str(), bad, misclassified);
    return 0;
}

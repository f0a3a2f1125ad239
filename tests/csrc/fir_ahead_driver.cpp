/* The "fir_ahead" rules of avdsp_plan_layout.h without a GPU (tests/test_gpu_fir_ahead.py):
 *     fir_ahead_driver rule CHAINS TAPS FRAMES      -> fir_ahead_by_plan: 1 the launch is staged when the option leaves it to the plan
 *     fir_ahead_driver stage OUT_STRIDE             -> ahead_stage_words: words of a staging block, 0 over the cap
 *     fir_ahead_driver cols N_OUT IO ... [N_OUT IO ...]   -> ahead_columns of plain FIR chains with these stores: "run|list: io io ..." */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

int main(int argc, char **argv)
{
    if (argc >= 5 && !strcmp(argv[1], "rule")) {
        printf("%d\n", fir_ahead_by_plan(atoll(argv[2]), atoi(argv[3]), atoi(argv[4])) ? 1 : 0);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "stage")) {
        printf("%lld\n", ahead_stage_words(atoi(argv[2])));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "cols")) {
        ChainTables t;
        for (int k = 2; k < argc;) {
            avdsp_chain c{};
            c.fir_taps = 16;
            c.n_out = atoi(argv[k++]);
            if (c.n_out < 0 || c.n_out > AVDSP_MAX_STORES || k + c.n_out > argc) return 2;
            for (int j = 0; j < c.n_out; j++) c.out_io[j] = atoi(argv[k++]);
            t.fir.push_back((int)t.chains.size());
            t.chains.push_back(c);
        }
        const AheadColumns A = ahead_columns(t);
        printf("%s:", A.run ? "run" : "list");
        for (int io : A.cols) printf(" %d", io);
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: fir_ahead_driver rule CHAINS TAPS FRAMES | stage OUT_STRIDE | cols N_OUT IO ...\n");
    return 2;
}

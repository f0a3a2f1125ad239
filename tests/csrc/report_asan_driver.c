/* report_asan_driver PROGRAM.bin ... -- the host's core reports and option calls under AddressSanitizer and UBSan, stand-alone (no HIP
 * device is touched).  Every program is loaded once per DSP_FORMAT into a heap buffer of exactly its size; every core then goes through
 * the ten dspRuntime...Info calls and dspRuntimeStrandInfo with the lowering options off, on and mixed, unsharded and as shard 1 of 3,
 * and a handful of option keys of every kind are read and set.  What counts is the sanitizer's silence: a refusal path that frees twice,
 * or a report that reads past the chains it was given, ends the run.  Built and run by tests/test_lowering_report.py. */
#include "avdsp_runtime.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
    static const char *lowerings[6] = { "chain_finish", "chain_delay", "fir_tail", "mux_tail", "chain_mem", "chain_copy" };
    static const char *keys[] = { "fir_impl", "device", "generic", "overlap", "fir_launch", "fir_lean", "ring_wait", "group_fanout", "profile",
                                  "ready_timeouts", "ready_test", "rate_count_static", "timing_pairs_3", "timing_pairs_9", "shard_rank",
                                  "fir_ahead_now", "levels", "profile_stride", "frame_server_idle_us", "no_such_option", "" };
    int reports = 0;
    for (int f = 1; f < argc; f++) {
        FILE *fp = fopen(argv[f], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
        fseek(fp, 0, SEEK_END);
        const long n = ftell(fp) / 4;
        fseek(fp, 0, SEEK_SET);
        unsigned *words = (unsigned *)malloc((size_t)n * 4);
        if (n < 12 || !words || fread(words, 4, (size_t)n, fp) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[f]); return 2; }
        fclose(fp);
        const long size = (long)words[1] + ((int)words[2] > 0 ? (int)words[2] : 0);
        for (int fmt = 2; fmt <= 6; fmt++) {
            opcode_t *buf = (opcode_t *)calloc((size_t)(size > n ? size : n), 4);
            memcpy(buf, words, (size_t)n * 4);
            const int rc = dspRuntimeInit(buf, (int)size, 48000, 1, 24);
            for (int set = 0; set < 3 && rc >= 0; set++) {
                for (int k = 0; k < 6; k++) dspRuntimeSetOption(lowerings[k], set == 1 || (set == 2 && k % 2));
                dspRuntimeSetShard(set == 2, set == 2 ? 3 : 1);
                for (int c = 1; c < 65; c++) {
                    opcode_t *p = dspFindCore(buf, c);
                    if (!p || (c > 1 && p == buf)) break;          /* (no DSP_CORE word: every number finds the program itself) */
                    int o[7];
                    dspRuntimeCoreInfo(fmt, p, o, o + 1, o + 2);
                    dspRuntimeFirGroupInfo(fmt, p, o, o + 1, o + 2);
                    dspRuntimeMuxInfo(fmt, p, o, o + 1, o + 2, o + 3);
                    dspRuntimeFinishInfo(fmt, p, o, o + 1);
                    dspRuntimeDelayInfo(fmt, p, o, o + 1);
                    dspRuntimeFirTailInfo(fmt, p, o, o + 1);
                    dspRuntimeMuxTailInfo(fmt, p, o, o + 1, o + 2);
                    dspRuntimeMemInfo(fmt, p, o, o + 1, o + 2);
                    dspRuntimeCopyInfo(fmt, p, o, 0);              /* (an output nobody wants) */
                    dspRuntimeShardInfo(fmt, p, o, o + 1, o + 2, o + 3, o + 4, o + 5, o + 6);
                    dspRuntimeStrandInfo(fmt, p, o, o + 1, o + 2);
                    reports += 11;
                }
            }
            for (unsigned k = 0; k < sizeof keys / sizeof keys[0]; k++) {
                dspRuntimeGetOption(keys[k]);
                dspRuntimeSetOption(keys[k], 1);
                dspRuntimeSetOption(keys[k], 0);
                dspRuntimeGetOption(keys[k]);
            }
            dspRuntimeSetShard(0, 1);
            dspRuntimeRelease();
            free(buf);
        }
        free(words);
    }
    printf("ok %d reports\n", reports);
    return 0;
}

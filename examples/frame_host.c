/*
 * frame_host.c -- a host in the shape of the reference's own (linux/avdsp_plugin.c:95-141, linux/dsprun.c): a samples[] array, and per
 * frame one dspRuntime_N(core, rundata, samples) call per core found by dspFindCore.  No extension calls: with AVDSP_FRAME_SERVER=1 in
 * its environment the library serves these calls from a resident wave (include/avdsp_runtime.h, "frame_server").
 *
 *   gcc -Iinclude -DDSP_FORMAT=2 examples/frame_host.c -Lavdsp_amd/lib -lavdsp_mi355x -Wl,-rpath,$PWD/avdsp_amd/lib -o frame_host
 *   ./frame_host prog.bin 48000 in.raw nbchin in_io_base out.raw nbchout out_io_base
 *
 * Prints the microseconds per core call (wall clock over the whole loop).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "compat/dsp_runtime.h"          /* DSP_RUNTIME_FORMAT(), dspSample_t (dsp_runtime.h:24-131) */

#define OPCODES_MAX 20000
#define CORES_MAX 8
#define SAMPLES_MAX 64

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: frame_host prog.bin fs in.raw nbchin in_io_base out.raw nbchout out_io_base\n"); return 2; }
    const int fs = atoi(argv[2]), nbchin = atoi(argv[4]), in_base = atoi(argv[5]);
    const int nbchout = atoi(argv[7]), out_base = atoi(argv[8]);
    if (in_base < 0 || out_base < 0 || nbchin < 1 || nbchout < 1 || in_base + nbchin > SAMPLES_MAX || out_base + nbchout > SAMPLES_MAX) {
        fprintf(stderr, "the windows must lie inside samples[%d]\n", SAMPLES_MAX); return 2;
    }

    static opcode_t opcodes[OPCODES_MAX];
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    (void)fread(opcodes, 4, OPCODES_MAX, f);
    fclose(f);

    int result = dspRuntimeInit(opcodes, OPCODES_MAX, fs, 12345, 24);          /* avdsp_plugin.c:316 */
    if (result < 0) { fprintf(stderr, "dspRuntimeInit: %d (%s)\n", result, dspRuntimeLastError()); return 1; }
    int *dataPtr = (int *)opcodes + result;                                   /* avdsp_plugin.c:322 */

    opcode_t *codestart[CORES_MAX];
    int nbcores = 0;
    for (; nbcores < CORES_MAX; nbcores++) {
        opcode_t *core = dspFindCore(opcodes, nbcores + 1);
        if (!core) break;
        codestart[nbcores] = dspFindCoreBegin(core);
    }

    f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 1; }
    fseek(f, 0, SEEK_END);
    long frames = ftell(f) / (4L * nbchin);
    fseek(f, 0, SEEK_SET);
    dspSample_t *src = (dspSample_t *)malloc((size_t)frames * nbchin * 4), *dst = (dspSample_t *)calloc((size_t)frames * nbchout, 4);
    if (fread(src, 4, (size_t)frames * nbchin, f) != (size_t)frames * nbchin) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    static dspSample_t samples[SAMPLES_MAX];                                  /* avdsp_plugin.c:93 inputOutput[] */
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long n = 0; n < frames; n++) {
        memset(samples + out_base, 0, (size_t)nbchout * sizeof samples[0]);
        memcpy(samples + in_base, src + n * nbchin, (size_t)nbchin * sizeof samples[0]);
        for (int nc = 0; nc < nbcores; nc++) {
            int rc = DSP_RUNTIME_FORMAT(dspRuntime)(codestart[nc], dataPtr, samples);
            if (rc < 0) { fprintf(stderr, "frame %ld core %d: %d (%s)\n", n, nc + 1, rc, dspRuntimeLastError()); return 1; }
        }
        memcpy(dst + n * nbchout, samples + out_base, (size_t)nbchout * sizeof samples[0]);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double us = ((double)(t1.tv_sec - t0.tv_sec) * 1e6 + (double)(t1.tv_nsec - t0.tv_nsec) / 1e3) / ((double)frames * (nbcores ? nbcores : 1));
    if (dspRuntimeSyncState(dataPtr) < 0) { fprintf(stderr, "sync: %s\n", dspRuntimeLastError()); return 1; }

    f = fopen(argv[6], "wb");
    fwrite(dst, 4, (size_t)frames * nbchout, f);
    fclose(f);
    printf("cores=%d frames=%ld us_per_call=%.2f state[0..3]=%08x %08x %08x %08x\n", nbcores, frames, us,
           (unsigned)dataPtr[0], (unsigned)dataPtr[1], (unsigned)dataPtr[2], (unsigned)dataPtr[3]);
    dspRuntimeRelease();
    return 0;
}

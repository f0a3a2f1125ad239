/* The route of a block launch (avdsp_plan_layout.h: launch_gate, launch_route) for facts given on the command line, built against that
 * header alone (tests/test_launch_route.py, tests/test_gpu_launch_route.py):
 *     launch_route_driver key=value ...
 * The keys are LaunchFacts' members and `ahead_apart`, `side_by_side` (the probes' answers); a key that is not given is 0.  One JSON
 * object on stdout: the gate's and the route's members by name. */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "avdsp_plan_layout.h"

using namespace avdsp_layout;

int main(int argc, char **argv)
{
    LaunchFacts f{};
    int ahead_apart = 0, side_by_side = 0;
    struct Key { const char *name; int *i; bool *b; };
    const Key keys[] = {
        {"overlap", &f.overlap, nullptr}, {"cu_split", &f.cu_split, nullptr}, {"fir_ahead", &f.fir_ahead, nullptr}, {"ready_words", &f.ready_words, nullptr},
        {"fir_launch", &f.fir_launch, nullptr}, {"fir_impl", &f.fir_impl, nullptr}, {"biquad_impl", &f.biquad_impl, nullptr}, {"nframes", &f.nframes, nullptr},
        {"out_stride", &f.out_stride, nullptr}, {"in_place", nullptr, &f.in_place}, {"overlap_ok", nullptr, &f.overlap_ok}, {"n_fir", &f.n_fir, nullptr},
        {"max_taps", &f.max_taps, nullptr}, {"n_ahead_cols", &f.n_ahead_cols, nullptr}, {"instances", &f.instances, nullptr}, {"n_sh_groups", &f.n_sh_groups, nullptr},
        {"has_taps64", nullptr, &f.has_taps64}, {"has_ready", nullptr, &f.has_ready}, {"inst_n", &f.inst_n, nullptr}, {"chain_inst", &f.chain_inst, nullptr},
        {"has_timeouts", nullptr, &f.has_timeouts}, {"timer_samples", nullptr, &f.timer_samples}, {"ahead_apart", &ahead_apart, nullptr}, {"side_by_side", &side_by_side, nullptr},
        {"n_fir_only", &f.n_fir_only, nullptr},
    };
    for (int a = 1; a < argc; a++) {
        const char *eq = strchr(argv[a], '=');
        const Key *hit = nullptr;
        if (eq) for (const Key &k : keys) if (strlen(k.name) == (size_t)(eq - argv[a]) && !strncmp(argv[a], k.name, eq - argv[a])) hit = &k;
        if (!hit) { fprintf(stderr, "launch_route_driver: '%s' is not key=value with a key of LaunchFacts\n", argv[a]); return 2; }
        const int v = atoi(eq + 1);
        if (hit->i) *hit->i = v; else *hit->b = v != 0;
    }
    const LaunchGate g = launch_gate(f);
    const LaunchRoute r = launch_route(f, g, ahead_apart, side_by_side);
    printf("{\"under\": %d, \"own_fir\": %d, \"ahead_candidate\": %d, \"probe_on\": %d, \"path\": %d, \"ready_mode\": %d, \"cascade_event\": %d, "
           "\"write_through\": %d, \"fir_waits_event\": %d, \"ready_acquire\": %d, \"fir_launch_mode\": %d, \"rides\": %d, \"side_by_side\": %d, \"fir_follows_fir\": %d}\n",
           g.under, g.own_fir, g.ahead_candidate, g.probe_on, r.path, r.ready_mode, r.cascade_event, r.write_through, r.fir_waits_event,
           r.ready_acquire, r.fir_launch_mode, r.rides, r.side_by_side, r.fir_follows_fir);
    return 0;
}

/*
 * avdsp_runtime.h -- C ABI of the MI355X-native AVDSP runtime (libavdsp_mi355x.so).
 *
 * Drop-in boundary: the five functions and the exported data below are exactly what the reference
 * runtime exports (module_avdsp/runtime/dsp_runtime.h:160-164, dsp_runtime.c:36-38,
 * dsp_header.c:10-86), so the reference hosts (linux/avdsp_plugin.c:126,178,316,328,336,
 * linux/dsprun.c:92,104,112,166, osx/dsprunosx.c:61,72,73,91) link against it unchanged.
 * The reference builds one library per DSP_FORMAT; this library carries the _2, _4 and _6 entry
 * points side by side (int64 / double+int samples / double+float samples).
 *
 * Everything that computes runs on the GPU (hand-written gfx950 kernels behind avdsp_hip.h).
 * There is NO CPU execution path in this library: a core that cannot be lowered to the device
 * kernels, a missing GPU, or a HIP error makes the call return a negative code and leaves a message
 * in dspRuntimeLastError().  (A CPU restatement exists under oracle/ -- test infrastructure only.)
 * Codes: -1 .. -6 the reference's (dsp_runtime.c:119-125,159-194: no header, no cores, checksum, opcode too new, buffer too
 * small; -1 / -2 from dspRuntimeReset: sample rate), -8 a core refused (no defined result / an offset outside the
 * buffer / a shape the call cannot take), -9 out of memory or table space, -10 a HIP error, -11 (sticky) a FIR wave of the overlap
 * mode gave up waiting for its cascade: the block is not valid, acknowledge with dspRuntimeReset() or
 * dspRuntimeSetOption("ready_timeouts", 0).
 *
 * Ownership is the reference's: the caller owns ONE contiguous int32 buffer holding the program
 * followed by the state ("data") area, dspRuntimeInit returns the program length so that
 * rundata = (int*)code + return value.  The device keeps a mirror of that buffer; state lives on
 * the device between blocks and is copied back by dspRuntimeSyncState() (checkpoint) or pushed by
 * dspRuntimeUploadState() (restore).
 */
#ifndef AVDSP_RUNTIME_H_
#define AVDSP_RUNTIME_H_

#include <stddef.h>

#include "avdsp_format.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- reference API (names, arguments, return codes unchanged) ---------------- */

/* dsp_runtime.c:42-59  -- numCore counts from 1; returns the DSP_CORE word (or the program start
 * when the program has no DSP_CORE and numCore... == first lookup), NULL when not found.          */
opcode_t *dspFindCore(opcode_t *codePtr, const int numCore);

/* dsp_runtime.c:62-77  -- skips CORE/NOP/PARAM/PARAM_NUM words in front of the executable part.   */
opcode_t *dspFindCoreBegin(opcode_t *ptr);

/* dsp_runtime.c:116-145 -- selects the sample-rate column, zeroes the state area (host mirror and
 * device), seeds dither.  0 ok, -1 unsupported fs, -2 fs outside the program's range.            */
int dspRuntimeReset(const int fs, int random, int defaultDither);

/* dsp_runtime.c:150-195 -- validates header, size, checksum, opcode level.  >= 0: program length in
 * words; -1 no header, -3 no cores, -4 checksum, -5 opcode too new, -6 buffer too small, or Reset's
 * code when fs != 0.  Extension: -7 when the program's encoding (header.format: 28 = Q28 integer,
 * 0 = float) would need dspChangeFormat for the entry point used later.          */
int dspRuntimeInit(opcode_t *codePtr, int maxSize, const int fs, int random, int defaultDither);

/* dsp_runtime.c:302-1314 -- one frame: samples[] is indexed by the program's IO numbers and is
 * read and written in place.  Returns 0 like the reference on success; negative on failure
 * (the reference cannot fail here; this implementation can: no GPU, core not lowerable).         */
int dspRuntime_2(opcode_t *core, int *rundata, int   *samples);   /* DSP_FORMAT_INT64        */
int dspRuntime_3(opcode_t *core, int *rundata, int   *samples);   /* DSP_FORMAT_FLOAT        */
int dspRuntime_4(opcode_t *core, int *rundata, int   *samples);   /* DSP_FORMAT_DOUBLE       */
int dspRuntime_5(opcode_t *core, int *rundata, float *samples);   /* DSP_FORMAT_FLOAT_FLOAT  */
int dspRuntime_6(opcode_t *core, int *rundata, float *samples);   /* DSP_FORMAT_DOUBLE_FLOAT */

extern dspHeader_t *dspHeaderPtr;           /* dsp_runtime.c:36 */
extern int          dspBiquadFreqSkip;      /* dsp_runtime.c:37 */
extern int          dspMantissa;            /* dsp_runtime.c:38 */
extern const char  *dspOpcodeText[DSP_MAX_OPCODE];                 /* dsp_header.c:10-73 */
long long dspQNM(double x, int n, int m);   /* dsp_header.c:75-77 */
long long dspQM64(double x, int m);         /* dsp_header.c:79-81 */
int       dspQM32(double x, int m);         /* dsp_header.c:83-85 */

/* ---------------- block extension (not in the reference) ----------------
 * Semantics: exactly nframes successive dspRuntime_N() calls over frame-interleaved buffers, i.e.
 * the host loop of linux/avdsp_plugin.c:98-141 for 32-bit samples:
 *     samples[in_io_base + k]  = in[n*in_stride + k]          k in [0, in_stride)
 *     dspRuntime_N(core, rundata, samples)
 *     out[n*out_stride + k]    = samples[out_io_base + k]     k in [0, out_stride)
 * Output slots the core never stores are left untouched.  in/out are HOST pointers here.
 * For the chain kernels the two windows must not overlap in IO numbers and must contain every IO the
 * core loads / stores.  The interpreter keeps a whole samples[] array per program, persistent like the
 * host's: slots outside the two windows are the program's own (values one core leaves for another, or
 * one frame for the next), and where the windows overlap the input is laid over the output.
 *
 * Two device paths sit behind these entry points.  A core that is a set of independent
 * LOAD|LOAD_GAIN -> BIQUADS* -> [FIR] -> [SAT0DB] -> STORE+ chains runs on parallel kernels in every
 * format (in 2, 4 and 6 a chain may also begin with LOAD_MUX, see dspRuntimeMuxInfo; and, with dspRuntimeSetOption("chain_finish", 1),
 * a chain without FIR and LOAD_MUX may end in SAT0DB_TPDF, SAT0DB_GAIN or SAT0DB_TPDF_GAIN instead of SAT0DB, and the core may begin
 * with one DSP_TPDF_CALC of the default width, see dspRuntimeFinishInfo; and, with dspRuntimeSetOption("chain_delay", 1), such a chain
 * may hold one DSP_DELAY behind its banks, see dspRuntimeDelayInfo; "fir_tail" and "mux_tail" lift the "without FIR" and the "without
 * LOAD_MUX" of both, see dspRuntimeFirTailInfo and dspRuntimeMuxTailInfo): 2, 4 and 6 on the section-pipelined cascade (biquad_row / biquad_row_i64 / biquad_pipe) and
 * the MFMA FIR (fir_tile); 3 and 5 -- float accumulators and the truncating dspMulFloatFloat -- on
 * chain_rows (a lane per chain and section) and fir_lane (a lane per chain and frame), with
 * chain_lane for single frames and cascades longer than 16 sections.  Any other core -- X/Y
 * arithmetic, TPDF dither, delay lines, LOAD_MUX in formats 3 and 5, RMS ... -- runs through the general device
 * interpreter (runs of identical strands on strand_lanes, a lane per strand).
 * Its frame-parallel kernel runs 64 frames of the block side by side (one
 * per lane, opcode by opcode) whenever the core hands nothing from one frame to the next except
 * opcode-private state (delay lines, filter state, meters ...), which is the case for every program
 * shipped with the reference; a core that does (a frame slot or memory read before it is written, a
 * TPDF_CALC behind its first use) runs frame by frame like the reference.  There is no CPU path. */
int dspRuntimeBlock_2(opcode_t *core, int *rundata, const int *in, int in_stride, int in_io_base,
                      int *out, int out_stride, int out_io_base, int nframes);
int dspRuntimeBlock_3(opcode_t *core, int *rundata, const int *in, int in_stride, int in_io_base,
                      int *out, int out_stride, int out_io_base, int nframes);
int dspRuntimeBlock_5(opcode_t *core, int *rundata, const float *in, int in_stride, int in_io_base,
                      float *out, int out_stride, int out_io_base, int nframes);
int dspRuntimeBlock_4(opcode_t *core, int *rundata, const int *in, int in_stride, int in_io_base,
                      int *out, int out_stride, int out_io_base, int nframes);
int dspRuntimeBlock_6(opcode_t *core, int *rundata, const float *in, int in_stride, int in_io_base,
                      float *out, int out_stride, int out_io_base, int nframes);

/* Same, with in/out resident in HBM (device pointers) and the work enqueued on `stream`
 * (a hipStream_t passed as void*, NULL = default stream).  Asynchronous: returns after enqueue. */
/* dspRuntimeBlock_N as a queue: submit returns once the block's copies and kernels are enqueued (its value: blocks in
 * flight, < 0 on error); up to four blocks are in flight, the copies of one under the kernels of another.  `in` and `out`
 * are pinned in place (hipHostRegister) and stay the library's -- allocated, unread, unwritten -- until
 * dspRuntimeBlockWait has let the block through; the registration ends there too, so a buffer may be freed as soon as
 * its block is back.  A host that cycles through the same few buffers sets dspRuntimeSetOption("host_pin", 1): the
 * registrations are then kept (registering 16 MB costs about as much as copying it) and the buffers must stay
 * allocated until "host_pin" is set back to 0, the program is released, or dspRuntimeRelease().
 * dspRuntimeBlockWait(m) returns when at most m submitted blocks are unfinished (oldest first; m = 0: all done) with
 * the number that still are.  Results are those of the same dspRuntimeBlock_N calls in the same order; every other
 * entry point waits for the queue by itself.  One core per block in flight: a program with several chain cores
 * submits core k+1 after dspRuntimeBlockWait(0) for core k (they share the output window), or uses dspRuntimeBlockAll. */
int dspRuntimeBlockSubmit(int format, opcode_t *core, int *rundata, const void *in, int in_stride, int in_io_base,
                          void *out, int out_stride, int out_io_base, int nframes);
int dspRuntimeBlockWait(int max_in_flight);

int dspRuntimeBlockDevice(int format, opcode_t *core, int *rundata,
                          const void *d_in, int in_stride, int in_io_base,
                          void *d_out, int out_stride, int out_io_base, int nframes, void *stream);

/* All cores of the loaded program over one block: the result of dspRuntimeBlock_N for core 1, 2, ... in turn
 * (the host loop of linux/avdsp_plugin.c:95-142 runs cores outermost too), in one call.  The samples cross PCIe
 * once instead of once per core, and cores that do not meet -- no frame slot, memory word (STORE_MEM, LOAD_MUX /
 * TPDF result), state range or dither global written by one and touched by the other -- run at the same time
 * on the device; cores that do are kept in program order.  Interpreted cores are cut further, into groups of
 * strands (LOAD ... STORE runs) that hand nothing to each other, which run side by side as well ("strand_split",
 * default 1).  dspRuntimeGetOption("levels") / ("cores") / ("pieces") tell how the latest call was arranged.  format = DSP_FORMAT 2..6;
 * in/out: int32 or float samples as in dspRuntimeBlock_N (host pointers) / device pointers + stream.       */
/* N instances of the loaded program side by side (extension; avdsp_host.c has the semantics): the reference is one program on one
 * core per process -- a host with many independent streams of the same program (a thousand stereo crossovers) loads it once.
 * Instance i: sample blocks at d_in + i * in_inst_words and d_out + i * out_inst_words (32-bit words), state of its own, copied
 * from the program's at the first block call after dspRuntimeSetInstances.  dspRuntimeInstanceState(i, dst) brings back instance
 * i's data area (dataSize words).  Cores for the frame-parallel interpreter (the reference's own
 * programs): an instance is a further copy of the device state (round 4); a program of CHAIN cores only (round 5): an instance is a further block of
 * chains in the chain kernels' launches -- 8 channels x 8 biquads in 512 instances are the 4096 rows of one cascade launch, 78 Gsamples/s
 * at 256-frame blocks -- with state, FIR history and parameters of its own in a copy of the mirror).  While a chain program runs as
 * instances the ordinary block calls on it are refused; dspRuntimeSetInstances(0) ends it (the single program continues from instance
 * 0's state, "strand_lanes" is what it was).  A program with cores of both kinds runs every core on the interpreter while it has
 * instances ("generic" reads 1 meanwhile; dspRuntimeSetInstances(0) gives it its chain plans back). */
int dspRuntimeSetInstances(int n);
int dspRuntimeBlockAllInstancesDevice(int format, int *rundata, const void *d_in, int in_stride, int in_io_base, size_t in_inst_words,
                                      void *d_out, int out_stride, int out_io_base, size_t out_inst_words, int nframes, void *stream);
int dspRuntimeInstanceState(int inst, int *dst);

int dspRuntimeBlockAll(int format, int *rundata, const void *in, int in_stride, int in_io_base,
                       void *out, int out_stride, int out_io_base, int nframes);
int dspRuntimeBlockAllDevice(int format, int *rundata, const void *d_in, int in_stride, int in_io_base,
                             void *d_out, int out_stride, int out_io_base, int nframes, void *stream);
/* the same with the plugin's packed PCM input (AVDSP_PCM_S16 / S24_3LE / S32, formats 2, 3, 4), unpacked once */
int dspRuntimeBlockAllPcm(int format, int *rundata, int pcm, const void *src, int in_stride, int in_io_base,
                          int *dst, int out_stride, int out_io_base, int nframes);

/* The host's sample-format step (linux/avdsp_plugin.c:103-121): `src` holds packed little-endian PCM,
 * frame-interleaved [nframes][in_stride]; pcm = AVDSP_PCM_S32 | AVDSP_PCM_S24_3LE | AVDSP_PCM_S16
 * (include/avdsp_hip.h).  The unpacking to s.31 words happens on the device; output is S32 like the
 * plugin's.  format = 2, 3 or 4 (the int-sample models).  dspRuntimeUnpackPcmDevice is the same
 * conversion alone, for producers whose PCM already sits in HBM (d_dst 16-byte aligned).          */
int dspRuntimeBlockPcm(int format, opcode_t *core, int *rundata, int pcm, const void *src, int in_stride, int in_io_base,
                       int *dst, int out_stride, int out_io_base, int nframes);
int dspRuntimeUnpackPcmDevice(int pcm, const void *d_src, int *d_dst, long long nsamples, void *stream);

/* The plugin's "tagoutput" option (linux/avdsp_plugin.c:133-137, key :262): bits 8..15 of the first output channel of a core
 * carry a count derived from the previous sample's upper half, so that a bit-perfect transport can be verified downstream:
 *     sample' = (sample & 0xFFFF0000) | (previoussample & 0x0000FF00);   previoussample = ((sample & 0xFFFF0000) >> 8) + 0x100
 * Call it after a core's block, on that core's first output column (column = its IO number - out_io_base), cores in program
 * order as the plugin's loop runs them; the carried value lives on the device.  Device-resident block, or host block.  */
int dspRuntimeTagOutputDevice(void *d_out, int out_stride, int column, int nframes, void *stream);
int dspRuntimeTagOutput(int *out, int out_stride, int column, int nframes);
int dspRuntimeTagOutputReset(int previoussample);

/* device state -> rundata (the buffer stays the checkpoint) / rundata -> device state (restore).
 * Sync also brings back the program words (DSP_STORE_MEM writes into the program's parameter
 * section, dsp_runtime.c:755-760).                                                              */
int dspRuntimeSyncState(int *rundata);
int dspRuntimeUploadState(const int *rundata);
/* The host edited parameters (gains, biquad coefficients, delay values, bypass flags, taps) in the program
 * words, as the reference allows between any two frames: carry the edits to the device.  State is kept. */
int dspRuntimeUploadParams(void);

/* ---------------- channel sharding across the GPUs of a node (not in the reference) ----------------
 * The reference has one notion of several executors: DSP_CORE segments meant for parallel XMOS threads, which its
 * Linux hosts run one after the other (linux/avdsp_plugin.c:95).  Here the unit is finer: the chains of a chain core
 * are independent channels (the lowering proves it: no IO stored twice, none both loaded and stored), so
 * `world` processes -- one per GPU -- each run a contiguous, balanced range of them and never exchange anything.
 *
 * dspRuntimeSetShard(rank, world): from now on every chain core of the loaded program is lowered to the chains
 * [lo, hi) of rank `rank` only, lo = rank*q + min(rank, r), hi = lo + q + (rank < r), (q, r) = divmod(chains, world).
 * It works on any loaded .bin (the cut is made after lowering, on the chain list), keeps the device state
 * (FIR histories return to the mirror and are picked up again), and (0, 1) switches it off.  The block calls'
 * windows then only need to cover the IO numbers of the rank's own chains: a host hands over its column slice
 *     in  = x + in_io_min-th column,  in_io_base  = in_io_min,  in_stride  = whatever pitch the slice has
 * and receives its slice of the output columns; dspRuntimeShardInfo() reports those IO ranges (host-only, nothing
 * runs).  Cores that are not chain cores (interpreter) are not cut: every rank runs them whole (replicas).
 * dspRuntimeSyncState() returns this rank's view: its own chains' state advanced, the other chains' untouched.
 * A rank whose range of a core is empty (more ranks than chains) launches nothing for that core and touches neither window -- unless
 * the core begins with a lowered DSP_TPDF_CALC ("chain_finish"): every rank runs that, because the cores behind it dither with what
 * it leaves in the program's globals.  Such a call stores no sample, but it is a block call like any other: hand it valid pointers
 * and windows at least one column wide (the ones the rank uses for its other cores will do).
 *
 * "shard_trees" (dspRuntimeSetOption, 0 or 1, default 0): with 0 a core that holds memory words ("chain_mem") is not
 * lowered while a shard is set -- a contiguous slice of chains may separate a STORE_MEM trunk from its LOAD_MEM branches -- and runs
 * whole on every rank, on the interpreter.  With 1 (and "chain_mem" 1) it is lowered and cut at TREE boundaries.  The tree of a chain:
 * a chain whose memory word has a trunk in the core belongs to that trunk's tree; every other chain (ordinary, or a branch of a word
 * nobody in the core writes) is a tree of its own.  A position p, 0 < p < chains, is open if no tree has a chain below p and a chain at
 * or above p (trees need not be adjacent: a tree closes everything between its first and its last chain); 0 and `chains` are open.
 * Rank k's lower boundary is the open position nearest to the balanced lo above, a tie goes to the lower position; its upper boundary
 * is rank k + 1's lower one.  The ranges stay contiguous, disjoint and cover the core, balanced by chain count as far as the trees let
 * them; a rank may come out empty (see below); a core without trees is cut exactly as above.  avdsp_amd/sharding.py
 * tree_shard_bounds() is the same rule.  Branches load no IO: a rank's input window is its trunks' and its ordinary chains'.
 * A trunk writes its word into THIS rank's mirror only, so such a core is lowered only if no opcode of another core reads or writes
 * one of its memory words -- as LOAD_MEM / STORE_MEM target or as a parameter (-8, "memory word %d is shared with another core: ...";
 * both cores of such a pair then run whole on every rank as with 0).  LOAD_STORE lists and instances stay refused under a shard.
 * After a block a rank's mirror holds its own trunks' words advanced and every other memory word as it was -- the same contract as
 * for state. */
int dspRuntimeSetShard(int rank, int world);
int dspRuntimeShardInfo(int format, opcode_t *core, int *total_chains, int *first_chain, int *nchains,
                        int *in_io_min, int *in_io_max, int *out_io_min, int *out_io_max);

/* Host-only: the tail of an interpreted core that is N >= 2 repetitions of one opcode sequence -- one strand per channel, the shape of
 * the reference's crossover programs -- runs with lane = strand (avdsp_hip.h, strand plans).  strands = 0: the core has no such tail, or
 * the run is too short for the current "strand_lanes" setting (default: more than 64 strands; 2: any run). */
int dspRuntimeStrandInfo(int format, opcode_t *core, int *strands, int *ops_per_strand, int *prefix_words);

/* Tunables: "fir_impl" 0 = plain tap loop, 1 = MFMA (fir_tile, default), 2 / 3 / 4 = the other MFMA kernels kept for comparison (fir_mfma,
 * fir_stream, fir_flow: same results); "biquad_impl" 0 = lane per channel,
 * 1 = section-pipelined (default: biquad_row where it applies, else biquad_pipe), 2 = round 2's biquad_pipe throughout; "interp_impl" 0 = interpreter always frame by frame, 1 = frame-parallel
 * where the core allows it (default); "strand_split" 0 = dspRuntimeBlockAll keeps cores whole; "strand_lanes" 0 = strand runs stay with the interpreter, 1 = runs of more than 64 strands on lanes (default: up to 64 strand groups get a wave each from the interpreter, which is faster), 2 = every run; "generic" 1 = every core through the interpreter;
 * "device" = HIP device ordinal (before the first block);
 * "overlap" (chain cores with cascades in front of FIRs, blocks resident on the device) 1 = the cascades run up to three blocks ahead of
 * the FIRs on a stream of the library's own -- the caller then guarantees that a block's INPUT is complete in memory when the call is made
 * (stream order no longer covers it); 2 = also the FIRs of consecutive blocks on two streams in turn, so that one starts while the other's
 * last workgroups leave (worth 3.5 % on a 4096-channel program, a loss below ~2000 channels) -- the caller then also guarantees that the
 * OUTPUT block of a call is not one an earlier call's FIR may still be writing (the caller's stream still waits for every block's end).
 * "fir_ahead" (under "overlap" 1) = "overlap" 2's arrangement of the FIRs WITHOUT its guarantee on the output: the FIRs of
 * consecutive blocks run on two streams of the library's own, each into a staging block of the library's, and a copy on the caller's
 * stream behind the FIR's event moves exactly the words the FIR chains store into the caller's block -- which is therefore only ever
 * written in the caller's stream order: one output block may serve every call, and work queued between two calls has read it before
 * the later call's words arrive.  -1 (default) = by the plan: plans of 8 M taps or more in all (FIR chains x the longest FIR: 4096 or
 * 2048 channels x 4096 taps, not their 8-GPU shards) and launches of 256 frames or more, and only once the four streams in play have
 * been seen to run side by side; 0 = never; 1 = whenever it is legal.  Never, whatever the value: in-place calls, chain instances,
 * output windows of more than 16384 words per frame, plans without an overlap mode (handed FIR chains, LOAD_MUX chains, a cascade that
 * stores itself), plans with impulse groups (dspRuntimeFirGroupInfo: their per-chain taps are made on a launch's own stream), a "fir_impl"
 * other than 1, "overlap" 0 / 2, "cu_split" -- such a call takes the path it always took.  dspRuntimeGetOption("fir_ahead_now") = 1 /
 * 0: what the latest launch did; ("fir_ahead_apart") = 1 / 0 / -1: the four streams were seen to run side by side / were not (a
 * forced staged launch is then correct and overlaps nothing) / not tried yet.  AVDSP_FIR_AHEAD=-1|0|1 in the environment when the
 * library is loaded is the option's default for a host that cannot call dspRuntimeSetOption (dspRuntimeGetOption reads that value).
 * Costs three staging blocks of 1024 frames of the widest output window (48 MB for 4096 channels).
 * Results are identical in every mode.  Under "overlap": "ring_wait" 1 (default) = the HOST waits (at most 1 ms, then it leaves it to the
 * stream after all) until the FIR three blocks back has ended before it enqueues a block's cascade -- the call then returns no more than
 * three blocks ahead of the device, and the cascades' stream carries no wait packet (worth 10 % on a 512-channel shard); 0 = that stream
 * waits.  "ready_words" = how a block's FIR finds its cascades' block: 0 an event between the two queues, 1 words published by the
 * cascade's waves and polled by the FIR's (slower), 2 words set by a kernel behind the cascade (no wait packet on the FIRs' stream),
 * -1 (default) = 2 where the FIR is the bound, else 0.  Round 5: ready words are only taken once kernels of the FIRs' stream and of the
 * cascades' stream have been SEEN to run side by side (a one-time probe per stream; dspRuntimeGetOption("side_by_side") 1 / 0 / -1 not
 * tried yet), and the cascades' stream is made anew while it shares a hardware queue with the FIRs' ("streams_remade" says how often) --
 * without that the mode does not overlap anything.  A FIR wave whose bounded wait for a ready word runs out all the same (a GPU that stops
 * running two queues at once) makes EVERY later call fail with -11 until dspRuntimeReset() or dspRuntimeSetOption("ready_timeouts", 0)
 * acknowledges; dspRuntimeGetOption("ready_timeouts") counts such waves, ("ready_mode") tells what the latest launch used.
 * "cu_split" k (experiment; 0 = off): under "overlap" the cascades' stream on k CUs of its own (8, 16, 32 ...; a CU mask),
 * the FIRs on a stream of the library's with the complementary mask (negative k: only the cascades masked); hand over a non-blocking
 * stream of your own with it -- CU-masked streams are blocking streams, beside the null stream every launch on them synchronises.
 * "group_fanout" 1 (default) = a chain core's cascades of up to 16 sections run as ONE launch whatever their lengths, longer ones side by
 * side over up to four streams; 0 = one launch per section count, one after the other (as through round 4; results identical).
 * "frame_server" 1 (opt-in; default 0, or 1 when the environment holds AVDSP_FRAME_SERVER=1 as the library loads) = dspRuntime_N calls
 * of interpreter cores go to ONE resident wave per program that keeps the program's state in LDS between frames,
 * bit-identical to the launch per call; up to three programs of a process have one at a time, everything else takes today's path.
 * "frame_server_idle_us" (50 .. 20000, default 1000) = the server leaves after that long without a request.  Read-only:
 * "frame_server_frames" (core calls served), "frame_server_launches" (servers started), "frame_server_fallbacks" (calls whose bounded
 * wait for the server ran out and that went the ordinary way) -- per device copy of the program, 0 before there is one.
 * "fir_split" 1 (opt-in, default 0): a fir_tile launch of at most one tile per SIMD cuts every tile's taps over two waves (within 1e-6 of
 * the reference, not its bits).  "fir_shared" 1 (default) = FIR chains that point at ONE impulse bank at the current rate, in groups of 16
 * chains or more, run as the columns of fir_shared's tiles (bit-identical); every other chain keeps fir_tile.  Only with
 * "fir_impl" 1, "overlap" 0, "fir_split" 0 and no chain instances -- everywhere else every chain takes today's path; 0 = every chain on
 * today's path.  Read-only: "fir_shared_chains" / "fir_shared_groups" = the chains / groups fir_shared took in the latest FIR launch of the
 * program (0 before there is one), "fir_shared_rows" = the row tiles per wave (R: 1, 2 or 4) of that launch, 0 when it did not take the path;
 * "fir_rows" forces its row tiles as it does fir_tile's.  dspRuntimeFirGroupInfo tells what the lowering groups.
 * A program's options are also the defaults of programs loaded later.                                */
int dspRuntimeSetOption(const char *key, int value);
int dspRuntimeGetOption(const char *key);

/* Kernel timing with HIP events on the launch stream: enable with dspRuntimeSetOption("profile", 1), or
 * ("profile", 2 * mask) to time only the kinds whose bit is set in mask (each event pair costs the stream a few
 * microseconds);
 * kind 0 = biquad cascade, 1 = FIR, 2 = pass-through, 3 = general interpreter frame by frame,
 * 4 = PCM unpack, 5 = general interpreter frame-parallel, 6 = strands on lanes, 7 = the LOAD_MUX stage in front
 * of the cascades (mux_tile / mux_plain).  Returns the summed duration (ms) and launch
 * count of the launches recorded since the previous read.                                        */
int dspRuntimeKernelTime(int kind, double *total_ms, int *launches);

/* Introspection of the lowered core (what the device plan contains), host-only.  nchains > 0: the
 * parallel chain kernels take it; nchains == 0: the general interpreter takes it; negative: neither
 * (encoding mismatch, an offset outside the buffer, an opcode with no defined result in this format). */
int dspRuntimeCoreInfo(int format, opcode_t *core, int *nchains, int *max_sections, int *max_taps);
/* Host-only, nothing runs on the GPU: the groups of 16 chains or more whose DSP_FIR points at one impulse bank at the current sample rate,
 * among the chains of the core this process runs (dspRuntimeSetShard) -- what "fir_shared" takes.  A core that the interpreter runs, or a
 * format without the chain FIR (2, 3, 5), has none. */
int dspRuntimeFirGroupInfo(int format, opcode_t *core, int *groups, int *grouped_chains, int *largest_group);
/* LOAD_MUX chain heads (dsp_runtime.c:871-897; formats 2, 4 and 6): a chain may begin with a weighted sum of several inputs instead of a
 * LOAD -- a mixing matrix in front of the chains.  A stage of its own in front of the cascades forms every chain's sum in the list's order,
 * one addition per entry like the reference (bit-identical, Inf / NaN / subnormal samples included), hands (float)ALU / ALU >> 28 to the
 * chain's first section or FIR, stores chains without a filter itself from the full accumulator, and leaves the block's last ALU in the
 * opcode's result word (dspRuntimeSyncState; another core may read it with LOAD_MEM_DATA).  Chains whose lists name the same IO sequence
 * (same length, same IOs, same order; the gains are free) form a mix group; groups of 16 chains or more run as a dense gains x samples
 * contraction on v_mfma_f64_16x16x4_f64 in formats 4 and 6 (mux_tile), everything else with a lane per (chain, frame) (mux_plain).
 * No IO a list names may be stored by a chain of the same core (the core then stays with the interpreter), and a block call's input
 * window must cover every list IO (dspRuntimeShardInfo's input range spans them).  Formats 3 and 5 keep such cores on the interpreter.
 * Limits, by design and not silently: a program with LOAD_MUX chains that gets dspRuntimeSetInstances(n > 1) runs every core on the
 * interpreter while it has instances (the rule of programs that mix chain and interpreter cores: "generic" reads 1 meanwhile); and a
 * plan with LOAD_MUX chains ignores "overlap" and the ready words -- its cascades follow the mux stage on the caller's stream.
 * dspRuntimeMuxInfo is host-only, nothing runs on the GPU: among the chains of the core this process runs (dspRuntimeSetShard, the
 * groups are formed after the cut) the chains that begin with LOAD_MUX, the groups of 16 or more, the chains in them and the longest
 * list.  A core the interpreter runs reports zeros; a LOAD_MUX whose table is damaged (no entries, an IO number outside the range, a
 * result word outside the state area) returns -8. */
int dspRuntimeMuxInfo(int format, opcode_t *core, int *mux_chains, int *groups, int *grouped_chains, int *longest_list);

/* Dressed finishes (opt-in: dspRuntimeSetOption("chain_finish", 1); default 0, every such core then runs on the interpreter as before).
 * In formats 2, 4 and 6 a chain's SAT0DB slot -- behind the banks, in front of the first STORE -- may hold DSP_SAT0DB_TPDF, DSP_SAT0DB_GAIN
 * or DSP_SAT0DB_TPDF_GAIN (dsp_runtime.c:478-534), and the core may begin, in front of its first LOAD, with one DSP_TPDF_CALC(n), n 0 or
 * the default dither (:537-545).  One wave (dither_block) then walks the generator over the block ahead of the cascades and leaves every
 * frame's addend in a table; the cascades keep the last section's whole accumulator and finish it with gain, addend, SAT0DB and the
 * format's STORE, bit for bit the reference's.  A core without the TPDF_CALC dithers with the value the program's globals hold when its
 * block starts (the reference's hosts run cores outer, frames inner).  Not lowered, i.e. on the interpreter as before: chains with a
 * DSP_FIR or a LOAD_MUX head, a TPDF_CALC anywhere else or of another width, a DSP_TPDF opcode, formats 3 and 5, any program in which
 * some core's TPDF_CALC asks for a width other than the default (the global width is then not constant), and every dressed core while
 * dspRuntimeSetInstances(n > 1) is in force.
 * dspRuntimeFinishInfo is host-only, nothing runs on the GPU: the chains with a dressed finish among the chains of the core this process
 * runs (dspRuntimeSetShard) and whether the core begins with a lowered TPDF_CALC.  A core the interpreter runs reports zeros. */
int dspRuntimeFinishInfo(int format, opcode_t *core, int *dressed_chains, int *tpdf_calc);

/* Delay lines (opt-in: dspRuntimeSetOption("chain_delay", 1); default 0, every core with a delay opcode then runs on the interpreter
 * as before and is refused by the chain lowering with the text it always had).  In formats 2, 4 and 6 a chain without DSP_FIR and
 * LOAD_MUX may hold ONE DSP_DELAY (dsp_runtime.c:769-794) behind its banks: in front of the SAT0DB slot (which may be empty) or between
 * that slot and the first STORE.  Both forms: dsp_DELAY_FixedMicroSec, and the parameter form whose microsecond word is read from the
 * device copy of the program at every launch and clamped to the line's size -- an edit of that word takes effect at the next block
 * without a new plan.  A chain may consist of LOAD, DELAY, STORE alone.  A delayed chain may carry a plain SAT0DB or none whatever
 * "chain_finish" says, a dressed finish only while "chain_finish" is 1 too.  The cascades hand every frame's whole accumulator to
 * chain_tail, one workgroup per chain, which runs delay, finish and STOREs in the chain's order; the line and its index word stay in
 * the state area where the reference keeps them, so dspRuntimeSyncState / UploadState / Reset need nothing new.  Not lowered, i.e. on
 * the interpreter as before (-8, a text of its own each): DSP_DELAY_DP and DSP_DELAY_1, a DSP_DELAY in front of the banks or behind a
 * STORE, two delays in one chain, a delayed chain with a DSP_FIR or a LOAD_MUX head or beside LOAD_MUX chains, formats 3 and 5, and any
 * program while dspRuntimeSetInstances(n > 1) is in force.
 * dspRuntimeDelayInfo is host-only, nothing runs on the GPU: the chains with a lowered delay among the chains of the core this process
 * runs (dspRuntimeSetShard), and the longest of their lines in samples at the current rate (parameter forms: what their word asks for
 * now, clamped).  A core the interpreter runs reports zeros. */
int dspRuntimeDelayInfo(int format, opcode_t *core, int *chains_delayed, int *longest_line);

/* Dressed finishes and delay lines behind a FIR (opt-in: dspRuntimeSetOption("fir_tail", 1); default 0, every core then takes the path
 * and is refused with the text it always had).  In formats 4 and 6 a chain with one DSP_FIR behind its optional banks may go on as
 * FIR -> [DELAY] -> [SAT0DB | SAT0DB_TPDF | SAT0DB_GAIN | SAT0DB_TPDF_GAIN] -> [DELAY] -> STORE(s): a "handed FIR chain", whose FIR
 * kernel (fir_tile's or fir_plain's HAND form) hands every frame's 64-bit accumulator to chain_tail instead of storing it.  The
 * dressed finish and a head TPDF_CALC still need "chain_finish" 1, the DELAY "chain_delay" 1, and all their rules hold (one delay, both
 * forms, a constant dither width, disjoint lines -- also disjoint from every FIR history --, no instances, no LOAD_MUX in the core).  A
 * bypassed DSP_FIR (offset 0 at the current rate, or length 0) no longer refuses such a chain: it is then an ordinary dressed / delayed
 * cascade chain.  Plain FIR chains of the same core stay what they are.  Limits: handed chains are in no fir_shared group (see
 * dspRuntimeFirGroupInfo), a plan that holds one runs back to back whatever "overlap" says, "fir_split" does not apply to their launch.
 * Not lowered (-8, a text each): the FIR pure-delay variant, formats 3 and 5 (and 2, which has no FIR), LOAD_MUX heads, DSP_DELAY_DP /
 * DSP_DELAY_1, a DSP_DELAY in front of the FIR, two FIRs in a chain.
 * dspRuntimeFirTailInfo is host-only, nothing runs on the GPU: the handed FIR chains among the chains of the core this process runs
 * (dspRuntimeSetShard) and how many of them have a delay.  A core the interpreter runs reports zeros. */
int dspRuntimeFirTailInfo(int format, opcode_t *core, int *handed_chains, int *of_them_delayed);

/* All of the above in a core with LOAD_MUX chain heads (opt-in: dspRuntimeSetOption("mux_tail", 1); default 0, every core then takes
 * the path and is refused with the text it always had).  The option lifts the "no LOAD_MUX" rule of "chain_finish", "chain_delay" and
 * "fir_tail" and replaces none of them: a dressed finish or a head TPDF_CALC still needs "chain_finish" 1, a DSP_DELAY "chain_delay" 1,
 * anything behind a FIR "fir_tail" 1 (formats 4 and 6).  In formats 2, 4 and 6 every chain of a core with LOAD_MUX chains -- whatever
 * its own head: LOAD_MUX, LOAD or LOAD_GAIN -- may then be what those options lower anywhere else, and the core may begin with a
 * TPDF_CALC.  A LOAD_MUX chain with sections or a FIR goes through the kernels those chains take elsewhere, from its column of the
 * stage's scratch block; one with neither is finished by the mux stage itself from the full accumulator (a dressed finish, no delay)
 * or handed to chain_tail as 64-bit accumulators (a delay) -- the TAIL forms of mux_tile and mux_plain, which only a plan with such a
 * chain launches.  Everything else those options refuse stays refused with its text; one check is new (-8): no delay line may share a
 * word of the state area with a LOAD_MUX result word.
 * dspRuntimeMuxTailInfo is host-only, nothing runs on the GPU: among the chains of the core this process runs (dspRuntimeSetShard),
 * if the core holds LOAD_MUX heads, those with a dressed finish, those with a delay, and the LOAD_MUX chains the stage finishes or hands
 * over itself.  A core without LOAD_MUX heads and a core the interpreter runs report zeros. */
int dspRuntimeMuxTailInfo(int format, opcode_t *core, int *dressed_chains, int *delayed_chains, int *stage_finished_or_handed);

/* "chain_mem" (dspRuntimeSetOption, 0 or 1, default 0): DSP_STORE_MEM and DSP_LOAD_MEM (dsp_runtime.c:750-766) on the chain
 * kernels of formats 2, 4 and 6 -- the crossover's shape, one conditioned input feeding several ways.  A trunk is LOAD | LOAD_GAIN,
 * [BIQUADS], STORE_MEM and has no STORE; a branch is LOAD_MEM and then whatever an ordinary chain may be behind its load, under the
 * options that lower it ("chain_delay", "chain_finish").  A frame runs the trunk first, then its branches; ordinary chains and other
 * trees may stand between them.  A branch of a word no chain of the core writes reads what the mirror holds when a launch starts (the
 * writer core's last frame, or an uploaded parameter).  After a launch both program words of a trunk hold its accumulator of the last
 * frame.  Refused with -8 and a text of its own, the core then on the interpreter as with 0: a STORE_MEM that is not its chain's last
 * opcode, two STORE_MEM of one word, words that overlap, a LOAD_MEM in front of the STORE_MEM of its word, a word that another opcode
 * reads as a parameter or that is no free PARAM word, a DSP_FIR or a LOAD_MUX head in or beside such chains, LOAD_MEM_DATA, formats 3
 * and 5, instances, a set shard (unless "shard_trees" is 1: dspRuntimeSetShard above).
 * dspRuntimeMemInfo is host-only, nothing runs on the GPU: the core's trunks, its branches, and the branches whose word no chain of
 * the core writes -- of the whole core, under a shard too.  A core without memory words and a core the interpreter runs report zeros. */
int dspRuntimeMemInfo(int format, opcode_t *core, int *trunks, int *branches, int *constant_branches);

/* "mem_fir" (dspRuntimeSetOption, 0 or 1, default 0): a DSP_FIR in a trunk or a branch of a "chain_mem" core, formats 4
 * and 6; without "chain_mem" the option does nothing.  A FIR trunk is LOAD | LOAD_GAIN, [BIQUADS], FIR, STORE_MEM: the FIR's sum is the
 * accumulator the STORE_MEM writes.  A FIR branch is LOAD_MEM, [BIQUADS], FIR and behind the FIR what an ordinary FIR chain may have:
 * nothing or SAT0DB and the STOREs, or, under "fir_tail" (with "chain_finish" / "chain_delay"), a DSP_DELAY on either side of a SAT0DB
 * or a dressed finish.  Without sections in front a branch's FIR takes the float the reference's FIR makes of the loaded accumulator.
 * Ordinary FIR chains may stand beside the trees, a bypassed DSP_FIR leaves an ordinary trunk or branch, and a branch of a word no
 * chain of the core writes may have a FIR like any other.  The chains of a core that holds a memory word are not offered to the
 * shared-impulse path: dspRuntimeFirGroupInfo reports no group for such a core.  Refused with -8 and a text of its own, the core then
 * on the interpreter: the FIR pure-delay variant, two FIRs in a chain, a DSP_DELAY in front of the FIR, format 2 (the int64 text),
 * formats 3 and 5, a delay line that shares words with a FIR's history, and whatever "chain_mem" and "fir_tail" refuse that is not
 * about a FIR beside memory words.  With 0 every core takes the path and the refusal text it had before the option existed.
 * dspRuntimeMemFirInfo is host-only, nothing runs on the GPU: over the whole core, the trunks with a FIR (taps at the current rate),
 * the branches with one, and of those branches the handed ones (a delay or a dressed finish behind the FIR).  A core without such
 * chains and a core the interpreter runs report zeros. */
int dspRuntimeMemFirInfo(int format, opcode_t *core, int *fir_trunks, int *fir_branches, int *of_them_handed);

/* "chain_copy" (dspRuntimeSetOption, 0 or 1, default 0): DSP_LOAD_STORE lists (dsp_runtime.c:738-747, samples[out] =
 * samples[in] pair by pair: the raw 32-bit word, no accumulator, no conversion, no store mask) in a core of chains, formats 2 to 6 --
 * in front of a head TPDF_CALC, between chains, behind a trunk's STORE_MEM, behind the last chain, or alone in a core.  The host
 * resolves the list's sequential meaning: a pair that reads an earlier pair's destination takes that pair's source, of two writers of
 * one IO the last wins, a pair that ends as a -> a is dropped.  What is left -- the live pairs -- is copied from the input window to the
 * output window by one launch per block call, beside the chains.  Refused with -8 and a text of its own, the core then on the
 * interpreter as with 0: a list between a chain's LOAD and its first STORE, a list of odd length, an IO number out of range, a pair
 * that reads an IO a chain of the core stores, a pair that writes an IO a chain of the core loads or stores, an IO that is source and
 * destination of live pairs, instances, a set shard.  Both windows of a block call must cover the live pairs' IOs
 * (dspRuntimeShardInfo's spans include them).  By the same reading, with the option on two chains of a core may STORE one IO: the
 * last one's words arrive, the earlier STORE is dropped (a chain left without any is lowered only where it has a DSP_DELAY, whose line
 * goes on; else -8 with its text).
 * dspRuntimeCopyInfo is host-only, nothing runs on the GPU: the pairs the core writes and the live pairs.  A core without lists and a
 * core the interpreter runs report zeros. */
int dspRuntimeCopyInfo(int format, opcode_t *core, int *pairs, int *live);

/* "chain_ways" (dspRuntimeSetOption, 0 or 1, default 0): X/Y forks and way operations in a core of chains.
 * Two-way forks, formats 2 to 6:  HEAD, COPYXY, <way A>, SWAPXY, <way B>  with HEAD a LOAD, a LOAD_GAIN or (under "chain_mem") a LOAD_MEM
 * and COPYXY the opcode directly behind it.  Each way is whatever an ordinary chain may be behind its head under the options that are
 * on, and ends in at least one STORE; way B becomes a chain of its own that loads the head again (a LOAD_MEM head: a second branch of
 * the word).  Way operations, formats 2, 4 and 6: a run of at most 4 DSP_GAIN / DSP_NEGX behind a chain's last BIQUADS -- or, without
 * banks, behind its head, COPYXY or SWAPXY -- and in front of its DSP_DELAY, SAT0DB slot and STOREs, applied in program order.
 * Refused with -8 and a text of its own, the core then on the interpreter as with 0: a COPYXY that is not directly behind a head or has
 * no SWAPXY in its chain, a SWAPXY without that COPYXY or before way A's first STORE, a second COPYXY or SWAPXY in a chain, a STORE_MEM
 * in a way, a fork behind a LOAD_MUX head, every other X/Y opcode; a GAIN or NEGX in front of a BIQUADS, behind a DSP_DELAY, a SAT0DB
 * or a STORE, a fifth one in a run, one in a chain with a DSP_FIR, in a trunk, in a core with LOAD_MUX heads, in formats 3 and 5, or
 * while the program has instances.  With 0 every core takes the path and the refusal text it had before the option existed.
 * dspRuntimeWaysInfo is host-only, nothing runs on the GPU: the forks of which this process runs a way (dspRuntimeCoreInfo counts each
 * way as a chain) and the chains this process runs that have way operations.  A core the interpreter runs reports zeros. */
int dspRuntimeWaysInfo(int format, opcode_t *core, int *forks, int *op_chains);

/* "chain_sum" (dspRuntimeSetOption, 0 or 1, default 0; effective only with "chain_mem" 1 and in formats 2, 4 and 6):
 * sum heads, a bus formed from memory words in front of a branch:
 *     LOAD_MEM(w0), ( LOAD_MEM(wk), ADDXY | SUBXY ){1 .. AVDSP_MAX_SUM_TERMS - 1}
 * Each later LOAD_MEM stands directly behind the head or behind the ADDXY / SUBXY before it, its ADDXY / SUBXY directly behind it (NOP,
 * PARAM, PARAM_NUM and SERIAL do not count).  A load moves X to Y, so at each step X is the newest word and Y the running value, which
 * becomes newest + running (ADDXY) or newest - running (SUBXY): nothing is reassociated, a word may occur twice.  Behind the head comes
 * whatever a LOAD_MEM branch may be under the options that are on, except a COPYXY fork.  Every term word is held to the rules of a
 * branch's word: a free word of a PARAM section, not overlapping another, not read as a parameter, its STORE_MEM -- if the core has
 * one -- in front of the head.
 * Refused with -8 and a text of its own, the core then on the interpreter as with 0: a LOAD_MEM behind a LOAD_MEM head without its
 * ADDXY / SUBXY, an ADDXY / SUBXY anywhere else, a ninth word, a COPYXY behind a sum head, a term in front of its word's STORE_MEM, a
 * sum head in a sharded core (also under "shard_trees").  A STORE_MEM in such a chain, instances and formats 3 and 5 keep the texts
 * they have.  With 0 every core takes the path and the refusal text it had before the option existed.
 * dspRuntimeSumInfo is host-only, nothing runs on the GPU: the sum heads of the core (dspRuntimeCoreInfo counts each as one chain,
 * dspRuntimeMemInfo as one branch) and the words they load in all.  A core the interpreter runs reports zeros. */
int dspRuntimeSumInfo(int format, opcode_t *core, int *heads, int *terms);

const char *dspRuntimeLastError(void);
void        dspRuntimeRelease(void);        /* frees device memory of every loaded program; the next Init starts clean */
/* Several programs in one process.  dspRuntimeInit(codePtr, ...) loads a program into a context of its own, keyed by the
 * caller's buffer (loading the same buffer again restarts that program); every call that takes a pointer into a program
 * -- a core, its data area -- addresses that program, and the reference's exported data (dspHeaderPtr, dspBiquadFreqSkip,
 * dspMantissa) follow.  Calls without one (dspRuntimeReset, options, shard, timers, tagoutput, wait) address the program
 * of the latest call that named one, or dspRuntimeSelect's.  Each program has its own device copy, GPU ("device"
 * option at the time of its first block call), shard and plans; an option set while a program is current also becomes
 * the default of programs loaded later.  One process can so drive several GPUs (one buffer per GPU, each with its
 * dspRuntimeSetShard), or several programs on one.  Up to 64.                                                    */
int         dspRuntimeSelect(const void *ptr_into_program);
int         dspRuntimeReleaseProgram(opcode_t *codePtr);

#ifdef __cplusplus
}
#endif
#endif /* AVDSP_RUNTIME_H_ */

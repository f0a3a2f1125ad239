/*
 * avdsp_interp.inc -- the GENERAL device path: a complete opcode interpreter in HIP, included into
 * avdsp_kernels.hip.  It executes any core the reference runtime executes
 * (module_avdsp/runtime/dsp_runtime.c:302-1314, all opcodes, DSP_FORMAT 2..6) on the GPU, one workgroup of
 * one wave per core.  Cores made of independent LOAD -> BIQUADS -> FIR -> STORE chains never come here: the
 * host lowers those to the pipelined / MFMA kernels.  This path exists so that programs with X/Y arithmetic,
 * TPDF dither, delay lines, LOAD_MUX, RMS ... (e.g. the reference's osx/crossoverLV6.bin) run behind the same
 * C ABI without a CPU fallback (SURVEY.md 8f, rank 2).
 *
 * Two kernels, one interpreter source (interp::run<FMT, WAVE>):
 *   interp_wave  lane l interprets frame l of a batch of 64 frames, opcode by opcode -- the reference's frame
 *                loop and opcode loop interchanged.  Exact whenever nothing but opcode-private state passes
 *                from one frame to the next, which the host establishes per core (avdsp_host.c, scan_generic).
 *   interp_core  lane 0 interprets frame after frame like the reference; takes the cores the other cannot.
 *
 * State lives where the reference keeps it: in the mirror of the caller's buffer (program words + data area,
 * same word layout, staged in LDS for the launch), plus the TPDF globals of dsp_tpdf.h:11-13,23,33 in a device
 * struct and the program's samples[] frame.  A launch writes back only what its core owns, so that cores which
 * do not meet can run at the same time (avdsp_hip_run_levels).
 */

struct TpdfLocal { int dither, mask; long long mask64; int shift; };      /* dsp_tpdf.h:15-21 */
struct TpdfGlobals {                                                    /* dsp_tpdf.h:11-13,23,33 */
    int value, random, default_dither;
    TpdfLocal global;
    unsigned xs[4];
};

struct GenericArgs {
    int  *buf;                       /* mirror: program words, data area from word prog_words */
    TpdfGlobals *tpdf;
    int   core_word, prog_words;
    int   end_word;                  /* stop in front of this opcode word (a core cut into strand groups); 0 = run to DSP_CORE / END */
    int   skip_from, skip_to;        /* jump from opcode word skip_from to skip_to (0: none) */
    int   freq_index, num_freq, biquad_skip, biquad_offset;
    unsigned delay_factor;
    int   scratch_len;               /* IO span of the scratch frame */
    unsigned *scratch;               /* the samples[] frame in HBM: persists between blocks and cores like the
                                        host's array (linux/avdsp_plugin.c:93 inputOutput[]) */
    int   frame_lds;                 /* LDS words set aside for the frame in front of the staged mirror */
    int   stage_words;               /* words of the mirror staged in LDS (0 = interpret out of HBM) */
    int   keep_words;                /* leading words never written back (the header) */
    int   batch_lds, batch_frames;   /* LDS word offset of the frame batch buffers; frames per batch */
    /* frame-parallel kernel only (interp_wave): */
    int   wave_span;                 /* frame slots kept per lane: IO span of the core and of the caller's windows */
    int   seq_words;                 /* LDS words for FIR sequences / cascade results (>= 128) */
    int   nvm, vm_word[16];          /* mirror words a frame writes and reads back later (memories, LOAD_MUX / TPDF results) */
    /* what the core owns = what a launch writes back (cores that do not meet may then run side by side): */
    const int *own; int nown;        /* mirror word ranges [lo, hi) in pairs; nown < 0: everything */
    int   tpdf_owner;                /* this core holds the TPDF_CALC: it writes the dither globals back */
    int  *tpdf_seq; int tpdf_role;   /* a core cut into pieces: the piece with the TPDF_CALC (role 1) leaves every frame's
                                        (value, white sample) pair in tpdf_seq[2 * frame], the later pieces of that core (role 2)
                                        take their frame's pair from there -- inside a core the dither value is per frame */
    unsigned written_io[8];          /* frame slots < 256 the core stores (nown >= 0) */
    int   nrd_slot, nwr_slot;        /* frame-parallel kernel: the slots to fetch from / deliver to the caller's rows; */
    unsigned char rd_slot[32], wr_slot[32];     /* < 0: too many */
    int   rows_whole;                /* per call: move / deliver the whole windows (unknown ownership, too many slots, or
                                        windows that share IO numbers: the input then shows through in the output rows) */
    unsigned *done_flag; unsigned done_seq;      /* single-frame host calls: the word in pinned host memory the kernel sets when everything it stores is
                                                    out (avdsp_kernels.hip frame_done; nullptr: none) */
    BlockIO io;
};

/* mirror words of the LDS copy that go back to HBM after a launch */
__device__ __forceinline__ void write_back_owned(const GenericArgs &a, int *buf, const int *prog, int lane)
{
    if (a.nown < 0) { for (int k = a.keep_words + lane; k < a.stage_words; k += 64) buf[k] = prog[k]; return; }
    for (int r = 0; r < a.nown; r++) {
        const int lo = max(a.own[2 * r], a.keep_words), hi = min(a.own[2 * r + 1], a.stage_words);
        for (int k = lo + lane; k < hi; k += 64) buf[k] = prog[k];
    }
}

namespace interp {

struct UniformWords {                                  /* payload words read as wave-uniform values */
    const int *p;
    int w0, w1;                                        /* the first two were fetched together with the head word */
    __device__ __forceinline__ int operator[](int k) const
    {
        return k == 0 ? w0 : k == 1 ? w1 : __builtin_amdgcn_readfirstlane(p[k]);
    }
};

/* The reference computes every product and sum as a separate IEEE operation; hipcc's default would fuse
 * a*b+c into one FMA (single rounding) and change float-format results.  The chain kernels are immune
 * (their products are exact in double), the interpreter is not. */
#pragma clang fp contract(off)

/* ---------------- dsp_ieee754.h restated for the device ---------------- */
/* mulop (avdsp_kernels.hip) without a branch: 64 frames in lockstep want straight-line code */
__device__ __forceinline__ double mulop_sel(float v)
{
    const unsigned u = __float_as_uint(v), e = u & 0x7F800000u;
    const double wide = widen_exp255(u), plain = (double)v;
    double d = e == 0x7F800000u ? wide : plain;
    return e == 0u ? 0.0 : d;
}
__device__ __forceinline__ double mul_fd(float a, float b) { return mulop_sel(a) * mulop_sel(b); }        /* :377-410, exact */

__device__ inline float mul_ff(float a, float b)                                                   /* :342-375, truncating */
{
    const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
    const int ea = (ua >> 23) & 255, eb = (ub >> 23) & 255;
    if (ea == 0 || eb == 0) return 0.0f;
    int e = ea + eb - 127;
    if (e < 1) return 0.0f;
    if ((ua ^ ub) & 0x80000000u) e |= 1 << 8;
    /* the reference multiplies the mantissas shifted left by 5 and keeps the product's upper word: ((ma << 5)(mb << 5)) >> 32 is
     * (ma mb) >> 22, and with both factors visibly below 2^24 the compiler takes the full-rate 24-bit multiplies */
    const unsigned ma = (ua & 0x7FFFFFu) | 0x800000u, mb = (ub & 0x7FFFFFu) | 0x800000u;
    unsigned hi = (unsigned)(((unsigned long long)ma * mb) >> 22);
    if (hi & (1u << 25)) { e++; hi >>= 2; } else hi >>= 1;
    hi &= (1u << 23) - 1;
    hi |= (unsigned)e << 23;
    return __uint_as_float(hi);
}

__device__ inline float int_to_float_scaled(int x, int shift)                                      /* :204-250 */
{
    /* no branch (round 5; every lane of the float-model chain kernels and of the frame-parallel interpreter comes through here per sample): the
     * magnitude normalised to bit 31, its top 24 bits the mantissa (truncated), 158 - the leading zeros the exponent -- INT_MIN one short, as the
     * reference's 7-step normaliser leaves it; the sign added to the exponent field the reference's way.  All 2^32 arguments at shift 31 and
     * 4e8 random (argument, shift) pairs compared with the branching form on the CPU. */
    const unsigned mag = x < 0 ? 0u - (unsigned)x : (unsigned)x;
    const int sign = x < 0 ? 256 : 0;
    const unsigned lz = (unsigned)__clz((int)mag);                                   /* (32 for 0: replaced below) */
    const unsigned norm = mag << (lz & 31u);
    const int e = (mag == 0x80000000u ? 157 : 158 - (int)lz) - shift;
    const unsigned r = ((norm >> 8) & 0x7FFFFFu) | ((unsigned)(e + sign) << 23);
    return __uint_as_float(x == 0 ? 0u : r);
}

__device__ inline double int_to_double_scaled(int x, int shift)                                    /* :253-298 */
{
    if (x == 0) return 0.0;
    if (x == (int)0x80000000u) return -ldexp(1.0, 23 - shift);
    return ldexp((double)x, -shift);
}

__device__ inline int s31_from_float(float f)                                                      /* :60-83 */
{
    const unsigned u = __float_as_uint(f);
    const int e = (u >> 23) & 255;
    if (e == 0) return 0;
    unsigned m = ((u & 0x7FFFFFu) | 0x800000u) << 8;
    const int n = 127 - e;
    if (n > 0) m >>= (n & 31);                 /* count modulo 32 beyond 2^-32, like the reference's x86-64 binaries */
    else m = 0x7FFFFFFFu;
    if (u & 0x80000000u) m = 0u - m;
    return (int)m;
}

__device__ inline float saturate_float(float f)                                                    /* :171-184 */
{
    const int e = (int)__float_as_uint(f) >> 23;
    if (e >= 127) return 1.0f;
    if (e < 0 && e >= -129) return -1.0f;
    return f;
}

__device__ inline float truncate_float(float f, int bit)                                           /* :112-139 */
{
    int i = (int)__float_as_uint(f);
    const int e = (i >> 23) & 255;
    if (e == 0) return 0.0f;
    const int n = 151 - bit - e;
    if (n > 0) {
        if (n >= 24) i = (i >= 0) ? 0 : (int)((unsigned)(256 + 128 - bit) << 23);
        else {
            const int mask = (int)(0xFFFFFFFFu << n);
            if (i < 0) i = (int)((unsigned)i + (unsigned)~mask);
            i &= mask;
        }
    }
    return __uint_as_float((unsigned)i);
}

__device__ inline double truncate_double(double d, int bit)                                        /* :142-168 */
{
    long long i = __double_as_longlong(d);
    const int e = (int)((i >> 52) & 2047);
    if (e == 0) return 0.0;
    const int n = 1076 - bit - e;
    if (n > 0) {
        if (n >= 53) {
            if (i >= 0) i = 0;
            else { const int hi = (int)((unsigned)(2048 + 1024 - bit) << 20); i = (long long)((unsigned long long)(long long)hi << 32); }
        } else {
            const long long mask = (long long)(~0ull << n);
            if (i < 0) i = (long long)((unsigned long long)i + (unsigned long long)~mask);
            i &= mask;
        }
    }
    return __longlong_as_double(i);
}

__device__ __forceinline__ float  shift_float(float f, int s)   { return __uint_as_float(__float_as_uint(f) + ((unsigned)s << 23)); }           /* :300-318 */
__device__ __forceinline__ double shift_double(double d, int s) { return __longlong_as_double((long long)((unsigned long long)__double_as_longlong(d) + ((unsigned long long)(long long)s << 52))); }

/* a - b with the NaN rule of the reference's platform.  NaN is not exotic in the float models: DSP_DITHER
 * makes Inf and NaN out of a zero error (it halves 0.0 through its exponent field, dsp_runtime.c:1121-1127).
 * SSE returns a NaN operand unchanged (quieted, sign kept; the first operand's when both are NaN); the
 * GPU subtracts by negating b, which flips the sign of b's NaN.  Everything else (add, mul, the default
 * NaN of Inf - Inf) already agrees. */
template <typename T> __device__ __forceinline__ T fsub(T a, T b)
{
    T r = a - b;
    if (b != b) r = (a != a) ? (a + a) : (b + b);     /* x + x quiets a NaN and keeps its sign */
    return r;
}

/* a op b for two accumulators that may both be NaN (double models; the float type FF has the rule built in):
 * SSE returns the first operand's NaN, else the second's, quieted, payload and sign untouched */
__device__ __forceinline__ bool nan_operand(double a, double b, double &r)
{
    if (a != a) { r = __longlong_as_double(__double_as_longlong(a) | 0x0008000000000000ll); return true; }
    if (b != b) { r = __longlong_as_double(__double_as_longlong(b) | 0x0008000000000000ll); return true; }
    return false;
}
/* add and mul hand a single NaN operand through like SSE does (quieted, sign and payload kept); only when BOTH
 * are NaN is the choice the GPU's (and the compiler's, which may commute): then the first operand's, quieted */
__device__ __forceinline__ double quiet_nan(double a) { return __longlong_as_double(__double_as_longlong(a) | 0x0008000000000000ll); }
__device__ __forceinline__ double xy_add(double a, double b) { const double r = a + b; return ((a != a) & (b != b)) ? quiet_nan(a) : r; }
__device__ __forceinline__ double xy_mul(double a, double b) { const double r = a * b; return ((a != a) & (b != b)) ? quiet_nan(a) : r; }
__device__ __forceinline__ double xy_div(double a, double b) { double r; return nan_operand(a, b, r) ? r : a / b; }

/* ---------------- subnormals: the reference runs with MXCSR.FTZ and MXCSR.DAZ ----------------
 * It is built -Ofast (CMakeLists.txt:7), so loading it switches the thread to flush-to-zero /
 * denormals-are-zero: every SSE arithmetic, compare and conversion instruction reads a subnormal operand
 * as signed zero and replaces a subnormal result by signed zero; plain moves, sign flips and the integer
 * bit manipulation of dsp_ieee754.h do not.  The tail of every decaying filter passes through this.
 *   ftz()           the flush itself
 *   FF              a float that computes that way: the accumulator type of the float-ALU models 3 and 5
 *   dn32() / up64() double -> float and float -> double conversions of the double-ALU models 4 and 6
 * (a subnormal double, < 2.2e-308, is out of reach for 32-bit audio and not modelled)              */
__device__ __forceinline__ float ftz(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x7F800000u) ? f : __uint_as_float(u & 0x80000000u);
}
/* Both interpreter kernels switch the wave's MODE register to flush single-precision subnormals at entry, like the
 * chain kernels (flush_f32_subnormals_like_the_reference, tools/denorm_mode_probe.hip): v_add / v_sub / v_mul_f32
 * and the f32 <-> f64 conversions then read a subnormal operand as signed zero and flush a subnormal result by
 * themselves, which is MXCSR.FTZ|DAZ at no instruction cost.  What the hardware mode does not cover stays in
 * software: compares and float -> int (ftz() below), and division, which goes through double (the compiler's f32
 * division sequence assumes the default mode; a double quotient rounded to float is the correctly rounded float
 * quotient, 53 >= 2*24+2). */
#ifndef AVDSP_INTERP_HW_FLUSH
#define AVDSP_INTERP_HW_FLUSH 1
#endif
#if AVDSP_INTERP_HW_FLUSH
__device__ __forceinline__ float  dn32(double d) { return (float)d; }
__device__ __forceinline__ double up64(float f)  { return (double)f; }
__device__ __forceinline__ float  fadd_flushed(float a, float b) { return a + b; }
__device__ __forceinline__ float  fsub_flushed(float a, float b) { return a - b; }
__device__ __forceinline__ float  fmul_flushed(float a, float b) { return a * b; }
__device__ __forceinline__ float  fdiv_flushed(float a, float b) { return (float)((double)a / (double)b); }
#else
__device__ __forceinline__ float  dn32(double d) { return ftz((float)d); }
__device__ __forceinline__ double up64(float f)  { return (double)ftz(f); }
__device__ __forceinline__ float  fadd_flushed(float a, float b) { return ftz(ftz(a) + ftz(b)); }
__device__ __forceinline__ float  fsub_flushed(float a, float b) { return ftz(ftz(a) - ftz(b)); }
__device__ __forceinline__ float  fmul_flushed(float a, float b) { return ftz(ftz(a) * ftz(b)); }
__device__ __forceinline__ float  fdiv_flushed(float a, float b) { return ftz(ftz(a) / ftz(b)); }
#endif

struct FF {
    float v;
    FF() = default;
    __device__ __forceinline__ FF(float f) : v(f) {}                       /* a move: nothing is flushed */
    __device__ __forceinline__ FF(int i) : v((float)i) {}
    __device__ __forceinline__ FF(unsigned i) : v((float)i) {}
    __device__ __forceinline__ explicit FF(double d) : v(dn32(d)) {}
    __device__ __forceinline__ explicit operator float() const { return v; }
    __device__ __forceinline__ explicit operator double() const { return up64(v); }
    __device__ __forceinline__ explicit operator int() const { return (int)ftz(v); }
    __device__ __forceinline__ FF operator-() const { return FF(-v); }
    /* NaN operands (DSP_DITHER makes them, see fsub): SSE hands back the first operand's NaN, quieted, else
     * the second's -- payload and sign untouched; the GPU's choice between two NaNs is its own */
    static __device__ __forceinline__ bool nan_in(float a, float b, float &r)
    {
        if (a != a) { r = __uint_as_float(__float_as_uint(a) | 0x00400000u); return true; }
        if (b != b) { r = __uint_as_float(__float_as_uint(b) | 0x00400000u); return true; }
        return false;
    }
    static __device__ __forceinline__ float both_nan(float a, float b, float r)      /* r = a op b; see xy_add */
    {
        return ((a != a) & (b != b)) ? __uint_as_float(__float_as_uint(a) | 0x00400000u) : r;
    }
    __device__ __forceinline__ FF &operator+=(FF b) { v = both_nan(v, b.v, fadd_flushed(v, b.v)); return *this; }
    __device__ __forceinline__ FF &operator-=(FF b) { float r; if (!nan_in(v, b.v, r)) r = fsub_flushed(v, b.v); v = r; return *this; }
    __device__ __forceinline__ FF &operator*=(FF b) { v = both_nan(v, b.v, fmul_flushed(v, b.v)); return *this; }
    __device__ __forceinline__ FF &operator/=(FF b) { float r; if (!nan_in(v, b.v, r)) r = fdiv_flushed(v, b.v); v = r; return *this; }
};
__device__ __forceinline__ FF operator+(FF a, FF b) { return a += b; }
__device__ __forceinline__ FF operator-(FF a, FF b) { return a -= b; }
__device__ __forceinline__ FF operator*(FF a, FF b) { return a *= b; }
__device__ __forceinline__ FF operator/(FF a, FF b) { return a /= b; }
__device__ __forceinline__ bool operator>(FF a, FF b)  { return ftz(a.v) > ftz(b.v); }
__device__ __forceinline__ bool operator<(FF a, FF b)  { return ftz(a.v) < ftz(b.v); }
__device__ __forceinline__ bool operator==(FF a, FF b) { return ftz(a.v) == ftz(b.v); }
__device__ __forceinline__ bool operator!=(FF a, FF b) { return ftz(a.v) != ftz(b.v); }
__device__ __forceinline__ FF xy_add(FF a, FF b) { return a + b; }
__device__ __forceinline__ FF xy_mul(FF a, FF b) { return a * b; }
__device__ __forceinline__ FF xy_div(FF a, FF b) { return a / b; }
__device__ __forceinline__ FF saturate_float(FF f)        { return FF(saturate_float(f.v)); }
__device__ __forceinline__ FF truncate_float(FF f, int b) { return FF(truncate_float(f.v, b)); }
__device__ __forceinline__ FF shift_float(FF f, int s)    { return FF(shift_float(f.v, s)); }

/* ---------------- arithmetic model traits (dsp_runtime.h:51-127) ---------------- */
template <int FMT> struct M;
template <> struct M<2> { using alu = long long; using smp = int;   using sp = int;   static constexpr bool alu_int = true,  alu64 = true,  smp_int = true;  };
template <> struct M<3> { using alu = FF;        using smp = int;   using sp = float; static constexpr bool alu_int = false, alu64 = false, smp_int = true;  };
template <> struct M<4> { using alu = double;    using smp = int;   using sp = float; static constexpr bool alu_int = false, alu64 = true,  smp_int = true;  };
template <> struct M<5> { using alu = FF;        using smp = float; using sp = float; static constexpr bool alu_int = false, alu64 = false, smp_int = false; };
template <> struct M<6> { using alu = double;    using smp = float; using sp = float; static constexpr bool alu_int = false, alu64 = true,  smp_int = false; };

template <int FMT> __device__ __forceinline__ typename M<FMT>::alu ld_alu(const int *p)
{
    if constexpr (M<FMT>::alu64) {
        const unsigned long long u = ((unsigned long long)(unsigned)p[1] << 32) | (unsigned)p[0];
        if constexpr (M<FMT>::alu_int) return (long long)u; else return __longlong_as_double((long long)u);
    } else return FF(__int_as_float(p[0]));
}
template <int FMT> __device__ __forceinline__ void st_alu(int *p, typename M<FMT>::alu v)
{
    if constexpr (M<FMT>::alu64) {
        unsigned long long u;
        if constexpr (M<FMT>::alu_int) u = (unsigned long long)v; else u = (unsigned long long)__double_as_longlong(v);
        p[0] = (int)(unsigned)u; p[1] = (int)(unsigned)(u >> 32);
    } else p[0] = __float_as_int(v.v);
}
/* parameter word -> accumulator-compatible value: Q28 int or float */
template <int FMT> __device__ __forceinline__ auto ld_par(const int *p)
{
    if constexpr (M<FMT>::alu_int) return p[0]; else return __int_as_float(p[0]);
}
template <int FMT> __device__ __forceinline__ typename M<FMT>::alu fmul(float a, float b)          /* :412-424 */
{
    if constexpr (M<FMT>::alu64) return mul_fd(a, b); else return FF(mul_ff(a, b));
}
/* acc += a*b (dspMaccFloatFloat).  With a float accumulator the reference's build does not add at all when
 * dspMulFloatFloat leaves through one of its "return 0.0" exits (-Ofast: x + 0.0 is x), so an accumulator
 * holding -0.0 -- a flushed negative underflow -- keeps its sign. */
template <int FMT> __device__ __forceinline__ typename M<FMT>::alu fmacc(typename M<FMT>::alu acc, float a, float b)
{
    if constexpr (M<FMT>::alu64) return acc + mul_fd(a, b);
    else {
        const int ea = (__float_as_uint(a) >> 23) & 255, eb = (__float_as_uint(b) >> 23) & 255;
        if (ea == 0 || eb == 0 || ea + eb - 127 < 1) return acc;
        return acc + FF(mul_ff(a, b));
    }
}
/* the int64 model's wrapping product, sum and difference (the reference's plain long long arithmetic, without the overflow C leaves
 * undefined): one definition for the interpreter, strand_lanes and chain_tail's way operations */
__device__ __forceinline__ long long wmul(long long x, long long y) { return (long long)((unsigned long long)x * (unsigned long long)y); }
__device__ __forceinline__ long long wadd(long long x, long long y) { return (long long)((unsigned long long)x + (unsigned long long)y); }
__device__ __forceinline__ long long wsub(long long x, long long y) { return (long long)((unsigned long long)x - (unsigned long long)y); }
/* accumulator <-> 32-bit float, the way the reference's instructions do it */
template <int FMT> __device__ __forceinline__ float to_sp(typename M<FMT>::alu X)
{
    if constexpr (M<FMT>::alu64) return dn32(X); else return X.v;
}
template <int FMT> __device__ __forceinline__ typename M<FMT>::alu to_alu(float f)
{
    if constexpr (M<FMT>::alu64) return up64(f); else return FF(f);
}
template <int FMT> __device__ __forceinline__ typename M<FMT>::alu from_int_scaled(int v, int shift)
{
    if constexpr (M<FMT>::alu64) return int_to_double_scaled(v, shift); else return FF(int_to_float_scaled(v, shift));
}
template <int FMT> __device__ __forceinline__ typename M<FMT>::alu sat0db(typename M<FMT>::alu v)
{
    if constexpr (M<FMT>::alu_int) return saturate64_031(v);
    else if constexpr (M<FMT>::alu64) return saturate_double_0db(v);
    else return saturate_float(v);
}

/* ---------------- TPDF: dsp_tpdf.h ---------------- */
__device__ __forceinline__ unsigned rotl32(unsigned x, unsigned k) { return (x << k) | (x >> (32 - k)); }

__device__ inline unsigned xoshiro128p(unsigned *s)                                                /* :35-49 */
{
    const unsigned r = s[0] + s[3], t = s[1] << 9;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl32(s[3], 11);
    return r;
}

template <int FMT>
__device__ inline int tpdf_prepare(const TpdfGlobals *g, const TpdfLocal *current, TpdfLocal *local, int dith)    /* :55-80 */
{
    if (dith == 0) dith = g->default_dither;
    if (dith == current->dither) return 1;
    local->dither = dith;
    local->mask = (int)(0xFFFFFFFFu << ((32 - dith) & 31));
    if constexpr (M<FMT>::alu_int) {
        local->mask64 = (long long)((unsigned long long)(long long)local->mask << 28);
        local->shift = 28 - dith + 1;
    }
    return 0;
}

template <int FMT>
__device__ inline typename M<FMT>::alu tpdf_apply(const TpdfGlobals *g, typename M<FMT>::alu x, const TpdfLocal *tp)   /* :133-156 */
{
    if constexpr (M<FMT>::alu_int) {
        long long t = g->value;
        t = tp->shift >= 0 ? (long long)((unsigned long long)t << (tp->shift & 63)) : (t >> ((-tp->shift) & 63));
        return (long long)((unsigned long long)x + (unsigned long long)t);
    } else return x + from_int_scaled<FMT>(g->value, 31 + tp->dither - 1);
}

template <int FMT>
__device__ inline typename M<FMT>::alu tpdf_truncate(typename M<FMT>::alu x, const TpdfLocal *tp)  /* :159-168 */
{
    if constexpr (M<FMT>::alu_int) return x & tp->mask64;
    else if constexpr (M<FMT>::alu64) return truncate_double(x, tp->dither);
    else return truncate_float(x, tp->dither);
}

/* A position counter read back from the state area (delay lines, tables, the histogram, the RMS line) indexes the
 * mirror: whatever the words hold -- foreign state uploaded by the host, another opcode's stray store -- the access
 * stays inside the opcode's own allocation.  Counters the reference could have produced pass unchanged. */
__device__ __forceinline__ int state_index(int v, int alloc) { return (unsigned)v < (unsigned)alloc ? v : 0; }

/* ---------------- biquad / FIR bodies for the non-pipelined path ---------------- */
/* one section, one frame (dsp_biquadSTD.h): state = accumulator + x1 x2 y1 y2 in the sample type; the value
 * handed to the next section is the accumulator narrowed to the sample type */
template <int FMT> struct BqState { typename M<FMT>::alu acc; int x1, x2, y1, y2; };

template <int FMT> __device__ __forceinline__ void bq_load(BqState<FMT> &q, const int *st)
{
    q.acc = ld_alu<FMT>(st); q.x1 = st[2]; q.x2 = st[3]; q.y1 = st[4]; q.y2 = st[5];
}
template <int FMT> __device__ __forceinline__ void bq_store(const BqState<FMT> &q, int *st)
{
    st_alu<FMT>(st, q.acc); st[2] = q.x1; st[3] = q.x2; st[4] = q.y1; st[5] = q.y2;
}

/* a * b + c on 64 bits, wrapping: one full-rate instruction */
__device__ __forceinline__ long long mad_i64_i32(int a, int b, long long c)
{
    long long d;
    asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c) : "vcc");
    return d;
}

/* xn / return value: the sample-typed word (int for the int64 model, float bits otherwise) */
template <int FMT>
__device__ __forceinline__ int bq_step(BqState<FMT> &q, int xw, const int *coef)
{
    if constexpr (M<FMT>::alu_int) {
        /* (v_mad_i64_i32 by name: inside a loop the compiler widens the coefficients ahead of it and then multiplies 64 x 32
         * bits with three quarter-rate instructions per product) */
        long long acc = q.acc;
        acc = mad_i64_i32(xw, coef[0], acc);
        acc = mad_i64_i32(q.x1, coef[1], acc);
        acc = mad_i64_i32(q.x2, coef[2], acc);
        acc = mad_i64_i32(q.y1, coef[3], acc);
        acc = mad_i64_i32(q.y2, coef[4], acc);
        const int hi = (int)(acc >> 32);
        if (hi >= (1 << 27)) acc = (1ll << 59) - 1;
        else if (hi <= 1 - (1 << 27)) acc = -(1ll << 59);
        q.acc = acc;
        q.y2 = q.y1; q.x2 = q.x1; q.x1 = xw;
        q.y1 = (int)(acc >> 28);
        return q.y1;
    } else {
        const float xn = __int_as_float(xw);
        typename M<FMT>::alu acc = q.acc;
        acc = fmacc<FMT>(acc, xn, __int_as_float(coef[0]));
        acc = fmacc<FMT>(acc, __int_as_float(q.x1), __int_as_float(coef[1]));
        acc = fmacc<FMT>(acc, __int_as_float(q.x2), __int_as_float(coef[2]));
        acc = fmacc<FMT>(acc, __int_as_float(q.y1), __int_as_float(coef[3]));
        acc = fmacc<FMT>(acc, __int_as_float(q.y2), __int_as_float(coef[4]));
        q.acc = acc;
        q.y2 = q.y1; q.x2 = q.x1; q.x1 = xw;
        q.y1 = __float_as_int(to_sp<FMT>(acc));
        return q.y1;
    }
}

template <int FMT> __device__ __forceinline__ int bq_input(typename M<FMT>::alu X)
{
    if constexpr (M<FMT>::alu_int) return (int)(X >> 28); else return __float_as_int(to_sp<FMT>(X));
}

template <int FMT>
__device__ inline typename M<FMT>::alu biquads(typename M<FMT>::alu X, const int *coef, int *st, int num, int skip)   /* dsp_biquadSTD.h */
{
    short n = (short)num;
    int xw = bq_input<FMT>(X);
    typename M<FMT>::alu acc = 0;
    while (n-- > 0) {
        BqState<FMT> q;
        bq_load<FMT>(q, st);
        xw = bq_step<FMT>(q, xw, coef);
        bq_store<FMT>(q, st);
        acc = q.acc;
        st += 6; coef += skip;
    }
    return acc;
}

template <int FMT>
__device__ inline typename M<FMT>::alu fir(float xn, const int *coef, int *st, int num)            /* dsp_firSTD.h:38-52 */
{
    typename M<FMT>::alu acc = 0;
    for (int i = 0; i < num; i++) {
        const float prev = __int_as_float(st[i]);
        st[i] = __float_as_int(xn);
        acc = fmacc<FMT>(acc, xn, __int_as_float(coef[i]));
        xn = prev;
    }
    return acc;
}

/* ---------------- frame-parallel forms (lane = frame of the batch) ---------------- */
/* frame slot s of lane l lives at samp[s * kLanePitch + l]: with an odd pitch both the opcodes (one slot, 64
 * lanes) and the block transposes (one frame, consecutive slots) touch 64 different LDS banks */
constexpr int kLanePitch = 65;

struct WaveCtx {
    int lane, nb;
    int frame0;              /* index in the block of the batch's first frame (of the frame, for the frame-by-frame kernel) */
    unsigned *vtmp;          /* 64 * 2 words */
    unsigned *vseq;          /* FIR input sequence / cascade results: seq_words (>= 128) */
    unsigned *vmem;          /* per-lane copies of the words listed in vm_word: [nvm][2][64] */
    const int *vm_word; int nvm;
    int *tpdf_seq;           /* GenericArgs::tpdf_seq as the kernel knows it (an instance's own; a pointer known to be HBM) */
};

/* The double-accumulator float models keep a section's operands widened (mulop) in registers: every MACC of
 * dsp_biquadSTD.h is then one FMA of an exact product, the form biquad_simple uses */
template <int FMT> struct BqWide { double acc, dx1, dx2, dy1, dy2; int x1, x2, y1, y2; };

template <int FMT>
__device__ __forceinline__ int bq_step_wide(BqWide<FMT> &q, int xw, const double *cd)
{
    const double dx = mulop_sel(__int_as_float(xw));
    double acc = q.acc;
    acc = __builtin_fma(dx, cd[0], acc);
    acc = __builtin_fma(q.dx1, cd[1], acc);
    acc = __builtin_fma(q.dx2, cd[2], acc);
    acc = __builtin_fma(q.dy1, cd[3], acc);
    acc = __builtin_fma(q.dy2, cd[4], acc);
    q.acc = acc;
    const float yn = dn32(acc);
    q.dy2 = q.dy1; q.dx2 = q.dx1; q.dx1 = dx; q.dy1 = mulop_sel(yn);
    q.y2 = q.y1; q.x2 = q.x1; q.x1 = xw; q.y1 = __float_as_int(yn);
    return q.y1;
}

/* v_writelane_b32: lane `lane` of v takes the uniform value (both operands scalar registers; the value may come straight from a
 * v_readlane -- only a lane SELECT written by the VALU needs wait states, and the selects here are SALU results) */
__device__ __forceinline__ int wave_writelane(int value, int lane, int v)
{
    value = __builtin_amdgcn_readfirstlane(value); lane = __builtin_amdgcn_readfirstlane(lane);      /* (no-ops where the compiler knows them uniform) */
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(value), "s"(lane));   /* (one scalar register per VALU instruction: the select goes through M0, which the compiler loads right in front of its own uses) */
    return v;
}

__device__ __forceinline__ void wave_writelane2(int value0, int value1, int lane, int &v0, int &v1)
{
    value0 = __builtin_amdgcn_readfirstlane(value0); value1 = __builtin_amdgcn_readfirstlane(value1); lane = __builtin_amdgcn_readfirstlane(lane);
    asm volatile("s_mov_b32 m0, %4\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0" : "+v"(v0), "+v"(v1) : "s"(value0), "s"(value1), "s"(lane));
}

constexpr int kWaveShr1 = 0x138;                        /* DPP wave_shr:1 (GFX9): lane l <- lane l - 1, lane 0 <- old */

/* The cascade of one BIQUADS opcode over the batch: lane s holds section s (state and coefficients in
 * registers) and the frames stream through, frame f reaching section s at step f + s -- the arrangement of
 * biquad_pipe.  nb + num - 1 steps instead of nb * num section updates one after the other; every section
 * update is the scalar cascade's.  Frames enter from and leave to per-lane registers (readlane with the
 * uniform step number, a select on the lane number), results move one lane up with a DPP shift: no LDS in the loop.        */
template <int FMT>
__device__ inline typename M<FMT>::alu wave_biquads(typename M<FMT>::alu X, const int *coef, int *st, int num, int skip, const WaveCtx &wc)
{
    constexpr bool WIDE = M<FMT>::alu64 && !M<FMT>::alu_int;
    const int lane = wc.lane, nb = wc.nb;
    int xin = bq_input<FMT>(X);                         /* this chunk of sections' input, frame = lane */
    int out[2] = {0, 0};                                /* the last section's accumulator, frame = lane */
    for (int c0 = 0; c0 < num; c0 += 64) {
        const int ns = min(64, num - c0);
        const bool mine = lane < ns;
        const bool more = c0 + 64 < num;                /* another chunk of sections follows: it takes this one's outputs */
        const unsigned late = mine ? (unsigned)lane : 0x40000000u;      /* step k carries a frame for this lane iff k - late < nb */
        BqState<FMT> q; q.acc = 0; q.x1 = q.x2 = q.y1 = q.y2 = 0;
        int c[5] = {0, 0, 0, 0, 0};
        if (mine) {
            bq_load<FMT>(q, st + 6 * (c0 + lane));
            const int *cp = coef + (c0 + lane) * skip;
            for (int k = 0; k < 5; k++) c[k] = cp[k];
        }
        int xnext = 0;
        /* one pass of the batch through the chunk.  section(x): this lane's section takes x, returns its output word;
         * acc_words: the accumulator as it stands.  Frames enter lane 0 by readlane with the uniform step number, move one lane up
         * with the DPP shift (lane 0 keeps the shift's old value: the entering frame), and leave the last section by
         * readlane / writelane into the lane of their frame: no LDS, no per-lane selects. */
        /* section(x, parity): the step number's parity as a compile-time constant where it can be had (the int64 form below keeps
         * its x and y pairs in registers that swap roles from step to step instead of being moved) */
        auto pass = [&](auto &&section, auto &&acc_words) {
            int y = 0;
            using even_t = std::integral_constant<int, 0>; using odd_t = std::integral_constant<int, 1>;
            auto step_any = [&](int x, int k) { if (k & 1) y = section(x, odd_t{}); else y = section(x, even_t{}); };
            auto enter = [&](int k) {                   /* lane l <- lane l - 1's output of the step before; lane 0 <- frame k */
                const int x0 = __builtin_amdgcn_readlane(xin, k);
                return __builtin_amdgcn_update_dpp(x0, y, kWaveShr1, 0xF, 0xF, false);
            };
            auto leave = [&](int k) {                   /* frame k - (ns - 1) leaves the last section */
                const int fo = k - (ns - 1);
                int a0 = 0, a1 = 0;
                acc_words(a0, a1);
                if constexpr (M<FMT>::alu64) wave_writelane2(__builtin_amdgcn_readlane(a0, ns - 1), __builtin_amdgcn_readlane(a1, ns - 1), fo, out[0], out[1]);
                else out[0] = wave_writelane(__builtin_amdgcn_readlane(a0, ns - 1), fo, out[0]);
                if (more) xnext = wave_writelane(__builtin_amdgcn_readlane(y, ns - 1), fo, xnext);
            };
            /* the pipeline fills (nothing leaves yet) ... */
            for (int k = 0; k < ns - 1; k++) {
                const int x = enter(min(k, nb - 1));
                if ((unsigned)k - late < (unsigned)nb) step_any(x, k);
            }
            /* ... runs with a frame in every section ... */
            /* (four steps per turn, written out: the compiler does not unroll a loop of lane exchanges with a remainder) */
            /* (lanes beyond the chunk's sections run along on zero coefficients: their state is never stored, and the loop needs
             * no look at who has work) */
            auto steady = [&](int k, auto pc) { const int x = enter(k); y = section(x, pc); leave(k); };
            int ks = ns - 1;
            if ((ks & 1) && ks < nb) { steady(ks, odd_t{}); ks++; }
            for (; ks + 4 <= nb; ks += 4) { steady(ks, even_t{}); steady(ks + 1, odd_t{}); steady(ks + 2, even_t{}); steady(ks + 3, odd_t{}); }
            for (; ks < nb; ks++) { const int x = enter(ks); step_any(x, ks); leave(ks); }
            /* ... and drains */
            for (int k = max(ns - 1, nb); k < nb + ns - 1; k++) {
                const int x = enter(nb - 1);
                if ((unsigned)k - late < (unsigned)nb) step_any(x, k);
                leave(k);
            }
        };
        if constexpr (WIDE) {
            /* the double-accumulator float models keep a section's operands widened: every MACC one FMA of an exact product */
            double cd[5];
            for (int k = 0; k < 5; k++) cd[k] = mulop(__int_as_float(c[k]));
            bool done = false;
#if AVDSP_INTERP_HW_FLUSH
            {
                /* First with the plain conversions: they are mulop() for every operand that is not Inf / NaN (which mulop widens on
                 * its own terms) -- subnormals read as zero in this kernel's float mode, and a zero's sign cannot reach the sum
                 * unless the accumulator came in as -0.  The largest exponent met says whether that held; else once more, below. */
                unsigned seen = max(max((unsigned)q.x1 << 1, (unsigned)q.x2 << 1), max((unsigned)q.y1 << 1, (unsigned)q.y2 << 1));
                if (__double_as_longlong(q.acc) == (long long)0x8000000000000000ull) seen = 0xFFFFFFFFu;
                double acc = q.acc;
                double dx1 = (double)__int_as_float(q.x1), dx2 = (double)__int_as_float(q.x2);
                double dy1 = (double)__int_as_float(q.y1), dy2 = (double)__int_as_float(q.y2);
                int x1 = q.x1, x2 = q.x2, y1 = q.y1, y2 = q.y2;
                pass([&](int x, auto) {
                         const double dx = (double)__int_as_float(x);
                         acc = __builtin_fma(dx, cd[0], acc); acc = __builtin_fma(dx1, cd[1], acc); acc = __builtin_fma(dx2, cd[2], acc);
                         acc = __builtin_fma(dy1, cd[3], acc); acc = __builtin_fma(dy2, cd[4], acc);
                         const float yn = (float)acc;
                         const int yb = __float_as_int(yn);
                         seen = max(seen, max((unsigned)x << 1, (unsigned)yb << 1));
                         dx2 = dx1; dx1 = dx; dy2 = dy1; dy1 = (double)yn;
                         x2 = x1; x1 = x; y2 = y1; y1 = yb;
                         return yb;
                     },
                     [&](int &a0, int &a1) { a0 = __double2loint(acc); a1 = __double2hiint(acc); });
                if (__ballot(seen >= 0xFF000000u) == 0) {
                    q.acc = acc; q.x1 = x1; q.x2 = x2; q.y1 = y1; q.y2 = y2;
                    done = true;
                }
            }
#endif
            if (!done) {
                BqWide<FMT> qw = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                qw.acc = q.acc; qw.x1 = q.x1; qw.x2 = q.x2; qw.y1 = q.y1; qw.y2 = q.y2;
                qw.dx1 = mulop(__int_as_float(q.x1)); qw.dx2 = mulop(__int_as_float(q.x2));
                qw.dy1 = mulop(__int_as_float(q.y1)); qw.dy2 = mulop(__int_as_float(q.y2));
                pass([&](int x, auto) { return bq_step_wide<FMT>(qw, x, cd); },
                     [&](int &a0, int &a1) { a0 = __double2loint(qw.acc); a1 = __double2hiint(qw.acc); });
                q.acc = qw.acc; q.x1 = qw.x1; q.x2 = qw.x2; q.y1 = qw.y1; q.y2 = qw.y2;
            }
        } else if constexpr (M<FMT>::alu_int) {
            /* int64: first without the saturation of dsp_biquadSTD.h:60-62 -- five v_mad_i64_i32, the largest high word tracked by the
             * way.  A chunk in which an accumulator left the clamp's range runs again from its untouched state with the clamp (not on
             * audio at sane levels; tests/test_gpu_edge.py's full-scale cases). */
            long long acc = q.acc;
            int x1 = q.x1, x2 = q.x2, y1 = q.y1, y2 = q.y2;
            unsigned reach = 0;
            pass([&](int x, auto) {
                     acc = mad_i64_i32(x, c[0], acc); acc = mad_i64_i32(x1, c[1], acc); acc = mad_i64_i32(x2, c[2], acc);
                     acc = mad_i64_i32(y1, c[3], acc); acc = mad_i64_i32(y2, c[4], acc);
                     reach = max(reach, (unsigned)(int)(acc >> 32) + 0x07FFFFFEu);      /* in range: <= 0x0FFFFFFD */
                     x2 = x1; x1 = x; y2 = y1;
                     y1 = (int)(acc >> 28);
                     return y1;
                 },
                 [&](int &a0, int &a1) { a0 = (int)acc; a1 = (int)(acc >> 32); });
            if (__ballot(reach > 0x0FFFFFFDu) == 0) { q.acc = acc; q.x1 = x1; q.x2 = x2; q.y1 = y1; q.y2 = y2; }
            else
                pass([&](int x, auto) { return bq_step<FMT>(q, x, c); },
                     [&](int &a0, int &a1) { int w[2] = {0, 0}; st_alu<FMT>(w, q.acc); a0 = w[0]; a1 = w[1]; });
        } else {
            /* float accumulator, truncating dspMulFloatFloat: the five software products of an update on operands TAKEN APART ONCE --
             * the coefficients for the batch, a sample when it enters the section (it is multiplied three times: as x, x1, x2), an output
             * when it is made -- word m = mantissa with hidden bit and the sign in bit 31, word e = biased exponent (a coefficient's less
             * 127; a large negative number for exponent 0, which makes "too small: the accumulator stays" one compare).  ff_macc is
             * dsp_ieee754.h:342-375's integer arithmetic, literally.  Two NaNs add the SSE way in the reference (FF::operator+=) and a
             * product whose exponent field filled up may read as one: the largest exponent sum is tracked, and a chunk that met one runs
             * again from its untouched state through bq_step. */
            struct Apart { unsigned m; int e; };
            auto apart = [](unsigned w, int bias) -> Apart {
                const int e = (int)(w >> 23 & 255u);
                return Apart{(w & 0x807FFFFFu) | 0x800000u, e ? e - bias : -4096};
            };
            auto whole = [](Apart v) -> int { return (int)((v.m & 0x807FFFFFu) | (unsigned)(v.e == -4096 ? 0 : v.e) << 23); };
            Apart cf[5];
            for (int k = 0; k < 5; k++) cf[k] = apart((unsigned)c[k], 127);
            int emax = 0;
            auto ff_macc = [&](float acc, Apart xo, Apart cc) -> float {
                const int e = xo.e + cc.e;
                const unsigned p = (unsigned)(((unsigned long long)(xo.m & 0xFFFFFFu) * (cc.m & 0xFFFFFFu)) >> 22);
                const unsigned up = p >> 25 & 1u;
                const unsigned e9 = ((unsigned)e | ((xo.m ^ cc.m) >> 23 & 0x100u)) + up;
                const unsigned word = ((p >> (1u + up)) & 0x7FFFFFu) | (e9 << 23);
                const float sum = acc + __uint_as_float(word);
                emax = max(emax, e);
                return e >= 1 ? sum : acc;
            };
            float acc = q.acc.v;
            Apart x1 = apart((unsigned)q.x1, 0), x2 = apart((unsigned)q.x2, 0), y1 = apart((unsigned)q.y1, 0), y2 = apart((unsigned)q.y2, 0);
            pass([&](int x, auto) {
                     const Apart xn = apart((unsigned)x, 0);
                     acc = ff_macc(acc, xn, cf[0]); acc = ff_macc(acc, x1, cf[1]); acc = ff_macc(acc, x2, cf[2]);
                     acc = ff_macc(acc, y1, cf[3]); acc = ff_macc(acc, y2, cf[4]);
                     x2 = x1; x1 = xn; y2 = y1; y1 = apart(__float_as_uint(acc), 0);
                     return __float_as_int(acc);
                 },
                 [&](int &a0, int &a1) { a0 = __float_as_int(acc); a1 = 0; });
            if (__ballot(emax >= 254) == 0) { q.acc = FF(acc); q.x1 = whole(x1); q.x2 = whole(x2); q.y1 = whole(y1); q.y2 = whole(y2); }
            else
                pass([&](int x, auto) { return bq_step<FMT>(q, x, c); },
                     [&](int &a0, int &a1) { int w[2] = {0, 0}; st_alu<FMT>(w, q.acc); a0 = w[0]; a1 = w[1]; });
        }
        if (mine) bq_store<FMT>(q, st + 6 * (c0 + lane));
        xin = xnext;
    }
    __syncthreads();
    return ld_alu<FMT>(out);
}

/* DSP_FIR over the batch: every frame's tap loop is the scalar one (same order of accumulation), reading
 * its inputs from one sequence = the delay line's history, oldest first, followed by the batch's inputs */
template <int FMT>
__device__ inline typename M<FMT>::alu wave_fir(float xn, const int *coef, int *st, int num, const WaveCtx &wc)
{
    const int lane = wc.lane, nb = wc.nb;
    int *seq = (int *)wc.vseq;
    for (int p = lane; p < num; p += 64) seq[p] = st[num - 1 - p];
    seq[num + lane] = __float_as_int(xn);
    __syncthreads();
    typename M<FMT>::alu acc = 0;
    const int *mine = seq + num + lane;
    for (int i = 0; i < num; i++) acc = fmacc<FMT>(acc, __int_as_float(mine[-i]), __int_as_float(coef[i]));
    for (int i = lane; i < num; i += 64) st[i] = seq[num + nb - 1 - i];
    __syncthreads();
    return acc;
}

/* ---------------- one frame, or one batch of frames side by side: dsp_runtime.c:302-1314 ----------------
 *
 * WAVE = false: the calling lane interprets one frame (samp[io] is the frame).
 * WAVE = true:  all 64 lanes call this together and lane l interprets frame l of a batch of nb frames,
 *   opcode by opcode (loop interchange of the reference's frame loop and opcode loop).  X, Y and the
 *   samples[] frame are per lane (samp[io * kLanePitch + lane]).  Opcodes without state are the same code on
 *   64 lanes; delay lines, FIR and the biquad cascade have frame-parallel forms below; everything else
 *   with state in the mirror (RMS, DCBLOCK, dither, tables, generators, TPDF_CALC ...) takes turns, lane
 *   after lane, in frame order.  The host only selects this form for cores where the interchange is
 *   exact: nothing a frame reads may have been left by the previous frame except opcode-private state
 *   (avdsp_host.c, scan_generic: "carried" analysis).                                                   */

template <int FMT, bool WAVE>
__device__ __forceinline__ void run(const GenericArgs &a, int *prog, unsigned *samp, TpdfGlobals *g, const WaveCtx &wc)
{
    using alu_t = typename M<FMT>::alu;
    using sp_t = typename M<FMT>::sp;
    constexpr bool AI = M<FMT>::alu_int, A64 = M<FMT>::alu64, SI = M<FMT>::smp_int;
    constexpr int AW = A64 ? 2 : 1;
    /* prog / samp / g arrive as separate pointers (not through the struct) so that, once inlined into the
     * LDS-staged kernel, the compiler can prove they are LDS and emit ds_* instead of flat accesses */
    int *rundata = prog + a.prog_words;
    TpdfLocal local = {0, 0, 0, 0};
    const TpdfLocal *tp = &g->global;
    alu_t X = 0, Y = 0;
    int pc = a.core_word;
    const int lane = WAVE ? wc.lane : 0, nb = WAVE ? wc.nb : 1;
    int gv = g->value, gr = g->random;             /* WAVE: this frame's TPDF value / white sample */
    if (a.tpdf_role == 2 && lane < nb) { const int *q = wc.tpdf_seq + 2 * (wc.frame0 + lane); gv = q[0]; gr = q[1]; }

    auto to_alu_i = [](int v) -> alu_t { return (alu_t)v; };
    /* sums and products whose two operands can both be NaN (the float models' DSP_DITHER makes NaN, see fsub): the
     * first operand's NaN wins, as in the SSE instruction the source line compiles to -- hipcc is free to commute
     * a plain a + b, and does so differently in the two kernels */
    auto radd = [&](alu_t p, alu_t q) -> alu_t { if constexpr (AI) return wadd(p, q); else return xy_add(p, q); };
    auto rmul = [&](alu_t p, alu_t q) -> alu_t { if constexpr (AI) return wmul(p, q); else return xy_mul(p, q); };
    auto ld_sp = [](const int *p) -> sp_t { if constexpr (AI) return p[0]; else return __int_as_float(p[0]); };
    auto st_sp = [](int *p, sp_t v) { if constexpr (AI) p[0] = v; else p[0] = __float_as_int(v); };
    auto S = [&](int io) -> unsigned & { if constexpr (WAVE) return samp[io * kLanePitch + lane]; else return samp[io]; };
    auto ld_smp = [&](int io) { if constexpr (SI) return (int)S(io); else return __uint_as_float(S(io)); };
    /* state that every frame overwrites (LOAD_MUX / TPDF results, memories): the last frame's value stays */
    auto st_last = [&](int *p, alu_t v) { if (!WAVE || lane == nb - 1) st_alu<FMT>(p, v); };
    /* lane after lane, in frame order; the barrier also orders the LDS traffic of one turn before the next */
    auto serial = [&](auto body) {
        if constexpr (WAVE) { for (int f = 0; f < nb; f++) { if (lane == f) body(); __syncthreads(); } }
        else body();
    };
    auto vm_find = [&](int word) -> int {
        if constexpr (WAVE) { for (int k = 0; k < wc.nvm; k++) if (wc.vm_word[k] == word) return k; }
        return -1;
    };
    auto vm_put = [&](int *p, alu_t v) {            /* this frame's copy of a word later opcodes of the frame read back */
        if constexpr (WAVE) {
            const int k = vm_find((int)(p - prog));
            if (k >= 0) {                               /* columns of 64: word j of entry k, lane l -> vmem[(2k + j) * 64 + l] */
                int tmp[2] = {0, 0};
                st_alu<FMT>(tmp, v);
                wc.vmem[(k * 2) * 64 + lane] = (unsigned)tmp[0];
                if constexpr (A64) wc.vmem[(k * 2 + 1) * 64 + lane] = (unsigned)tmp[1];
            }
        }
    };
    auto vm_store = [&](int *p, alu_t v) { st_last(p, v); vm_put(p, v); };
    auto vm_load = [&](int *p) -> alu_t {
        if constexpr (WAVE) {
            const int k = vm_find((int)(p - prog));
            if (k >= 0) {
                int tmp[2] = {(int)wc.vmem[(k * 2) * 64 + lane], A64 ? (int)wc.vmem[(k * 2 + 1) * 64 + lane] : 0};
                return ld_alu<FMT>(tmp);
            }
        }
        return ld_alu<FMT>(p);
    };
    /* Opcodes whose state runs from frame to frame (WAVE): every lane walks the frames in order with the
     * state in its own registers -- uniform, redundant work, no LDS round trip and no divergence per frame --
     * and frame f's lane keeps what the walk gave its frame.  body(x, y, v): one frame's update; x, y = that
     * frame's X and Y, v = its TPDF value. */
    auto lane_of = [&](alu_t v, int f) -> alu_t {
        int t[2] = {0, 0};
        st_alu<FMT>(t, v);
        t[0] = __builtin_amdgcn_readlane(t[0], f);
        if constexpr (A64) t[1] = __builtin_amdgcn_readlane(t[1], f);
        return ld_alu<FMT>(t);
    };
    auto turns_x = [&](auto body) {
        if constexpr (WAVE) {
            for (int f = 0; f < nb; f++) {
                alu_t x = lane_of(X, f), y = 0;
                body(x, y, __builtin_amdgcn_readlane(gv, f));
                if (lane == f) X = x;
            }
        } else body(X, Y, gv);
    };
    auto turns_xy = [&](auto body) {
        if constexpr (WAVE) {
            for (int f = 0; f < nb; f++) {
                alu_t x = lane_of(X, f), y = lane_of(Y, f);
                body(x, y, __builtin_amdgcn_readlane(gv, f));
                if (lane == f) { X = x; Y = y; }
            }
        } else body(X, Y, gv);
    };
    /* state back into the mirror after a walk: every lane holds the same words */
    auto uniform_store = [&](auto stores) {
        if constexpr (WAVE) { if (lane == 0) stores(); __syncthreads(); } else stores();
    };
    auto tpdf_add_v = [&](alu_t x, int v) -> alu_t {        /* dsp_tpdf.h:133-156 */
        if constexpr (AI) {
            long long t = v;
            t = tp->shift >= 0 ? (long long)((unsigned long long)t << (tp->shift & 63)) : (t >> ((-tp->shift) & 63));
            return (long long)((unsigned long long)x + (unsigned long long)t);
        } else return x + from_int_scaled<FMT>(v, 31 + tp->dither - 1);
    };
    auto tpdf_add = [&](alu_t x) -> alu_t {         /* dsp_tpdf.h:133-156 with this frame's value */
        if constexpr (AI) {
            long long t = gv;
            t = tp->shift >= 0 ? (long long)((unsigned long long)t << (tp->shift & 63)) : (t >> ((-tp->shift) & 63));
            return (long long)((unsigned long long)x + (unsigned long long)t);
        } else return x + from_int_scaled<FMT>(gv, 31 + tp->dither - 1);
    };

    /* The head word and the first two payload words of the NEXT opcode are requested from LDS as soon as
     * the current head is decoded, so their round trip overlaps the current opcode's work (nothing an
     * opcode stores can be another opcode's head or leading payload: STORE_MEM targets live in PARAM
     * sections, which are skipped).  The two words behind the last opcode are still inside the buffer. */
    int f0 = prog[pc], f1 = prog[pc + 1], f2 = prog[pc + 2];
    for (;;) {
        /* everything that steers control flow or addresses is made wave-uniform (SGPR): the switch then
         * compiles to scalar compares and branches instead of a per-case exec-mask waterfall */
        const unsigned head = (unsigned)__builtin_amdgcn_readfirstlane(f0);
        const int op = (int)(head >> 16);
        const unsigned skip = head & 0xFFFFu;
        int *ptr = prog + pc;                          /* opcode word: offsets into the program are relative to it */
        int *wp = ptr + 1;                             /* payload */
        const UniformWords w{wp, __builtin_amdgcn_readfirstlane(f1), __builtin_amdgcn_readfirstlane(f2)};
        f0 = ptr[skip]; f1 = ptr[skip + 1]; f2 = ptr[skip + 2];
        if (skip == 0 || op == DSP_CORE || op == DSP_END_OF_CODE || pc == a.end_word) break;        /* :321-331 */
        switch (op) {
        case DSP_NOP: case DSP_PARAM: case DSP_PARAM_NUM: case DSP_SERIAL: break;
        case DSP_SWAPXY: { const alu_t t = X; X = Y; Y = t; break; }
        case DSP_COPYXY: Y = X; break;
        case DSP_COPYYX: X = Y; break;
        case DSP_CLRXY:  X = 0; Y = 0; break;
        case DSP_ADDXY: if constexpr (AI) X = wadd(X, Y); else X = xy_add(X, Y); break;
        case DSP_ADDYX: if constexpr (AI) Y = wadd(Y, X); else Y = xy_add(Y, X); break;
        case DSP_SUBXY: if constexpr (AI) X = wsub(X, Y); else X = fsub(X, Y); break;
        case DSP_SUBYX: if constexpr (AI) Y = wsub(Y, X); else Y = fsub(Y, X); break;
        case DSP_NEGX:  if constexpr (AI) X = wsub(0, X); else X = -X; break;
        case DSP_NEGY:  if constexpr (AI) Y = wsub(0, Y); else Y = -Y; break;
        case DSP_MULXY: if constexpr (AI) X = wmul(X, Y); else X = xy_mul(X, Y); break;
        case DSP_DIVXY: if constexpr (AI) { if (Y != 0 && !(X == (long long)0x8000000000000000ull && Y == -1)) X /= Y; } else X = xy_div(X, Y); break;
        case DSP_DIVYX: if constexpr (AI) { if (X != 0 && !(Y == (long long)0x8000000000000000ull && X == -1)) Y /= X; } else Y = xy_div(Y, X); break;
        case DSP_AVGXY: if constexpr (AI) X = X / 2 + Y / 2; else X = xy_add(X / 2, Y / 2); break;
        case DSP_AVGYX: if constexpr (AI) Y = X / 2 + Y / 2; else Y = xy_add(Y / 2, X / 2); break;      /* two NaNs: the destination's wins (the build accumulates into Y) */
        case DSP_SHIFT: {                              /* :390-405 */
            const int s = w[0];
            if constexpr (AI) {
                if (s >= 0) X = (long long)((unsigned long long)X << ((s >= 100 ? 28 : s) & 63));
                else X = X >> ((s <= -100 ? 28 : -s) & 63);
            } else if constexpr (A64) X = shift_double(X, s);
            else X = shift_float(X, s);
            break; }
        case DSP_SQRTX:                                /* :438-461 */
            if constexpr (AI) {
                unsigned res = 0;
                if (X >> 32) { for (unsigned bit = 1u << 30; bit; bit >>= 1) { const unsigned t = res | bit; if (X >= (long long)((unsigned long long)t * t)) res = t; } }
                else { for (unsigned bit = 1u << 15; bit; bit >>= 1) { unsigned t = res | bit; t *= t; if (X >= (long long)t) res = t; } }
                X = res;
            } else X = (alu_t)sqrt((double)X);            /* cvtss2sd / sqrtsd / cvtsd2ss for the float ALU: FF's conversions flush */
            break;
        case DSP_SAT0DB: X = sat0db<FMT>(X); break;    /* :464-475 */
        case DSP_SAT0DB_TPDF: X = sat0db<FMT>(tpdf_add(X)); break;
        case DSP_SAT0DB_GAIN: case DSP_SAT0DB_TPDF_GAIN: {      /* :494-534 */
            const int *gp = ptr + w[0];
            if constexpr (AI) X = wmul(X >> 28, (long long)gp[0]);
            else X = fmul<FMT>(to_sp<FMT>(X), __int_as_float(gp[0]));
            if (op == DSP_SAT0DB_TPDF_GAIN) X = tpdf_add(X);
            X = sat0db<FMT>(X);
            break; }
        case DSP_TPDF_CALC: {                          /* :537-545; the generator is one sequence over the frames */
            const int dith = w[0]; int *res = rundata + w[1];
            if constexpr (WAVE) {
                /* the draws are data independent: every lane steps the generator through the batch (uniform
                 * work, registers only) and keeps the pair of its own frame.  A first frame that finds another
                 * dither width in the globals only installs the new one: no draw, X = 0 (dsp_tpdf.h:55-80). */
                const int want = dith ? dith : g->default_dither;
                const int first = (want == g->global.dither) ? 0 : 1;
                unsigned xs[4] = {g->xs[0], g->xs[1], g->xs[2], g->xs[3]};
                const alu_t before = ld_alu<FMT>(res);
                __syncthreads();
                if (first && lane == 0) tpdf_prepare<FMT>(g, &g->global, &g->global, dith);
                int r1 = 0, r2 = 0;
                for (int f = first; f < nb; f++) {
                    const int a1 = (int)xoshiro128p(xs), a2 = (int)xoshiro128p(xs);
                    if (lane == f) { r1 = a1; r2 = a2; }
                }
                alu_t kept = before;
                if (lane >= first) {
                    const int r = (r1 >> 1) + (r2 >> 1);
                    gv = r; gr = r2;
                    if constexpr (AI) X = r; else X = from_int_scaled<FMT>(r, 31);
                    kept = X;
                } else X = 0;
                if (lane == nb - 1) {
                    g->xs[0] = xs[0]; g->xs[1] = xs[1]; g->xs[2] = xs[2]; g->xs[3] = xs[3];
                    if (lane >= first) { g->value = gv; g->random = gr; st_alu<FMT>(res, X); }
                }
                vm_put(res, kept);
                if (a.tpdf_role == 1 && lane < nb) { int *q = wc.tpdf_seq + 2 * (wc.frame0 + lane); q[0] = gv; q[1] = gr; }
                __syncthreads();
            } else {
                if (tpdf_prepare<FMT>(g, &g->global, &g->global, dith)) {
                    const int r1 = (int)xoshiro128p(g->xs), r2 = (int)xoshiro128p(g->xs);
                    g->random = r2;
                    const int r = (r1 >> 1) + (r2 >> 1);
                    g->value = r;
                    if constexpr (AI) X = r; else X = from_int_scaled<FMT>(r, 31);
                    st_alu<FMT>(res, X);
                } else X = 0;
                gv = g->value; gr = g->random;
                if (a.tpdf_role == 1) { int *q = wc.tpdf_seq + 2 * wc.frame0; q[0] = gv; q[1] = gr; }
            }
            break; }
        case DSP_TPDF:                                 /* :547-562 */
            if (!tpdf_prepare<FMT>(g, tp, &local, w[0])) tp = &local;
            if constexpr (AI) X = gv; else X = from_int_scaled<FMT>(gv, 31);
            vm_store(rundata + w[1], X);
            break;
        case DSP_WHITE: if constexpr (AI) X = gr; else X = from_int_scaled<FMT>(gr, 31); break;
        case DSP_LOAD: {                               /* :565-583 */
            Y = X;
            const auto s = ld_smp(w[0]);
            if constexpr (AI) X = s;
            else if constexpr (SI) X = from_int_scaled<FMT>(s, 31);
            else X = to_alu<FMT>(s);
            break; }
        case DSP_LOAD_GAIN: {                          /* :586-607 */
            Y = X;
            const auto s = ld_smp(w[0]);
            const int *gp = ptr + w[1];
            if constexpr (AI) X = wmul((long long)s, (long long)gp[0]);
            else if constexpr (SI) X = fmul<FMT>(int_to_float_scaled(s, 31), __int_as_float(gp[0]));
            else { X = to_alu<FMT>(s); X *= to_alu<FMT>(__int_as_float(gp[0])); }
            break; }
        case DSP_STORE:                                /* :610-633 */
            if constexpr (AI) S(w[0]) = (unsigned)((int)X & tp->mask);
            else if constexpr (SI) {
                if constexpr (A64) S(w[0]) = (unsigned)(s31_from_double(X) & tp->mask);
                else S(w[0]) = (unsigned)(s31_from_float(X.v) & tp->mask);
            } else S(w[0]) = __float_as_uint(to_sp<FMT>(X));
            break;
        case DSP_LOAD_STORE: { unsigned n = skip - 1; int *q = wp; while (n >= 2) { S(q[1]) = S(q[0]); q += 2; n -= 2; } break; }   /* :738-747 */
        case DSP_GAIN: { const int *gp = ptr + w[0]; if constexpr (AI) X = wmul(X, (long long)gp[0]); else X *= to_alu<FMT>(__int_as_float(gp[0])); break; }
        case DSP_VALUE: Y = X; if constexpr (AI) X = ptr[w[0]]; else X = to_alu<FMT>(__int_as_float(ptr[w[0]])); break;
        case DSP_VALUE_INT: Y = X; X = to_alu_i(ptr[w[0]]); break;
        case DSP_MUL_VALUE: if constexpr (AI) X = wmul(X, (long long)w[0]); else X *= to_alu<FMT>(__int_as_float(w[0])); break;
        case DSP_DIV_VALUE:
            if constexpr (AI) { if (w[0] != 0 && !(X == (long long)0x8000000000000000ull && w[0] == -1)) X /= w[0]; }
            else X /= to_alu<FMT>(__int_as_float(w[0]));
            break;
        case DSP_MUL_VALUE_INT: if constexpr (AI) X = wmul(X, (long long)w[0]); else X *= w[0]; break;
        case DSP_DIV_VALUE_INT:
            if constexpr (AI) { if (w[0] != 0 && !(X == (long long)0x8000000000000000ull && w[0] == -1)) X /= w[0]; }
            else X /= w[0];
            break;
        case DSP_AND_VALUE_INT: if constexpr (AI) X &= (long long)w[0]; break;
        case DSP_DELAY_1: {
            Y = X; int *m = rundata + w[0];
            if constexpr (WAVE) {                       /* X[l] <- X[l-1], lane 0 <- the stored word, the last frame's X stays */
                unsigned *t = wc.vtmp;
                const alu_t old = ld_alu<FMT>(m);
                st_alu<FMT>((int *)t + lane * AW, X);
                __syncthreads();
                const alu_t prev = lane ? ld_alu<FMT>((int *)t + (lane - 1) * AW) : old;
                st_last(m, X);
                X = prev;
                __syncthreads();
            } else { const alu_t t = ld_alu<FMT>(m); st_alu<FMT>(m, X); X = t; }
            break; }
        case DSP_LOAD_MEM: Y = X; X = vm_load(ptr + w[0]); break;
        case DSP_STORE_MEM: vm_store(ptr + w[0], X); break;
        case DSP_LOAD_MEM_DATA: X = vm_load(rundata + w[0]); break;
        case DSP_DELAY: case DSP_DELAY_DP: {           /* :769-824 */
            const unsigned maxSize = (unsigned)w[0];
            int *d = rundata + w[1];
            const int usOff = w[2];
            unsigned n;
            if (usOff == 0) n = (unsigned)(((unsigned long long)maxSize * a.delay_factor) >> 32);
            else {
                const unsigned short us = (unsigned short)ptr[usOff];
                n = (unsigned)(((unsigned long long)us * a.delay_factor) >> 32);
                if (n > maxSize) n = maxSize;
            }
            n = (unsigned)__builtin_amdgcn_readfirstlane((int)n);
            if (n) {
                const int alloc = usOff ? (int)maxSize : (int)n;       /* words the encoder set aside for the line */
                auto one = [&] {
                    int index = state_index(d[0], alloc);
                    if (op == DSP_DELAY) { int *line = d + 1 + index; const sp_t v = ld_sp(line); if constexpr (AI) st_sp(line, (sp_t)X); else st_sp(line, to_sp<FMT>(X)); if constexpr (AI) X = v; else X = to_alu<FMT>(v); }
                    else { int *line = d + 1 + index * AW; const alu_t v = ld_alu<FMT>(line); st_alu<FMT>(line, X); X = v; }
                    index++;
                    if ((unsigned)index >= n) index = 0;
                    d[0] = index;
                };
                if constexpr (WAVE) {
                    const unsigned index = (unsigned)state_index(__builtin_amdgcn_readfirstlane(d[0]), alloc);
                    if (index >= n) serial(one);        /* a line shortened under a running index: frame by frame */
                    else {
                        /* frame l uses slot (index + l) mod n: it reads what the line held if this is the slot's
                         * first visit in the batch (l < n), else what frame l - n put there; the last visitor's
                         * word stays in the line */
                        const unsigned slot = (index + (unsigned)lane) % n;
                        unsigned *t = wc.vtmp;
                        if (op == DSP_DELAY) {
                            sp_t mine; if constexpr (AI) mine = (sp_t)X; else mine = to_sp<FMT>(X);
                            st_sp((int *)t + lane, mine);
                            __syncthreads();
                            int *line = d + 1 + slot;
                            const sp_t v = (unsigned)lane < n ? ld_sp(line) : ld_sp((int *)t + (lane - (int)n));
                            __syncthreads();
                            if (lane < nb && (unsigned)lane + n >= (unsigned)nb) st_sp(line, mine);
                            if constexpr (AI) X = v; else X = to_alu<FMT>(v);
                        } else {
                            st_alu<FMT>((int *)t + lane * AW, X);
                            __syncthreads();
                            int *line = d + 1 + slot * AW;
                            const alu_t v = (unsigned)lane < n ? ld_alu<FMT>(line) : ld_alu<FMT>((int *)t + (lane - (int)n) * AW);
                            __syncthreads();
                            if (lane < nb && (unsigned)lane + n >= (unsigned)nb) st_alu<FMT>(line, X);
                            X = v;
                        }
                        if (lane == 0) d[0] = (int)((index + (unsigned)nb) % n);
                        __syncthreads();
                    }
                } else one();
            }
            break; }
        case DSP_BIQUADS: {                            /* :827-849 */
            int *st = rundata + w[0];
            const int *bank = ptr + w[1];
            if (__builtin_amdgcn_readfirstlane(bank[1])) {
                const int num = (short)__builtin_amdgcn_readfirstlane(bank[0]);
                if constexpr (WAVE) X = wave_biquads<FMT>(X, bank + a.biquad_offset, st, num, a.biquad_skip, wc);
                else X = biquads<FMT>(X, bank + a.biquad_offset, st, num, a.biquad_skip);
            }
            break; }
        case DSP_LOAD_MUX: {                           /* :871-897 */
            const int *t = ptr + w[0];
            short n = (short)__builtin_amdgcn_readfirstlane(*t++);
            X = 0;
            while (n-- > 0) {
                const auto s = ld_smp(__builtin_amdgcn_readfirstlane(*t++));
                const int gw = *t++;
                if constexpr (AI) X = wadd(X, wmul((long long)s, (long long)gw));
                else if constexpr (SI) X = fmacc<FMT>(X, int_to_float_scaled(s, 31), __int_as_float(gw));
                else X = fmacc<FMT>(X, s, __int_as_float(gw));
            }
            vm_store(rundata + w[1], X);
            break; }
        case DSP_DATA_TABLE: {                         /* :900-923 */
            const int div = w[1], size = w[2];
            int *ip = rundata + w[3];
            const int *tab = ptr + w[4];
            const int gainw = w[0];
            auto value = [&](int raw) {
                if constexpr (AI) X = wmul((long long)raw, (long long)gainw);
                else if constexpr (SI) X = fmul<FMT>((float)raw, __int_as_float(gainw));
                else X = fmul<FMT>(__int_as_float(raw), __int_as_float(gainw));
            };
            auto one = [&] {
                int index = state_index(*ip, size);
                const int raw = tab[index];
                index += div;
                if (index >= size) index -= size;
                *ip = index;
                value(raw);
            };
            if constexpr (WAVE) {
                const int index0 = __builtin_amdgcn_readfirstlane(*ip);
                if (index0 < 0 || index0 >= size) serial(one);        /* a counter outside its table (foreign state): frame by frame */
                else {                                                 /* the host checked 0 <= div <= size: the counter is (index0 + f div) mod size */
                    __syncthreads();
                    const int mine = (int)(((long long)index0 + (long long)lane * div) % size);
                    value(tab[mine]);
                    if (lane == 0) *ip = (int)(((long long)index0 + (long long)nb * div) % size);
                    __syncthreads();
                }
            } else one();
            break; }
        case DSP_FIR: {                                /* :928-969; the int64 tap loop is refused by the host */
            const int off = w[a.freq_index];
            const int *after = wp + a.num_freq;
            if (off) {
                const int *imp = ptr + off;
                const int length = __builtin_amdgcn_readfirstlane(*imp++);
                int *st = rundata + __builtin_amdgcn_readfirstlane(after[0]);
                const int delay = length >> 16;
                if (delay) {
                    serial([&] {
                        int index = state_index((int)ld_sp(st), delay);
                        int *line = st + 1 + index;
                        const sp_t v = ld_sp(line);
                        if constexpr (AI) st_sp(line, (int)(X >> 28)); else st_sp(line, to_sp<FMT>(X));
                        if constexpr (AI) X = v; else X = to_alu<FMT>(v);
                        index++;
                        if (index >= delay) index = 0;
                        st_sp(st, (sp_t)index);
                    });
                } else if (length > 0) {
                    if constexpr (!AI) {
                        if constexpr (WAVE) X = wave_fir<FMT>(to_sp<FMT>(X), imp, st, length, wc);
                        else X = fir<FMT>(to_sp<FMT>(X), imp, st, length);
                    }
                }
            }
            break; }
        case DSP_RMS: {                                /* :972-1060 */
            unsigned *d = (unsigned *)(rundata + w[0]);
            const unsigned delay = (unsigned)w[1];
            const int *tab = wp + 2 + a.freq_index * 2;
            const unsigned maxCounter = (unsigned)__builtin_amdgcn_readfirstlane(tab[0]);
            const int factor = __builtin_amdgcn_readfirstlane(tab[1]);
            int *sumSq = (int *)(d + 5), *avgp = sumSq + AW, *ring = sumSq + 2 * AW;
            unsigned cnt = d[0], ridx = (unsigned)state_index((int)d[1], (int)delay), d2 = d[2], d3 = d[3], d4 = d[4];
            alu_t sum = ld_alu<FMT>(sumSq), avg = ld_alu<FMT>(avgp);
            turns_xy([&](alu_t &x, alu_t &y, int) {
                const unsigned counter = cnt + 1;
                if constexpr (AI) {
                    const int sx = (int)(((long long)(int)x * factor) >> 32);
                    const int sy = factor > 0 ? sx : (int)(((long long)(int)y * factor) >> 32);
                    x = wadd(sum, wmul((long long)sx, (long long)sy));
                } else { if (factor > 0) x *= x; else x = rmul(x, y); x = radd(x, sum); }
                if (counter >= maxCounter) {
                    if (delay) {                            /* the averaging line stays in the mirror: visited once per maxCounter frames */
                        int *line = ring + (int)ridx * AW;
                        const alu_t old = ld_alu<FMT>(line);
                        st_alu<FMT>(line, x);
                        /* float models: X + (avg - old), the order the reference's -Ofast build evaluates (source: X -= old; X += avg) */
                        if constexpr (AI) x = wadd(wsub(x, old), avg); else x = radd(x, fsub(avg, old));
                        ridx++;
                        if (ridx >= delay) ridx = 0;
                    }
                    avg = x;
                    cnt = 0;
                    sum = (alu_t)0;
                    x = (alu_t)d2;
                } else {
                    sum = x;
                    cnt = counter;
                    if constexpr (AI) {
                        if (counter == 1) { d4 = 1u << 30; d3 = 0; x = d2; }
                        else {
                            const unsigned bit = d4;
                            if (bit) { const unsigned t = d3 | bit; if (avg >= (long long)((unsigned long long)t * t)) d3 = t; d4 = bit >> 1; x = d2; }
                            else { x = d3; d2 = (unsigned)x; }
                        }
                    } else x = (alu_t)sqrt((double)avg);
                }
            });
            uniform_store([&] {
                d[0] = cnt; d[1] = ridx;
                if constexpr (AI) { d[2] = d2; d[3] = d3; d[4] = d4; }
                st_alu<FMT>(sumSq, sum); st_alu<FMT>(avgp, avg);
            });
            break; }
        case DSP_DCBLOCK: {                            /* :1063-1095 */
            int *accp = rundata + w[0], *dp = accp + AW;
            const int polew = w[1 + a.freq_index];
            alu_t acc = ld_alu<FMT>(accp);
            int px = dp[0], py = dp[1];
            turns_x([&](alu_t &x, alu_t &, int) {
                if constexpr (AI) {
                    int xn = (int)(x >> 28);
                    const int before = px;
                    px = xn;
                    xn = (int)((unsigned)xn - (unsigned)before);
                    x = acc;
                    x = wadd(x, wmul((long long)xn, 1ll << 28));
                    x = wadd(x, wmul((long long)py, (long long)polew));
                    acc = x;
                    py = (int)(x >> 28);
                } else {
                    const float xn = to_sp<FMT>(x);
                    const float before = __int_as_float(px);
                    px = __float_as_int(xn);
                    x = acc;
                    const float yb = to_sp<FMT>(x);
                    /* float accumulator: (acc + xn) - px is what the reference's -Ofast build evaluates for
                     * the source's acc + (xn - px); its binaries are the parity target (DESIGN.md, quirks) */
                    /* (when the accumulator and the sample are both NaN the build's addss has the sample first) */
                    if constexpr (A64) x = radd(x, up64(fsub(FF(xn), FF(before)).v)); else x = fsub(FF(xn) + x, FF(before));
                    x = fmacc<FMT>(x, yb, __int_as_float(polew));
                    acc = x;
                }
            });
            uniform_store([&] { st_alu<FMT>(accp, acc); dp[0] = px; if constexpr (AI) dp[1] = py; });
            break; }
        case DSP_DITHER: {                             /* :1112-1136 */
            int *e = rundata + w[0];
            alu_t e0 = ld_alu<FMT>(e), e1 = ld_alu<FMT>(e + AW), e2 = ld_alu<FMT>(e + 2 * AW);
            turns_x([&](alu_t &x, alu_t &, int v) {
                alu_t t0 = e0;
                const alu_t t1 = e1, t2 = e2;
                if constexpr (AI) { x = wadd(x, t0); t0 >>= 1; x = wadd(wsub(x, t1), t2); }
                else { x = radd(x, t0); if constexpr (A64) t0 = shift_double(t0, -1); else t0 = shift_float(t0, -1); x = fsub(x, t1); x = radd(x, t2); }
                e1 = t0;
                e2 = t1;
                const alu_t s = x;
                x = tpdf_truncate<FMT>(tpdf_add_v(x, v), tp);
                if constexpr (AI) e0 = wsub(s, x); else e0 = fsub(s, x);
            });
            uniform_store([&] { st_alu<FMT>(e, e0); st_alu<FMT>(e + AW, e1); st_alu<FMT>(e + 2 * AW, e2); });
            break; }
        case DSP_DITHER_NS2: {                         /* :1138-1171 */
            int *e = rundata + w[0];
            const int *tab = ptr + w[1] + a.freq_index * 3;
            const int c0 = tab[0], c1 = tab[1], c2 = tab[2];
            sp_t e0 = ld_sp(e), e1 = ld_sp(e + 1), e2 = ld_sp(e + 2);
            turns_x([&](alu_t &x, alu_t &, int v) {
                if constexpr (AI) {
                    x = wadd(x, wmul((long long)e0, (long long)c0));
                    x = wadd(x, wmul((long long)e1, (long long)c1));
                    x = wadd(x, wmul((long long)e2, (long long)c2));
                } else {
                    x = fmacc<FMT>(x, e0, __int_as_float(c0));
                    x = fmacc<FMT>(x, e1, __int_as_float(c1));
                    x = fmacc<FMT>(x, e2, __int_as_float(c2));
                }
                e2 = e1;
                e1 = e0;
                const alu_t s = x;
                x = tpdf_truncate<FMT>(tpdf_add_v(x, v), tp);
                if constexpr (AI) e0 = (int)(wsub(s, x) >> 28); else e0 = to_sp<FMT>(fsub(s, x));
            });
            uniform_store([&] { st_sp(e, e0); st_sp(e + 1, e1); st_sp(e + 2, e2); });
            break; }
        case DSP_DISTRIB: {                            /* :1175-1210; the histogram stays in the mirror */
            const int io = w[0], size = w[1];
            int *d = rundata + w[2];
            int *bins = d + 1;
            const int middle = size >> 1;
            int index = state_index(d[0], size);
            int shown = 0;                              /* what this lane's frame puts into samples[io] */
            auto one = [&](alu_t x) -> int {
                sp_t s;
                if constexpr (AI) s = (sp_t)x; else s = to_sp<FMT>(x);
                if (s != 0) {
                    int pos;
                    if constexpr (AI) pos = (int)(((long long)s * size) >> 32);
                    else {
                        /* the reference's cvttss2si: NaN and anything outside int range convert to INT_MIN (v_cvt_i32_f32 gives 0 / saturates) */
                        const auto p = s * middle;
                        pos = (p > -2147483648.0f && p < 2147483648.0f) ? (int)p : (int)0x80000000u;
                    }
                    pos = (int)((unsigned)pos + (unsigned)middle);
                    if (pos >= 0 && pos < size) bins[pos]++;
                }
                int value = bins[index];
                if (value == 0) value = index ? bins[index - 1] : bins[1];
                index++;
                if (index >= size) index = 0;
                return value;
            };
            if constexpr (WAVE) {
                for (int f = 0; f < nb; f++) { const int value = one(lane_of(X, f)); if (lane == f) shown = value; }
            } else shown = one(X);
            uniform_store([&] { d[0] = index; });
            if constexpr (SI) S(io) = (unsigned)shown; else S(io) = __float_as_uint(int_to_float_scaled(shown, 31));
            break; }
        case DSP_DIRAC: case DSP_SQUAREWAVE: {         /* :1213-1261, float models (int models refused by the host) */
            int *d = rundata + w[0];
            const int maxCount = w[2 + a.freq_index], ampw = w[1];
            auto value = [&](int counter) {
                if constexpr (!AI) {
                    if (op == DSP_DIRAC) { if (counter == 0) X = __int_as_float(ampw); }
                    else X = fmul<FMT>(counter <= maxCount / 2 ? 0.5f : -0.5f, __int_as_float(ampw));
                }
            };
            auto one = [&] {
                int counter = *d;
                value(counter);
                counter++;
                if (counter >= maxCount) counter = 0;
                *d = counter;
            };
            if constexpr (WAVE) {
                const int c0 = __builtin_amdgcn_readfirstlane(*d);
                if (maxCount < 1 || c0 < 0 || c0 >= maxCount) serial(one);      /* no plain modulo sequence: frame by frame */
                else {
                    __syncthreads();
                    value((int)(((long long)c0 + lane) % maxCount));
                    if (lane == 0) *d = (int)(((long long)c0 + nb) % maxCount);
                    __syncthreads();
                }
            } else one();
            break; }
        case DSP_CLIP: {                               /* :1264-1274 */
            alu_t thr;
            if constexpr (AI) thr = (long long)((unsigned long long)(1u << 31) * (unsigned long long)(unsigned)w[0]);
            else thr = to_alu<FMT>(__int_as_float(w[0]));
            if constexpr (AI) { if (X > thr) X = thr; else if (X < -thr) X = -thr; }
            else {      /* max then min, NaN -> -threshold: the reference's -Ofast build (maxsd, minsd); see the oracle */
                X = (X > -thr) ? X : -thr;
                X = (X < thr) ? X : thr;
            }
            break; }
        case DSP_SINE: {                               /* :1284-1305 after the compile fix, float models */
            int *d = rundata + w[0];
            if constexpr (!AI) {
                const float gn = __int_as_float(w[1]), eps = __int_as_float(w[2 + a.freq_index]);
                alu_t sx = ld_alu<FMT>(d), sy = ld_alu<FMT>(d + AW);
                turns_xy([&](alu_t &x, alu_t &y, int) {
                    x = sx;
                    y = (x == 0) ? to_alu<FMT>(gn) : sy;
                    x = radd(x, to_alu<FMT>(-eps) * y);
                    y = radd(y, to_alu<FMT>(eps) * x);
                    sy = y;
                    sx = x;
                });
                uniform_store([&] { st_alu<FMT>(d + AW, sy); st_alu<FMT>(d, sx); });
            }
            break; }
        default: break;
        }
        pc += (int)skip;
        if (pc == a.skip_from) {                       /* (0 = none: no opcode sits at word 0) */
            pc = a.skip_to;
            f0 = prog[pc]; f1 = prog[pc + 1]; f2 = prog[pc + 2];
        }
    }
}

template <int FMT>
__device__ __forceinline__ void run_frame(const GenericArgs &a, int *prog, unsigned *samp, TpdfGlobals *g, int frame)
{
    WaveCtx wc{};
    wc.frame0 = frame;
    wc.tpdf_seq = a.tpdf_seq;
    run<FMT, false>(a, prog, samp, g, wc);
}

#pragma clang fp contract(fast)

}  // namespace interp

/* One workgroup of one wave per core.  The mirror (program + state, usually a few thousand words) and
 * the scratch frame are staged in LDS for the whole block, so the per-opcode pointer chasing of the
 * interpreter costs LDS latency instead of HBM latency; everything the core may have written goes back
 * at the end.  Lane 0 interprets, the wave moves the frames.                                        */
template <int FMT, bool STAGED>
__global__ __launch_bounds__(64) void interp_core(const GenericArgs a)
{
#if AVDSP_INTERP_HW_FLUSH
    if constexpr (FMT != 2) flush_f32_subnormals_like_the_reference();
#endif
    extern __shared__ unsigned lds_words[];
    __shared__ TpdfGlobals tg;
    const int lane = threadIdx.x;
    unsigned *samp;
    int *prog;
    if constexpr (STAGED) {                                  /* frame and mirror both live in LDS for the block */
        samp = lds_words;
        prog = (int *)(lds_words + a.frame_lds);
        for (int k = lane; k < a.stage_words; k += 64) prog[k] = a.buf[k];
        for (int k = lane; k < a.scratch_len; k += 64) samp[k] = a.scratch[k];
    } else {
        samp = a.scratch;
        prog = a.buf;
    }
    if (lane == 0) tg = *a.tpdf;
    __syncthreads();
    /* frames move between HBM and LDS in batches (one HBM round trip per batch instead of two per frame) */
    unsigned *inb = lds_words + a.batch_lds, *outb = inb + a.batch_frames * a.io.in_stride;
    for (int n0 = 0; n0 < a.io.nframes; n0 += a.batch_frames) {
        const int nb = min(a.batch_frames, a.io.nframes - n0);
        for (int k = lane; k < nb * a.io.in_stride; k += 64) inb[k] = a.io.in[(size_t)n0 * a.io.in_stride + k];
        for (int k = lane; k < nb * a.io.out_stride; k += 64) outb[k] = a.io.out[(size_t)n0 * a.io.out_stride + k];
        __syncthreads();
        for (int j = 0; j < nb; j++) {
            /* samples[] for this frame: the output window keeps whatever the caller's buffer holds (slots the
             * core never stores stay as they were), then the input window is laid over it
             * (linux/avdsp_plugin.c:100-123) */
            for (int k = lane; k < a.io.out_stride; k += 64) samp[a.io.out_base + k] = outb[j * a.io.out_stride + k];
            __syncthreads();
            for (int k = lane; k < a.io.in_stride; k += 64) samp[a.io.in_base + k] = inb[j * a.io.in_stride + k];
            __syncthreads();
            if (lane == 0) interp::run_frame<FMT>(a, prog, samp, &tg, n0 + j);
            __syncthreads();
            for (int k = lane; k < a.io.out_stride; k += 64) outb[j * a.io.out_stride + k] = samp[a.io.out_base + k];
            __syncthreads();
        }
        if (a.rows_whole) { for (int k = lane; k < nb * a.io.out_stride; k += 64) a.io.out[(size_t)n0 * a.io.out_stride + k] = outb[k]; }
        else {      /* only the slots this core stores: another core may be delivering its own into the same rows */
            for (int k = lane; k < nb * a.io.out_stride; k += 64) {
                const int sl = a.io.out_base + k % a.io.out_stride;
                if (sl < 256 && (a.written_io[sl >> 5] >> (sl & 31) & 1u)) a.io.out[(size_t)n0 * a.io.out_stride + k] = outb[k];
            }
        }
        __syncthreads();
    }
    if constexpr (STAGED) {
        write_back_owned(a, a.buf, prog, lane);
        if (a.nown < 0) { for (int k = lane; k < a.scratch_len; k += 64) a.scratch[k] = samp[k]; }
        else for (int k = lane; k < 256 && k < a.scratch_len; k += 64) if (a.written_io[k >> 5] >> (k & 31) & 1u) a.scratch[k] = samp[k];
    }
    if (lane == 0 && (a.tpdf_owner || a.nown < 0)) *a.tpdf = tg;
    if (a.done_flag) {                                       /* (one wave: every lane's stores are behind the barrier, lane 0's release covers the wave's) */
        __syncthreads();
        if (lane == 0) __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

/* The frame-parallel form: one wave per core, lane l interprets frame l of each batch of 64 frames
 * (interp::run<FMT, true>).  LDS = [frame slots x 64 lanes][mirror][exchange vectors][per-lane memories]
 * [sequence buffer]; the host has checked that the core carries nothing from frame to frame outside
 * opcode-private state and that all of this fits.                                                      */
/* The HBM pointers of a launch, by value: a pointer that arrives as (part of) a kernel argument is known to point into HBM; one
 * loaded from a table in memory is not, and every access through it becomes a FLAT instruction -- one that may touch LDS, so the
 * compiler also waits for ALL memory and LDS traffic wherever any of it is used.  The grid kernels say what their table's pointers
 * are (in_hbm) and hand them on in registers; the table entry itself is read in place (a local copy of it lives in scratch memory:
 * its arrays are indexed at run time). */
struct WaveRoots { int *buf; TpdfGlobals *tpdf; unsigned *scratch; int *tpdf_seq; const unsigned *in; unsigned *out; };
template <class T> __device__ __forceinline__ T *in_hbm(T *p)
{   /* (through an integer: a cast pair generic -> global -> generic is folded away before it can tell anybody anything) */
    return (T *)(__attribute__((address_space(1))) T *)(unsigned long long)p;
}
__device__ __forceinline__ WaveRoots roots_of(const GenericArgs &a) { return WaveRoots{a.buf, a.tpdf, a.scratch, a.tpdf_seq, a.io.in, a.io.out}; }
__device__ __forceinline__ WaveRoots roots_in_hbm(const WaveRoots &r) { return WaveRoots{in_hbm(r.buf), in_hbm(r.tpdf), in_hbm(r.scratch), in_hbm(r.tpdf_seq), in_hbm(r.in), in_hbm(r.out)}; }

template <int FMT>
__device__ __forceinline__ void interp_wave_body(const GenericArgs &a, const WaveRoots r)
{
#if AVDSP_INTERP_HW_FLUSH
    if constexpr (FMT != 2) flush_f32_subnormals_like_the_reference();
#endif
    extern __shared__ unsigned lds_words[];
    __shared__ TpdfGlobals tg;
    const int lane = threadIdx.x;
    unsigned *samp = lds_words;
    int *prog = (int *)(lds_words + a.frame_lds);
    interp::WaveCtx wc;
    wc.lane = lane;
    wc.vtmp = lds_words + a.batch_lds;
    wc.vmem = wc.vtmp + 128;
    wc.vseq = wc.vmem + a.nvm * 128;
    wc.vm_word = a.vm_word; wc.nvm = a.nvm;
    wc.tpdf_seq = r.tpdf_seq;
    for (int k = lane; k < a.stage_words; k += 64) prog[k] = r.buf[k];
    /* every frame starts from the persistent frame: fetched once (coalesced, parked in the sequence buffer),
     * then spread over the lanes */
    for (int k = lane; k < a.wave_span; k += 64) wc.vseq[k] = r.scratch[k];
    if (lane == 0) tg = *r.tpdf;
    __syncthreads();
    for (int k = 0; k < a.wave_span; k++) samp[k * interp::kLanePitch + lane] = wc.vseq[k];
    __syncthreads();
    /* rows of the caller's blocks <-> slot columns.  Lane l moves frame l's row: with one wave the instruction
     * count is what matters, not coalescing.  Normally only the slots the core reads before storing them are
     * fetched and only the slots it stores are delivered (lists from the host's scan); with too many of them the
     * whole windows move, as 16-byte accesses where their layout allows. */
    const bool lists = !a.rows_whole;
    const bool wide_out = (a.io.out_stride & 3) == 0 && ((size_t)r.out & 15) == 0;
    const bool wide_in = (a.io.in_stride & 3) == 0 && ((size_t)r.in & 15) == 0;
    auto row_in = [&](const unsigned *row, int base, int stride, bool wide) {
        unsigned *col = samp + base * interp::kLanePitch + lane;
        if (wide) {
            for (int k = 0; k < stride; k += 4) {
                const uint4 v = *(const uint4 *)(row + k);
                col[(k + 0) * interp::kLanePitch] = v.x; col[(k + 1) * interp::kLanePitch] = v.y;
                col[(k + 2) * interp::kLanePitch] = v.z; col[(k + 3) * interp::kLanePitch] = v.w;
            }
        } else for (int k = 0; k < stride; k++) col[k * interp::kLanePitch] = row[k];
    };
    int last = 0;
    for (int n0 = 0; n0 < a.io.nframes; n0 += 64) {
        const int nb = min(64, a.io.nframes - n0);
        wc.nb = nb; wc.frame0 = n0; last = nb - 1;
        if (lane < nb) {
            /* output window first (slots the core never stores keep the caller's words), the input window
             * laid over it (linux/avdsp_plugin.c:100-123) */
            const unsigned *orow = r.out + (size_t)(n0 + lane) * a.io.out_stride;
            const unsigned *irow = r.in + (size_t)(n0 + lane) * a.io.in_stride;
            if (lists) {
                for (int i = 0; i < a.nrd_slot; i++) {
                    const int sl = a.rd_slot[i];
                    if (sl >= a.io.in_base && sl < a.io.in_base + a.io.in_stride) samp[sl * interp::kLanePitch + lane] = irow[sl - a.io.in_base];
                    else if (sl >= a.io.out_base && sl < a.io.out_base + a.io.out_stride) samp[sl * interp::kLanePitch + lane] = orow[sl - a.io.out_base];
                }
            } else {
                row_in(orow, a.io.out_base, a.io.out_stride, wide_out);
                row_in(irow, a.io.in_base, a.io.in_stride, wide_in);
            }
        }
        __syncthreads();
        interp::run<FMT, true>(a, prog, samp, &tg, wc);
        __syncthreads();
        if (lane < nb) {
            unsigned *row = r.out + (size_t)(n0 + lane) * a.io.out_stride;
            const unsigned *col = samp + a.io.out_base * interp::kLanePitch + lane;
            if (lists) {
                for (int i = 0; i < a.nwr_slot; i++) {
                    const int sl = a.wr_slot[i];
                    if (sl >= a.io.out_base && sl < a.io.out_base + a.io.out_stride) row[sl - a.io.out_base] = samp[sl * interp::kLanePitch + lane];
                }
            } else if (wide_out) {
                for (int k = 0; k < a.io.out_stride; k += 4)
                    *(uint4 *)(row + k) = make_uint4(col[(k + 0) * interp::kLanePitch], col[(k + 1) * interp::kLanePitch],
                                                     col[(k + 2) * interp::kLanePitch], col[(k + 3) * interp::kLanePitch]);
            } else for (int k = 0; k < a.io.out_stride; k++) row[k] = col[k * interp::kLanePitch];
        }
    }
    __syncthreads();
    write_back_owned(a, r.buf, prog, lane);
    /* the last frame's samples[] persist: what the core stored (everything, if the host could not tell) */
    if (a.nown < 0) { for (int k = lane; k < a.wave_span; k += 64) r.scratch[k] = samp[k * interp::kLanePitch + last]; }
    else for (int k = lane; k < a.wave_span; k += 64) if (a.written_io[k >> 5] >> (k & 31) & 1u) r.scratch[k] = samp[k * interp::kLanePitch + last];
    if (lane == 0 && (a.tpdf_owner || a.nown < 0)) *r.tpdf = tg;
}

template <int FMT>
__global__ __launch_bounds__(64) void interp_wave(const GenericArgs a) { interp_wave_body<FMT>(a, roots_of(a)); }

/* Several cores (or strand groups of cores) that do not meet, in one launch: workgroup b runs table[b].  The
 * hardware queues behind HIP streams are few (four by default); a level with more pieces than that would
 * queue up behind itself on side streams, one grid does not. */
template <int FMT>
__global__ __launch_bounds__(64) void interp_wave_grid(const GenericArgs *__restrict__ table)
{
    const GenericArgs &a = table[blockIdx.x];
    interp_wave_body<FMT>(a, roots_in_hbm(roots_of(a)));
}

/* The same grid for N INSTANCES of the program at once (dspRuntimeSetInstances): instance i is a copy of the whole device state --
 * mirror (program words + data area), dither globals, samples[] frame, per-frame dither pairs -- with sample blocks of its own;
 * workgroup b runs piece b % n of instance b / n.  A program of two channels cannot fill a GPU; a thousand of them can. */
struct InstanceStrides {
    int n;                                              /* pieces of the level */
    int *buf; size_t buf_words;                         /* instances 1 ..: mirror copies, buf_words apart */
    TpdfGlobals *tpdf;
    unsigned *scratch; size_t frame_words;
    int *tpdf_seq; size_t seq_words;
    size_t in_words, out_words;                         /* instance i's sample blocks: io.in + i * in_words, io.out + i * out_words */
};
template <int FMT>
__global__ __launch_bounds__(64) void interp_wave_instances(const GenericArgs *__restrict__ table, const InstanceStrides st)
{
    const int inst = blockIdx.x / st.n;
    const GenericArgs &a = table[blockIdx.x - inst * st.n];
    WaveRoots r = roots_of(a);
    if (inst) {
        const size_t k = (size_t)(inst - 1);
        r.buf = st.buf + k * st.buf_words;
        r.tpdf = st.tpdf + k;
        r.scratch = st.scratch + k * st.frame_words;
        if (r.tpdf_seq) r.tpdf_seq = st.tpdf_seq + k * st.seq_words;
    }
    r.in += (size_t)inst * st.in_words;
    r.out += (size_t)inst * st.out_words;
    interp_wave_body<FMT>(a, roots_in_hbm(r));
}

/* ------------------------------------------------------------------------------------------
 * strand_lanes<FMT>: lane = strand (include/avdsp_hip.h, strand plans).  Every lane runs the same micro-operations on its own
 * operands, F frames at a time: X and Y of the F frames live in registers, an operation is dispatched once per batch (uniform
 * control) and applied to the F frames, opcodes with state (BIQUADS section by section, DELAY) load it once per batch and walk the
 * frames in order.  The arithmetic is the interpreter's own (the same functions, dsp_runtime.c:337-969 restated above), so the
 * results are the interpreter's, which the reference's goldens pin.
 * Frame slots: a LOAD of an IO inside the call's input window reads the block, of any other IO the program's persistent samples[]
 * frame (nobody in the stretch stores it: the host checked); a STORE goes to the output window's column and, for the block's last
 * frame, into the persistent frame (what the interpreter leaves there).
 * ---------------------------------------------------------------------------------------- */
struct StrandArgs {
    int *buf; const TpdfGlobals *tpdf; const int *tpdf_seq; int tpdf_role;
    const avdsp_strand_op *ops; int nops; const int *args; int nargs, nstrands, nres;
    int prog_words, biquad_skip, biquad_offset; unsigned delay_factor;
    unsigned *scratch;
    BlockIO io;
#ifdef AVDSP_BQ_STAMPS
    unsigned long long *stamps;
#endif
};
#ifdef AVDSP_BQ_STAMPS
#define STRAND_STAMP(k) do { if (F > 1 && blockIdx.x == 0 && n0 == 8 * F && (k) < 32) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) a.stamps[k] = t_; } } while (0)
#else
#define STRAND_STAMP(k) do { } while (0)
#endif

/* The per-lane table (LDS, column c of lane l at tab[c * 64 + l]): what an operation needs that does not change during the block
 * -- IO numbers, gains, coefficients, a memory word's value, a delay line's length -- is fetched ONCE per launch (the chain of
 * loads argument row -> parameter word would otherwise sit in front of every operation of every batch), and the state that runs
 * through the block -- biquad sections, delay-line counters -- lives there between the batches and goes back at the end. */
template <int FMT>
__device__ __forceinline__ void strand_resolve(const StrandArgs &a, const int *ar, int *tab, int lane)
{
    using namespace interp;
    constexpr int AW = M<FMT>::alu64 ? 2 : 1;
    for (int i = 0; i < a.nops; i++) {
        const avdsp_strand_op o = a.ops[i];
        int *t = tab + o.rcol * 64 + lane;
        switch (__builtin_amdgcn_readfirstlane(o.op)) {
        case AVDSP_SOP_LOAD: case AVDSP_SOP_STORE: case AVDSP_SOP_SHIFT: case AVDSP_SOP_STORE_MEM: t[0] = ar[o.a0]; break;
        case AVDSP_SOP_LOAD_GAIN: t[0] = ar[o.a0]; t[64] = a.buf[ar[o.a1]]; break;
        case AVDSP_SOP_GAIN: case AVDSP_SOP_SAT0DB_GAIN: case AVDSP_SOP_SAT0DB_TPDF_GAIN: t[0] = a.buf[ar[o.a0]]; break;
        case AVDSP_SOP_LOAD_MEM: { const int *p = a.buf + ar[o.a0]; for (int k = 0; k < AW; k++) t[64 * k] = p[k]; break; }
        case AVDSP_SOP_DELAY: case AVDSP_SOP_DELAY_DP: {      /* dsp_runtime.c:769-790 */
            const unsigned maxSize = (unsigned)ar[o.a0];
            const int dw = ar[o.a1], usw = ar[o.a2];
            unsigned n;
            if (usw == 0) n = (unsigned)(((unsigned long long)maxSize * a.delay_factor) >> 32);
            else {
                const unsigned short us = (unsigned short)a.buf[usw];
                n = (unsigned)(((unsigned long long)us * a.delay_factor) >> 32);
                if (n > maxSize) n = maxSize;
            }
            const int alloc = usw ? (int)maxSize : (int)n;
            t[0] = (int)n; t[64] = alloc; t[128] = dw; t[192] = n ? state_index(a.buf[dw], alloc) : 0;
            break; }
        case AVDSP_SOP_BIQUADS: {
            const int sw = ar[o.a0];
            const int *bank = a.buf + ar[o.a1];
            const int num = __builtin_amdgcn_readfirstlane(o.imm);
            t[0] = bank[1]; t[64] = sw;
            const int *coef = bank + a.biquad_offset, *st = a.buf + sw;
            for (int sct = 0; sct < num; sct++) {
                int *q = t + 64 * (2 + 11 * sct);
                for (int k = 0; k < 5; k++) q[64 * k] = coef[k];
                for (int k = 0; k < 6; k++) q[64 * (5 + k)] = st[k];
                coef += a.biquad_skip; st += 6;
            }
            break; }
        default: break;
        }
    }
}

template <int FMT>
__device__ __forceinline__ void strand_write_back(const StrandArgs &a, const int *tab, int lane)
{
    for (int i = 0; i < a.nops; i++) {
        const avdsp_strand_op o = a.ops[i];
        const int *t = tab + o.rcol * 64 + lane;
        const int op = __builtin_amdgcn_readfirstlane(o.op);
        if (op == AVDSP_SOP_DELAY || op == AVDSP_SOP_DELAY_DP) { if (t[0]) a.buf[t[128]] = t[192]; }
        else if (op == AVDSP_SOP_BIQUADS) {
            if (t[0]) {
                int *st = a.buf + t[64];
                const int num = __builtin_amdgcn_readfirstlane(o.imm);
                for (int sct = 0; sct < num; sct++) {
                    const int *q = t + 64 * (2 + 11 * sct + 5);
                    for (int k = 0; k < 6; k++) st[k] = q[64 * k];
                    st += 6;
                }
            }
        }
    }
}

/* the frames of a batch are compile-time indices from the first pass on: X[f] / Y[f] then become 2F separate registers
 * (an array indexed by a loop counter is turned into one 2F-register vector before the loop is unrolled, and every
 * partial update of it into a copy of the lot) */
template <class Fn, int... Is>
__device__ __forceinline__ void strand_frames_impl(Fn &&fn, std::integer_sequence<int, Is...>) { (fn(std::integral_constant<int, Is>{}), ...); }
#define STRAND_FRAMES(f, ...) \
    strand_frames_impl([&](auto f##_c) __attribute__((always_inline)) { constexpr int f = decltype(f##_c)::value; (void)f; __VA_ARGS__ }, \
                       std::make_integer_sequence<int, F>{})

/* what SAT0DB_TPDF adds for a dither value (dsp_tpdf.h:133-156) */
template <int FMT>
__device__ __forceinline__ typename interp::M<FMT>::alu strand_dither(int gv, const TpdfLocal &tp)
{
    using namespace interp;
    typename M<FMT>::alu d;
    if constexpr (M<FMT>::alu_int) {
        long long t = gv;
        d = tp.shift >= 0 ? (long long)((unsigned long long)t << (tp.shift & 63)) : (t >> ((-tp.shift) & 63));
    } else d = from_int_scaled<FMT>(gv, 31 + tp.dither - 1);
    int w[2] = {0, 0};
    st_alu<FMT>(w, d);
    asm volatile("" : "+v"(w[0]), "+v"(w[1]));             /* (worked out here, not in front of every use) */
    return ld_alu<FMT>(w);
}

template <int FMT, int F, bool USEY>
__device__ __forceinline__ void strand_batch(const StrandArgs &a, int *tab, int *xch, const int *lops, int lane, int n0, bool last_batch,
                                             typename interp::M<FMT>::alu (&X)[F], typename interp::M<FMT>::alu (&Y)[F], const TpdfLocal &tp, typename interp::M<FMT>::alu dconst)
{
    using namespace interp;
    using alu_t = typename M<FMT>::alu;
    using sp_t = typename M<FMT>::sp;
    constexpr bool AI = M<FMT>::alu_int, A64 = M<FMT>::alu64, SI = M<FMT>::smp_int;
    constexpr bool WIDE = A64 && !AI;
    constexpr int AW = A64 ? 2 : 1;
    /* this frame's dither value: published per frame by the piece that holds the core's TPDF_CALC, else the program's current one.
     * One fetch for the batch (lane f takes frame f's), and what SAT0DB_TPDF adds (dsp_tpdf.h:133-156) worked out here, once per
     * frame and batch: the value is uniform, so its special cases would be scalar branches in front of every use */
    alu_t dv[F];
    if (a.tpdf_role == 2) {
        int *gl = xch + 2 * 16 * 64;                          /* 16 words between the exchange area and the operation list */
        const int nact = min(64, a.nstrands - (int)blockIdx.x * 64);           /* the wave's lanes 0 .. nact-1 are at work */
        for (int k = lane; k < F; k += nact) gl[k] = a.tpdf_seq[2 * (n0 + k)];
        STRAND_FRAMES(f, dv[f] = strand_dither<FMT>(__builtin_amdgcn_readfirstlane(gl[f]), tp););
    } else { STRAND_FRAMES(f, dv[f] = dconst;); }
    auto tpdf_add = [&](alu_t x, alu_t d) -> alu_t { if constexpr (AI) return wadd(x, d); else return x + d; };
    for (int i = 0; i < a.nops; i++) {
        STRAND_STAMP(i);
        /* (the operation list sits in LDS: a global fetch per operation would cost a round trip each, longer than most operations) */
        const int *ow = lops + i * (int)(sizeof(avdsp_strand_op) / 4);
        avdsp_strand_op o;
        o.op = __builtin_amdgcn_readfirstlane(ow[0]); o.imm = __builtin_amdgcn_readfirstlane(ow[4]); o.rcol = __builtin_amdgcn_readfirstlane(ow[5]);
        const int op = o.op;
        int *t = tab + o.rcol * 64 + lane;
        switch (op) {
        case AVDSP_SOP_LOAD: case AVDSP_SOP_LOAD_GAIN: {      /* dsp_runtime.c:565-607 */
            const int io = t[0];
            const bool inwin = io >= a.io.in_base && io < a.io.in_base + a.io.in_stride;
            const unsigned *src = inwin ? a.io.in + (size_t)n0 * a.io.in_stride + (io - a.io.in_base) : a.scratch + io;
            const size_t step = inwin ? (size_t)a.io.in_stride : 0;
            int gw = 0;
            if (op == AVDSP_SOP_LOAD_GAIN) gw = t[64];
            unsigned raw[F];
            STRAND_FRAMES(f, raw[f] = src[f * step];);
            if (op == AVDSP_SOP_LOAD) {
                STRAND_FRAMES(f,
                    if constexpr (USEY) Y[f] = X[f];
                    if constexpr (AI) X[f] = (int)raw[f];
                    else if constexpr (SI) X[f] = from_int_scaled<FMT>((int)raw[f], 31);
                    else X[f] = to_alu<FMT>(__uint_as_float(raw[f])););
            } else {
                STRAND_FRAMES(f,
                    if constexpr (USEY) Y[f] = X[f];
                    if constexpr (AI) X[f] = wmul((long long)(int)raw[f], (long long)gw);
                    else if constexpr (SI) X[f] = fmul<FMT>(int_to_float_scaled((int)raw[f], 31), __int_as_float(gw));
                    else { X[f] = to_alu<FMT>(__uint_as_float(raw[f])); X[f] *= to_alu<FMT>(__int_as_float(gw)); });
            }
            break; }
        case AVDSP_SOP_GAIN: {                                /* :636-640 */
            const int gw = t[0];
            STRAND_FRAMES(f, if constexpr (AI) X[f] = wmul(X[f], (long long)gw); else X[f] *= to_alu<FMT>(__int_as_float(gw)););
            break; }
        /* (USEY false: no operation of the strand reads Y -- the host of the plan has looked -- and Y is not kept at all) */
        case AVDSP_SOP_COPYXY: if constexpr (USEY) { STRAND_FRAMES(f, Y[f] = X[f];); } break;
        case AVDSP_SOP_COPYYX: if constexpr (USEY) { STRAND_FRAMES(f, X[f] = Y[f];); } break;
        case AVDSP_SOP_SWAPXY: if constexpr (USEY) { STRAND_FRAMES(f, const alu_t tt = X[f]; X[f] = Y[f]; Y[f] = tt;); } break;
        case AVDSP_SOP_ADDXY:  if constexpr (USEY) { STRAND_FRAMES(f, if constexpr (AI) X[f] = wadd(X[f], Y[f]); else X[f] = xy_add(X[f], Y[f]);); } break;
        case AVDSP_SOP_ADDYX:  if constexpr (USEY) { STRAND_FRAMES(f, if constexpr (AI) Y[f] = wadd(Y[f], X[f]); else Y[f] = xy_add(Y[f], X[f]);); } break;
        case AVDSP_SOP_SUBXY:  if constexpr (USEY) { STRAND_FRAMES(f, if constexpr (AI) X[f] = wsub(X[f], Y[f]); else X[f] = fsub(X[f], Y[f]);); } break;
        case AVDSP_SOP_SUBYX:  if constexpr (USEY) { STRAND_FRAMES(f, if constexpr (AI) Y[f] = wsub(Y[f], X[f]); else Y[f] = fsub(Y[f], X[f]);); } break;
        case AVDSP_SOP_NEGX:   STRAND_FRAMES(f, if constexpr (AI) X[f] = wsub(0, X[f]); else X[f] = -X[f];); break;
        case AVDSP_SOP_SHIFT: {                               /* :390-405 */
            const int s = t[0];
            STRAND_FRAMES(f,
                if constexpr (AI) {
                    if (s >= 0) X[f] = (long long)((unsigned long long)X[f] << ((s >= 100 ? 28 : s) & 63));
                    else X[f] = X[f] >> ((s <= -100 ? 28 : -s) & 63);
                } else if constexpr (A64) X[f] = shift_double(X[f], s);
                else X[f] = shift_float(X[f], s););
            break; }
        case AVDSP_SOP_SAT0DB: STRAND_FRAMES(f, X[f] = sat0db<FMT>(X[f]);); break;
        case AVDSP_SOP_SAT0DB_TPDF: STRAND_FRAMES(f, X[f] = sat0db<FMT>(tpdf_add(X[f], dv[f]));); break;
        case AVDSP_SOP_SAT0DB_GAIN: case AVDSP_SOP_SAT0DB_TPDF_GAIN: {       /* :494-534 */
            const int gw = t[0];
            const bool dith = op == AVDSP_SOP_SAT0DB_TPDF_GAIN;
            STRAND_FRAMES(f,
                if constexpr (AI) X[f] = wmul(X[f] >> 28, (long long)gw);
                else X[f] = fmul<FMT>(to_sp<FMT>(X[f]), __int_as_float(gw));
                if (dith) X[f] = tpdf_add(X[f], dv[f]);
                X[f] = sat0db<FMT>(X[f]););
            break; }
        case AVDSP_SOP_STORE: {                               /* :610-633 */
            const int io = t[0];
            const bool outwin = io >= a.io.out_base && io < a.io.out_base + a.io.out_stride;
            unsigned *dst = a.io.out + (size_t)n0 * a.io.out_stride + (io - a.io.out_base);
            unsigned w[F];
            STRAND_FRAMES(f,
                if constexpr (AI) w[f] = (unsigned)((int)X[f] & tp.mask);
                else if constexpr (SI) {
                    if constexpr (A64) w[f] = (unsigned)(s31_from_double(X[f]) & tp.mask);
                    else w[f] = (unsigned)(s31_from_float(X[f].v) & tp.mask);
                } else w[f] = __float_as_uint(to_sp<FMT>(X[f])););
            if (outwin) { STRAND_FRAMES(f, dst[(size_t)f * a.io.out_stride] = w[f];); }
            if (last_batch) a.scratch[io] = w[F - 1];
            break; }
        case AVDSP_SOP_LOAD_MEM: {                            /* :749-757 */
            int tmp[2] = {t[0], A64 ? t[64] : 0};
            const alu_t v = ld_alu<FMT>(tmp);
            STRAND_FRAMES(f, if constexpr (USEY) Y[f] = X[f]; X[f] = v;);
            break; }
        case AVDSP_SOP_STORE_MEM:                             /* :760-766: the word keeps the last frame's value */
            if (last_batch) st_alu<FMT>(a.buf + t[0], X[F - 1]);
            break;
        case AVDSP_SOP_DELAY: case AVDSP_SOP_DELAY_DP: {      /* :769-824 */
            const unsigned n = (unsigned)t[0];
            if (n) {
                int *d = a.buf + t[128];
                /* slot of frame f: the reference's counter stepped frame by frame.  It may start beyond a shortened line: that
                 * slot is then visited once, and the cycle 0 .. n-1 starts with the batch's second frame */
                int pos[F + 1];
                pos[0] = t[192];
                const int odd = (unsigned)pos[0] >= n ? 1 : 0;
                STRAND_FRAMES(f, const int nx = pos[f] + 1; pos[f + 1] = (unsigned)nx >= n ? 0 : nx;);
                /* a slot visited twice in the batch (lines shorter than the batch) holds what the earlier frame put there, n
                 * frames before: the batch's inputs go through the lane's column of the exchange area */
                int *xl = xch + lane;
                if (op == AVDSP_SOP_DELAY) {
                    int in[F], old[F];
                    STRAND_FRAMES(f, old[f] = d[1 + pos[f]];);
                    STRAND_FRAMES(f, if constexpr (AI) in[f] = (int)(sp_t)X[f]; else in[f] = __float_as_int(to_sp<FMT>(X[f])); xl[f * 64] = in[f];);
                    STRAND_FRAMES(f,
                        const int k = f - (int)n;
                        int v = old[f];
                        if (f > 0) { const int e = xl[max(k, 0) * 64]; if (k >= odd) v = e; }
                        if constexpr (AI) X[f] = (sp_t)v; else X[f] = to_alu<FMT>(__int_as_float(v)););
                    STRAND_FRAMES(f, d[1 + pos[f]] = in[f];);
                } else {
                    int in[F][2], old[F][2];
                    STRAND_FRAMES(f, for (int k = 0; k < AW; k++) old[f][k] = d[1 + pos[f] * AW + k];);
                    STRAND_FRAMES(f, in[f][1] = 0; st_alu<FMT>(in[f], X[f]); for (int k = 0; k < AW; k++) xl[(k * F + f) * 64] = in[f][k];);
                    STRAND_FRAMES(f,
                        const int k = f - (int)n;
                        int v[2] = {old[f][0], AW > 1 ? old[f][1] : 0};
                        if (f > 0) {
                            const int e0 = xl[max(k, 0) * 64], e1 = AW > 1 ? xl[(F + max(k, 0)) * 64] : 0;
                            if (k >= odd) { v[0] = e0; v[1] = e1; }
                        }
                        X[f] = ld_alu<FMT>(v););
                    STRAND_FRAMES(f, for (int k = 0; k < AW; k++) d[1 + pos[f] * AW + k] = in[f][k];);
                }
                t[192] = pos[F];
            }
            break; }
        case AVDSP_SOP_BIQUADS: {                             /* :827-849, dsp_biquadSTD.h: section by section over the batch's frames */
            const int num = __builtin_amdgcn_readfirstlane(o.imm);
            if (t[0]) {
                int xw[F];
                STRAND_FRAMES(f, xw[f] = bq_input<FMT>(X[f]););
                for (int sct = 0; sct < num; sct++) {
                    int *q = t + 64 * (2 + 11 * sct);
                    const bool last = sct == num - 1;
                    int cw[5], sw[6];
#pragma unroll
                    for (int k = 0; k < 5; k++) cw[k] = q[64 * k];
#pragma unroll
                    for (int k = 0; k < 6; k++) sw[k] = q[64 * (5 + k)];
                    BqState<FMT> st;
                    bq_load<FMT>(st, sw);
                    if constexpr (WIDE) {
                        /* operands kept widened: every MACC one FMA of an exact product (wave_biquads) */
                        double cd[5];
#pragma unroll
                        for (int k = 0; k < 5; k++) cd[k] = mulop(__int_as_float(cw[k]));
#if AVDSP_INTERP_HW_FLUSH
                        /* First with the plain conversions: they are mulop() for every operand that is not Inf / NaN (which mulop
                         * widens on its own terms) -- subnormals read as zero in this kernel's float mode, and a zero's sign cannot
                         * reach the sum unless the accumulator came in as -0.  The largest exponent met says whether that held. */
                        unsigned seen = max(max((unsigned)st.x1 << 1, (unsigned)st.x2 << 1), max((unsigned)st.y1 << 1, (unsigned)st.y2 << 1));
                        if (__double_as_longlong(st.acc) == (long long)0x8000000000000000ull) seen = 0xFFFFFFFFu;
                        double acc = st.acc;
                        double dx1 = (double)__int_as_float(st.x1), dx2 = (double)__int_as_float(st.x2);
                        double dy1 = (double)__int_as_float(st.y1), dy2 = (double)__int_as_float(st.y2);
                        int yw[F]; double yacc[F];
                        STRAND_FRAMES(f,
                            const double dx = (double)__int_as_float(xw[f]);
                            seen = max(seen, (unsigned)xw[f] << 1);
                            acc = __builtin_fma(dx, cd[0], acc); acc = __builtin_fma(dx1, cd[1], acc); acc = __builtin_fma(dx2, cd[2], acc);
                            acc = __builtin_fma(dy1, cd[3], acc); acc = __builtin_fma(dy2, cd[4], acc);
                            const float yn = (float)acc;
                            yw[f] = __float_as_int(yn); yacc[f] = acc;
                            seen = max(seen, (unsigned)yw[f] << 1);
                            dx2 = dx1; dx1 = dx; dy2 = dy1; dy1 = (double)yn;);
                        if (__ballot(seen >= 0xFF000000u) == 0) {
                            st.acc = acc;
                            if constexpr (F > 1) { st.x2 = xw[F - 2]; st.y2 = yw[F - 2]; } else { st.x2 = st.x1; st.y2 = st.y1; }
                            st.x1 = xw[F - 1]; st.y1 = yw[F - 1];
                            STRAND_FRAMES(f, xw[f] = yw[f]; if (last) X[f] = yacc[f];);
                        } else
#endif
                        {
                            BqWide<FMT> qw;
                            qw.acc = st.acc; qw.x1 = st.x1; qw.x2 = st.x2; qw.y1 = st.y1; qw.y2 = st.y2;
                            qw.dx1 = mulop(__int_as_float(st.x1)); qw.dx2 = mulop(__int_as_float(st.x2));
                            qw.dy1 = mulop(__int_as_float(st.y1)); qw.dy2 = mulop(__int_as_float(st.y2));
                            STRAND_FRAMES(f, xw[f] = bq_step_wide<FMT>(qw, xw[f], cd); if (last) X[f] = qw.acc;);
                            st.acc = qw.acc; st.x1 = qw.x1; st.x2 = qw.x2; st.y1 = qw.y1; st.y2 = qw.y2;
                        }
                    } else {
                        STRAND_FRAMES(f, xw[f] = bq_step<FMT>(st, xw[f], cw); if (last) X[f] = st.acc;);
                    }
                    bq_store<FMT>(st, sw);
#pragma unroll
                    for (int k = 0; k < 6; k++) q[64 * (5 + k)] = sw[k];
                }
            }
            break; }
        default: break;
        }
    }
    STRAND_STAMP(a.nops);
}

template <int FMT, bool USEY>
__global__ __launch_bounds__(64) void strand_lanes(const StrandArgs a)
{
#if AVDSP_INTERP_HW_FLUSH
    if constexpr (FMT != 2) flush_f32_subnormals_like_the_reference();
#endif
    using alu_t = typename interp::M<FMT>::alu;
    extern __shared__ unsigned lds_words[];
    int *tab = reinterpret_cast<int *>(lds_words);
    const int lane = threadIdx.x;
    const int sidx = blockIdx.x * 64 + lane;
    int *xch = tab + max(a.nres, 1) * 64;            /* the delay lines' exchange area: 2 x 16 words per lane */
    int *lops = xch + 2 * 16 * 64 + 16;              /* the operation list (behind the batch's 16 dither values) */
    for (int k = lane; k < a.nops * (int)(sizeof(avdsp_strand_op) / 4); k += 64) lops[k] = reinterpret_cast<const int *>(a.ops)[k];
    __syncthreads();
    if (sidx >= a.nstrands) return;
    const int *ar = a.args + (size_t)sidx * a.nargs;
    strand_resolve<FMT>(a, ar, tab, lane);
    const TpdfLocal tp = a.tpdf->global;
    const alu_t dconst = strand_dither<FMT>(a.tpdf->value, tp);       /* (no piece publishes per-frame values: the program's current one) */
    constexpr int F = 16;
    const int N = a.io.nframes;
    int n0 = 0;
    /* X and Y are per frame: a strand's first opcode replaces X, and nothing reads the Y it finds (the cut's condition) */
    for (; n0 + F <= N; n0 += F) {
        alu_t X[F], Y[F];
        STRAND_FRAMES(f, X[f] = 0; Y[f] = 0;);
        strand_batch<FMT, F, USEY>(a, tab, xch, lops, lane, n0, n0 + F == N, X, Y, tp, dconst);
    }
    for (; n0 < N; n0++) {
        alu_t X[1] = {0}, Y[1] = {0};
        strand_batch<FMT, 1, USEY>(a, tab, xch, lops, lane, n0, n0 + 1 == N, X, Y, tp, dconst);
    }
    strand_write_back<FMT>(a, tab, lane);
}

/* A piece that is a DSP_TPDF_CALC and nothing else (what stays in front of a strand run): the walk of interp::run<FMT, true>'s
 * DSP_TPDF_CALC over the whole block without the interpreter around it -- no program staged, no rows moved, whatever the program's
 * size.  Every lane steps the generator through each batch of 64 frames and keeps its own frame's pair (dsp_runtime.c:537-545,
 * dsp_tpdf.h:55-80: a first frame that finds another dither width only installs the new one). */
template <int FMT>
__global__ __launch_bounds__(64) void tpdf_walk(const GenericArgs a, int dith, int result_word, int nframes)
{
    using namespace interp;
    using alu_t = typename M<FMT>::alu;
    TpdfGlobals *g = a.tpdf;
    const int lane = threadIdx.x;
    const int want = dith ? dith : g->default_dither;
    const int first = (want == g->global.dither) ? 0 : 1;
    unsigned xs[4] = {g->xs[0], g->xs[1], g->xs[2], g->xs[3]};
    int gv = g->value, gr = g->random;
    __syncthreads();
    if (first && lane == 0) tpdf_prepare<FMT>(g, &g->global, &g->global, dith);
    for (int n0 = 0; n0 < nframes; n0 += 64) {
        const int nb = min(64, nframes - n0), fst = n0 ? 0 : first;
        int r1 = 0, r2 = 0;
        for (int f = fst; f < nb; f++) {
            const int a1 = (int)xoshiro128p(xs), a2 = (int)xoshiro128p(xs);
            if (lane == f) { r1 = a1; r2 = a2; }
        }
        if (lane >= fst) { gv = (r1 >> 1) + (r2 >> 1); gr = r2; }
        if (a.tpdf_role == 1 && lane < nb) { int *q = a.tpdf_seq + 2 * (n0 + lane); q[0] = gv; q[1] = gr; }
        if (n0 + nb == nframes && lane == nb - 1) {
            g->xs[0] = xs[0]; g->xs[1] = xs[1]; g->xs[2] = xs[2]; g->xs[3] = xs[3];
            if (lane >= fst) {
                g->value = gv; g->random = gr;
                alu_t X;
                if constexpr (M<FMT>::alu_int) X = gv; else X = from_int_scaled<FMT>(gv, 31);
                st_alu<FMT>(a.buf + result_word, X);
            }
        }
    }
}

/* dspTpdfInit (dsp_tpdf.h:85-99) on the device copy of the globals */
__global__ void tpdf_init_kernel(TpdfGlobals *g, int seed, int default_dither)
{
    g->random = seed;
    g->value = 0;
    g->default_dither = default_dither;
    g->global.dither = -1;
    int dith = default_dither;
    g->global.dither = dith;
    g->global.mask = (int)(0xFFFFFFFFu << ((32 - dith) & 31));
    g->global.mask64 = (long long)((unsigned long long)(long long)g->global.mask << 28);    /* int64 model only */
    g->global.shift = 28 - dith + 1;
    const unsigned s = (unsigned)seed;
    g->xs[0] = s | 1;
    g->xs[1] = interp::rotl32(s | 8, 7);
    g->xs[2] = interp::rotl32(s | 16, 11);
    g->xs[3] = interp::rotl32(s | 24, 17);
}

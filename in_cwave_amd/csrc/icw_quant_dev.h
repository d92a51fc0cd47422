/*
 * icw_quant_dev.h -- device helpers that icw_graph_dev.h (the elementwise render inside K2 and
 * KF2) and icw_render.hip (the serial and row renders) share: the quantiser steps of
 * sound_render_value and the single-instruction conversions and maxima they use.  Include after
 * <hip/hip_runtime.h> and icw_device.h, under `#pragma clang fp contract(off)`.
 */
#ifndef ICW_QUANT_DEV_H
#define ICW_QUANT_DEV_H

#define ICW_SQRT2 (1.4142135623730950488016887242097)

/* The rounding step of sound_render_value (sound_render.c:757-767) in fewer instructions, same bits:
 * q - ro is q + (-ro) in IEEE arithmetic, and ro / -ro differ only in the sign bit of the high
 * word, so one 32-bit select replaces the two 64-bit ones.  Then the peak: `aq > pk ? aq : pk`
 * equals fmax(pk, aq) here, because pk never holds a NaN and fmax returns the number when aq is
 * NaN (the reference's `cv > pv` is false for a NaN as well, sound_render.c:770-779). */
__device__ __forceinline__ double icw_round_q(double q, double round_offset, int sign_delta, int &delta)
{
    const bool neg = q < 0.0;
    const unsigned long long rb = (unsigned long long)__double_as_longlong(round_offset);
    const unsigned hi = (unsigned)(rb >> 32) ^ (neg ? 0x80000000u : 0u);
    delta = neg ? sign_delta : 0;
    return q + __longlong_as_double((long long)(((unsigned long long)hi << 32) | (rb & 0xffffffffull)));
}

/* The clip stage of sound_render_value (sound_render.c:782-797) as it reaches the integer:
 * q >= hi -> hi - 1, q <= lo -> lo + 1, then (int) truncation.  hi and lo are integers (hi >= 1,
 * lo <= -2), so for q in [hi-1, hi) the reference keeps q and truncates it to hi - 1, and for q in
 * (lo, lo+1] to lo + 1: min(q, hi - 1) / max(., lo + 1) give the same integer for every q, with
 * two instructions on the render's serial chain instead of two compares and four selects.  The
 * clip counts come from the same comparisons, off the chain.  A NaN q is the caller's case. */
__device__ __forceinline__ int icw_clamp_int(double q, const IcwRenderK &k, unsigned &clips)
{
    clips += (q >= k.hi ? 1u : 0u) + (q <= k.lo ? 1u : 0u);
    return (int)fmax(fmin(q, k.hi - 1.0), k.lo + 1.0);
}

/* The q of sound_render_value for ROUND render + flat shaper (sound_render.c:747-767): x * norm_mul
 * - prev_ns_err (0.0) + rnd * dth_mul (0.0 * dth_mul = +0.0), then +- round_offset by the sign.
 * x - 0.0 is x; the + 0.0, and a mid-riser's +- 0.0 (round_offset 0, sign_delta -1), change only a
 * zero's sign, which nothing downstream sees -- the peak takes fabs, the clip stage compares and
 * truncates, and (int) +-0.0 is 0 -- so they are not executed; a mid-tread's +- 0.5 of a -0.0 is +0.5
 * either way (-0.0 < 0 is false).  A norm_mul of 1.0 (16 sign bits) is not multiplied: x is a sum
 * or product, never a signalling NaN, and x * 1.0 is x. */
__device__ __forceinline__ double icw_round_in(double x, const IcwRenderK &k, int &delta)
{
    if (k.norm_mul != 1.0) x = x * k.norm_mul;
    if (k.sign_delta) {
        delta = x < 0.0 ? k.sign_delta : 0;
        return x;
    }
    return icw_round_q(x, k.round_offset, k.sign_delta, delta);
}

/* the rendered integer of one channel-sample (ROUND + flat), q for the caller's meters */
__device__ __forceinline__ int icw_render_round_q(double input, const IcwRenderK &k, double &q)
{
    int delta;
    q = icw_round_in(input, k, delta);
    /* x86 cvttsd2si semantics: NaN -> INT_MIN ("integer indefinite") */
    const int vc = (int)fmax(fmin(q, k.hi - 1.0), k.lo + 1.0);   /* icw_clamp_int without the counts */
    const int v = isnan(q) ? (int)0x80000000 : vc;
    return (v + delta) << k.norm_shift;
}

/* The q of a dithered render with the flat shaper (sound_render.c:711-767): the dither term d =
 * rnd * dth_mul comes from K3a (the same product), input = x * norm_mul - prev_ns_err is x * norm_mul
 * exactly (ns_empty keeps prev_ns_err at 0.0, sound_render.c:396-400, and x - 0.0 is x, a -0.0
 * included), qinput = input + d; then the rounding offset as icw_round_in (a mid-riser's +- 0.0
 * changes only a zero's sign, which nothing downstream sees). */
__device__ __forceinline__ double icw_round_in_d(double x, double d, const IcwRenderK &k, int &delta)
{
    if (k.norm_mul != 1.0) x = x * k.norm_mul;
    x = x + d;
    if (k.sign_delta) {
        delta = x < 0.0 ? k.sign_delta : 0;
        return x;
    }
    return icw_round_q(x, k.round_offset, k.sign_delta, delta);
}

/* sound_render_value for a flat-shaper render (sound_render.c:691-809): elementwise.  DITH: the
 * dither term d of a RPDF / TPDF / STPDF / GAUSS render (K3a's); ROUND has none. */
template <bool DITH = false>
__device__ __forceinline__ int icw_render_round(double input, const IcwRenderK &k, unsigned &clips, double &pk,
                                                double d = 0.0)
{
    int delta;
    const double q = DITH ? icw_round_in_d(input, d, k, delta) : icw_round_in(input, k, delta);
    pk = fmax(pk, fabs(q));
    /* x86 cvttsd2si semantics: NaN -> INT_MIN ("integer indefinite") */
    const int vc = icw_clamp_int(q, k, clips);    /* unconditional: a NaN counts no clip */
    int v = isnan(q) ? (int)0x80000000 : vc;
    return (v + delta) << k.norm_shift;
}

__device__ __forceinline__ int icw_cvt_sat_i32(double q)
{
    int v;
    asm("v_cvt_i32_f64_e32 %0, %1" : "=v"(v) : "v"(q));
    return v;
}

__device__ __forceinline__ int icw_med3_i32(int x, int lo, int hi)
{
    int v;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(v) : "v"(x), "v"(lo), "v"(hi));
    return v;
}

/* max(m, |q|) and max(a, b) as one v_max_f64 each: IEEE maxNum returns the number for a quiet NaN
 * operand, as fmax; written out because the compiler canonicalised both operands of every fmax here
 * (two more v_max_f64 per sample).  The operands are sums and products, never signalling NaNs. */
__device__ __forceinline__ double icw_vmax_abs(double m, double q)
{
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(m), "v"(q));
    return r;
}

__device__ __forceinline__ double icw_vmax(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

/* max(|a|, |b|) as one v_max_f64: a NaN operand gives the other magnitude (maxNum), two NaNs a NaN */
__device__ __forceinline__ double icw_vmax_abs2(double a, double b)
{
    double r;
    asm("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

#endif

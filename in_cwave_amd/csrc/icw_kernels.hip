/*
 * icw_kernels.hip -- gfx950 (CDNA4) kernels of the in_cwave Hilbert -> modulator -> render path.
 *
 * Built with `-ffp-contract=off` and no fast-math; every floating-point expression below keeps
 * the operand order of the reference so that results are bit-identical to the x86 SSE2 build
 * of in_cwave (IEEE binary64, round-to-nearest, no FMA contraction, denormals preserved).
 *
 * Kernel roles (DESIGN.md "Kernels"; the serial IIR recurrence K1 lives in icw_iir.hip):
 *   icw_unpack_frames  K0: unpack + fade + the quadrature mix into per-chain filter inputs.
 *   icw_output      one thread per frame.  Everything that is NOT on the recurrence: the output
 *                   Kahan sum y[n] = sum d_i z_i + d0*c_i z_i (hblpf.c:1029-1043) from the w
 *                   window (frame-parallel), the fs/4 un-mix (lpf_hilbert_quad.c:129-156), the
 *                   DSP graph (adv_modulator.c:637-751) and the elementwise render
 *                   (sound_render.c:691-809, ROUND/flat).  Coalesced tile loads via LDS.
 *   icw_graph_serial   K4 (serial form).
 * The dither generator and the renders (K3a / K3b / K3c) live in icw_render.hip.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/icw.h"
#include "icw_device.h"
#include "icw_iir_dev.h"
#include "icw_launch.h"
#include "icw_libm.h"

#pragma clang fp contract(off)

#define ICW_PI (3.1415926535897932384626433832795029)

#include "icw_quant_dev.h"

#include "icw_unpack_dev.h"

/* input of the I (f=0) / Q (f=1) filter for Hilbert phase k (lpf_hilbert_quad.c:133-151):
 *   I: {x, +0, -x, +0}   Q: {+0, -x, +0, x}.  K0 writes the nonzero values of both into one row per
 * channel; the recurrences supply the +0.0 (icw_iir_dev.h: icw_chain_x). */

/* the fade and the signed filter-input row of one real frame (v: the unpacked L, R samples) */
__device__ __forceinline__ void icw_store_frame(const IcwK0Args &a, int t, int s, double (&v)[2])
{
    const long long ix = a.pos[s] + a.t0 + t;
    const double fd = icw_fade(ix, a.fade[s * 3 + 0], a.fade[s * 3 + 1], a.fade[s * 3 + 2]);
    if (fd >= 0.0) {
        v[0] *= fd;
        v[1] *= fd;
    }
    /* one row per channel, s*2 + ch: the I filter's nonzero inputs sit at the even phases, the Q
     * filter's at the odd ones, so the channel's signed sample {x, -x, -x, x}[k] serves both -- the
     * I filter reads it where k is even (x, -x), the Q filter where k is odd (-x, x), and each takes
     * the literal +0.0 at the other phases itself (icw_chain_x): 16 B per stereo frame, not 32 */
    double *xs = a.xd + (size_t)s * 2 * a.x_pitch + t;
    const int nchw = a.dedup ? 1 : 2;          /* mono dedup: K1 reads the left row only */
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        if (ch < nchw) {
            const unsigned k = (a.hq_phase[s * 2 + ch] + (unsigned)(a.t0 + t)) & 3u;
            xs[(size_t)ch * a.x_pitch] = (k == 0u || k == 3u) ? v[ch] : -v[ch];
        }
    }
}

/* Input prep (K0): unpack + fade each frame once (xwave_unpack_csample, xwave_reader.c:908-1001)
 * and lay out the filter inputs of the quadrature mix of hq_rp_process (lpf_hilbert_quad.c:129-156):
 * the I filter {x, +0, -x, +0} and the Q filter {+0, -x, +0, x} by sample phase, both in one row
 * s*2 + ch of signed samples (below).  Mono input feeds the right converter with the left value,
 * exactly the reference's reuse of `val` (xwave_reader.c:988).  Complex input: four rows
 * s*4 + ch*2 + {I, Q}. */
__device__ __forceinline__ void icw_unpack_frame(const IcwK0Args &a, int t, int s)
{
    const unsigned char *fp = a.in + (size_t)s * a.in_stride + (size_t)t * a.fsz;
    const long long ix = a.pos[s] + a.t0 + t;
    const double fd = icw_fade(ix, a.fade[s * 3 + 0], a.fade[s * 3 + 1], a.fade[s * 3 + 2]);
    if (a.fmt >= ICW_FMT_CW_F64) {
        /* complex (CWAVE) sample: I/Q per channel, mono -> R = L, fade on all four
         * (xwave_reader.c:939-966); rows s*4 + ch*2 + {I, Q} */
        double q[4];
        icw_unpack_iq(fp, a.fmt, q[0], q[1]);
        if (a.nch > 1) icw_unpack_iq(fp + a.csz, a.fmt, q[2], q[3]);
        else { q[2] = q[0]; q[3] = q[1]; }
        if (fd >= 0.0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] *= fd;
        }
        double *xs = a.xd + (size_t)s * 4 * a.x_pitch + t;
#pragma unroll
        for (int i = 0; i < 4; ++i) xs[(size_t)i * a.x_pitch] = q[i];
        return;
    }
    const uintptr_t al = (uintptr_t)(a.in + (size_t)s * a.in_stride) | (uintptr_t)a.fsz;
    icw_fmt_dispatch(a.fmt, al, [&](auto fc, auto ac) {
        constexpr int F = decltype(fc)::value;
        constexpr bool AL = decltype(ac)::value != 0;
        double v[2];
        v[0] = icw_unpack_f<F, AL>(fp);
        v[1] = a.nch > 1 ? icw_unpack_f<F, AL>(fp + a.csz) : v[0];
        icw_store_frame(a, t, s, v);
    });
}

__global__ __launch_bounds__(256) void icw_unpack_frames(IcwK0Args a)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < a.T) icw_unpack_frame(a, t, blockIdx.y);
}

#include "icw_fir_dev.h"

/* KF: the converter alone, one workgroup per channel and 2048-frame tile of a stream; I / Q rows
 * go out coalesced through LDS to the CWAVE rows K2 reads */
__global__ __launch_bounds__(256) void icw_fir_hilbert(IcwFirArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double xs[];   /* staged inputs (padded), taps, Q */
    constexpr int TF = 256 * ICW_FIR_R;
    const int ch = blockIdx.y, s = blockIdx.z;
    const int tt = blockIdx.x * TF;
    const int M = a.M, c = M >> 1;
    const int sh = (8 - ((c - 1) & 7)) & 7;          /* c - 1 + sh = 8 a */
    const int av = (c - 1 + sh) >> 3;
    const int nf = min(TF, a.T - tt);
    icw_fir_stage<1>(a, s, ch, xs, 0, tt, TF, sh, threadIdx.x, 256);
    const int px = (icw_fir_phys(sh + M + TF + 24) + 2) & ~1;   /* even: the next row stays 16-byte aligned */
    double *qs = xs + px + ((a.nt + 1) & ~1);
    icw_ctap *gs = (icw_ctap *)a.g;
    __syncthreads();
    double acc[ICW_FIR_R];
    icw_fir_sums(xs, gs, a.nt, threadIdx.x, av, sh, c, acc);
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) qs[ICW_FIR_R * threadIdx.x + r] = acc[r];
    __syncthreads();
    double *rowI = a.xd + ((size_t)s * 4 + ch * 2) * a.x_pitch + tt;
    double *rowQ = rowI + a.x_pitch;
    const bool mono = a.nch == 1;
    for (int f = threadIdx.x; f < nf; f += 256) {
        const double vi = xs[icw_fir_phys(f + 8 * av + 1)], vq = qs[f];
        rowI[f] = vi;
        rowQ[f] = vq;
        if (mono) {
            rowI[f + 2 * a.x_pitch] = vi;
            rowQ[f + 2 * a.x_pitch] = vq;
        }
    }
}


/* ------------------------------------------------------------- output kernel (K2) ------- */
struct IcwLR { double lre, lim, rre, rim; };

/* output Kahan sum of iir_rp_process_kahan (hblpf.c:1029-1043) for the sample whose delay line
 * is z_i = win[N-1-i] (win = w[t-N .. t-1]); baseline form (hblpf.c:898-925) needs w[t]=win[N] */
/* the same sums for NC chains at once, interleaved by term: each coefficient is live for one
 * term of all NC chains instead of across NC whole sums (with the chains back to back, all 2N
 * coefficients stay live in SGPRs and spill to VGPR lanes -- a v_readlane per use) */
/* FP_CHECK on: the output half of the WITH FP CHECKS branches of iir_rp_process_kahan / _baseline
 * (hblpf.c:1058-1095, 928-950) for one chain, whose delay line is z_i = win[N-1-i].  ti = FC(z * c_i)
 * is the loop-back kernel's product (counted there), so here it is only applied.  Compact on
 * purpose (run-time loops, FC() not inlined): a diagnostic mode. */
__device__ __noinline__ double icw_iir_out_fc(const double *win, int N, int kahan, const double *pc,
                                              const double *pd, double d0, IcwFes &f)
{
    if (kahan) {
        double z = win[N - 1];
        double t = icw_fc_nc(z * pc[0]);
        double S = icw_fc(z * pd[0], f), C = 0.0, Y, T;
#pragma unroll 1
        for (int k = 0; k < 2 * N - 1; ++k) {
            /* steps: t0 * d0, then per i >= 1: z * d_i, t_i * d0 */
            const int i = (k + 1) >> 1;
            double x;
            if (k == 0) x = icw_fc(t * d0, f);
            else if (k & 1) { z = win[N - 1 - i]; t = icw_fc_nc(z * pc[i]); x = icw_fc(z * pd[i], f); }
            else x = icw_fc(t * d0, f);
            Y = icw_fc(x - C, f);                            /* kahan_step_fes, hblpf.c:995-1005 */
            T = icw_fc(S + Y, f);
            C = icw_fc(icw_fc(T - S, f) - Y, f);
            S = T;
        }
        return S;
    }
    double so = 0.0;
#pragma unroll 1
    for (int i = 0; i < N; ++i) so = icw_fc(so + icw_fc(win[N - 1 - i] * pd[i], f), f);
    return icw_fc(icw_fc(win[N] * d0, f) + so, f);
}

template <int N, bool KAHAN, int NC>
__device__ __forceinline__ void icw_iir_out_n(const double *const (&win)[NC], const double *pc, const double *pd,
                                              double d0, double (&y)[NC])
{
    if (KAHAN) {
        double S[NC], C[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double z = win[c][N - 1];
            const double t0 = z * pc[0];
            double Y, T;
            S[c] = z * pd[0];
            C[c] = 0.0;
            const double x = t0 * d0;
            Y = x - C[c]; T = S[c] + Y; C[c] = (T - S[c]) - Y; S[c] = T;
        }
#pragma unroll
        for (int i = 1; i < N; ++i) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double z = win[c][N - 1 - i];
                const double ti = z * pc[i];
                double x = z * pd[i], Y, T;
                Y = x - C[c]; T = S[c] + Y; C[c] = (T - S[c]) - Y; S[c] = T;
                x = ti * d0;
                Y = x - C[c]; T = S[c] + Y; C[c] = (T - S[c]) - Y; S[c] = T;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = S[c];
    } else {
        double so[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) so[c] = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int c = 0; c < NC; ++c) so[c] += win[c][N - 1 - i] * pd[i];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = win[c][N] * d0 + so[c];
    }
}

template <int N, bool KAHAN>
__device__ __forceinline__ double icw_iir_out(const double *win, const double (&pc)[20],
                                              const double (&pd)[20], double d0)
{
    if (KAHAN) {
        double z = win[N - 1];
        double t0 = z * pc[0];
        double S = z * pd[0], C = 0.0, Y, T;
        double x = t0 * d0;
        Y = x - C; T = S + Y; C = (T - S) - Y; S = T;
#pragma unroll
        for (int i = 1; i < N; ++i) {
            z = win[N - 1 - i];
            const double ti = z * pc[i];
            x = z * pd[i];
            Y = x - C; T = S + Y; C = (T - S) - Y; S = T;
            x = ti * d0;
            Y = x - C; T = S + Y; C = (T - S) - Y; S = T;
        }
        return S;
    } else {
        double so = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) so += win[N - 1 - i] * pd[i];
        return win[N] * d0 + so;
    }
}

/* x / SQRT2 correctly rounded, as dsp_master divides (adv_modulator.c:498-501), in 3 FP64 operations
 * instead of the 11 of a general division (div_scale x 2, rcp, 5 fma, mul, div_fmas, div_fixup):
 *     q0 = RN(x r),  e = RN(x - q0 c) (one fma),  q = RN(q0 + e r) (one fma),  r = RN(1/c).
 * Error: |q0 + e r - x/c| < 2^-51 ulp(x/c) for 2^-900 <= |x| <= DBL_MAX (q0 is within 2 ulp, e within
 * one rounding of the exact remainder, r within half an ulp of 1/c), so q can differ from RN(x/c)
 * only where x/c lies within 2^-51 ulp of a rounding midpoint.  With c = C 2^-52 (C odd) those
 * are the significands X with (2M + 1) C - 2^53 X = k (X >= C) or (2M + 1) C - 2^54 X = k (X < C)
 * for an odd |k| < 8 -- one residue class mod C each, a handful of X in [2^52, 2^53); every one of
 * them, up to |k| <= 63, gives RN(x/c) here (tests/test_libm.py::test_div_sqrt2_hard_cases, which
 * solves for them and checks this arithmetic in exact rationals).  Zeros (a -0.0 would come out
 * +0.0), tiny values (a subnormal remainder or quotient), infinities and NaNs take the division. */
/* The range test is on the result: |q| >= 2^-900 holds for no NaN (an infinite x gives a NaN q) and
 * implies |x| >= 2^-899.5 (q is within a few ulp of x / c wherever it is not a NaN), so it keeps q
 * only inside the range above, in one compare. */
__device__ __forceinline__ double icw_div_sqrt2_fast(double x)
{
    constexpr double rc = 0x1.6a09e667f3bccp-1;          /* RN(1 / c) */
    const double q0 = x * rc;
    const double e = __builtin_fma(-q0, ICW_SQRT2, x);
    return __builtin_fma(e, rc, q0);
}

__device__ __forceinline__ bool icw_div_sqrt2_ok(double q)
{
#if ICW_FIR_DIAG & 1
    return true;
#else
    return fabs(q) >= 0x1p-900;
#endif
}

__device__ __forceinline__ double icw_div_sqrt2(double x)
{
    double q = icw_div_sqrt2_fast(x);
    if (!icw_div_sqrt2_ok(q)) q = x / ICW_SQRT2;
    return q;
}

__device__ __forceinline__ double icw_master(int tout, double re, double im)
{
    switch (tout) {
    case ICW_S_RE: return re;
    case ICW_S_IM: return im;
    case ICW_S_ADD_REIM: return icw_div_sqrt2(re + im);
    case ICW_S_SUB_REIM: return icw_div_sqrt2(re - im);
    }
    return 0.0;
}

/* The value registers of the DSP program live in LDS, [reg][component][thread]: a register index
 * is wave-uniform and data-dependent, and a register array in VGPRs is demoted to scratch memory
 * by the compiler (measured: 256 B per frame written to HBM, 4.5 GB WRITE_SIZE per 16.8 M-frame
 * launch).  Lane-contiguous LDS rows are bank-conflict free. */
struct IcwRegFile {
    double *base;   /* lds + tid */
    __device__ __forceinline__ void get(int r, IcwLR &v) const
    {
        const double *p = base + (size_t)r * 4 * ICW_K2_TILE;
        v.lre = p[0]; v.lim = p[ICW_K2_TILE]; v.rre = p[2 * ICW_K2_TILE]; v.rim = p[3 * ICW_K2_TILE];
    }
    __device__ __forceinline__ void set(int r, const IcwLR &v) const
    {
        double *p = base + (size_t)r * 4 * ICW_K2_TILE;
        p[0] = v.lre; p[ICW_K2_TILE] = v.lim; p[2 * ICW_K2_TILE] = v.rre; p[3 * ICW_K2_TILE] = v.rim;
    }
};

/* row of frame t in the rotation table: frame-major, or (perm_q > 0, the fused FIR kernel, whose
 * lanes hold 4 or 8 consecutive frames) frames 8 apart in consecutive rows, so that a wave's loads
 * of one frame slot cover 1-2 KB contiguously instead of one row every 128 / 256 B */
__device__ __forceinline__ size_t icw_trig_index(int t, int perm_q)
{
    return perm_q ? (size_t)(t & 7) * (size_t)perm_q + (size_t)(t >> 3) : (size_t)t;
}

/* rotate (re,im) by e^{j phi} given cos/sin (adv_modulator.c:546-547, 576-577) */
__device__ __forceinline__ void icw_rot(double re, double im, double cs, double sn, double &ore, double &oim)
{
    ore = re * cs - im * sn;
    oim = re * sn + im * cs;
}

/* modulator frame counter -> norm_omega of frame t of the call (adv_modulator.c:611-625).
 * n0 is the call-start counter.  In scaled mode the reference takes the first frame's omega from
 * the raw counter and wraps only when it advances (n = (n + 1) % scale_sr), so a counter left at or
 * above a new, lower scale by a track switch (icw_set_input without clr_nframe) is used as is once,
 * and frame t >= 1 sees (n0 + t) mod scale_sr. */
__device__ __forceinline__ double icw_omega(unsigned long long n0, long long t, int scaled, unsigned long long ssr,
                                            uint32_t sample_rate)
{
    if (scaled) {
        /* n0 < ssr except after a rate change, so one subtraction covers any call shorter than ssr
         * frames (1000 s of audio) -- the 64-bit remainder is the rare path */
        unsigned long long n = n0 + (unsigned long long)t;
        if (t != 0 && n >= ssr) n = (n - ssr < ssr) ? n - ssr : n % ssr;
        return (2.0 * ICW_PI) * ((double)n) / ((double)ssr);
    }
    return (2.0 * ICW_PI) * ((double)(n0 + (unsigned long long)t)) / (double)sample_rate;
}

/* The rotation factor e^{j phi} of channel c of an active Shift / PM node at norm_omega
 * (dsp_shift adv_modulator.c:519-550, dsp_pm adv_modulator.c:554-583).  The one definition used by
 * the per-frame table kernel and by the inline path, so both produce the same bits.  fmod is exact;
 * cos / sin are glibc's own (icw_libm.h): the reference's cos + sin pair is one sincos() call in a
 * gcc build, PM's inner sin() is glibc's FMA variant -- so the factors, and everything after them,
 * are bit-identical to the CPU path. */
/* The compiled DSP program is read through the constant address space: its fields are wave-uniform
 * and the kernels never write it, so they come in by scalar loads into SGPRs.  Through a plain
 * pointer the compiler could not prove the kernel's own stores (output, bus, pre-render) leave it
 * alone, and every op field became a vector load, a full vmcnt(0) wait and a v_readfirstlane per
 * use -- in KF2's graph phase ~half of its 1 050 VALU instructions per wave (c2fir SQ pass,
 * profiles/r04_c2fir_phases.json). */
typedef const __attribute__((address_space(4))) IcwProg icw_cprog;
typedef const __attribute__((address_space(4))) IcwOp icw_cop;
__device__ __forceinline__ icw_cprog *icw_prog_c(const IcwProg *p) { return (icw_cprog *)p; }

__device__ __forceinline__ void icw_trig(icw_cop &op, int c, double omega, double &cs, double &sn)
{
    const double ph = fmod(omega * op.f[c], 2.0 * ICW_PI);
    if (op.mode == ICW_MODE_SHIFT) {
        icw_lm_sincos(ph, sn, cs);
        if (op.neg[c]) sn = -sn;
    } else {
        const double psi = op.lp[c] * (icw_lm_sin_fma(ph + op.pp[c]) + op.fa[c]);
        icw_lm_sincos(psi, sn, cs);
    }
}

/* icw_trig out of line, for the per-stream fallback of K2 / K4 (a stream whose frame counter is
 * not stream 0's): inlined, glibc's sincos path added ~45 VGPRs to K2 and cost it a wave per SIMD
 * (141 -> 3 waves) although the per-frame rotation table serves every stream in step. */
__device__ __noinline__ double2 icw_trig_call(icw_cop &op, int c, double omega)
{
    double cs, sn;
    icw_trig(op, c, omega, cs, sn);
    return make_double2(cs, sn);
}

/* One DSP node on its mixed input d (adv_modulator.c:669-751): channel exchange, I/Q swap,
 * gains, then Master (-> lOut/rOut) or Shift / PM / Mix (-> o, returns true).  trow: this frame's
 * row of the rotation table (nullable: compute the factors inline). */
template <bool TRIG = true, bool TAB = false>
__device__ __forceinline__ bool icw_exec_op(icw_cop &op, IcwLR d, double omega, IcwLR &o, double &lOut,
                                            double &rOut, const double *trow = nullptr)
{
    double xt;
    switch (op.xch) {
    case ICW_XCH_SWAP:
        xt = d.lre; d.lre = d.rre; d.rre = xt;
        xt = d.lim; d.lim = d.rim; d.rim = xt;
        break;
    case ICW_XCH_LEFTONLY: d.rre = d.lre; d.rim = d.lim; break;
    case ICW_XCH_RIGHTONLY: d.lre = d.rre; d.lim = d.rim; break;
    case ICW_XCH_MIXLR:
        d.lre = d.rre = (d.lre + d.rre) / 2.0;
        d.lim = d.rim = (d.lim + d.rim) / 2.0;
        break;
    default: break;
    }
    if (op.iqinv[0]) { xt = d.lre; d.lre = d.lim; d.lim = xt; }
    if (op.iqinv[1]) { xt = d.rre; d.rre = d.rim; d.rim = xt; }
    d.lre *= op.gain[0]; d.lim *= op.gain[0];
    d.rre *= op.gain[1]; d.rim *= op.gain[1];
    switch (op.mode) {
    case ICW_MODE_MASTER:
        lOut = icw_master(op.tout[0], d.lre, d.lim);
        rOut = icw_master(op.tout[1], d.rre, d.rim);
        return false;
    case ICW_MODE_SHIFT:
    case ICW_MODE_PM: {
        if constexpr (!TRIG) { o = d; return true; }   /* no active Shift/PM in the program */
        double cs, sn;
        if (op.act[0]) {
            if (TAB || trow) { cs = trow[op.tslot[0] * 2]; sn = trow[op.tslot[0] * 2 + 1]; }
            else { const double2 f = icw_trig_call(op, 0, omega); cs = f.x; sn = f.y; }
            icw_rot(d.lre, d.lim, cs, sn, o.lre, o.lim);
        } else { o.lre = d.lre; o.lim = d.lim; }
        if (op.act[1]) {
            if (TAB || trow) { cs = trow[op.tslot[1] * 2]; sn = trow[op.tslot[1] * 2 + 1]; }
            else { const double2 f = icw_trig_call(op, 1, omega); cs = f.x; sn = f.y; }
            icw_rot(d.rre, d.rim, cs, sn, o.rre, o.rim);
        } else { o.rre = d.rre; o.rim = d.rim; }
        return true;
    }
    default: /* MIX */
        o = d;
        return true;
    }
}

/* One frame's `in` through the rest of the block (K2 and the fused converter KF2): the bus-form
 * hand-off, or the DSP list (adv_modulator.c:637-751) on the LDS register file, the pre-render
 * doubles and the elementwise ROUND render with the meters' per-thread parts. */
/* DEFER: the rendered integers go to dv[0..1] instead of the output row (KF2 stores 4 frames at once) */
/* the chain-program signatures compiled straight (ICW_SIG_*, icw_device.h) */
template <bool TRIG, int R, bool ROWP, int SIG, int I>
__device__ __forceinline__ void icw_chain_sig(const IcwK2Args &a, icw_cprog *P, int t0, int T, const IcwLR (&in)[R],
                                              IcwLR (&prev)[R], double (&lOut)[R], double (&rOut)[R], double *bus_s,
                                              bool has_last, int lastr, uint32_t tro_lane, size_t tro_u, size_t tro_step);

/* one frame's rendered integers to the output row (16-bit: one dword per frame; 24-bit: 6 bytes) */
__device__ __forceinline__ void icw_frame_store(const IcwK2Args &a, int s, int t, int vl, int vr)
{
    unsigned char *o = a.out + (size_t)s * a.out_stride;
    if (a.rk.is24) {
        unsigned char *q = o + (size_t)t * 6;
        q[0] = (unsigned char)vl; q[1] = (unsigned char)(vl >> 8); q[2] = (unsigned char)(vl >> 16);
        q[3] = (unsigned char)vr; q[4] = (unsigned char)(vr >> 8); q[5] = (unsigned char)(vr >> 16);
    } else {
        const unsigned pk = ((unsigned)vl & 0xffffu) | ((unsigned)vr << 16);
        *(unsigned *)(o + (size_t)t * 4) = pk;
    }
}

/* (K2 keeps the exact form for every frame: its render-only form, KF2's icw_sig_fast per frame,
 * measured C3 -0.3 %, C4 -0.5 % on one box -- K2 runs beside the recurrence, which bounds C3 / C4) */
template <bool TRIG, bool TAB = false, bool DEFER = false>
__device__ __forceinline__ void icw_frame_graph(const IcwK2Args &a, icw_cprog *P, const IcwRegFile &R, int s,
                                                int t, const IcwLR &in, bool use_tab, unsigned &clip_l,
                                                unsigned &clip_r, double &pk_l, double &pk_r, int *dv = nullptr,
                                                size_t tab_off = 0)
{
    /* tab_off: the stream's slab of the rotation table (per-stream lists; 0: the one table) */
    const int T = a.T;
    if (a.iq_out) {
        /* bus-form graph: the serial graph kernel takes it from here (do_render == 0) */
        double *q = a.iq_out + ((size_t)s * T + t) * 4;
        q[0] = in.lre; q[1] = in.lim; q[2] = in.rre; q[3] = in.rim;
    } else {
        const double *trow = use_tab ? a.trig_tab + tab_off + icw_trig_index(t, a.trig_perm_q) * a.trig_pitch : nullptr;
        const double omega = (TRIG && !use_tab) ? icw_omega(a.n_frame[s], a.t0 + t, a.scaled, a.ssr, a.sample_rate)
                                                : 0.0;
        /* DSP list (adv_modulator.c:637-751) */
        /* persistent bus at the block's last frame: slot 0 = in, then each written slot's
         * final value from the op that writes it (compile_graph: op.wb_slot) */
        const bool last = t == T - 1;
        double *bus_s = a.bus + (size_t)s * ICW_N_INPUTS * 4;
        if (last) { bus_s[0] = in.lre; bus_s[1] = in.lim; bus_s[2] = in.rre; bus_s[3] = in.rim; }
        double lOut = 0.0, rOut = 0.0;
        const int sig = P->sig & ~ICW_SIG_UNIT;
        if (P->chain && (sig == ICW_SIG_M || sig == ICW_SIG_SM || sig == ICW_SIG_PSXM) && (!TRIG || use_tab)) {
            /* a specialised chain signature, factors from the table (or none): the ops straight */
            IcwLR inr[1] = {in}, pv[1] = {in};
            double lo[1] = {0.0}, ro[1] = {0.0};
            const uint32_t tro = TRIG ? (uint32_t)(icw_trig_index(t, a.trig_perm_q) * a.trig_pitch) : 0u;
            if (sig == ICW_SIG_M)
                icw_chain_sig<TRIG, 1, true, ICW_SIG_M, 0>(a, P, t, T, inr, pv, lo, ro, bus_s, last, 0, tro, tab_off, 0);
            else if (sig == ICW_SIG_SM)
                icw_chain_sig<TRIG, 1, true, ICW_SIG_SM, 0>(a, P, t, T, inr, pv, lo, ro, bus_s, last, 0, tro, tab_off, 0);
            else
                icw_chain_sig<TRIG, 1, true, ICW_SIG_PSXM, 0>(a, P, t, T, inr, pv, lo, ro, bus_s, last, 0, tro, tab_off, 0);
            lOut = lo[0];
            rOut = ro[0];
        } else if (P->chain) {
            /* chain program: `in` and the previous op's output in registers, no register file */
            IcwLR prev = in;
            for (int oi = 0; oi < P->n_ops; ++oi) {
                icw_cop &op = P->ops[oi];
                IcwLR d;
                if (P->bypass) {
                    d = in;
                } else {
                    d.lre = d.lim = d.rre = d.rim = 0.0;
                    if (op.chain_in & 1) { d.lre += in.lre; d.lim += in.lim; d.rre += in.rre; d.rim += in.rim; }
                    if (op.chain_in & 2) { d.lre += prev.lre; d.lim += prev.lim; d.rre += prev.rre; d.rim += prev.rim; }
                }
                IcwLR o;
                if (icw_exec_op<TRIG, TAB>(op, d, omega, o, lOut, rOut, trow)) {
                    prev = o;
                    if (last && op.wb_slot >= 0) {
                        double *b = bus_s + op.wb_slot * 4;
                        b[0] = o.lre; b[1] = o.lim; b[2] = o.rre; b[3] = o.rim;
                    }
                }
            }
        } else {
        R.set(0, in);
        for (int oi = 0; oi < P->n_ops; ++oi) {
            icw_cop &op = P->ops[oi];
            IcwLR d;
            if (P->bypass) {
                d = in;
            } else {
                d.lre = d.lim = d.rre = d.rim = 0.0;
                for (int q = 0; q < op.n_in; ++q) {
                    IcwLR v;
                    R.get(op.in_reg[q], v);
                    d.lre += v.lre; d.lim += v.lim; d.rre += v.rre; d.rim += v.rim;
                }
            }
            IcwLR o;
            if (icw_exec_op<TRIG, TAB>(op, d, omega, o, lOut, rOut, trow)) {
                R.set(op.out_reg, o);
                if (last && op.wb_slot >= 0) {
                    double *b = bus_s + op.wb_slot * 4;
                    b[0] = o.lre; b[1] = o.lim; b[2] = o.rre; b[3] = o.rim;
                }
            }
        }
        }   /* register file */

        if (a.pre) {
            double *p = a.pre + (size_t)s * a.pre_stride + (size_t)t * 2;
            p[0] = lOut; p[1] = rOut;
        }
        if (a.do_render) {
            int vl, vr;
            if (a.dith) {
                /* a dithered render with the flat shaper: K3a's terms of this frame, rows 2s, 2s + 1 */
                const double *dd = a.dith + (size_t)(2 * s) * a.dith_pitch + t;
                const double dl = dd[0], dr = dd[a.dith_pitch];
                vl = icw_render_round<true>(lOut, a.rk, clip_l, pk_l, dl);
                vr = icw_render_round<true>(rOut, a.rk, clip_r, pk_r, dr);
            } else {
                vl = icw_render_round(lOut, a.rk, clip_l, pk_l);
                vr = icw_render_round(rOut, a.rk, clip_r, pk_r);
            }
            if constexpr (DEFER) {
                dv[0] = vl;
                dv[1] = vr;
                return;
            }
            icw_frame_store(a, s, t, vl, vr);
        }
    }
}

/* A chain program's op fields as the frame loop uses them, read once per op for all the frames a
 * lane holds (not per frame: the op list lives in global memory, and the loads came back after
 * every store of the frame loop) */
struct IcwOpK {
    int mode, chain_in, xch, iq0, iq1, tout0, tout1, act0, act1, ts0, ts1, wb;
    double g0, g1;
};

__device__ __forceinline__ IcwOpK icw_op_k(icw_cop &op)
{
    IcwOpK k;
    k.mode = op.mode; k.chain_in = op.chain_in; k.xch = op.xch;
    k.iq0 = op.iqinv[0]; k.iq1 = op.iqinv[1];
    k.tout0 = op.tout[0]; k.tout1 = op.tout[1];
    k.act0 = op.act[0]; k.act1 = op.act[1];
    k.ts0 = op.tslot[0]; k.ts1 = op.tslot[1];
    k.wb = op.wb_slot;
    k.g0 = op.gain[0]; k.g1 = op.gain[1];
    return k;
}

/* R frames of one lane (t0 + r; the first nv are in the block) through a chain program, op by op:
 * the op's fields are read once for the R frames and their rotation factors (the per-frame table,
 * every stream in step) are loaded together before the arithmetic.  Per frame the arithmetic of
 * icw_frame_graph + icw_exec_op in the same order, so the bits are the same; the rendered integers
 * go to dv (0 for frames past the block).
 * ROWP: the caller knows where the R frames' table rows are -- frame r's row at
 * a.trig_tab + tro_u + r * tro_step + tro_lane, the first two wave-uniform, the last the lane's (KF2's
 * lanes hold consecutive frames of a tile inside the block, icw_fir_graph) -- so a load needs no
 * per-frame index arithmetic and no clamp.
 * Three shortcuts, each exact: a gain of 1.0 is not multiplied (x * 1.0 is x for every value that is
 * not a signalling NaN, and d is a sum or a converted input here, never one); the bus writes of the
 * block's last frame are tested once per call (one lane of the launch holds it); and the clip
 * counters take one compare per call -- a clip needs |q| >= min(hi, -lo) (clip_abs), so only a call
 * whose largest |q| reaches that counts its samples one by one (a NaN q clips nothing, and fmax
 * passes it over, as the per-sample compares did). */
/* One op of a chain program over the R frames (the body of icw_chain_frames).  MODE / CIN >= 0: the
 * op's mode and chain inputs known at compile time (a specialised signature, ICW_SIG_*), so the
 * compiler keeps only that op's arithmetic and no merges between the modes' results; -1: read from
 * the program (the generic loop).  The other fields are wave-uniform scalars either way. */
template <bool TRIG, int R, bool ROWP, int MODE, int CIN>
__device__ __forceinline__ void icw_chain_op(const IcwK2Args &a, icw_cop &op, bool bypass, int t0, int T,
                                             const IcwLR (&in)[R], IcwLR (&prev)[R], double (&lOut)[R],
                                             double (&rOut)[R], double *bus_s, bool has_last, int lastr,
                                             uint32_t tro_lane, size_t tro_u, size_t tro_step)
{
    constexpr bool plain = MODE >= 0;   /* a signature op: plain fields (compile_graph, IcwProg.sig) */
    const IcwOpK k = icw_op_k(op);
    const int mode = MODE >= 0 ? MODE : k.mode;
    const int cin = CIN >= 0 ? CIN : k.chain_in;
    const bool rot = TRIG && (mode == ICW_MODE_SHIFT || mode == ICW_MODE_PM);
    const bool act0 = plain || k.act0, act1 = plain || k.act1;
    double cs[R][2], sn[R][2];
    if (rot) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            /* (cos, sin) of a channel: one 16-byte load (rows and columns are 16-byte aligned) */
            const double *trow = ROWP ? a.trig_tab + tro_u + (size_t)r * tro_step + tro_lane
                                      : a.trig_tab + icw_trig_index(min(t0 + r, T - 1), a.trig_perm_q) * a.trig_pitch;
            const double2 f0 = act0 ? *(const double2 *)(trow + k.ts0 * 2) : make_double2(0.0, 0.0);
            const double2 f1 = act1 ? *(const double2 *)(trow + k.ts1 * 2) : make_double2(0.0, 0.0);
            cs[r][0] = f0.x; sn[r][0] = f0.y;
            cs[r][1] = f1.x; sn[r][1] = f1.y;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        IcwLR d;
        if (bypass) {
            d = in[r];
        } else {
            d.lre = d.lim = d.rre = d.rim = 0.0;
            if (cin & 1) { d.lre += in[r].lre; d.lim += in[r].lim; d.rre += in[r].rre; d.rim += in[r].rim; }
            if (cin & 2) { d.lre += prev[r].lre; d.lim += prev[r].lim; d.rre += prev[r].rre; d.rim += prev[r].rim; }
        }
        double xt;
        if (!plain) {
            switch (k.xch) {
            case ICW_XCH_SWAP:
                xt = d.lre; d.lre = d.rre; d.rre = xt;
                xt = d.lim; d.lim = d.rim; d.rim = xt;
                break;
            case ICW_XCH_LEFTONLY: d.rre = d.lre; d.rim = d.lim; break;
            case ICW_XCH_RIGHTONLY: d.lre = d.rre; d.lim = d.rim; break;
            case ICW_XCH_MIXLR:
                d.lre = d.rre = (d.lre + d.rre) / 2.0;
                d.lim = d.rim = (d.lim + d.rim) / 2.0;
                break;
            default: break;
            }
            if (k.iq0) { xt = d.lre; d.lre = d.lim; d.lim = xt; }
            if (k.iq1) { xt = d.rre; d.rre = d.rim; d.rim = xt; }
        }
        if (k.g0 != 1.0) { d.lre *= k.g0; d.lim *= k.g0; }
        if (k.g1 != 1.0) { d.rre *= k.g1; d.rim *= k.g1; }
        if (mode == ICW_MODE_MASTER) {
            lOut[r] = icw_master(plain ? ICW_S_ADD_REIM : k.tout0, d.lre, d.lim);
            rOut[r] = icw_master(plain ? ICW_S_ADD_REIM : k.tout1, d.rre, d.rim);
            continue;
        }
        IcwLR o = d;
        if (rot) {
            if (act0) icw_rot(d.lre, d.lim, cs[r][0], sn[r][0], o.lre, o.lim);
            if (act1) icw_rot(d.rre, d.rim, cs[r][1], sn[r][1], o.rre, o.rim);
        }
        prev[r] = o;
    }
    if (mode != ICW_MODE_MASTER && k.wb >= 0 && has_last) {
        double *b = bus_s + k.wb * 4;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == lastr) { b[0] = prev[r].lre; b[1] = prev[r].lim; b[2] = prev[r].rre; b[3] = prev[r].rim; }
    }
}

/* op I of signature SIG (ICW_SIG_*, above) */
template <int SIG, int I>
struct icw_sig_op {
    static constexpr int mode = (SIG >> (4 + 4 * I)) & 3;
    static constexpr int cin = (SIG >> (6 + 4 * I)) & 3;
};

template <bool TRIG, int R, bool ROWP, int SIG, int I>
__device__ __forceinline__ void icw_chain_sig(const IcwK2Args &a, icw_cprog *P, int t0, int T, const IcwLR (&in)[R],
                                              IcwLR (&prev)[R], double (&lOut)[R], double (&rOut)[R], double *bus_s,
                                              bool has_last, int lastr, uint32_t tro_lane, size_t tro_u, size_t tro_step)
{
    if constexpr (I < (SIG & 15)) {
        icw_chain_op<TRIG, R, ROWP, icw_sig_op<SIG, I>::mode, icw_sig_op<SIG, I>::cin>(
            a, P->ops[I], false, t0, T, in, prev, lOut, rOut, bus_s, has_last, lastr, tro_lane, tro_u, tro_step);
        icw_chain_sig<TRIG, R, ROWP, SIG, I + 1>(a, P, t0, T, in, prev, lOut, rOut, bus_s, has_last, lastr, tro_lane,
                                                 tro_u, tro_step);
    }
}

/* The render-only form of a signature pass (no pre-render doubles requested, no lane holding the
 * block's last frame): the same rendered integers and meters in about half the instructions (KF2's
 * graph phase, c2fir: ~800 -> ~410 VALU per wave, profiles/r04_c2fir_sq.json).
 *  - An op's input is the sum in + prev without the reference's leading 0.0 + (adv_modulator.c:655-665).
 *    0.0 + x differs from x only for x = -0.0, and in this arithmetic (products, sums, the division by
 *    SQRT2 -- no reciprocal, no sign test) a zero's sign changes nothing but zero signs downstream.
 *    The render cannot see one (below), so the integers and meters are the exact pass's; the pre-render
 *    doubles and the bus state can, which is why those calls and frames take icw_chain_frames' path.
 *  - Gains of 1.0 on every op but the Master (ICW_SIG_UNIT, the BASELINE lists) are left out at
 *    compile time; any other gain of 1.0 is branched over (the compiler had turned the uniform test
 *    into a multiply and two selects per double).
 *  - The division by SQRT2: icw_div_sqrt2's three operations for every value, then one test per value
 *    and one divergent branch per op for those outside its range.
 *  - The render (sound_render_value, ROUND + flat shaper, sound_render.c:747-797): q = x * norm_mul +
 *    copysign(round_offset, x) -- for the mid-riser (offset 0) x + +-0 with x's own sign is x exactly,
 *    for the mid-tread it is the reference's x +- 0.5 except at x = -0.0, where -0.5 and +0.5 both
 *    truncate to 0 and have the same magnitude for the peak and the clip tests; the truncation as
 *    v_cvt_i32_f64 (saturating), and the clip stage (an integer clamp into [lo + 1, hi - 1]: the same
 *    integer as min(q, hi - 1), max(., lo + 1), then (int), for every q that is not a NaN) only in a pass whose
 *    largest |q| reaches min(hi, -lo) -- below it the clamp changes nothing; a NaN q -- INT_MIN, as
 *    x86's cvttsd2si gives -- takes a divergent branch of its own (icw_fast_render). */
/* The render of the R frames (see above).  MR: mid-riser, q = x (x + +-0.0 with x's sign is x) and
 * delta = -1 below zero; mid-tread: q = copysign(|x| + 0.5, x), the reference's x +- 0.5 (-0.0 gives
 * -0.5, harmless as above), delta 0.  The integer is the saturating conversion; the clamp to
 * [lo + 1, hi - 1] is needed only where |q| reaches clip_abs = min(hi, -lo) -- the pass's meter test
 * -- so it is applied there with the clip counts.  Then the NaN samples: INT_MIN (delta 0). */
template <bool MR, bool SH0, int R>
__device__ __forceinline__ void icw_fast_render(const IcwRenderK &rk, const double (&x)[R][2], int (&dv)[R][2],
                                                double &lm_l, double &lm_r, unsigned &clip_l, unsigned &clip_r)
{
    /* SH0: norm_shift 0 (full sign bits, the usual case) -- no shift after the integer, so the
     * mid-riser's delta folds into one subtract-with-borrow of the compare */
    const int sh = SH0 ? 0 : rk.norm_shift;
    static_assert(R >= 2, "the meters start from the first two frames");
    double q[R][2];
    int del[R][2];
    bool nan = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if constexpr (MR) {
                q[r][c] = x[r][c];
                del[r][c] = x[r][c] < 0.0 ? -1 : 0;               /* sign_delta -1 (icw_launch_fir_graph checks) */
            } else {
                q[r][c] = __builtin_copysign(fabs(x[r][c]) + rk.round_offset, x[r][c]);
                del[r][c] = 0;
            }
            dv[r][c] = (int)((unsigned)(icw_cvt_sat_i32(q[r][c]) + del[r][c]) << sh);
            nan |= q[r][c] != q[r][c];
        }
    }
    /* the largest |q| of the frames (a NaN q counts as nothing, as fmax from 0.0 does; all-NaN
     * frames give a NaN here, which no comparison passes and the peak's v_max_f64 skips) */
    lm_l = icw_vmax_abs2(q[0][0], q[1][0]);
    lm_r = icw_vmax_abs2(q[0][1], q[1][1]);
#pragma unroll
    for (int r = 2; r < R; ++r) {
        lm_l = icw_vmax_abs(lm_l, q[r][0]);
        lm_r = icw_vmax_abs(lm_r, q[r][1]);
    }
    if (icw_vmax(lm_l, lm_r) >= rk.clip_abs) {
        /* the host's integer bounds (SGPRs), integer min / max: (int)rk.lo is a VALU conversion, whose
         * result the compiler hoisted to the kernel entry and spilled (+1.6 B of scratch writes per
         * c2fir frame), and a v_med3_i32 wants VGPR operands */
        const int lo1 = rk.lo1, hi1 = rk.hi1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            clip_l += (q[r][0] >= rk.hi ? 1u : 0u) + (q[r][0] <= rk.lo ? 1u : 0u);
            clip_r += (q[r][1] >= rk.hi ? 1u : 0u) + (q[r][1] <= rk.lo ? 1u : 0u);
#pragma unroll
            for (int c = 0; c < 2; ++c)
                dv[r][c] = (int)((unsigned)(min(max(icw_cvt_sat_i32(q[r][c]), lo1), hi1) + del[r][c]) << sh);
        }
    }
    if (nan) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (q[r][c] != q[r][c]) dv[r][c] = (int)(0x80000000u << sh);
    }
}

/* 16 bytes at a wave-uniform base + a lane's 32-bit byte offset, as a raw buffer load: the base goes
 * into the descriptor (SGPRs), so no address arithmetic runs on the VALU -- a global load took a
 * v_lshl_add_u64 per load (the lane offset held as 64 bits), 4-8 per pass of the fused converter */
__device__ __forceinline__ double2 icw_ld_row2(const double *base, uint32_t lane_bytes)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, 0x7fffffff, 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lane_bytes, 0, 0);
    double2 d;
    d.x = __longlong_as_double((long long)(((unsigned long long)v[1] << 32) | v[0]));
    d.y = __longlong_as_double((long long)(((unsigned long long)v[3] << 32) | v[2]));
    return d;
}

template <bool TRIG, int R, int SIG, int I>
__device__ __forceinline__ void icw_sig_fast_ops(const IcwK2Args &a, icw_cprog *P, const IcwLR (&in)[R],
                                                 IcwLR (&prev)[R], double (&lOut)[R], double (&rOut)[R],
                                                 uint32_t tro_lane, size_t tro_u, size_t tro_step)
{
    if constexpr (I < (SIG & 15)) {
        constexpr int mode = icw_sig_op<SIG, I>::mode, cin = icw_sig_op<SIG, I>::cin;
        constexpr bool rot = TRIG && (mode == ICW_MODE_SHIFT || mode == ICW_MODE_PM);
        icw_cop &op = P->ops[I];
        double cs[R][2], sn[R][2];
        if constexpr (rot) {
            const int ts0 = op.tslot[0], ts1 = op.tslot[1];
            /* a wave-uniform row base (SGPRs) + the lane's 32-bit byte offset */
            const uint32_t lane_b = tro_lane * 8u;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double2 f0 = icw_ld_row2(a.trig_tab + tro_u + (size_t)r * tro_step + ts0 * 2, lane_b);
                const double2 f1 = icw_ld_row2(a.trig_tab + tro_u + (size_t)r * tro_step + ts1 * 2, lane_b);
                cs[r][0] = f0.x; sn[r][0] = f0.y;
                cs[r][1] = f1.x; sn[r][1] = f1.y;
            }
        }
        IcwLR d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (cin == 1) d[r] = in[r];
            else if constexpr (cin == 2) d[r] = prev[r];
            else if constexpr (cin == 3) {
                d[r].lre = in[r].lre + prev[r].lre; d[r].lim = in[r].lim + prev[r].lim;
                d[r].rre = in[r].rre + prev[r].rre; d[r].rim = in[r].rim + prev[r].rim;
            } else {
                d[r].lre = d[r].lim = d[r].rre = d[r].rim = 0.0;
            }
        }
        constexpr bool unit = (SIG & ICW_SIG_UNIT) && mode != ICW_MODE_MASTER;
        const double g0 = op.gain[0], g1 = op.gain[1];
        if (!unit && (ICW_SCALAR_UNIT ? !op.unit_gain[0] : g0 != 1.0)) {
            asm volatile("");
#pragma unroll
            for (int r = 0; r < R; ++r) { d[r].lre *= g0; d[r].lim *= g0; }
        }
        if (!unit && (ICW_SCALAR_UNIT ? !op.unit_gain[1] : g1 != 1.0)) {
            asm volatile("");
#pragma unroll
            for (int r = 0; r < R; ++r) { d[r].rre *= g1; d[r].rim *= g1; }
        }
        if constexpr (mode == ICW_MODE_MASTER) {
            double x[R][2];
            bool slow = false;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                x[r][0] = d[r].lre + d[r].lim;
                x[r][1] = d[r].rre + d[r].rim;
                lOut[r] = icw_div_sqrt2_fast(x[r][0]);
                rOut[r] = icw_div_sqrt2_fast(x[r][1]);
                slow |= !icw_div_sqrt2_ok(lOut[r]) || !icw_div_sqrt2_ok(rOut[r]);
            }
            if (slow) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (!icw_div_sqrt2_ok(lOut[r])) lOut[r] = x[r][0] / ICW_SQRT2;
                    if (!icw_div_sqrt2_ok(rOut[r])) rOut[r] = x[r][1] / ICW_SQRT2;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if constexpr (rot) {
                    icw_rot(d[r].lre, d[r].lim, cs[r][0], sn[r][0], prev[r].lre, prev[r].lim);
                    icw_rot(d[r].rre, d[r].rim, cs[r][1], sn[r][1], prev[r].rre, prev[r].rim);
                } else {
                    prev[r] = d[r];
                }
            }
        }
        icw_sig_fast_ops<TRIG, R, SIG, I + 1>(a, P, in, prev, lOut, rOut, tro_lane, tro_u, tro_step);
    }
}

template <bool TRIG, int R, int SIG>
__device__ __forceinline__ void icw_sig_fast(const IcwK2Args &a, icw_cprog *P, const IcwLR (&in)[R], unsigned &clip_l,
                                             unsigned &clip_r, double &pk_l, double &pk_r, int (&dv)[R][2],
                                             uint32_t tro_lane, size_t tro_u, size_t tro_step)
{
    IcwLR prev[R];
    double lOut[R], rOut[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        prev[r] = in[r];
        lOut[r] = rOut[r] = 0.0;
    }
    icw_sig_fast_ops<TRIG, R, SIG, 0>(a, P, in, prev, lOut, rOut, tro_lane, tro_u, tro_step);
    const IcwRenderK &rk = a.rk;
    double x[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) { x[r][0] = lOut[r]; x[r][1] = rOut[r]; }
    if (ICW_SCALAR_UNIT ? !rk.unit_mul : rk.norm_mul != 1.0) {
        asm volatile("");
#pragma unroll
        for (int r = 0; r < R; ++r) { x[r][0] *= rk.norm_mul; x[r][1] *= rk.norm_mul; }
    }
    double lm_l, lm_r;
    if (ICW_RENDER_SH0 && rk.norm_shift == 0) {
        if (rk.sign_delta != 0) icw_fast_render<true, true, R>(rk, x, dv, lm_l, lm_r, clip_l, clip_r);
        else icw_fast_render<false, true, R>(rk, x, dv, lm_l, lm_r, clip_l, clip_r);
    } else {
        if (rk.sign_delta != 0) icw_fast_render<true, false, R>(rk, x, dv, lm_l, lm_r, clip_l, clip_r);
        else icw_fast_render<false, false, R>(rk, x, dv, lm_l, lm_r, clip_l, clip_r);
    }
    pk_l = icw_vmax(pk_l, lm_l);
    pk_r = icw_vmax(pk_r, lm_r);
}

template <bool TRIG, int R, bool ROWP = false, int SIG = 0>
__device__ __forceinline__ void icw_chain_frames(const IcwK2Args &a, icw_cprog *P, int s, int t0, int nv,
                                                 const IcwLR (&in)[R], unsigned &clip_l, unsigned &clip_r,
                                                 double &pk_l, double &pk_r, int (&dv)[R][2], uint32_t tro_lane = 0,
                                                 size_t tro_u = 0, size_t tro_step = 0)
{
    const int T = a.T;
    double *bus_s = a.bus + (size_t)s * ICW_N_INPUTS * 4;
    const int lastr = T - 1 - t0;                    /* the block's last frame is frame lastr here */
    const bool has_last = lastr >= 0 && lastr < nv;
    if constexpr (SIG != 0 && ROWP) {
        /* the render-only form when no lane of the wave needs the exact doubles */
        if (!a.pre && __all(nv == R && !has_last)) {
            icw_sig_fast<TRIG, R, SIG>(a, P, in, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, tro_u, tro_step);
            return;
        }
    }
    IcwLR prev[R];
    double lOut[R], rOut[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        prev[r] = in[r];
        lOut[r] = rOut[r] = 0.0;
    }
    if (has_last) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == lastr) { bus_s[0] = in[r].lre; bus_s[1] = in[r].lim; bus_s[2] = in[r].rre; bus_s[3] = in[r].rim; }
    }
    if constexpr (SIG != 0) {
        /* a signature has no bypass: a bypassed list is the Master alone reading nothing (chain_in 0) */
        icw_chain_sig<TRIG, R, ROWP, SIG & ~ICW_SIG_UNIT, 0>(a, P, t0, T, in, prev, lOut, rOut, bus_s, has_last, lastr,
                                                             tro_lane, tro_u, tro_step);
    } else {
        const bool bypass = P->bypass != 0;
        for (int oi = 0; oi < P->n_ops; ++oi)
            icw_chain_op<TRIG, R, ROWP, -1, -1>(a, P->ops[oi], bypass, t0, T, in, prev, lOut, rOut, bus_s, has_last, lastr,
                                                tro_lane, tro_u, tro_step);
    }
    const IcwRenderK &rk = a.rk;
    double q[R][2], lm_l = 0.0, lm_r = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        dv[r][0] = dv[r][1] = 0;
        q[r][0] = q[r][1] = 0.0;
        if (r < nv) {
            if (a.pre) {
                double *p = a.pre + (size_t)s * a.pre_stride + (size_t)(t0 + r) * 2;
                p[0] = lOut[r]; p[1] = rOut[r];
            }
#if ICW_FIR_DIAG & 2
            q[r][0] = lOut[r]; q[r][1] = rOut[r];
            dv[r][0] = (int)lOut[r]; dv[r][1] = (int)rOut[r];
#else
            dv[r][0] = icw_render_round_q(lOut[r], rk, q[r][0]);
            dv[r][1] = icw_render_round_q(rOut[r], rk, q[r][1]);
#endif
            lm_l = fmax(lm_l, fabs(q[r][0]));
            lm_r = fmax(lm_r, fabs(q[r][1]));
        }
    }
    pk_l = fmax(pk_l, lm_l);
    pk_r = fmax(pk_r, lm_r);
    if (fmax(lm_l, lm_r) >= rk.clip_abs) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            clip_l += (q[r][0] >= rk.hi ? 1u : 0u) + (q[r][0] <= rk.lo ? 1u : 0u);
            clip_r += (q[r][1] >= rk.hi ? 1u : 0u) + (q[r][1] <= rk.lo ? 1u : 0u);
        }
    }
}

/* the chain frames of one call through the program's signature when it is a specialised one */
template <bool TRIG, int R>
__device__ __forceinline__ void icw_chain_frames_rowp(const IcwK2Args &a, icw_cprog *P, int sig, int s, int t0, int nv,
                                                      const IcwLR (&in)[R], unsigned &clip_l, unsigned &clip_r,
                                                      double &pk_l, double &pk_r, int (&dv)[R][2], uint32_t tro_lane,
                                                      size_t tro_u, size_t tro_step)
{
    /* a plain Shift / PM always rotates, so a kernel without TRIG sees only the Master signature and
     * carries only that one: with all of them the mono kernel spilled in its loop (c3fir WRITE_SIZE
     * 1.98 against 1.09 GB per launch).  The TRIG kernels keep the Master case they never take: without
     * it the stereo kernel's allocation spilled instead (c2fir 96 against 67 MB). */
    if constexpr (TRIG) {
        switch (sig) {
        case ICW_SIG_M:
        case ICW_SIG_M | ICW_SIG_UNIT:
            icw_chain_frames<TRIG, R, true, ICW_SIG_M | ICW_SIG_UNIT>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r,
                                                                    dv, tro_lane, tro_u, tro_step);
            return;
        case ICW_SIG_SM:
            icw_chain_frames<TRIG, R, true, ICW_SIG_SM>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r, dv, tro_lane,
                                                        tro_u, tro_step);
            return;
        case ICW_SIG_SM | ICW_SIG_UNIT:
            icw_chain_frames<TRIG, R, true, ICW_SIG_SM | ICW_SIG_UNIT>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r,
                                                                     dv, tro_lane, tro_u, tro_step);
            return;
        case ICW_SIG_PSXM:
            icw_chain_frames<TRIG, R, true, ICW_SIG_PSXM>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r, dv, tro_lane,
                                                          tro_u, tro_step);
            return;
        case ICW_SIG_PSXM | ICW_SIG_UNIT:
            icw_chain_frames<TRIG, R, true, ICW_SIG_PSXM | ICW_SIG_UNIT>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l,
                                                                       pk_r, dv, tro_lane, tro_u, tro_step);
            return;
        default: break;
        }
    } else {
        if (sig == ICW_SIG_M || sig == (ICW_SIG_M | ICW_SIG_UNIT)) {
            icw_chain_frames<TRIG, R, true, ICW_SIG_M | ICW_SIG_UNIT>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r, dv,
                                                                    tro_lane, tro_u, tro_step);
            return;
        }
    }
    icw_chain_frames<TRIG, R, true>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, tro_u, tro_step);
}

/* The stereo I / Q exchange between lane l (channel L) and lane l + 32 (channel R) of a wave: with
 * a = x[r] and b = x[r + 4] of each lane, afterwards a = L's value and b = R's value of the lane's
 * frame (lane l: frame r, lane l + 32: frame r + 4).  v_permlane32_swap trades the upper half of one
 * VGPR with the lower half of another on the VALU, two per double, where __shfl_xor(x, 32) took two
 * ds_bpermute round trips through the LDS plus a select (c2fir kernel 0.331 -> 0.328 ms, c4fir
 * 3.114 -> 3.084 ms, profiles/r03_fir_swap_ab.jsonl). */
__device__ __forceinline__ void icw_swap32(double &a, double &b)
{
    const unsigned long long ua = __double_as_longlong(a), ub = __double_as_longlong(b);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)ua, (unsigned)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false);
    a = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
    b = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
}

/* peak / clip reduction slots of a workgroup: per channel two per wave, one per 16-lane row (icw_meters_wg;
 * every caller runs ICW_K2_TILE threads, KF2's launch bound included) */
#define ICW_PK_SLOTS (ICW_K2_TILE / 32)
static_assert(ICW_K2_TILE == 256, "icw_fir_graph launches 256 threads and shares icw_meters_wg's slots");

/* every lane of a 16-lane row gets the row's largest value, for doubles >= +0.0 that are never a NaN
 * (so v_max_f64 without canonicalising, and any order gives the same value): DPP row_ror 8, 4, 2, 1,
 * each two v_mov_b32_dpp and one v_max_f64.  Full EXEC. */
template <int CTRL>
__device__ __forceinline__ double icw_dpp_max_nn(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return icw_vmax(v, __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)));
}

__device__ __forceinline__ double icw_row_max_nn(double v)
{
    v = icw_dpp_max_nn<0x128>(v);                    /* row_ror:8 */
    v = icw_dpp_max_nn<0x124>(v);                    /* row_ror:4 */
    v = icw_dpp_max_nn<0x122>(v);                    /* row_ror:2 */
    return icw_dpp_max_nn<0x121>(v);                 /* row_ror:1 */
}

/* the sum over a 16-lane row, in every lane of it (the same rotations) */
__device__ __forceinline__ unsigned icw_row_sum_u32(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x122, 0xf, 0xf, false);
    return v + (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x121, 0xf, 0xf, false);
}

/* per-workgroup meters (ICW_K2_TILE threads, full EXEC): row reduce, LDS, one atomic per
 * stream/channel.  The peaks are maxima of |q| from +0.0 (fmax / v_max_f64 return the number for a
 * NaN operand), so they are >= +0.0 and never a NaN, and their maximum is the same in any order; the
 * clip counts are sums of integers.  The two channels share one reduction: v_permlane32_swap leaves
 * lanes 0-31 with channel L's values of lanes l and l + 32 and lanes 32-63 with channel R's (one
 * max), each 16-lane row is reduced by DPP, and lanes 0 and 16 (L) / 32 and 48 (R) hand their row's
 * maximum to the final reduction -- ~15 VALU per wave where two device-library wave reductions
 * (-inf fills, canonicalising maxima, cross-row steps) took ~75 in the fused converter's graph phase.
 * The counts are reduced only when a lane of the wave clipped (a ballot), the usual case being none. */
__device__ __forceinline__ void icw_meters_wg(const IcwK2Args &a, int s, unsigned clip_l, unsigned clip_r, double pk_l,
                                              double pk_r, unsigned (*red_clip)[ICW_PK_SLOTS],
                                              double (*red_pk)[ICW_PK_SLOTS])
{
    const int tl = threadIdx.x, ln = tl & 63, wv = tl >> 6;
    const bool any_clip = __any((clip_l | clip_r) != 0u);
    if (any_clip) {
        const auto c = __builtin_amdgcn_permlane32_swap(clip_l, clip_r, false, false);
        const unsigned cs = icw_row_sum_u32(c[0] + c[1]);
        if ((ln & 15) == 0) red_clip[ln >> 5][2 * wv + ((ln >> 4) & 1)] = cs;
    } else if ((ln & 15) == 0) {
        red_clip[ln >> 5][2 * wv + ((ln >> 4) & 1)] = 0u;
    }
    icw_swap32(pk_l, pk_r);
    const double pk = icw_row_max_nn(icw_vmax(pk_l, pk_r));
    if ((ln & 15) == 0) red_pk[ln >> 5][2 * wv + ((ln >> 4) & 1)] = pk;
    __syncthreads();
    if (tl < 2) {
        unsigned cs = 0; double pm = 0.0;
        for (int i = 0; i < ICW_PK_SLOTS; ++i) { cs += red_clip[tl][i]; pm = fmax(pm, red_pk[tl][i]); }
        if (cs) atomicAdd(&a.clips[s * 2 + tl], cs);
        if (pm > 0.0) atomicMax(&a.peak_bits[s * 2 + tl], (unsigned long long)__double_as_longlong(pm));
    }
}

/* One frame of K2: the four chains' output sums from their w rows (w[c]: the row at the frame's
 * window, w[c][N] the state after the frame), the de-subnorm counts, the fs/4 un-mix, then the
 * frame graph.  dup: mono input with bit-identical converters, chains 2-3 are copies of 0-1. */
template <int N, bool KAHAN, bool TRIG, bool FCK>
__device__ __forceinline__ void icw_output_frame(const IcwK2Args &a, icw_cprog *P, const IcwRegFile &R, int s,
                                                 int t, const double *const (&w)[4], bool dup, const double *lc,
                                                 IcwFes (&fes)[2], bool count_sn, unsigned (&sn)[4], bool use_tab,
                                                 unsigned &clip_l, unsigned &clip_r, double &pk_l, double &pk_r,
                                                 size_t tab_off = 0)
{
    IcwLR in;
    if (a.cw) {
        /* complex (CWAVE) input: the analytic signal as read (xwave_reader.c:939-966) */
        const double *xs = a.xin + (size_t)s * 4 * a.x_pitch + t;
        in.lre = xs[0]; in.lim = xs[a.x_pitch]; in.rre = xs[2 * a.x_pitch]; in.rim = xs[3 * a.x_pitch];
    } else {
        const int nc = dup ? 2 : 4;
        if (count_sn) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < nc) sn[c] += (w[c][N] == 0.0) ? 1u : 0u;
        }
        /* filter outputs of the 4 chains (L-I, L-Q, R-I, R-Q) */
        double y[4];
        if constexpr (FCK) {
#pragma unroll 1
            for (int c = 0; c < 4; ++c) y[c] = icw_iir_out_fc(w[c], N, KAHAN, lc, lc + 20, a.d0, fes[c >> 1]);
        } else if (dup) {
            const double *const wins[2] = {w[0], w[1]};
            double y2[2];
            icw_iir_out_n<N, KAHAN, 2>(wins, lc, lc + 20, a.d0, y2);
            y[0] = y[2] = y2[0];
            y[1] = y[3] = y2[1];
        } else {
            icw_iir_out_n<N, KAHAN, 4>(w, lc, lc + 20, a.d0, y);
        }
        /* fs/4 un-mix (lpf_hilbert_quad.c:129-156) */
        double oI[2], oQ[2];
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const double yi = y[ch * 2], yq = y[ch * 2 + 1];
            const unsigned kq = (a.hq_phase[s * 2 + ch] + (unsigned)(a.t0 + t)) & 3u;
            switch (kq) {
            case 0: oI[ch] = yi * 2.0; oQ[ch] = yq * 2.0; break;
            case 1: oI[ch] = -yq * 2.0; oQ[ch] = yi * 2.0; break;
            case 2: oI[ch] = -yi * 2.0; oQ[ch] = -yq * 2.0; break;
            default: oI[ch] = yq * 2.0; oQ[ch] = -yi * 2.0; break;
            }
        }
        in.lre = oI[0]; in.lim = oQ[0]; in.rre = oI[1]; in.rim = oQ[1];
    }
    icw_frame_graph<TRIG>(a, P, R, s, t, in, use_tab, clip_l, clip_r, pk_l, pk_r, nullptr, tab_off);
}

/* the workgroup's de-subnorm counts, one atomic per chain (nc chains computed; dup: the right
 * converters ran identically, so they rejected the same samples) */
__device__ __forceinline__ void icw_sn_wg(const IcwK2Args &a, int s, const unsigned (&sn)[4], int nc,
                                          unsigned (*red_sn)[ICW_K2_TILE / 64])
{
    const int tl = threadIdx.x, wv = tl >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        unsigned v = sn[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((tl & 63) == 0) red_sn[c][wv] = v;
    }
    __syncthreads();
    if (tl < 4) {
        unsigned long long tot = 0;
        for (int i = 0; i < ICW_K2_TILE / 64; ++i) tot += red_sn[tl < nc ? tl : tl - 2][i];
        if (tot) atomicAdd(&a.sncnt[(size_t)s * 4 + tl], tot);
    }
}

/* Output kernel (K2).  A workgroup owns a.tpw (<= ICW_K2_TPW) consecutive 256-frame tiles of one
 * stream (fewer when a launch would have too few workgroups to spread over the chip).
 * The w window of tile k+1 is loaded into registers while tile k is computed, then written to the
 * other half of a double-buffered LDS window: the global-load latency hides behind FP64 work and
 * the meters reduce once per workgroup.  TRIG = the program has an active Shift / PM node.
 * MIX = per-stream DSP lists (a.prog_id): the workgroup's stream picks its program and its slab of
 * the rotation table once, before the tile loop -- both wave-uniform, the program pointer stays in
 * the constant address space.  The MIX = false instances are the kernels of a one-list context. */
#ifndef ICW_K2_MINWG
#define ICW_K2_MINWG 1
#endif
template <int N, bool KAHAN, bool TRIG, bool FCK = false, bool MIX = false>
__device__ __forceinline__ void icw_output_body(const IcwK2Args &a, int bx, int s, double *lregs)
{
    constexpr int TILE = ICW_K2_TILE;
    constexpr int NR = N + 1;                        /* window rows past the tile (row N+t: w[t]) */
    __shared__ double lw[2][4][TILE + 24];
    /* lregs: the DSP register file [n_regs][4][TILE] in dynamic LDS */
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    const int tl = threadIdx.x;
    const int T = a.T;
    const int tw0 = bx * TILE * a.tpw;
    const int ntile = min(a.tpw, (T - tw0 + TILE - 1) / TILE);

    /* mono input, converters bit-identical at block start (K1's flag) and in phase: the right
     * filter outputs are copies of the left ones this block */
    const bool dup = !FCK && !a.cw && a.nch == 1 && a.info_dup && a.info_dup[s * 2] && a.info_dup[s * 2 + 1] &&
                     a.hq_phase[s * 2] == a.hq_phase[s * 2 + 1];
    IcwFes fes[2] = {};
    const int nc = dup ? 2 : 4;
    /* the per-frame rotation table holds this stream's factors when its counter is in step */
    bool use_tab = TRIG && a.trig_tab && a.n_frame[s] == a.n_frame[0];
    icw_cprog *P = icw_prog_c(a.prog);
    size_t tab_off = 0;
    if constexpr (MIX) {
        const __attribute__((address_space(4))) int32_t *id = (const __attribute__((address_space(4))) int32_t *)a.prog_id;
        P += id[s];
        const int slab = id[a.n_streams + s];
        use_tab = TRIG && a.trig_tab && slab >= 0 && a.n_frame[s] == a.n_frame[id[2 * a.n_streams + s]];
        tab_off = slab >= 0 ? (size_t)slab * a.slab_stride : 0;
    }
    double pf[4][2];
    auto load_tile = [&](int k) {
        const int tt = tw0 + k * TILE;
        const int nrow = min(TILE, T - tt) + NR;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < nc) {
                const double *src = a.w + (size_t)(s * 4 + c) * a.w_pitch + tt;
                pf[c][0] = tl < nrow ? src[tl] : 0.0;
                pf[c][1] = (tl < NR && tl + TILE < nrow) ? src[tl + TILE] : 0.0;
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < nc) {
                lw[buf][c][tl] = pf[c][0];
                if (tl < NR) lw[buf][c][tl + TILE] = pf[c][1];
            }
        }
    };
    if (!a.cw) {
        load_tile(0);
        store_tile(0);
        __syncthreads();
    }

    IcwRegFile R;
    R.base = lregs + tl;
    /* slots read but never written in the frame hold their block-start values */
    for (int r = 0; r < P->n_persist; ++r) {
        const double *b = a.bus + ((size_t)s * ICW_N_INPUTS + P->persist_slot[r]) * 4;
        IcwLR v; v.lre = b[0]; v.lim = b[1]; v.rre = b[2]; v.rim = b[3];
        R.set(P->persist_reg[r], v);
    }
    /* the 2N output-sum coefficients are read from LDS (broadcast) at their one use per frame:
     * held in SGPRs they crowd out the program's operands and spill to VGPR lanes, a v_readlane
     * per use.  `zk` (a runtime zero) keeps the loads inside the tile loop. */
    __shared__ double lcoef[40];
    if (tl < 40) lcoef[tl] = tl < 20 ? a.pc[tl] : a.pd[tl - 20];
    __syncthreads();

    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    /* de-subnorm rejections of this workgroup's frames, per chain: the reject stores exactly +0.0
     * (hblpf.c:1046-1050) and every |sum| < 1 is rejected, so a w row equal to 0.0 is one count */
    const bool count_sn = !a.cw && a.sncnt;
    unsigned sn[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < ntile; ++k) {
        const bool more = !a.cw && k + 1 < ntile;
        if (more) load_tile(k + 1);
        const int t = tw0 + k * TILE + tl;
        const double (&W)[4][TILE + 24] = lw[k & 1];
        const int zk = a.zero * k;
        if (t < T) {
            const double *const w[4] = {&W[0][tl], &W[1][tl], &W[2][tl], &W[3][tl]};
            if constexpr (MIX)
                icw_output_frame<N, KAHAN, TRIG, FCK>(a, P, R, s, t, w, dup, lcoef + zk, fes, count_sn, sn, use_tab,
                                                      clip_l, clip_r, pk_l, pk_r, tab_off);
            else
                icw_output_frame<N, KAHAN, TRIG, FCK>(a, P, R, s, t, w, dup, lcoef + zk, fes, count_sn, sn, use_tab,
                                                      clip_l, clip_r, pk_l, pk_r);
        }
        if (more) {
            /* the other half was last read in tile k-1, before the previous barrier */
            store_tile((k + 1) & 1);
            __syncthreads();
        }
    }

    if constexpr (FCK) {
        icw_fes_flush(fes[0], a.fes + (size_t)s * 4 * ICW_FES_PITCH);
        icw_fes_flush(fes[1], a.fes + ((size_t)s * 4 + 1) * ICW_FES_PITCH);
    }
    if (count_sn) {
        __shared__ unsigned red_sn[4][TILE / 64];
        icw_sn_wg(a, s, sn, nc, red_sn);
    }
    if (a.do_render) icw_meters_wg(a, s, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
}

template <int N, bool KAHAN, bool TRIG, bool FCK = false, bool MIX = false>
__global__ __launch_bounds__(ICW_K2_TILE, ICW_K2_MINWG) void icw_output(IcwK2Args a)
{
    extern __shared__ __attribute__((aligned(16))) double lregs[];   /* [n_regs][4][TILE] */
    icw_output_body<N, KAHAN, TRIG, FCK, MIX>(a, blockIdx.x, blockIdx.y, lregs);
}

/* Fused FIR converter + graph + render (KF2): one workgroup per stream and 1024-frame tile (2048
 * for mono).  Wave w owns frames [256 w, 256 w + 256) of the tile: lanes 0-31 sum channel L's
 * outputs and lanes 32-63 channel R's, 8 consecutive frames each (icw_fir_sums).  A lane pair
 * (l, l + 32) then swaps half of its I / Q values (v_permlane32_swap), so lane l holds both channels
 * of frames 0-3 of its eight and lane l + 32 of frames 4-7, and each takes its 4 frames straight
 * through K2's per-frame code (icw_frame_graph: DSP list, pre-render, ROUND render, meters).  The
 * analytic signal never leaves the registers (KF + K2 move 32 B per frame through HBM twice); the
 * sums are KF's, in the same order, so the results are KF + K2's bit for bit.  Dynamic LDS: the
 * padded inputs of each computed channel, the taps, the DSP register file. */
/* Occupancy: 4 workgroups per CU (4 waves per SIMD, <= 128 VGPRs).  TAB: every stream of the launch
 * is in step with the rotation table (the host's frame-counter mirror says so), so the per-stream
 * fallback (icw_trig_call) is compiled out.  With the call in the kernel the allocator kept values
 * live across it in scratch -- 44 B per thread written to HBM, most of the kernel's 2.95x write
 * traffic (profiles/r02_c2fir_pmc.json: 198 MB per launch against 67 MB of output); giving that
 * variant 168 VGPRs instead (3 workgroups per CU) removed the spills but cost c2fir 22 %. */

/* NC: computed channels (1: mono input, 2: stereo), a template parameter so that each form gets its
 * own register allocation (the mono graph phase holds 8 frames per lane, the stereo one 4) */
#if ICW_FIR_STAMPS
/* diagnostic build only (tools/fir_phases.py): per workgroup of the last KF2 launch, wave 0's
 * shader-clock stamps at the phase boundaries and the 100 MHz clock at its start and end */
__device__ unsigned long long icw_fir_stp[(1 << 16) * 8];
#define ICW_FIR_STAMP(k)                                                                              \
    do {                                                                                              \
        if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < (1u << 16))                     \
            icw_fir_stp[(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] =                            \
                ((k) == 0 || (k) == 7) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int icw_fir_stamps_read(unsigned long long *dst, size_t n)
{
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(icw_fir_stp), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#else
#define ICW_FIR_STAMP(k) do { } while (0)
#endif

/* KF2's mono chain form: the lane's ICW_FIR_R frames (from t0, nv of them in the block) two at a time
 * through one signature (SIG; 0: the generic op loop, ROWP: rows at known offsets), the rendered
 * frames packed into w (16-bit: w[0..8), 24-bit: 12 words).  B24 is a template parameter: with a
 * runtime flag the compiler merged the two packings' stores into one store at a selected index, which
 * put w in scratch -- c3fir wrote 6.3 GB per launch against 4.3 GB of output (profiles/r05_c3fir_pmc.json) */
template <bool TRIG, int SIG, bool ROWP, bool B24>
__device__ __forceinline__ void icw_mono_passes(const IcwK2Args &a, icw_cprog *P, int s, int t0, int nv,
                                                const double (&vi)[ICW_FIR_R], const double (&q)[ICW_FIR_R],
                                                unsigned &clip_l, unsigned &clip_r, double &pk_l, double &pk_r,
                                                unsigned (&w)[ICW_FIR_R / 2 * 3], uint32_t tro_lane, size_t pq)
{
#pragma unroll
    for (int hh = 0; hh < ICW_FIR_R; hh += 2) {
        IcwLR in2[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            in2[r].lre = in2[r].rre = vi[hh + r];
            in2[r].lim = in2[r].rim = q[hh + r];
        }
        int dv[2][2];
        const int n2 = min(2, max(nv - hh, 0));
        if constexpr (!ROWP)
            icw_chain_frames<TRIG, 2>(a, P, s, t0 + hh, n2, in2, clip_l, clip_r, pk_l, pk_r, dv);
        else if constexpr (SIG != 0)
            icw_chain_frames<TRIG, 2, true, SIG>(a, P, s, t0 + hh, n2, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane,
                                                 (size_t)hh * pq, pq);
        else
            icw_chain_frames<TRIG, 2, true>(a, P, s, t0 + hh, n2, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane,
                                            (size_t)hh * pq, pq);
        if constexpr (B24) {
            const unsigned l0 = (unsigned)dv[0][0] & 0xffffffu, r0 = (unsigned)dv[0][1] & 0xffffffu;
            const unsigned l1 = (unsigned)dv[1][0] & 0xffffffu, r1 = (unsigned)dv[1][1] & 0xffffffu;
            w[hh / 2 * 3 + 0] = l0 | (r0 << 24);
            w[hh / 2 * 3 + 1] = (r0 >> 8) | (l1 << 16);
            w[hh / 2 * 3 + 2] = (l1 >> 16) | (r1 << 8);
        } else {
            w[hh] = ((unsigned)dv[0][0] & 0xffffu) | ((unsigned)dv[0][1] << 16);
            w[hh + 1] = ((unsigned)dv[1][0] & 0xffffu) | ((unsigned)dv[1][1] << 16);
        }
    }
}

/* ICW_FIR_OCC 5 (96 VGPRs) spills and ran 2.4x slower (profiles/r03_fir_swap_ab.jsonl) */
template <bool TRIG, bool TAB, int NC>
__global__ __launch_bounds__(256, ICW_FIR_OCC) void icw_fir_graph(IcwFirArgs f, IcwK2Args a)
{
    ICW_FIR_STAMP(0);
    ICW_FIR_STAMP(1);                                /* diagnostic build: 0 / 7 = 100 MHz clock, 1-6 shader clock */
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    /* workgroups in stream-fastest order (the grid is streams x tiles): the workgroups of one tile run
     * together, so its rotation-table rows come from the L2 for every stream, where tile-fastest order
     * swept the whole block's table once per stream (a 2^20-frame block's table is 32 MB: c2fir 37 HBM
     * bytes per frame against 9.4) */
    const int s = blockIdx.x;
    constexpr int nchc = NC;
    const int TF = 256 * ICW_FIR_R / nchc;
    const int tt = (blockIdx.y + f.tile0) * TF;
    const int M = f.M, c = M >> 1;
    const int sh = (8 - ((c - 1) & 7)) & 7;
    const int av = (c - 1 + sh) >> 3;
    const int nf = min(TF, f.T - tt);
    const int px = (icw_fir_phys(sh + M + TF + 24) + 2) & ~1;   /* doubles per staged channel (even) */
    double *lregs = lds + nchc * px + ((f.nt + 1) & ~1);
    icw_ctap *gs = (icw_ctap *)f.g;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ch = nchc == 2 ? lane >> 5 : 0;
    const int ll = nchc == 2 ? wv * 32 + (lane & 31) : threadIdx.x;   /* lane index within the channel */
    if (nchc == 2) icw_fir_stage<2>(f, s, 0, lds, px, tt, TF, sh, threadIdx.x, 256);
    else icw_fir_stage<1>(f, s, 0, lds, px, tt, TF, sh, threadIdx.x, 256);
    ICW_FIR_STAMP(2);
    __syncthreads();
    ICW_FIR_STAMP(3);
    double q[ICW_FIR_R], vi[ICW_FIR_R];
#if ICW_FIR_CUT >= 2
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) q[r] = 0.0;
#else
    icw_fir_sums(lds + ch * px, gs, f.nt, ll, av, sh, c, q);
#endif
    const int ix = 8 * av + 1;                               /* logical index of x[tt - c] */
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) vi[r] = lds[ch * px + icw_fir_phys(ICW_FIR_R * ll + r + ix)];
#if ICW_FIR_STAMPS
    if (threadIdx.x == 0 && q[0] + vi[0] == 1.2345e300) icw_fir_stp[0] = 1;     /* the sums before stamp 4 */
#endif
    ICW_FIR_STAMP(4);
#if ICW_FIR_CUT
    /* diagnostic build only (VALU accounting by phase): no graph, no render */
    {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < ICW_FIR_R; ++r) acc += q[r] + vi[r];
        if (acc == 1.2345e300) a.out[threadIdx.x] = 1;
        return;
    }
#endif

    icw_cprog *P = icw_prog_c(a.prog);
    IcwRegFile Rf;
    Rf.base = lregs + threadIdx.x;
    for (int r = 0; r < P->n_persist; ++r) {
        const double *b = a.bus + ((size_t)s * ICW_N_INPUTS + P->persist_slot[r]) * 4;
        IcwLR v; v.lre = b[0]; v.lim = b[1]; v.rre = b[2]; v.rim = b[3];
        Rf.set(P->persist_reg[r], v);
    }
    const bool use_tab = TAB || (TRIG && a.trig_tab && a.n_frame[s] == a.n_frame[0]);
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    if (nchc == 2) {
        /* lane l (L) keeps frames 0-3 and gets R's values of them; lane l + 32 (R) frames 4-7.  Their
         * rendered frames are stored together: lane l's four at byte 32 ll, lane l + 32's at 32 ll + 16
         * (16-bit output), so one 16-byte store per lane covers the wave's 1 KB contiguously.  One
         * 4-byte store per frame instead put 2 of every 32 bytes in each store instruction, and the L2
         * wrote the partial sectors out 2.3x over (r03_c2fir_pmc.json before this change: WRITE_SIZE
         * 153 MB per launch against 67 MB of output). */
        const int h = ch ? 4 : 0;
        int dv[4][2];
        const int fr0 = ICW_FIR_R * ll + h;
        if (ICW_CHAIN4 && P->chain && (TAB || !TRIG) && !a.iq_out && a.do_render && !a.dith) {
            /* chain program, factors from the table (or none): the four frames op by op, two per
             * pass (four at once spill at 128 VGPRs), each pass's I / Q exchange just before it.
             * Frame tt + fr0 + hh + j (tt a multiple of 8, fr0 = 8 ll + h) sits in table row
             * (h + hh + j) q + tt / 8 + ll (icw_trig_index, q = trig_perm_q): a per-lane part and a
             * uniform one.  The last tile of a launch block keeps the clamped index (frames past
             * the block would point past the table). */
            const bool rowp = (TRIG || P->sig) && tt + TF <= f.T;
            const int sig = P->sig;
            const size_t pq = (size_t)a.trig_perm_q * a.trig_pitch;
            const uint32_t tro_lane = (uint32_t)(((size_t)h * a.trig_perm_q + (size_t)(tt >> 3) + ll) * a.trig_pitch);
#pragma unroll
            for (int hh = 0; hh < 4; hh += 2) {
                IcwLR in2[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int r = hh + j;
                    double xl = vi[r], xr = vi[r + 4], yl = q[r], yr = q[r + 4];
                    icw_swap32(xl, xr);
                    icw_swap32(yl, yr);
                    in2[j].lre = xl; in2[j].lim = yl; in2[j].rre = xr; in2[j].rim = yr;
                }
                int dv2[2][2];
                if (rowp)
                    icw_chain_frames_rowp<TRIG, 2>(a, P, sig, s, tt + fr0 + hh, min(2, max(nf - fr0 - hh, 0)), in2, clip_l,
                                                   clip_r, pk_l, pk_r, dv2, tro_lane, (size_t)hh * pq, pq);
                else
                    icw_chain_frames<TRIG, 2>(a, P, s, tt + fr0 + hh, min(2, max(nf - fr0 - hh, 0)), in2, clip_l, clip_r,
                                              pk_l, pk_r, dv2);
                dv[hh][0] = dv2[0][0]; dv[hh][1] = dv2[0][1];
                dv[hh + 1][0] = dv2[1][0]; dv[hh + 1][1] = dv2[1][1];
            }
        } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double xl = vi[r], xr = vi[r + 4], yl = q[r], yr = q[r + 4];
            icw_swap32(xl, xr);
            icw_swap32(yl, yr);
            const int fr = fr0 + r;
            dv[r][0] = dv[r][1] = 0;
            if (fr < nf) {
                IcwLR in;
                in.lre = xl; in.lim = yl; in.rre = xr; in.rim = yr;
                icw_frame_graph<TRIG, TAB, true>(a, P, Rf, s, tt + fr, in, use_tab, clip_l, clip_r, pk_l, pk_r, dv[r]);
            }
        }
        }
        if (a.do_render && !a.iq_out) {
            unsigned char *o = a.out + (size_t)s * a.out_stride;
            const int nv = min(4, nf - fr0);
            if (a.rk.is24) {
                /* 6 bytes per frame: 24 contiguous bytes per lane */
                unsigned char *p = o + (size_t)(tt + fr0) * 6;
                if (nv == 4 && !((uintptr_t)p & 7)) {
                    unsigned w[6];
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        const unsigned l0 = (unsigned)dv[r][0] & 0xffffffu, r0 = (unsigned)dv[r][1] & 0xffffffu;
                        const unsigned l1 = (unsigned)dv[r + 1][0] & 0xffffffu, r1 = (unsigned)dv[r + 1][1] & 0xffffffu;
                        w[r / 2 * 3 + 0] = l0 | (r0 << 24);
                        w[r / 2 * 3 + 1] = (r0 >> 8) | (l1 << 16);
                        w[r / 2 * 3 + 2] = (l1 >> 16) | (r1 << 8);
                    }
                    uint2 *q2 = (uint2 *)p;
                    q2[0] = make_uint2(w[0], w[1]);
                    q2[1] = make_uint2(w[2], w[3]);
                    q2[2] = make_uint2(w[4], w[5]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (r >= nv) break;
                        unsigned char *b = p + r * 6;
                        const int vl = dv[r][0], vr = dv[r][1];
                        b[0] = (unsigned char)vl; b[1] = (unsigned char)(vl >> 8); b[2] = (unsigned char)(vl >> 16);
                        b[3] = (unsigned char)vr; b[4] = (unsigned char)(vr >> 8); b[5] = (unsigned char)(vr >> 16);
                    }
                }
            } else {
                unsigned pk[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) pk[r] = ((unsigned)dv[r][0] & 0xffffu) | ((unsigned)dv[r][1] << 16);
                unsigned *p = (unsigned *)(o + (size_t)(tt + fr0) * 4);
                if (nv == 4 && !((uintptr_t)p & 15)) {
                    *(uint4 *)p = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r < nv) p[r] = pk[r];
                }
            }
        }
    } else if (ICW_CHAIN4 && P->chain && (TAB || !TRIG) && !a.iq_out && a.do_render && !a.dith) {
        /* mono input, chain program: the lane's 8 frames op by op, two at a time, and their 8
         * rendered frames stored together (32 / 48 contiguous bytes per lane) */
        const int fr0 = ICW_FIR_R * ll;
        const bool b24 = a.rk.is24;
        unsigned w[ICW_FIR_R / 2 * 3];               /* packed output: 16-bit frames in w[0..8) */
        /* table rows as in the stereo form: frame tt + 8 ll + hh + j at row (hh + j) q + tt / 8 + ll */
        const bool rowp = (TRIG || P->sig) && tt + TF <= f.T;
        const int sig = P->sig;
        const size_t pq = (size_t)a.trig_perm_q * a.trig_pitch;
        const uint32_t tro_lane = (uint32_t)(((size_t)(tt >> 3) + ll) * a.trig_pitch);
        /* the signature is chosen once for the lane's four passes (inside the pass loop every pass
         * carried all variants while the eight inputs stayed live, and the rotating kernel spilled) */
#define ICW_MONO(SIGV, RP)                                                                                    \
    do {                                                                                                      \
        if (b24) icw_mono_passes<TRIG, SIGV, RP, true>(a, P, s, tt + fr0, nf - fr0, vi, q, clip_l, clip_r, pk_l,  \
                                                       pk_r, w, tro_lane, pq);                                \
        else icw_mono_passes<TRIG, SIGV, RP, false>(a, P, s, tt + fr0, nf - fr0, vi, q, clip_l, clip_r, pk_l,    \
                                                    pk_r, w, tro_lane, pq);                                   \
    } while (0)
        if (!rowp) {
            ICW_MONO(0, false);
        } else if constexpr (TRIG) {
            switch (sig) {
            case ICW_SIG_M:
            case ICW_SIG_M | ICW_SIG_UNIT: ICW_MONO(ICW_SIG_M | ICW_SIG_UNIT, true); break;
            case ICW_SIG_SM: ICW_MONO(ICW_SIG_SM, true); break;
            case ICW_SIG_SM | ICW_SIG_UNIT: ICW_MONO(ICW_SIG_SM | ICW_SIG_UNIT, true); break;
            case ICW_SIG_PSXM: ICW_MONO(ICW_SIG_PSXM, true); break;
            case ICW_SIG_PSXM | ICW_SIG_UNIT: ICW_MONO(ICW_SIG_PSXM | ICW_SIG_UNIT, true); break;
            default: ICW_MONO(0, true); break;
            }
        } else {
            if (sig == ICW_SIG_M || sig == (ICW_SIG_M | ICW_SIG_UNIT)) ICW_MONO(ICW_SIG_M | ICW_SIG_UNIT, true);
            else ICW_MONO(0, true);
        }
#undef ICW_MONO
        unsigned char *o = a.out + (size_t)s * a.out_stride;
        const int nv = min(ICW_FIR_R, max(nf - fr0, 0));
        if (b24) {
            unsigned char *p = o + (size_t)(tt + fr0) * 6;
            if (nv == ICW_FIR_R && !((uintptr_t)p & 7)) {
                uint2 *q2 = (uint2 *)p;
#pragma unroll
                for (int i = 0; i < ICW_FIR_R / 2 * 3 / 2; ++i) q2[i] = make_uint2(w[2 * i], w[2 * i + 1]);
            } else {
                /* byte r of the packed run is byte r of the output */
#pragma unroll
                for (int i = 0; i < ICW_FIR_R * 6; ++i)
                    if (i < nv * 6) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            unsigned *p = (unsigned *)(o + (size_t)(tt + fr0) * 4);
            if (nv == ICW_FIR_R && !((uintptr_t)p & 15)) {
                *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
                *(uint4 *)(p + 4) = make_uint4(w[4], w[5], w[6], w[7]);
            } else {
#pragma unroll
                for (int r = 0; r < ICW_FIR_R; ++r)
                    if (r < nv) p[r] = w[r];
            }
        }
    } else {
#pragma unroll 1
        for (int r = 0; r < ICW_FIR_R; ++r) {
            const int fr = ICW_FIR_R * ll + r;
            if (fr < nf) {
                IcwLR in;
                in.lre = in.rre = vi[r];
                in.lim = in.rim = q[r];
                icw_frame_graph<TRIG, TAB>(a, P, Rf, s, tt + fr, in, use_tab, clip_l, clip_r, pk_l, pk_r);
            }
        }
    }
    ICW_FIR_STAMP(5);
    if (a.do_render) icw_meters_wg(a, s, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
    ICW_FIR_STAMP(6);
    ICW_FIR_STAMP(7);
}

/* KF2's signature form (icw_fir_sig): the tiles of a launch block before the one holding its last
 * frame, for a chain program of one of the specialised signatures (ICW_SIG_*), a ROUND / flat render
 * and no pre-render doubles -- the production form of the BASELINE FIR legs.  Every lane then takes
 * icw_chain_frames' render-only branch (full frames, no block-end bus write), so the kernel holds only
 * the staging, the sums, that branch (SIG and the output depth B24 at compile time) and the meters:
 * icw_fir_graph's register allocation is set by its generic paths (the per-frame graph, the exact
 * chain pass, the runtime signature switch), and their scalars spilled to VGPR lanes in the hot
 * phases.  icw_launch_fir_graph runs the last tile of each stream through icw_fir_graph (tile0).
 * Same staging, sums and render arithmetic, so the bytes and meters are icw_fir_graph's. */
/* Occupancy of the signature form: without the generic paths it fits 114 VGPRs at 4 workgroups per CU,
 * no scratch.  It also fits 96 (5 per CU) with 4-tap register blocks in the sums, and the mono form 80
 * (6 per CU): measured the same within the box noise (c2fir -1 / +1.7 %, c4fir +0.5 / +0.8 %, c3fir
 * -1.9 / +0.2 %, profiles/r06_fir_sig_ab.txt) with 24 more VALU and 48 more LDS instructions per wave,
 * so the FP64 pipe, not latency, bounds it at 4. */
#ifndef ICW_FIR_SIG_OCC
#define ICW_FIR_SIG_OCC 4
#endif
#ifndef ICW_FIR_SIG_OCC1
#define ICW_FIR_SIG_OCC1 4                           /* the mono form */
#endif
#ifndef ICW_FIR_SIG_NTAP
#define ICW_FIR_SIG_NTAP ICW_FIR_NTAP
#endif
template <int SIG, int NC, bool B24>
__global__ __launch_bounds__(256, NC == 2 ? ICW_FIR_SIG_OCC : ICW_FIR_SIG_OCC1) void icw_fir_sig(IcwFirArgs f, IcwK2Args a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    constexpr bool TRIG = (SIG & ~ICW_SIG_UNIT) != ICW_SIG_M;
    constexpr int TF = 256 * ICW_FIR_R / NC;
    const int s = blockIdx.x;
    const int tt = blockIdx.y * TF;
    const int M = f.M, c = M >> 1;
    const int sh = (8 - ((c - 1) & 7)) & 7;
    const int av = (c - 1 + sh) >> 3;
    const int px = (icw_fir_phys(sh + M + TF + 24) + 2) & ~1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ch = NC == 2 ? lane >> 5 : 0;
    const int ll = NC == 2 ? wv * 32 + (lane & 31) : threadIdx.x;
    icw_fir_stage<NC>(f, s, 0, lds, px, tt, TF, sh, threadIdx.x, 256);
    __syncthreads();
    double q[ICW_FIR_R], vi[ICW_FIR_R];
    icw_fir_sums<ICW_FIR_SIG_NTAP>(lds + ch * px, (icw_ctap *)f.g, f.nt, ll, av, sh, c, q);
    const int ix = 8 * av + 1;
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) vi[r] = lds[ch * px + icw_fir_phys(ICW_FIR_R * ll + r + ix)];
    icw_cprog *P = icw_prog_c(a.prog);
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    const size_t pq = (size_t)a.trig_perm_q * a.trig_pitch;
    unsigned char *o = a.out + (size_t)s * a.out_stride;
    if constexpr (NC == 2) {
        /* lane l (L) frames 0-3 of its eight with R's values swapped in, lane l + 32 frames 4-7 */
        const int h = ch ? 4 : 0;
        const int fr0 = ICW_FIR_R * ll + h;
        const uint32_t tro_lane = (uint32_t)(((size_t)h * a.trig_perm_q + (size_t)(tt >> 3) + ll) * a.trig_pitch);
        int dv[4][2];
#pragma unroll
        for (int hh = 0; hh < 4; hh += 2) {
            IcwLR in2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int r = hh + j;
                double xl = vi[r], xr = vi[r + 4], yl = q[r], yr = q[r + 4];
                icw_swap32(xl, xr);
                icw_swap32(yl, yr);
                in2[j].lre = xl; in2[j].lim = yl; in2[j].rre = xr; in2[j].rim = yr;
            }
            int dv2[2][2];
            icw_sig_fast<TRIG, 2, SIG>(a, P, in2, clip_l, clip_r, pk_l, pk_r, dv2, tro_lane, (size_t)hh * pq, pq);
            dv[hh][0] = dv2[0][0]; dv[hh][1] = dv2[0][1];
            dv[hh + 1][0] = dv2[1][0]; dv[hh + 1][1] = dv2[1][1];
        }
        if constexpr (B24) {
            unsigned char *p = o + (size_t)(tt + fr0) * 6;
            unsigned w[6];
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const unsigned l0 = (unsigned)dv[r][0] & 0xffffffu, r0 = (unsigned)dv[r][1] & 0xffffffu;
                const unsigned l1 = (unsigned)dv[r + 1][0] & 0xffffffu, r1 = (unsigned)dv[r + 1][1] & 0xffffffu;
                w[r / 2 * 3 + 0] = l0 | (r0 << 24);
                w[r / 2 * 3 + 1] = (r0 >> 8) | (l1 << 16);
                w[r / 2 * 3 + 2] = (l1 >> 16) | (r1 << 8);
            }
            if (!((uintptr_t)p & 7)) {
                uint2 *q2 = (uint2 *)p;
                q2[0] = make_uint2(w[0], w[1]);
                q2[1] = make_uint2(w[2], w[3]);
                q2[2] = make_uint2(w[4], w[5]);
            } else {
#pragma unroll
                for (int i = 0; i < 24; ++i) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            unsigned pk[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) pk[r] = ((unsigned)dv[r][0] & 0xffffu) | ((unsigned)dv[r][1] << 16);
            unsigned *p = (unsigned *)(o + (size_t)(tt + fr0) * 4);
            if (!((uintptr_t)p & 15)) {
                *(uint4 *)p = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = pk[r];
            }
        }
    } else {
        /* mono: the lane's 8 frames two at a time, packed as icw_mono_passes does */
        const int fr0 = ICW_FIR_R * ll;
        const uint32_t tro_lane = (uint32_t)(((size_t)(tt >> 3) + ll) * a.trig_pitch);
        int dl[ICW_FIR_R], dr[ICW_FIR_R];
        if (!TRIG && f.lr_same) {
            /* both channels run the same arithmetic on the same inputs (mono input, a Master whose two
             * gains are the same double: icw_launch_fir_graph's lr_same), so a pass takes two frames in
             * its L / R slots and each result serves both channels: half the graph and render */
#pragma unroll
            for (int hh = 0; hh < ICW_FIR_R; hh += 4) {
                IcwLR in2[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    in2[r].lre = vi[hh + 2 * r];
                    in2[r].lim = q[hh + 2 * r];
                    in2[r].rre = vi[hh + 2 * r + 1];
                    in2[r].rim = q[hh + 2 * r + 1];
                }
                int dv[2][2];
                icw_sig_fast<TRIG, 2, SIG>(a, P, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, 0, pq);
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) dl[hh + 2 * r + c] = dr[hh + 2 * r + c] = dv[r][c];
            }
            /* the slots held frames: every frame's clips and peak count for both channels */
            clip_l = clip_r = clip_l + clip_r;
            pk_l = pk_r = icw_vmax(pk_l, pk_r);
        } else {
#pragma unroll
            for (int hh = 0; hh < ICW_FIR_R; hh += 2) {
                IcwLR in2[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    in2[r].lre = in2[r].rre = vi[hh + r];
                    in2[r].lim = in2[r].rim = q[hh + r];
                }
                int dv[2][2];
                icw_sig_fast<TRIG, 2, SIG>(a, P, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, (size_t)hh * pq, pq);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    dl[hh + r] = dv[r][0];
                    dr[hh + r] = dv[r][1];
                }
            }
        }
        unsigned w[ICW_FIR_R / 2 * 3];
#pragma unroll
        for (int hh = 0; hh < ICW_FIR_R; hh += 2) {
            if constexpr (B24) {
                const unsigned l0 = (unsigned)dl[hh] & 0xffffffu, r0 = (unsigned)dr[hh] & 0xffffffu;
                const unsigned l1 = (unsigned)dl[hh + 1] & 0xffffffu, r1 = (unsigned)dr[hh + 1] & 0xffffffu;
                w[hh / 2 * 3 + 0] = l0 | (r0 << 24);
                w[hh / 2 * 3 + 1] = (r0 >> 8) | (l1 << 16);
                w[hh / 2 * 3 + 2] = (l1 >> 16) | (r1 << 8);
            } else {
                w[hh] = ((unsigned)dl[hh] & 0xffffu) | ((unsigned)dr[hh] << 16);
                w[hh + 1] = ((unsigned)dl[hh + 1] & 0xffffu) | ((unsigned)dr[hh + 1] << 16);
            }
        }
        if constexpr (B24) {
            unsigned char *p = o + (size_t)(tt + fr0) * 6;
            if (!((uintptr_t)p & 7)) {
                uint2 *q2 = (uint2 *)p;
#pragma unroll
                for (int i = 0; i < ICW_FIR_R / 2 * 3 / 2; ++i) q2[i] = make_uint2(w[2 * i], w[2 * i + 1]);
            } else {
#pragma unroll
                for (int i = 0; i < ICW_FIR_R * 6; ++i) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            unsigned *p = (unsigned *)(o + (size_t)(tt + fr0) * 4);
            if (!((uintptr_t)p & 15)) {
                *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
                *(uint4 *)(p + 4) = make_uint4(w[4], w[5], w[6], w[7]);
            } else {
#pragma unroll
                for (int r = 0; r < ICW_FIR_R; ++r) p[r] = w[r];
            }
        }
    }
    icw_meters_wg(a, s, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
}

/* Per-frame rotation table: the Shift / PM factors of frame t depend only on the modulator frame
 * counter, which all streams of a batch share while they are in step (same call-start counter).
 * One thread per frame evaluates each active channel's factor once (icw_trig, the same code as
 * the inline path); K2 reads the row instead of running fmod / sin / sincos per stream. */
/* y: the slab (per-stream DSP lists, a.slabs: program y's factors at its reference stream's counter) */
template <bool SLAB = false>
__device__ __forceinline__ void icw_trig_row(const IcwTrigArgs &a, int t, int y = 0)
{
    icw_cprog *P = icw_prog_c(a.prog);
    int ref = 0;
    double *tab = a.tab;
    if constexpr (SLAB) {
        const __attribute__((address_space(4))) int32_t *sl = (const __attribute__((address_space(4))) int32_t *)a.slabs;
        P += sl[y];
        ref = sl[a.n_slabs + y];
        tab += (size_t)y * a.slab_stride;
    }
    const double omega = icw_omega(a.n_frame[ref], a.t0 + t, a.scaled, a.ssr, a.sample_rate);
    double *row = tab + icw_trig_index(t, a.perm_q) * a.trig_pitch;
    for (int oi = 0; oi < P->n_ops; ++oi) {
        icw_cop &op = P->ops[oi];
        if (op.mode != ICW_MODE_SHIFT && op.mode != ICW_MODE_PM) continue;
        for (int c = 0; c < 2; ++c) {
            if (!op.act[c]) continue;
            double cs, sn;
            icw_trig(op, c, omega, cs, sn);
            row[op.tslot[c] * 2] = cs;
            row[op.tslot[c] * 2 + 1] = sn;
        }
    }
}

__global__ __launch_bounds__(256) void icw_trig_table(IcwTrigArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    if (a.slabs) icw_trig_row<true>(a, t, blockIdx.y);
    else icw_trig_row(a, t);
}

/* ------------------------------------------------------- serial graph kernel (K4) ------ */
/* Bus form of the DSP list, for lists whose nodes read a slot before it is written in the frame
 * (a one-frame delay -- feedback loops included): the reference's own per-frame semantics
 * (adv_modulator.c:636-751) with the 27-slot bus of the stream held in LDS, one lane per stream,
 * frames in order.  `in` comes from the output kernel (Hilbert or complex input), lOut/rOut go
 * to the serial render kernel. */
__global__ __launch_bounds__(64) void icw_graph_serial(IcwK4Args a)
{
    __shared__ double bus[ICW_N_INPUTS * 4][64];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * 64 + lane;
    if (s >= a.n_streams) return;
    double *gb = a.bus + (size_t)s * ICW_N_INPUTS * 4;
    for (int k = 0; k < ICW_N_INPUTS * 4; ++k) bus[k][lane] = gb[k];
    icw_cprog *P = icw_prog_c(a.prog);
    const unsigned long long n0 = a.n_frame[s];
    const double *iq = a.iq + (size_t)s * a.T * 4;
    double *pre = a.pre + (size_t)s * a.pre_stride;
    for (int t = 0; t < a.T; ++t) {
        const double omega = P->needs_omega ? icw_omega(n0, a.t0 + t, a.scaled, a.ssr, a.sample_rate) : 0.0;
        bus[0][lane] = iq[(size_t)t * 4 + 0];
        bus[1][lane] = iq[(size_t)t * 4 + 1];
        bus[2][lane] = iq[(size_t)t * 4 + 2];
        bus[3][lane] = iq[(size_t)t * 4 + 3];
        double lOut = 0.0, rOut = 0.0;
        for (int oi = 0; oi < P->n_ops; ++oi) {
            icw_cop &op = P->ops[oi];
            IcwLR d;
            if (P->bypass) {
                d.lre = bus[0][lane]; d.lim = bus[1][lane]; d.rre = bus[2][lane]; d.rim = bus[3][lane];
            } else {
                d.lre = d.lim = d.rre = d.rim = 0.0;
                const uint32_t m = op.in_mask;
                for (int k = 0; k < ICW_N_INPUTS; ++k) {
                    if (!((m >> k) & 1u)) continue;
                    d.lre += bus[k * 4 + 0][lane]; d.lim += bus[k * 4 + 1][lane];
                    d.rre += bus[k * 4 + 2][lane]; d.rim += bus[k * 4 + 3][lane];
                }
            }
            IcwLR o;
            if (icw_exec_op(op, d, omega, o, lOut, rOut)) {
                const int q = op.out_slot * 4;
                bus[q + 0][lane] = o.lre; bus[q + 1][lane] = o.lim; bus[q + 2][lane] = o.rre; bus[q + 3][lane] = o.rim;
            }
        }
        pre[(size_t)t * 2] = lOut;
        pre[(size_t)t * 2 + 1] = rOut;
    }
    for (int k = 0; k < ICW_N_INPUTS * 4; ++k) gb[k] = bus[k][lane];
}

/* Call-end bookkeeping: the reader position, the Hilbert phases (not for complex input -- the
 * converters were not called) and the modulator frame counter advance by the call's frames. */
__device__ __forceinline__ void icw_advance_stream(const IcwAdvArgs &a, int s)
{
    a.pos[s] += a.n;
    if (!a.cw) {
        a.hq_phase[s * 2 + 0] = (a.hq_phase[s * 2 + 0] + (unsigned)a.n) & 3u;
        a.hq_phase[s * 2 + 1] = (a.hq_phase[s * 2 + 1] + (unsigned)a.n) & 3u;
    }
    const unsigned long long n0 = a.n_frame[s];
    a.n_frame[s] = a.scaled ? (n0 + (unsigned long long)a.n) % a.ssr : n0 + (unsigned long long)a.n;
    if (s == 0 && a.err_copy) *a.err_copy = *a.err;
}

__global__ __launch_bounds__(64) void icw_advance(IcwAdvArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s < a.n_streams) icw_advance_stream(a, s);
}

/* K5's overlapped form (a.ovl, the launcher checks that the rows fit in LDS): after K0, waves 0-1
 * run the recurrence with its w rows in LDS and publish how many frames are final
 * (icw_iir_row_body<N, true>); waves 2-3 take the output phase frame by frame behind it -- wave w
 * the 64-frame groups g = w, w + 2, ..: the group's rotation factors (no dependence on the
 * recurrence), then, once its rows are final, its outputs.  The output phase's ~20 us (576 frames)
 * but its last group hide behind the recurrence.  Per frame the same code as K2 (icw_output_frame),
 * so the results are the pipeline's bit for bit. */
__device__ __forceinline__ void icw_s1_stamp(unsigned long long *stp, int k)
{
    if (stp && threadIdx.x == 0) {
        stp[2 * k] = __builtin_amdgcn_s_memtime();
        stp[2 * k + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

template <int N, bool TRIG>
__device__ __forceinline__ void icw_s1_overlapped(const IcwS1Args &a, double *lregs)
{
    auto stamp = [&a](int k) { icw_s1_stamp(a.stamps, k); };
    __shared__ double coef[40];
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS], red_sn[4][ICW_K2_TILE / 64];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    const IcwK2Args &a2 = a.k2;
    const int tid = threadIdx.x, T = a2.T;
    double *rows = lregs + a.rows_off;
    int *prog = (int *)(rows + (size_t)4 * a.lpitch);
    if (tid < 2) prog[tid] = 0;
    if (tid < 40) coef[tid] = tid < 20 ? a2.pc[tid] : a2.pd[tid - 20];
    /* mono input with bit-identical converters in phase (K2's `dup`): the flags as the block starts,
     * read before the recurrence updates them */
    const bool dup = a2.nch == 1 && a.k1.lr_equal[0] && a.k1.lr_equal[1] && a2.hq_phase[0] == a2.hq_phase[1];
    __syncthreads();
    stamp(1);
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    unsigned sn[4] = {0u, 0u, 0u, 0u};
    const bool count_sn = a2.sncnt != nullptr;
    if (tid < 128) {
        icw_iir_row_body<N, true>(a.k1, tid, rows, a.lpitch, prog);
    } else {
        const int k = tid - 128, w2 = k >> 6, lane = k & 63;
        icw_cprog *P = icw_prog_c(a2.prog);
        IcwRegFile R;
        R.base = lregs + tid;
        for (int r = 0; r < P->n_persist; ++r) {
            const double *b = a2.bus + (size_t)P->persist_slot[r] * 4;
            IcwLR v; v.lre = b[0]; v.lim = b[1]; v.rre = b[2]; v.rim = b[3];
            R.set(P->persist_reg[r], v);
        }
        const bool use_tab = TRIG && a2.trig_tab;
        IcwFes fes[2] = {};
        const volatile __attribute__((address_space(3))) int *vp = (__attribute__((address_space(3))) int *)prog;
        for (int g = w2; g * 64 < T; g += 2) {
            const int t = g * 64 + lane;
            const int need = min(g * 64 + 64, T);
            if (a.has_trig && t < T) icw_trig_row(a.trig, t);
            /* bounded: a recurrence that never published (never in a healthy run) flags the call's
             * error and the wave goes on, so the grid drains */
            for (unsigned spin = 0; min(vp[0], vp[1]) < need; ++spin) {
                if (spin >= (1u << 24)) {
                    if (lane == 0 && a.k1.err) atomicOr(a.k1.err, 1);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            asm volatile("" ::: "memory");
            if (t < T) {
                const size_t lp = a.lpitch;
                const double *const w[4] = {rows + t, rows + lp + t, rows + 2 * lp + t, rows + 3 * lp + t};
                icw_output_frame<N, true, TRIG, false>(a2, P, R, 0, t, w, dup, coef + a2.zero * g, fes, count_sn,
                                                       sn, use_tab, clip_l, clip_r, pk_l, pk_r);
            }
        }
    }
    __syncthreads();
    stamp(2);
    if (count_sn) icw_sn_wg(a2, 0, sn, dup ? 2 : 4, red_sn);
    icw_meters_wg(a2, 0, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
    stamp(3);
}

/* K5 icw_stream1: one stream's whole launch block in ONE workgroup -- the per-call form of the
 * drop-in boundary (icw_amod_process_samples: playback.c:619 renders 576-frame blocks, NS_PERTIME,
 * in_cwave.h:133).  The pipeline's four launches (K0, K1r, K2, icw_advance) and their ~6 us gaps
 * become phases of one kernel, separated by workgroup barriers; each phase runs the same device
 * code as its kernel, so the results are the pipeline's bit for bit:
 *   1. all 256 threads: unpack + fade + quadrature mix of the block (K0) into the xd rows;
 *   2. waves 0-1: the row-broadcast recurrence (K1r: filter f = wave, one 16-lane row per channel);
 *   3. all threads: output sums, un-mix, DSP list, ROUND render, meters (K2, a.tpw tiles of 256);
 *   4. thread 0: reader position, Hilbert phases, frame counter (icw_advance).
 * The stores of one phase reach the next one's loads through the barrier's workgroup-scope
 * release / acquire (one CU, one vector L1). */
template <int N, bool TRIG>
__global__ __launch_bounds__(ICW_K2_TILE) void icw_stream1(IcwS1Args a)
{
    extern __shared__ __attribute__((aligned(16))) double lregs[];   /* K2's register file */
    /* diagnostic build only (ICW_S1_STAMPS, tools/s1_phases.py): shader-clock and 100 MHz stamps at
     * the phase boundaries */
    auto stamp = [&a](int k) { icw_s1_stamp(a.stamps, k); };
    stamp(0);
    /* K0: all the block's loads first (the zero-copy input is read across PCIe: one round trip per
     * pass instead of one per frame -- a frame's stores could alias the next frame's loads), then the
     * fades and the stores */
    const IcwK0Args &a0 = a.k0;
    const bool mono = a0.nch == 1;
    icw_fmt_dispatch(a0.fmt, (uintptr_t)a0.in | (uintptr_t)a0.fsz, [&](auto fc, auto ac) {
        constexpr int F = decltype(fc)::value;
        constexpr bool AL = decltype(ac)::value != 0;
        for (int t0 = 0; t0 < a0.T; t0 += 4 * ICW_K2_TILE) {
            double v[4][2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = t0 + k * ICW_K2_TILE + (int)threadIdx.x;
                if (t < a0.T) {
                    const unsigned char *fp = a0.in + (size_t)t * a0.fsz;
                    v[k][0] = icw_unpack_f<F, AL>(fp);
                    v[k][1] = mono ? v[k][0] : icw_unpack_f<F, AL>(fp + a0.csz);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = t0 + k * ICW_K2_TILE + (int)threadIdx.x;
                if (t < a0.T) icw_store_frame(a0, t, 0, v[k]);
            }
        }
    });
    if (a.ovl) {
        icw_s1_overlapped<N, TRIG>(a, lregs);
    } else {
        __syncthreads();
        stamp(1);
        /* waves 0-1 (SIMDs 0, 1): the recurrence; waves 2-3 (SIMDs 2, 3), idle otherwise: the block's
         * Shift / PM rotation factors, which depend only on the frame counter, for the output phase */
        if (threadIdx.x < 128) icw_iir_row_body<N>(a.k1, threadIdx.x);
        else if (a.has_trig)
            for (int t = (int)threadIdx.x - 128; t < a.trig.T; t += 128) icw_trig_row(a.trig, t);
        __syncthreads();
        stamp(2);
        icw_output_body<N, true, TRIG>(a.k2, 0, 0, lregs);
        __syncthreads();
        stamp(3);
    }
    if (a.adv.done) {
        /* every wave waits for its own zero-copy output stores to be acknowledged before the barrier
         * (a workgroup-scope release need not wait on vmcnt outside threadgroup-split mode), so thread
         * 0's system-scope fence below covers the whole workgroup's output, not only wave 0's */
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        icw_advance_stream(a.adv, 0);
        if (a.adv.done) {
            /* write the output and the error flag back to host memory, then the call's sequence
             * number the host polls for */
            __threadfence_system();
            __hip_atomic_store(a.adv.done, a.adv.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

/* ---------------------------------------------------------------- launch wrappers ------- */
extern "C" hipError_t icw_launch_unpack(const IcwK0Args *a, hipStream_t st)
{
    dim3 grid((a->T + 255) / 256, a->n_streams);
    hipLaunchKernelGGL(icw_unpack_frames, grid, dim3(256), 0, st, *a);
    return hipGetLastError();
}

/* dynamic LDS of the FIR kernels: staged channels (padded), taps, Q, the DSP register file */
static size_t fir_lds(int M, int nt, int nchc, int tf, int n_regs)
{
    const int sh = (8 - ((M / 2 - 1) & 7)) & 7;
    const int nl = sh + M + tf + 24;
    const size_t px = (size_t)(nl + ICW_FIR_PAD * (nl >> 3) + 2) & ~(size_t)1;
    return ((size_t)nchc * px + (size_t)((nt + 1) & ~1) + (size_t)nchc * tf + (size_t)n_regs * 4 * ICW_K2_TILE) *
           sizeof(double);
}

static bool fir_ok(int M, int nt)
{
    return M >= 2 && M <= ICW_FIR_MAX_M && !(M & 1) && nt >= 1 && 2 * nt - 1 <= M / 2;
}

/* LDS above 64 KB per workgroup needs the kernel attribute (gfx950: 160 KB per CU) */
static hipError_t fir_lds_attr(const void *fn, size_t lds)
{
    return lds > 64 * 1024 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

extern "C" hipError_t icw_launch_fir(const IcwFirArgs *a, hipStream_t st)
{
    if (!fir_ok(a->M, a->nt)) return hipErrorInvalidValue;
    constexpr int TF = 256 * ICW_FIR_R;
    const size_t lds = fir_lds(a->M, a->nt, 1, TF, 0);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (fir_lds_attr((const void *)icw_fir_hilbert, lds) != hipSuccess) return hipErrorInvalidValue;
    dim3 grid((a->T + TF - 1) / TF, a->nch > 1 ? 2 : 1, a->n_streams);
    hipLaunchKernelGGL(icw_fir_hilbert, grid, dim3(256), lds, st, *a);
    return hipGetLastError();
}

/* bytes of dynamic LDS the fused converter needs (0: more than a workgroup may hold -- run KF + K2) */
extern "C" size_t icw_fir_graph_lds(int M, int nt, int nch, int n_regs)
{
    const int nchc = nch > 1 ? 2 : 1;
    const size_t lds = fir_lds(M, nt, nchc, 256 * ICW_FIR_R / nchc, n_regs) - (size_t)256 * ICW_FIR_R * sizeof(double);
    return lds <= 96 * 1024 ? lds : 0;
}

/* in_step: every stream of the launch is in step with the rotation table (a->trig_tab) */
template <int NC>
static hipError_t launch_fir_graph_nc(const IcwFirArgs *f, const IcwK2Args *a, int in_step, size_t lds, hipStream_t st)
{
    const int TF = 256 * ICW_FIR_R / NC;
    dim3 grid(f->n_streams, (f->T + TF - 1) / TF - f->tile0);  /* stream-fastest (icw_fir_graph); <= 1 024 tiles */
    const void *fn = !a->trig ? (const void *)icw_fir_graph<false, false, NC>
                   : in_step ? (const void *)icw_fir_graph<true, true, NC> : (const void *)icw_fir_graph<true, false, NC>;
    if (fir_lds_attr(fn, lds) != hipSuccess) return hipErrorInvalidValue;
    if (!a->trig) hipLaunchKernelGGL((icw_fir_graph<false, false, NC>), grid, dim3(256), lds, st, *f, *a);
    else if (in_step) hipLaunchKernelGGL((icw_fir_graph<true, true, NC>), grid, dim3(256), lds, st, *f, *a);
    else hipLaunchKernelGGL((icw_fir_graph<true, false, NC>), grid, dim3(256), lds, st, *f, *a);
    return hipGetLastError();
}

/* the signature form over tiles [0, ntile) of every stream */
template <int SIG, int NC, bool B24>
static hipError_t launch_fir_sig_t(const IcwFirArgs *f, const IcwK2Args *a, int ntile, size_t lds, hipStream_t st)
{
    const void *fn = (const void *)icw_fir_sig<SIG, NC, B24>;
    if (fir_lds_attr(fn, lds) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL((icw_fir_sig<SIG, NC, B24>), dim3(f->n_streams, ntile), dim3(256), lds, st, *f, *a);
    return hipGetLastError();
}

template <int NC, bool B24>
static hipError_t launch_fir_sig_d(const IcwFirArgs *f, const IcwK2Args *a, int sig, int ntile, size_t lds,
                                   hipStream_t st)
{
    switch (sig) {
    case ICW_SIG_M:
    case ICW_SIG_M | ICW_SIG_UNIT: return launch_fir_sig_t<ICW_SIG_M | ICW_SIG_UNIT, NC, B24>(f, a, ntile, lds, st);
    case ICW_SIG_SM: return launch_fir_sig_t<ICW_SIG_SM, NC, B24>(f, a, ntile, lds, st);
    case ICW_SIG_SM | ICW_SIG_UNIT: return launch_fir_sig_t<ICW_SIG_SM | ICW_SIG_UNIT, NC, B24>(f, a, ntile, lds, st);
    case ICW_SIG_PSXM: return launch_fir_sig_t<ICW_SIG_PSXM, NC, B24>(f, a, ntile, lds, st);
    case ICW_SIG_PSXM | ICW_SIG_UNIT: return launch_fir_sig_t<ICW_SIG_PSXM | ICW_SIG_UNIT, NC, B24>(f, a, ntile, lds, st);
    default: return hipErrorInvalidValue;
    }
}

static bool fir_sig_known(int sig)
{
    switch (sig) {
    case ICW_SIG_M: case ICW_SIG_M | ICW_SIG_UNIT: case ICW_SIG_SM: case ICW_SIG_SM | ICW_SIG_UNIT:
    case ICW_SIG_PSXM: case ICW_SIG_PSXM | ICW_SIG_UNIT: return true;
    default: return false;
    }
}

extern "C" hipError_t icw_launch_fir_graph(const IcwFirArgs *f, const IcwK2Args *a, int in_step, int sig_on,
                                           hipStream_t st)
{
    if (!fir_ok(f->M, f->nt)) return hipErrorInvalidValue;
    /* the render-only form (icw_fast_render) takes the quantiser from sign_delta alone: mid-riser
     * (sign_delta -1, round_offset 0) or mid-tread (0, 0.5), the only pairs render_consts gives */
    if (a->rk.sign_delta != 0 ? (a->rk.sign_delta != -1 || a->rk.round_offset != 0.0) : a->rk.round_offset != 0.5)
        return hipErrorInvalidValue;
    const size_t lds = icw_fir_graph_lds(f->M, f->nt, f->nch, a->n_regs);
    if (!lds) return hipErrorInvalidValue;
    if (in_step && !(a->trig && a->trig_tab)) return hipErrorInvalidValue;
    const int nc = f->nch > 1 ? 2 : 1, TF = 256 * ICW_FIR_R / nc;
    IcwFirArgs fl = *f;
    fl.tile0 = 0;
    /* the signature form takes the tiles before the one holding the block's last frame when every
     * lane of them would take icw_chain_frames' render-only branch: a chain program of a known
     * signature, its rotation factors (if any) from the table, a render here, no pre-render doubles,
     * no I / Q hand-off, no dither rows.  sig_on 0 (IcwTuning.fir_sig): icw_fir_graph for every tile. */
    const int sig = f->sig;
    const bool rot = (sig & ~ICW_SIG_UNIT) != ICW_SIG_M;
    if (sig_on && ICW_CHAIN4 && fir_sig_known(sig) && (rot ? (a->trig && in_step) : !a->trig) && a->do_render &&
        !a->iq_out && !a->pre && !a->dith) {
        const int nsig = (f->T - 1) / TF;
        if (nsig > 0) {
            const bool b24 = a->rk.is24 != 0;
            const size_t ls = icw_fir_graph_lds(f->M, f->nt, f->nch, 0);   /* no DSP register file */
            const hipError_t e = nc == 2 ? (b24 ? launch_fir_sig_d<2, true>(f, a, sig, nsig, ls, st)
                                                : launch_fir_sig_d<2, false>(f, a, sig, nsig, ls, st))
                                         : (b24 ? launch_fir_sig_d<1, true>(f, a, sig, nsig, ls, st)
                                                : launch_fir_sig_d<1, false>(f, a, sig, nsig, ls, st));
            if (e != hipSuccess) return e;
            fl.tile0 = nsig;
        }
    }
    return nc == 2 ? launch_fir_graph_nc<2>(&fl, a, in_step, lds, st) : launch_fir_graph_nc<1>(&fl, a, in_step, lds, st);
}

template <int N, bool K>
static hipError_t launch_k2_t(IcwK2Args a, hipStream_t st)
{
    /* ICW_K2_TPW tiles per workgroup (the next window loads hide behind a tile's work, one meter
     * atomic per 1024 frames); a small launch (the one-stream drop-in: 576 frames) uses fewer
     * tiles per workgroup so that its tiles run side by side */
    int tpw = ICW_K2_TPW;
    while (tpw > 1 && (long)((a.T + ICW_K2_TILE * tpw - 1) / (ICW_K2_TILE * tpw)) * a.n_streams < 512) tpw >>= 1;
    a.tpw = tpw;
    const int span = ICW_K2_TILE * tpw;
    dim3 grid((a.T + span - 1) / span, a.n_streams);
    const size_t lds = (size_t)a.n_regs * 4 * ICW_K2_TILE * sizeof(double);
    if (a.prog_id) {
        /* per-stream DSP lists: the instances that select the program per workgroup */
        if (a.fes && !a.cw) hipLaunchKernelGGL((icw_output<N, K, true, true, true>), grid, dim3(ICW_K2_TILE), lds, st, a);
        else if (a.trig) hipLaunchKernelGGL((icw_output<N, K, true, false, true>), grid, dim3(ICW_K2_TILE), lds, st, a);
        else hipLaunchKernelGGL((icw_output<N, K, false, false, true>), grid, dim3(ICW_K2_TILE), lds, st, a);
        return hipGetLastError();
    }
    if (a.fes && !a.cw) hipLaunchKernelGGL((icw_output<N, K, true, true>), grid, dim3(ICW_K2_TILE), lds, st, a);
    else if (a.trig) hipLaunchKernelGGL((icw_output<N, K, true>), grid, dim3(ICW_K2_TILE), lds, st, a);
    else hipLaunchKernelGGL((icw_output<N, K, false>), grid, dim3(ICW_K2_TILE), lds, st, a);
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_output(const IcwK2Args *a, int nord, int kahan, hipStream_t st)
{
    switch (nord) {
    case 15: return kahan ? launch_k2_t<15, true>(*a, st) : launch_k2_t<15, false>(*a, st);
    case 18: return kahan ? launch_k2_t<18, true>(*a, st) : launch_k2_t<18, false>(*a, st);
    case 19: return kahan ? launch_k2_t<19, true>(*a, st) : launch_k2_t<19, false>(*a, st);
    case 20: return kahan ? launch_k2_t<20, true>(*a, st) : launch_k2_t<20, false>(*a, st);
    }
    return hipErrorInvalidValue;
}

extern "C" hipError_t icw_launch_trig_table(const IcwTrigArgs *a, hipStream_t st)
{
    hipLaunchKernelGGL(icw_trig_table, dim3((a->T + 255) / 256, a->slabs ? a->n_slabs : 1), dim3(256), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_graph_serial(const IcwK4Args *a, hipStream_t st)
{
    hipLaunchKernelGGL(icw_graph_serial, dim3((a->n_streams + 63) / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}

template <int N>
static hipError_t launch_s1_t(IcwS1Args a, hipStream_t st)
{
    a.k2.tpw = (a.k2.T + ICW_K2_TILE - 1) / ICW_K2_TILE;
    const size_t regs = (size_t)a.k2.n_regs * 4 * ICW_K2_TILE * sizeof(double);
    a.lpitch = (a.k2.T + N + 2) & ~1;
    a.rows_off = a.k2.n_regs * 4 * ICW_K2_TILE;
    const size_t rows = (size_t)4 * a.lpitch * sizeof(double) + 16;
    a.ovl = a.ovl && regs + rows <= ICW_S1_OVL_LDS;
    const size_t lds = regs + (a.ovl ? rows : 0);
    if (lds > 64 * 1024) {
        const hipError_t e = a.k2.trig ? hipFuncSetAttribute((const void *)icw_stream1<N, true>,
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                       : hipFuncSetAttribute((const void *)icw_stream1<N, false>,
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (a.k2.trig) hipLaunchKernelGGL((icw_stream1<N, true>), dim3(1), dim3(ICW_K2_TILE), lds, st, a);
    else hipLaunchKernelGGL((icw_stream1<N, false>), dim3(1), dim3(ICW_K2_TILE), lds, st, a);
    return hipGetLastError();
}

/* K5: one stream, one launch block of at most ICW_S1_MAX frames, real input, Kahan + reject (the
 * row recurrence), register-form graph, ROUND / flat render, no FP_CHECK -- the host checks */
extern "C" hipError_t icw_launch_stream1(const IcwS1Args *a, int nord, hipStream_t st)
{
    if (a->k0.T != a->k2.T || a->k1.T != a->k2.T || a->k2.T <= 0 || a->k2.T > ICW_S1_MAX || a->k2.n_streams != 1 ||
        a->k2.cw || a->k2.fes || a->k2.iq_out || !a->k2.do_render)
        return hipErrorInvalidValue;
    switch (nord) {
    case 15: return launch_s1_t<15>(*a, st);
    case 18: return launch_s1_t<18>(*a, st);
    case 19: return launch_s1_t<19>(*a, st);
    case 20: return launch_s1_t<20>(*a, st);
    }
    return hipErrorInvalidValue;
}

extern "C" hipError_t icw_launch_advance(const IcwAdvArgs *a, hipStream_t st)
{
    hipLaunchKernelGGL(icw_advance, dim3((a->n_streams + 63) / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}

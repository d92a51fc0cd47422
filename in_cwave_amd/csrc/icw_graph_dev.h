/*
 * icw_graph_dev.h -- per-frame device code shared by K2 (icw_kernels.hip) and KF2 (icw_fir.hip): output sums,
 * rotation factors, the DSP list in register and chain form, the ROUND / flat render, the lane exchange, meters.
 * Included after icw_device.h, icw_iir_dev.h, icw_libm.h, icw_quant_dev.h, icw_unpack_dev.h, icw_fir_dev.h.
 */
#ifndef ICW_GRAPH_DEV_H_
#define ICW_GRAPH_DEV_H_

#define ICW_PI (3.1415926535897932384626433832795029)

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

/* one stream's own rate, where the streams of a launch differ (icw_set_stream_input) */
struct IcwRate {
    unsigned long long ssr;
    uint32_t sample_rate;
};

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
template <bool TRIG, bool TAB = false, bool DEFER = false, bool RATE = false>
__device__ __forceinline__ void icw_frame_graph(const IcwK2Args &a, icw_cprog *P, const IcwRegFile &R, int s,
                                                int t, const IcwLR &in, bool use_tab, unsigned &clip_l,
                                                unsigned &clip_r, double &pk_l, double &pk_r, int *dv = nullptr,
                                                size_t tab_off = 0, const IcwRate *rt = nullptr)
{
    /* tab_off: the stream's slab of the rotation table (per-stream lists; 0: the one table);
     * rt: the stream's own rate, read by the RATE instances only (per-stream inputs) */
    const int T = a.T;
    if (a.iq_out) {
        /* bus-form graph: the serial graph kernel takes it from here (do_render == 0) */
        double *q = a.iq_out + ((size_t)s * T + t) * 4;
        q[0] = in.lre; q[1] = in.lim; q[2] = in.rre; q[3] = in.rim;
    } else {
        const double *trow = use_tab ? a.trig_tab + tab_off + icw_trig_index(t, a.trig_perm_q) * a.trig_pitch : nullptr;
        double omega;
        if constexpr (RATE)
            omega = (TRIG && !use_tab) ? icw_omega(a.n_frame[s], a.t0 + t, a.scaled, rt->ssr, rt->sample_rate) : 0.0;
        else
            omega = (TRIG && !use_tab) ? icw_omega(a.n_frame[s], a.t0 + t, a.scaled, a.ssr, a.sample_rate) : 0.0;
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
 * per-frame index arithmetic and no clamp.  Without ROWP tro_u is the stream's slab of the table (KF2's
 * per-stream form; 0: the one table).
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
                                      : a.trig_tab + tro_u + icw_trig_index(min(t0 + r, T - 1), a.trig_perm_q) * a.trig_pitch;
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
#define ICW_ROWP_ALIAS(S) case (S):
#define ICW_ROWP_CASE(S)                                                                                             \
    case (S):                                                                                                        \
        icw_chain_frames<TRIG, R, true, (S)>(a, P, s, t0, nv, in, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, tro_u,     \
                                             tro_step);                                                              \
        return;
            ICW_SIG_LIST(ICW_ROWP_ALIAS, ICW_ROWP_CASE)
#undef ICW_ROWP_ALIAS
#undef ICW_ROWP_CASE
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

#endif /* ICW_GRAPH_DEV_H_ */

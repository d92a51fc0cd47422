/*
 * icw_fir_dev.h -- device code of the FIR Hilbert converter shared by its kernels (KF, KF2 and the
 * CWAVE encoder KFE): the tile geometry, the staging of a tile's inputs in LDS, the register-blocked tap
 * sums, the packing and the store of a lane's rendered frames, and the dispatch on a chain signature.
 * Included after icw_device.h and icw_unpack_dev.h.
 */
#ifndef ICW_FIR_DEV_H_
#define ICW_FIR_DEV_H_

/* FIR Hilbert converter: real PCM -> the analytic signal a CWAVE file holds (cwave.h:40,56-58:
 * "Hilbert FIR filter order" k_M, "filter parameter" k_beta; the converter itself is not part of
 * in_cwave).  Order M (even, M + 1 taps), centre c = M/2, odd taps only:
 *     I[n] = x[n - c],   Q[n] = sum_{m = 1, 3, .., <= c} g_m * (x[n - c - m] - x[n - c + m])
 * with the sum taken in ascending m as acc = fma(g_m, d_m, acc) from +0.0 -- the oracle's order, so
 * the result is bit-identical.  x is the unpacked, faded input of K0 (xwave_unpack_csample,
 * xwave_reader.c:908-936), mono feeding R with L.
 *
 * Register blocking.  A lane sums 8 consecutive outputs of one channel.  For 8 taps at a time it
 * loads the 22 inputs their left operands span and the 22 of the right ones, then runs the 64
 * subtract + FMA pairs from registers: 44 LDS reads per 64 output-taps instead of 128.  The staged
 * inputs carry one pad double after every 8 (physical index i + i/8), so the 32 lanes of a
 * ds_read_b64 group, 9 doubles apart, hit 64 distinct banks; a staging shift `sh` puts every lane's
 * window at the same phase of that pattern, so all offsets inside a block are immediates.  Taps past
 * the last multiple of 8 run one at a time. */
#define ICW_FIR_R 8                                  /* outputs per lane */
#ifndef ICW_FIR_VEC
#define ICW_FIR_VEC 1                                /* FIR staging: 16-byte loads, one LDS base per thread */
#endif
#ifndef ICW_FIR_INTERIOR
#define ICW_FIR_INTERIOR 1                           /* FIR staging: the interior tiles' short form */
#endif
#ifndef ICW_FIR_OCC
#define ICW_FIR_OCC 4                                /* KF2 workgroups per CU the register budget is sized for */
#endif
#ifndef ICW_FIR_CUT
#define ICW_FIR_CUT 0                                /* diagnostic: 1 no graph, 2 no sums either (VALU by phase) */
#endif
#ifndef ICW_FIR_DIAG
#define ICW_FIR_DIAG 0                               /* diagnostic, not exact: 1 no division slow path, 2 no render */
#endif
#ifndef ICW_FIR_STAMPS
#define ICW_FIR_STAMPS 0                             /* diagnostic: KF2 phase stamps (tools/fir_phases.py) */
#endif
#ifndef ICW_CHAIN4
#define ICW_CHAIN4 1                                 /* KF2: chain programs op by op over a lane's frames */
#endif

/* The staged inputs carry ICW_FIR_PAD pad doubles after every 8 (physical index i + PAD (i / 8)).  With
 * 2 a lane's window (8 outputs apart: 10 doubles = 20 dwords) starts 16-byte aligned at every lane, and
 * the sums read it two doubles at a time (ds_read_b128, conflict-free over each 16-lane group: 20 l
 * mod 64 covers the 64 banks once), half the LDS instructions of the 1-pad layout's ds_read_b64. */
#ifndef ICW_FIR_PAD
#define ICW_FIR_PAD 2
#endif
#if ICW_FIR_PAD != 1 && ICW_FIR_PAD != 2
#error "ICW_FIR_PAD: icw_fir_block's window reads are written for 1 or 2 pad doubles per 8"
#endif
#ifndef ICW_SCALAR_UNIT
#define ICW_SCALAR_UNIT 1                            /* A/B: unit gains / norm_mul tested on scalar flags */
#endif
#ifndef ICW_RENDER_SH0
#define ICW_RENDER_SH0 1                             /* A/B: the render-only form specialised for norm_shift 0 */
#endif
__host__ __device__ __forceinline__ constexpr int icw_fir_phys(int i) { return i + ICW_FIR_PAD * (i >> 3); }

/* Tile geometry, for the kernels and for the launchers' LDS sizes alike.  Order M, centre c = M / 2:
 *   sh  staging shift, c - 1 + sh = 8 av: every lane's window starts at the same phase of the pad pattern;
 *   px  doubles of one staged channel of a TF-frame tile (pad, history, tile, margin), even, so the next
 *       channel's row stays 16-byte aligned. */
__host__ __device__ __forceinline__ constexpr int icw_fir_sh(int c) { return (8 - ((c - 1) & 7)) & 7; }
__host__ __device__ __forceinline__ constexpr int icw_fir_av(int c, int sh) { return (c - 1 + sh) >> 3; }
__host__ __device__ __forceinline__ constexpr int icw_fir_px(int sh, int M, int TF) { return (icw_fir_phys(sh + M + TF + 24) + 2) & ~1; }
__host__ __device__ __forceinline__ constexpr int icw_fir_px(int M, int TF) { return icw_fir_px(icw_fir_sh(M >> 1), M, TF); }

/* inputs of NC channels from ch0 for the outputs [tt, tt + nout) of a launch block, at logical
 * index i <-> frame j = tt - M + i - sh (zero outside [-M, T)), channel k at xs + k * px; the
 * history after the block is written by the tile that owns each of its frames.  The stereo form
 * computes a frame's address, validity and fade once for both channels. */
template <int FMT, bool AL, int NC>
__device__ __forceinline__ void icw_fir_stage_t(const IcwFirArgs &f, int s, int ch0, double *xs, int px, int tt,
                                                int nout, int sh, int tid, int nthr)
{
    const int T = f.T, M = f.M;
    const unsigned char *src = f.in + (size_t)s * f.in_stride + (size_t)ch0 * f.csz;
    const long long p0 = f.pos[s] + f.t0;
    const long long ns = f.fade[s * 3 + 0], fi = f.fade[s * 3 + 1], fo = f.fade[s * 3 + 2];
    const double *hin = f.hist_in + ((size_t)s * 2 + ch0) * M;
    double *hout = f.hist_out + ((size_t)s * 2 + ch0) * M;
    const bool mono = f.nch == 1;
    const int nl = sh + M + nout + 24;               /* logical extent: pad, history, tile, margin */
    const int nf = min(nout, T - tt);
    /* uniform over the tile: no fade anywhere in the frames it stages (icw_fade returns "none" for
     * fi <= ix <= ns - fo and for ix >= ns), and whether any staged frame precedes the block (the
     * history).  The fade's two FP64 divisions and the history loads were computed for every input
     * and made the staging ~half of the kernel's VALU instructions (r03_c2fir_sq.json). */
    const long long ja = max(tt - M, 0), jb = (long long)tt + nf - 1;
    const bool nofade = p0 + ja >= fi && (p0 + jb <= ns - fo || p0 + ja >= ns);
    const bool need_hist = tt < M + sh;
    /* 8 consecutive frames per thread and pass, their loads issued together (clamped in range,
     * selected after): the staging is load-latency bound otherwise */
    constexpr int V = 8;
    /* An interior tile of a packed typed format (i16 / i32 / f32, the file frame exactly the computed
     * channels): a thread's 8 frames are 8 * frame-size contiguous bytes, read by 16-byte loads from
     * one address, unpacked from the registers (the same conversions as icw_unpack_f), and written to
     * 8 consecutive LDS doubles per channel (logical 8t..8t+7 sit at physical 9t..9t+7) from one base.
     * Only the threads at the ends of the staged range select zeros.  With M >= 32 every frame a
     * thread loads lies in [0, T) (tt >= M + sh, and the last load ends 30 frames past the tile's
     * outputs, tt + nout <= T - M).  The per-frame address, clamp and select of the general form were
     * most of the staging's VALU instructions (c2fir: ~150 per wave). */
    if constexpr (ICW_FIR_VEC && AL && (FMT == ICW_FMT_I16 || FMT == ICW_FMT_I32 || FMT == ICW_FMT_F32)) {
        constexpr int CS = FMT == ICW_FMT_I16 ? 2 : 4;
        constexpr int FB = NC * CS;                       /* bytes per frame */
        constexpr int NW = V * FB / 4;                    /* 32-bit words per thread and pass */
        const unsigned char *b0 = src + (size_t)(tt - M - sh) * f.fsz;
        if (nofade && !need_hist && tt + nf <= T - M && M >= 32 && f.fsz == FB && !((uintptr_t)b0 & 15)) {
            const int lim = sh + M + nf;                  /* logical [sh, lim) holds inputs, the rest zeros */
            for (int i0 = tid * V; i0 < nl; i0 += nthr * V) {
                const uint4 *p = (const uint4 *)(b0 + (size_t)i0 * FB);
                uint32_t w[NW];
#pragma unroll
                for (int k = 0; k < NW / 4; ++k) {
                    const uint4 q4 = p[k];
                    w[4 * k] = q4.x; w[4 * k + 1] = q4.y; w[4 * k + 2] = q4.z; w[4 * k + 3] = q4.w;
                }
                double v[NC][V];
#pragma unroll
                for (int e = 0; e < V; ++e) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        const int si = e * NC + k;            /* sample index in the thread's run */
                        if constexpr (FMT == ICW_FMT_I16) {
                            const uint32_t u = w[si >> 1];
                            v[k][e] = (double)((si & 1) ? ((int)u >> 16) : (int)(short)(u & 0xffffu));
                        } else if constexpr (FMT == ICW_FMT_I32) {
                            v[k][e] = ((double)(int)w[si]) / 65536.0;
                        } else {
                            v[k][e] = 32768.0 * (double)__uint_as_float(w[si]);
                        }
                    }
                }
                double *d = xs + icw_fir_phys(i0);
                if (i0 >= sh && i0 + V <= lim) {
#pragma unroll
                    for (int k = 0; k < NC; ++k)
#pragma unroll
                        for (int e = 0; e < V; ++e) d[k * px + e] = v[k][e];
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const int i = i0 + e;
                        if (i < nl) {
#pragma unroll
                            for (int k = 0; k < NC; ++k) d[k * px + e] = (i >= sh && i < lim) ? v[k][e] : 0.0;
                        }
                    }
                }
            }
            return;
        }
    }
    if (ICW_FIR_INTERIOR && NC == 2 && nofade && !need_hist && tt + nf <= T - M) {
        /* an interior tile (most of them): no fade, no history to read or write -- a frame is its
         * input inside [tt - M, tt + nf) and zero outside (c2fir +3 %, c4fir +3 %; the mono form
         * measured 1 % slower with it, so it keeps the general one) */
        for (int i0 = tid * V; i0 < nl; i0 += nthr * V) {
            double raw[NC][V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int jr = min(tt - M + i0 + e - sh, T - 1);
                const unsigned char *p = src + (size_t)jr * f.fsz;
#pragma unroll
                for (int k = 0; k < NC; ++k) raw[k][e] = icw_unpack_f<FMT, AL>(p + k * f.csz);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int i = i0 + e;
                const bool in = i >= sh && i < sh + M + nf;
                if (i < nl) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) xs[k * px + icw_fir_phys(i)] = in ? raw[k][e] : 0.0;
                }
            }
        }
        return;
    }
    for (int i0 = tid * V; i0 < nl; i0 += nthr * V) {
        double raw[NC][V], his[NC][V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int j = tt - M + i0 + e - sh;
            const int jr = min(max(j, 0), T - 1);
            const unsigned char *p = src + (size_t)jr * f.fsz;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                raw[k][e] = icw_unpack_f<FMT, AL>(p + k * f.csz);
                his[k][e] = 0.0;
            }
        }
        if (need_hist) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int h = min(max(tt + i0 + e - sh, 0), M - 1);
#pragma unroll
                for (int k = 0; k < NC; ++k) his[k][e] = hin[k * M + h];
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int i = i0 + e;
            const int j = tt - M + i - sh;
            double v[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) v[k] = 0.0;
            if (i >= sh && j < tt + nf) {
                if (j < 0) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) v[k] = his[k][e];
                } else {
#pragma unroll
                    for (int k = 0; k < NC; ++k) v[k] = raw[k][e];
                    if (!nofade) {
                        const double fd = icw_fade(p0 + j, ns, fi, fo);
                        if (fd >= 0.0) {
#pragma unroll
                            for (int k = 0; k < NC; ++k) v[k] *= fd;
                        }
                    }
                }
                if (j >= T - M && (j >= tt || tt == 0)) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) hout[k * M + j - (T - M)] = v[k];
                    if (NC == 1 && mono) hout[M + j - (T - M)] = v[0];
                }
            }
            if (i < nl) {
#pragma unroll
                for (int k = 0; k < NC; ++k) xs[k * px + icw_fir_phys(i)] = v[k];
            }
        }
    }
}

/* the staging of NC channels, its format and alignment resolved once (uniform) per workgroup */
template <int NC>
__device__ __forceinline__ void icw_fir_stage(const IcwFirArgs &f, int s, int ch0, double *xs, int px, int tt,
                                              int nout, int sh, int tid, int nthr)
{
    const uintptr_t al = (uintptr_t)(f.in + (size_t)s * f.in_stride) | (uintptr_t)f.fsz;
    icw_fmt_dispatch(f.fmt, al, [&](auto fc, auto ac) {
        icw_fir_stage_t<decltype(fc)::value, decltype(ac)::value != 0, NC>(f, s, ch0, xs, px, tt, nout, sh, tid,
                                                                           nthr);
    });
}

/* the stream's own input replaces the launch's: format, sizes, channels, and the block offset at its own
 * frame size (icw_unpack_frames_mixed); a null table leaves the launch's one input */
__device__ __forceinline__ void icw_fir_own_input(IcwFirArgs &f, int s)
{
    if (f.desc) {
        const __attribute__((address_space(4))) IcwInDesc *d = (const __attribute__((address_space(4))) IcwInDesc *)f.desc + s;
        f.fmt = d->fmt;
        f.csz = d->csz;
        f.fsz = d->fsz;
        f.nch = d->nch;
        f.in += (size_t)f.t0 * f.fsz;
    }
}

/* the stream's own converter replaces the launch's (icw_set_stream_fir): order, taps, and its rows of the two
 * history buffers -- hoff doubles into them, laid so that the staging's (s * 2 + ch) * M lands there; a null
 * table leaves the launch's one converter.  What depends on M (icw_fir_sh / _av / _px, the LDS carve-up) is
 * computed after this, per workgroup, inside the launch's LDS, which is sized for its widest entry */
__device__ __forceinline__ void icw_fir_own_conv(IcwFirArgs &f, int s)
{
    if (f.conv) {
        const __attribute__((address_space(4))) IcwFirConv *d = (const __attribute__((address_space(4))) IcwFirConv *)f.conv + s;
        f.M = d->M;
        f.nt = d->nt;
        f.g = d->g;
        const ptrdiff_t off = (ptrdiff_t)d->hoff - (ptrdiff_t)s * 2 * f.M;
        f.hist_in += off;
        f.hist_out += off;
    }
}

/* The taps through the constant address space: every lane of a wave reads the same tap, so they
 * come in by scalar loads into SGPRs (the FMA takes one SGPR operand) and leave the LDS pipe to the
 * inputs -- which bounds the sums: 52 -> 44 LDS reads per 8-tap block of a lane's 8 outputs. */
typedef const __attribute__((address_space(4))) double icw_ctap;

/* one NTAP-tap block (k0 = NTAP b) of a lane's 8 outputs: bl / br = physical index of the first input
 * of the left / right window (both at phase 2 of the pad pattern; NTAP 4 or 8 keeps it there) */
#ifndef ICW_FIR_NTAP
#define ICW_FIR_NTAP 8                               /* taps per register block of the sums */
#endif
template <int NTAP>
__device__ __forceinline__ void icw_fir_block(const double *xs, icw_ctap *gs, int k0, int bl, int br,
                                              double (&acc)[ICW_FIR_R])
{
    static_assert(NTAP == 4 || NTAP == 8, "a window step of whole pad groups");
    constexpr int W = ICW_FIR_R + 2 * NTAP - 2;
    double L[W], Rt[W], g[NTAP];
    if constexpr (ICW_FIR_PAD == 2) {
        /* elements e, e + 1 (e even) never straddle a pad: the window starts at logical phase 2 */
#pragma unroll
        for (int e = 0; e < W; e += 2) {
            const double2 v = *(const double2 *)(xs + bl + e + 2 * ((e + 2) >> 3));
            L[e] = v.x;
            L[e + 1] = v.y;
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int e = 0; e < W; e += 2) {
            const double2 v = *(const double2 *)(xs + br + e + 2 * ((e + 2) >> 3));
            Rt[e] = v.x;
            Rt[e + 1] = v.y;
            asm volatile("" ::: "memory");
        }
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            L[e] = xs[bl + e + ((e + 2) >> 3)];
            asm volatile("" ::: "memory");               /* no ds_read2 pairing: 2 x 2 cycles, not 8 */
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            Rt[e] = xs[br + e + ((e + 2) >> 3)];
            asm volatile("" ::: "memory");
        }
    }
#pragma unroll
    for (int j = 0; j < NTAP; ++j) g[j] = gs[k0 + j];
#pragma unroll
    for (int j = 0; j < NTAP; ++j) {
#pragma unroll
        for (int r = 0; r < ICW_FIR_R; ++r)
            acc[r] = __builtin_fma(g[j], L[r - 2 * j + 2 * NTAP - 2] - Rt[r + 2 * j], acc[r]);
    }
}

/* Q of a lane's 8 outputs tt + 8 ll + r; a = (c - 1 + sh) / 8.  The taps in ascending order, in
 * register blocks of ICW_FIR_NTAP, then one by one */
template <int NB = ICW_FIR_NTAP>
__device__ __forceinline__ void icw_fir_sums(const double *xs, icw_ctap *gs, int nt, int ll, int a, int sh, int c,
                                             double (&acc)[ICW_FIR_R])
{
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) acc[r] = 0.0;
    const int nb = nt / NB;
    constexpr int G = 8 + ICW_FIR_PAD;                  /* physical doubles per group of 8 */
    constexpr int GS = G * NB / 4;                      /* physical step of a window per block */
    int bl = G * (ll + a - NB / 4) + 2, br = G * (ll + a) + 2;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        icw_fir_block<NB>(xs, gs, NB * b, bl, br, acc);
        bl -= GS;
        br += GS;
    }
    const int A = 8 * a;
#pragma unroll 1
    for (int k = nb * NB; k < nt; ++k) {
        const double gk = gs[k];
#pragma unroll
        for (int r = 0; r < ICW_FIR_R; ++r) {
            const int li = 8 * ll + A + r - 2 * k, ri = 8 * ll + A + 2 + r + 2 * k;
            acc[r] = __builtin_fma(gk, xs[icw_fir_phys(li)] - xs[icw_fir_phys(ri)], acc[r]);
        }
    }
    (void)sh; (void)c;
}

/* Two rendered stereo frames as they lie in the output: 16-bit l0 r0 l1 r1 in two dwords, 24-bit in three.
 * The depth B24 is a template parameter here and in icw_store_packed, and every index into a lane's packed
 * words w is a constant once the callers' loops are unrolled: with a runtime depth flag the compiler merged
 * the two packings' stores into one store at a selected index, which put w in scratch -- c3fir wrote 6.3 GB
 * per launch against 4.3 GB of output (profiles/r05_c3fir_pmc.json). */
template <bool B24>
__device__ __forceinline__ void icw_pack2(int l0, int r0, int l1, int r1, unsigned *w)
{
    if constexpr (B24) {
        const unsigned a0 = (unsigned)l0 & 0xffffffu, b0 = (unsigned)r0 & 0xffffffu;
        const unsigned a1 = (unsigned)l1 & 0xffffffu, b1 = (unsigned)r1 & 0xffffffu;
        w[0] = a0 | (b0 << 24);
        w[1] = (b0 >> 8) | (a1 << 16);
        w[2] = (a1 >> 16) | (b1 << 8);
    } else {
        w[0] = ((unsigned)l0 & 0xffffu) | ((unsigned)r0 << 16);
        w[1] = ((unsigned)l1 & 0xffffu) | ((unsigned)r1 << 16);
    }
}
#define ICW_PACK2_WORDS(B24) ((B24) ? 3 : 2)         /* dwords icw_pack2 writes */

/* The first nv of a lane's NFR (4 or 8) packed frames w to their place p in the output row: 16-byte (16-bit)
 * / 8-byte (24-bit) stores when p is so aligned and nv == NFR, else dwords (16-bit; p is dword-aligned for
 * every output the library lays out itself) or bytes (24-bit; byte i of the packed run is byte i of the
 * output). */
template <bool B24, int NFR, int NW>
__device__ __forceinline__ void icw_store_packed(unsigned char *p, const unsigned (&w)[NW], int nv)
{
    static_assert((NFR == 4 || NFR == 8) && NW >= NFR / 2 * ICW_PACK2_WORDS(B24), "w holds the NFR frames");
    if constexpr (B24) {
        if (nv == NFR && !((uintptr_t)p & 7)) {
            uint2 *q2 = (uint2 *)p;
#pragma unroll
            for (int i = 0; i < NFR * 6 / 8; ++i) q2[i] = make_uint2(w[2 * i], w[2 * i + 1]);
        } else {
#pragma unroll
            for (int i = 0; i < NFR * 6; ++i)
                if (i < nv * 6) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
        }
    } else {
        unsigned *d = (unsigned *)p;
        if (nv == NFR && !((uintptr_t)p & 15)) {
#pragma unroll
            for (int i = 0; i < NFR; i += 4) *(uint4 *)(d + i) = make_uint4(w[i], w[i + 1], w[i + 2], w[i + 3]);
        } else {
#pragma unroll
            for (int r = 0; r < NFR; ++r)
                if (r < nv) d[r] = w[r];
        }
    }
}

/* A runtime signature as the compile-time constant of its specialised code (ICW_SIG_LIST, icw_device.h:
 * the Master signature without the unit flag runs the code of the one with it -- it has no other op whose
 * gain the flag could skip): f(icw_ic<SIG>) for a listed one, false for any other. */
template <class F>
__host__ __device__ __forceinline__ bool icw_sig_dispatch(int sig, F &&f)
{
    switch (sig) {
#define ICW_SIG_ALIAS_(S) case (S):
#define ICW_SIG_CASE_(S) case (S): f(icw_ic<(S)>{}); return true;
        ICW_SIG_LIST(ICW_SIG_ALIAS_, ICW_SIG_CASE_)
#undef ICW_SIG_ALIAS_
#undef ICW_SIG_CASE_
    default: return false;
    }
}

#endif /* ICW_FIR_DEV_H_ */

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
 *   icw_graph_serial   K4 (serial form); icw_graph_serial_mixed: the same over streams with different programs.
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

/* K0 over streams with different inputs (icw_set_stream_input).  The workgroup column is one stream,
 * so its descriptor is wave-uniform: read through the constant address space (as K2's prog_id rows)
 * it comes in by scalar loads, the format dispatch stays a uniform branch and fmt / csz / fsz / nch
 * stay in SGPRs.  The frame's own code is icw_unpack_frame's, on the stream's frame size and row
 * address (the aligned / unaligned choice included).  Real formats only (the host checks). */
__global__ __launch_bounds__(256) void icw_unpack_frames_mixed(IcwK0MixArgs m)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    const __attribute__((address_space(4))) IcwInDesc *d = (const __attribute__((address_space(4))) IcwInDesc *)m.desc + s;
    IcwK0Args a = m.k0;
    a.fmt = d->fmt;
    a.csz = d->csz;
    a.fsz = d->fsz;
    a.nch = d->nch;
    a.in += (size_t)a.t0 * a.fsz;      /* the block's first frame of this stream */
    if (t < a.T) icw_unpack_frame(a, t, s);
}

#include "icw_fir_dev.h"
#include "icw_graph_dev.h"

/* ------------------------------------------------------------- output kernel (K2) ------- */
/* One frame of K2: the four chains' output sums from their w rows (w[c]: the row at the frame's
 * window, w[c][N] the state after the frame), the de-subnorm counts, the fs/4 un-mix, then the
 * frame graph.  dup: mono input with bit-identical converters, chains 2-3 are copies of 0-1. */
template <int N, bool KAHAN, bool TRIG, bool FCK, bool RATE = false>
__device__ __forceinline__ void icw_output_frame(const IcwK2Args &a, icw_cprog *P, const IcwRegFile &R, int s,
                                                 int t, const double *const (&w)[4], bool dup, const double *lc,
                                                 IcwFes (&fes)[2], bool count_sn, unsigned (&sn)[4], bool use_tab,
                                                 unsigned &clip_l, unsigned &clip_r, double &pk_l, double &pk_r,
                                                 size_t tab_off = 0, const IcwRate *rt = nullptr)
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
    if constexpr (RATE)
        icw_frame_graph<TRIG, false, false, true>(a, P, R, s, t, in, use_tab, clip_l, clip_r, pk_l, pk_r, nullptr, tab_off, rt);
    else
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
/* the stream's channels: the call's, or (MIX) its own from the selection rows */
template <bool MIX>
__device__ __forceinline__ int icw_stream_nch(const IcwK2Args &a, int s)
{
    if constexpr (MIX) return ((const __attribute__((address_space(4))) int32_t *)a.prog_id)[4 * a.n_streams + s];
    else return a.nch;
}

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
    const bool dup = !FCK && !a.cw && icw_stream_nch<MIX>(a, s) == 1 && a.info_dup && a.info_dup[s * 2] && a.info_dup[s * 2 + 1] &&
                     a.hq_phase[s * 2] == a.hq_phase[s * 2 + 1];
    [[maybe_unused]] IcwRate rt;
    if constexpr (MIX) {
        /* the stream's own rate from the selection rows (it replaces a.ssr / a.sample_rate) */
        const __attribute__((address_space(4))) int32_t *id = (const __attribute__((address_space(4))) int32_t *)a.prog_id;
        rt.sample_rate = (uint32_t)id[3 * a.n_streams + s];
        rt.ssr = (unsigned long long)rt.sample_rate * ICW_HZ_SCALE;
    }
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
                icw_output_frame<N, KAHAN, TRIG, FCK, true>(a, P, R, s, t, w, dup, lcoef + zk, fes, count_sn, sn, use_tab,
                                                            clip_l, clip_r, pk_l, pk_r, tab_off, &rt);
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

/* K2's direct-input form, for a call over CWAVE streams with different inputs (icw_set_stream_input
 * with icw_enable_stream_cwave): no K0 runs and no xd rows exist -- the workgroup reads its stream's
 * file frames itself.  One stream per workgroup, so the descriptor is wave-uniform: read through the
 * constant address space it comes in by scalar loads, and the format / alignment choice is made once,
 * before the workgroup's loads (icw_cw_dispatch), not per sample.  A workgroup issues the loads of all
 * its a.tpw tiles up front -- one typed load per channel pair where the row is aligned to the pair --
 * then per frame: mono duplicate, fade on all four values (xwave_reader.c:939-966), and the frame
 * graph exactly as icw_output's MIX instances run it for a.cw (the stream's own list, rate and slab
 * from the selection rows).  No quadrature IIR sums, so no N / KAHAN instances; the Hilbert phases and
 * rings are not touched.  K4 and the serial renders read its iq / rpre rows as they read K2's. */
template <bool TRIG>
__global__ __launch_bounds__(ICW_K2_TILE, ICW_K2_MINWG) void icw_output_cw(IcwK2Args a, IcwDinArgs d)
{
    constexpr int TILE = ICW_K2_TILE;
    extern __shared__ __attribute__((aligned(16))) double lregs[];   /* [n_regs][4][TILE] */
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    const int tl = threadIdx.x, s = blockIdx.y;
    const int T = a.T;
    const int tw0 = blockIdx.x * TILE * a.tpw;
    const int ntile = min(a.tpw, (T - tw0 + TILE - 1) / TILE);

    const __attribute__((address_space(4))) int32_t *id = (const __attribute__((address_space(4))) int32_t *)a.prog_id;
    IcwRate rt;
    rt.sample_rate = (uint32_t)id[3 * a.n_streams + s];
    rt.ssr = (unsigned long long)rt.sample_rate * ICW_HZ_SCALE;
    icw_cprog *P = icw_prog_c(a.prog) + id[s];
    const int slab = id[a.n_streams + s];
    const bool use_tab = TRIG && a.trig_tab && slab >= 0 && a.n_frame[s] == a.n_frame[id[2 * a.n_streams + s]];
    const size_t tab_off = slab >= 0 ? (size_t)slab * a.slab_stride : 0;

    const __attribute__((address_space(4))) IcwInDesc *ds = (const __attribute__((address_space(4))) IcwInDesc *)d.desc + s;
    const uint32_t fmt = ds->fmt, csz = ds->csz, fsz = ds->fsz;
    const bool stereo = ds->nch > 1;
    const unsigned char *row = d.in + (size_t)s * d.in_stride;
    const uintptr_t al = (uintptr_t)row | (uintptr_t)fsz;
    row += (size_t)(a.t0 + tw0) * fsz;                 /* the workgroup's first frame */

    double q[ICW_K2_TPW][4];
    icw_cw_dispatch(fmt, al, [&](auto fc, auto ac) {
        constexpr int F = decltype(fc)::value;
        constexpr bool AL = decltype(ac)::value != 0;
#pragma unroll
        for (int k = 0; k < ICW_K2_TPW; ++k) {
            if (k < ntile && tw0 + k * TILE + tl < T) {
                const unsigned char *fp = row + (size_t)(k * TILE + tl) * fsz;
                icw_unpack_iq_f<F, AL>(fp, q[k][0], q[k][1]);
                if (stereo) icw_unpack_iq_f<F, AL>(fp + csz, q[k][2], q[k][3]);
                else { q[k][2] = q[k][0]; q[k][3] = q[k][1]; }
            }
        }
    });

    IcwRegFile R;
    R.base = lregs + tl;
    /* slots read but never written in the frame hold their block-start values */
    for (int r = 0; r < P->n_persist; ++r) {
        const double *b = a.bus + ((size_t)s * ICW_N_INPUTS + P->persist_slot[r]) * 4;
        IcwLR v; v.lre = b[0]; v.lim = b[1]; v.rre = b[2]; v.rim = b[3];
        R.set(P->persist_reg[r], v);
    }
    const long long pos0 = d.pos[s] + a.t0;
    const long long ns = d.fade[s * 3 + 0], fi = d.fade[s * 3 + 1], fo = d.fade[s * 3 + 2];
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
#pragma unroll
    for (int k = 0; k < ICW_K2_TPW; ++k) {
        const int t = tw0 + k * TILE + tl;
        if (k < ntile && t < T) {
            const double fd = icw_fade(pos0 + t, ns, fi, fo);
            if (fd >= 0.0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) q[k][i] *= fd;
            }
            IcwLR in;
            in.lre = q[k][0]; in.lim = q[k][1]; in.rre = q[k][2]; in.rim = q[k][3];
            icw_frame_graph<TRIG, false, false, true>(a, P, R, s, t, in, use_tab, clip_l, clip_r, pk_l, pk_r, nullptr, tab_off, &rt);
        }
    }
    if (a.do_render) icw_meters_wg(a, s, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
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
    [[maybe_unused]] uint32_t rate = 0;
    if constexpr (SLAB) {
        const __attribute__((address_space(4))) int32_t *sl = (const __attribute__((address_space(4))) int32_t *)a.slabs;
        P += sl[y];
        ref = sl[a.n_slabs + y];
        rate = (uint32_t)sl[2 * a.n_slabs + y];      /* the slab's own rate: slabs are keyed by (list, rate) */
        tab += (size_t)y * a.slab_stride;
    }
    double omega;
    if constexpr (SLAB) omega = icw_omega(a.n_frame[ref], a.t0 + t, a.scaled, (unsigned long long)rate * ICW_HZ_SCALE, rate);
    else omega = icw_omega(a.n_frame[ref], a.t0 + t, a.scaled, a.ssr, a.sample_rate);
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
/* MIXIN: streams with different inputs -- each lane takes its stream's own rate from a.desc (a
 * lane-varying load, once per launch) */
template <bool MIXIN>
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
    unsigned long long ssr = a.ssr;
    uint32_t rate = a.sample_rate;
    if constexpr (MIXIN) {
        ssr = a.desc[s].ssr;
        rate = a.desc[s].sample_rate;
    }
    const double *iq = a.iq + (size_t)s * a.T * 4;
    double *pre = a.pre + (size_t)s * a.pre_stride;
    for (int t = 0; t < a.T; ++t) {
        const double omega = P->needs_omega ? icw_omega(n0, a.t0 + t, a.scaled, ssr, rate) : 0.0;
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

/* the mixed K4's bus in LDS: rows [slot * 4 + component] of W doubles, one per lane (b is the lane's column) */
struct IcwBusW {
    double *b;
    int W;
    __device__ __forceinline__ double &operator[](int k) const { return b[k * W]; }
};

/* one stream's frames of a block through its bus-form program P, in order: K4's body statement for
 * statement, over a bus whose rows have the launch's length.  K4 keeps its own text: routed through this
 * function its two instances no longer compiled to the instructions they had */
template <bool MIXIN, class BUS>
__device__ __forceinline__ void icw_graph_serial_run(const IcwK4Args &a, icw_cprog *P, int s, const BUS &bus)
{
    double *gb = a.bus + (size_t)s * ICW_N_INPUTS * 4;
    for (int k = 0; k < ICW_N_INPUTS * 4; ++k) bus[k] = gb[k];
    const unsigned long long n0 = a.n_frame[s];
    unsigned long long ssr = a.ssr;
    uint32_t rate = a.sample_rate;
    if constexpr (MIXIN) {
        ssr = a.desc[s].ssr;
        rate = a.desc[s].sample_rate;
    }
    const double *iq = a.iq + (size_t)s * a.T * 4;
    double *pre = a.pre + (size_t)s * a.pre_stride;
    for (int t = 0; t < a.T; ++t) {
        const double omega = P->needs_omega ? icw_omega(n0, a.t0 + t, a.scaled, ssr, rate) : 0.0;
        bus[0] = iq[(size_t)t * 4 + 0];
        bus[1] = iq[(size_t)t * 4 + 1];
        bus[2] = iq[(size_t)t * 4 + 2];
        bus[3] = iq[(size_t)t * 4 + 3];
        double lOut = 0.0, rOut = 0.0;
        for (int oi = 0; oi < P->n_ops; ++oi) {
            icw_cop &op = P->ops[oi];
            IcwLR d;
            if (P->bypass) {
                d.lre = bus[0]; d.lim = bus[1]; d.rre = bus[2]; d.rim = bus[3];
            } else {
                d.lre = d.lim = d.rre = d.rim = 0.0;
                const uint32_t m = op.in_mask;
                for (int k = 0; k < ICW_N_INPUTS; ++k) {
                    if (!((m >> k) & 1u)) continue;
                    d.lre += bus[k * 4 + 0]; d.lim += bus[k * 4 + 1];
                    d.rre += bus[k * 4 + 2]; d.rim += bus[k * 4 + 3];
                }
            }
            IcwLR o;
            if (icw_exec_op(op, d, omega, o, lOut, rOut)) {
                const int q = op.out_slot * 4;
                bus[q + 0] = o.lre; bus[q + 1] = o.lim; bus[q + 2] = o.rre; bus[q + 3] = o.rim;
            }
        }
        pre[(size_t)t * 2] = lOut;
        pre[(size_t)t * 2 + 1] = rOut;
    }
    for (int k = 0; k < ICW_N_INPUTS * 4; ++k) gb[k] = bus[k];
}

/* K4 over streams with different bus-form programs (icw_enable_stream_bus): the call's streams cut into runs
 * of one list entry (IcwK4Run, icw_device.h).  A workgroup is one wave and finds its run by a binary search
 * over the runs' first workgroups -- scalar loads through the constant address space -- so the program is a
 * scalar pointer as in K4, and the body is K4's.  The bus rows hold m.W lanes, the launch's widest run in a
 * workgroup, in dynamic LDS: a call whose streams each carry their own list has one lane per workgroup, and
 * at 64-lane rows (55 296 bytes) two of them would fill a CU's LDS.  [slot][lane] order as in K4: the lanes
 * of a wave read consecutive doubles. */
template <bool MIXIN>
__global__ __launch_bounds__(64) void icw_graph_serial_mixed(IcwK4MixArgs m)
{
    extern __shared__ __attribute__((aligned(16))) double busw[];   /* [ICW_N_INPUTS * 4][m.W] */
    const __attribute__((address_space(4))) IcwK4Run *r = (const __attribute__((address_space(4))) IcwK4Run *)m.runs;
    int lo = 0, hi = m.n_runs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (r[mid].wg0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    r += lo;
    const int lane = ((int)blockIdx.x - r->wg0) * 64 + (int)threadIdx.x;     /* the stream's index in its run */
    const int s = r->s0 + lane;
    if (lane >= r->n || (int)threadIdx.x >= m.W || s >= m.k4.n_streams) return;
    icw_graph_serial_run<MIXIN>(m.k4, icw_prog_c(m.k4.prog) + r->entry, s, IcwBusW{busw + threadIdx.x, m.W});
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

__global__ __launch_bounds__(64) void icw_advance_mixed(IcwAdvMixArgs m)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= m.adv.n_streams) return;
    IcwAdvArgs a = m.adv;
    a.ssr = m.desc[s].ssr;             /* the stream's own wrap (a lane-varying load) */
    icw_advance_stream(a, s);
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

extern "C" hipError_t icw_launch_unpack_mixed(const IcwK0MixArgs *a, hipStream_t st)
{
    if (!a->desc) return hipErrorInvalidValue;
    dim3 grid((a->k0.T + 255) / 256, a->k0.n_streams);
    hipLaunchKernelGGL(icw_unpack_frames_mixed, grid, dim3(256), 0, st, *a);
    return hipGetLastError();
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

/* K2's direct-input form: CWAVE streams with different inputs, the selection rows and the descriptor
 * table set (the host checks the formats and that in_stride holds every stream's frames) */
extern "C" hipError_t icw_launch_output_cw(const IcwK2Args *a2, const IcwDinArgs *d, hipStream_t st)
{
    if (!a2->cw || !a2->prog_id || !d->in || !d->pos || !d->fade || !d->desc) return hipErrorInvalidValue;
    IcwK2Args a = *a2;
    int tpw = ICW_K2_TPW;               /* as launch_k2_t: fewer tiles per workgroup while the grid is small */
    while (tpw > 1 && (long)((a.T + ICW_K2_TILE * tpw - 1) / (ICW_K2_TILE * tpw)) * a.n_streams < 512) tpw >>= 1;
    a.tpw = tpw;
    const int span = ICW_K2_TILE * tpw;
    dim3 grid((a.T + span - 1) / span, a.n_streams);
    const size_t lds = (size_t)a.n_regs * 4 * ICW_K2_TILE * sizeof(double);
    if (a.trig) hipLaunchKernelGGL((icw_output_cw<true>), grid, dim3(ICW_K2_TILE), lds, st, a, *d);
    else hipLaunchKernelGGL((icw_output_cw<false>), grid, dim3(ICW_K2_TILE), lds, st, a, *d);
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_trig_table(const IcwTrigArgs *a, hipStream_t st)
{
    hipLaunchKernelGGL(icw_trig_table, dim3((a->T + 255) / 256, a->slabs ? a->n_slabs : 1), dim3(256), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_graph_serial(const IcwK4Args *a, hipStream_t st)
{
    if (a->desc) hipLaunchKernelGGL(icw_graph_serial<true>, dim3((a->n_streams + 63) / 64), dim3(64), 0, st, *a);
    else hipLaunchKernelGGL(icw_graph_serial<false>, dim3((a->n_streams + 63) / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}

/* the mixed K4: n_wgs one-wave workgroups over the runs (the host cut them: icw_k4_cut_runs) */
extern "C" hipError_t icw_launch_graph_serial_mixed(const IcwK4MixArgs *m, int n_wgs, hipStream_t st)
{
    if (!m->runs || m->n_runs <= 0 || n_wgs <= 0 || m->W < 1 || m->W > 64) return hipErrorInvalidValue;
    const size_t lds = (size_t)ICW_N_INPUTS * 4 * (size_t)m->W * sizeof(double);
    if (m->k4.desc) hipLaunchKernelGGL(icw_graph_serial_mixed<true>, dim3(n_wgs), dim3(64), lds, st, *m);
    else hipLaunchKernelGGL(icw_graph_serial_mixed<false>, dim3(n_wgs), dim3(64), lds, st, *m);
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

extern "C" hipError_t icw_launch_advance_mixed(const IcwAdvMixArgs *a, hipStream_t st)
{
    if (!a->desc) return hipErrorInvalidValue;
    hipLaunchKernelGGL(icw_advance_mixed, dim3((a->adv.n_streams + 63) / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}

/*
 * icw_render.hip -- gfx950 (CDNA4) kernels of the renders that are serial per channel: the dither
 * generator (K3a: icw_dith_twist / icw_dith_samples / icw_dith_fix), the serial render (K3b:
 * icw_render_serial), the row render (K3c: icw_render_rowc) and the FP_CHECK render (icw_render_fc),
 * with their launchers.  The elementwise render lives in the output kernels (icw_kernels.hip); KR
 * (icw_render_mixed) is that render as a kernel of its own, for a call over streams with different renders.
 *
 * Built like icw_kernels.hip (`-ffp-contract=off`, no fast-math): every floating-point expression
 * keeps the operand order of the reference.
 *
 * Two includes are wider than what is used: icw_iir_dev.h for the FP_CHECK census (IcwFes, icw_fc,
 * icw_fes_flush) and icw_unpack_dev.h for the one-line icw_ic, so an edit of the IIR or unpack device
 * code rebuilds this unit too.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/icw.h"
#include "icw_device.h"
#include "icw_iir_dev.h"
#include "icw_launch.h"

#pragma clang fp contract(off)

#include "icw_quant_dev.h"
#include "icw_unpack_dev.h"   /* icw_ic */

/* ------------------------------------------------------ serial render kernel (K3) ------ */
/* sound_render_value (sound_render.c:691-809) for the dithered / noise-shaped renders, whose
 * state (MT19937 position, sloped-TPDF memory, noise-shaper feedback) is serial per channel: the
 * dither generator (the MT19937 words, mt_jrnd.c:99-124) first, then the renders, shaper history in
 * registers (identical sums to the ring of ns_fir/ns_iir, sound_render.c:403-489). */
__device__ __forceinline__ uint32_t icw_mt_twist_word(uint32_t u, uint32_t v)
{
    const uint32_t y = (u & 0x80000000u) | (v & 0x7fffffffu);
    return (y >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ uint32_t icw_mt_temper(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

#define ICW_SQRT6 (2.4494897427831780981972840747059)

/* Cooperative dither generation (K3f's redo, icw_dither_coop_body): one wave per render channel.  The random term of
 * sound_render_value (sound_render.c:711-756) depends only on the channel's MT19937 stream, so the
 * stream is produced 624 words at a time by the whole wave:
 *   twist     the 624-word regeneration (mt_jrnd.c:105-120) in three dependency phases
 *             ([0,227) from old words; [227,454) and [454,623) from words new by then; then 623);
 *   window    words idx..623 tempered in parallel; word pairs -> dsopen values (mt_jrnd.c:218-256);
 *             a rejected pair (+-1.0) yields no value -- the reference just draws the next pair --
 *             so accepted values are compacted with a ballot prefix count;
 *   samples   V consecutive values per sample (RPDF 1, TPDF 2, STPDF 1 + the previous, GAUSS 12),
 *             one lane per sample.
 * A pair or a sample may straddle windows (one carried word, < V carried values).  The block ends
 * exactly after its last sample, so idx is where the reference's would be. */
__device__ __forceinline__ void icw_coop_twist(uint32_t *mt, int lane)
{
    uint32_t r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        if (i < 227) r[q] = mt[i + 397] ^ icw_mt_twist_word(mt[i], mt[i + 1]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        if (i < 227) mt[i] = r[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 227 + lane + 64 * q;
        if (i < 454) r[q] = mt[i - 227] ^ icw_mt_twist_word(mt[i], mt[i + 1]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 227 + lane + 64 * q;
        if (i < 454) mt[i] = r[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = 454 + lane + 64 * q;
        if (i < 623) r[q] = mt[i - 227] ^ icw_mt_twist_word(mt[i], mt[i + 1]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = 454 + lane + 64 * q;
        if (i < 623) mt[i] = r[q];
    }
    __syncthreads();
    if (lane == 0) mt[623] = mt[396] ^ icw_mt_twist_word(mt[623], mt[0]);
    __syncthreads();
}

/* the generator g's samples of the block (or chunk) the sequential way: from the state in a.mt /
 * a.mt_idx / rs[0], or (bk) from the chunk's backup K3t made -- K3f's redo of a channel whose words
 * held a rejected pair */
template <int RT>
__device__ __forceinline__ void icw_dither_coop_body(const IcwK3Args &a, int g, const uint32_t *bk)
{
    constexpr int V = RT == ICW_RENDER_GAUSS ? 12 : (RT == ICW_RENDER_TPDF ? 2 : 1);
    __shared__ uint32_t mt[624];
    __shared__ uint32_t tw[626];           /* the window's word list: [carried word] + tempered mt[idx..623] */
    __shared__ double vals[313 + 16];      /* [carried values] + the window's accepted values */
    __shared__ short pidx[313];            /* pair index of each accepted value of the window */
    const int lane = threadIdx.x;          /* one wave per generator: everything below is wave-uniform */
    double *rs = a.rs + (size_t)g * ICW_RSTATE;
    int idx;
    double prev_rnd;
    if (bk) {
        for (int i = lane; i < 624; i += 64) mt[i] = bk[i];
        idx = (int)bk[624];
        prev_rnd = *(const double *)(bk + 626);
    } else {
        for (int i = lane; i < 624; i += 64) mt[i] = a.mt[(size_t)i * a.mt_pitch + g];
        idx = a.mt_idx[g];
        prev_rnd = rs[0];
    }
    const double dth_mul = a.rk.dth_mul;
    /* generator-major (dith_gm): the wave's samples of a window are one contiguous run, each store
     * instruction writes 64 consecutive doubles; time-major: one double per row (K3b's layout) */
    double *dd = a.dith_gm ? a.dith + (size_t)g * a.dith_pitch : a.dith + g;
    const size_t dp = a.dith_gm ? 1 : a.dith_pitch;
    const int T = a.T;
    int t = 0, k = 0, c = 0;               /* samples done, carried values, carried word (0/1) */
    uint32_t cword = 0;
    __syncthreads();
    while (t < T) {
        if (idx >= 624) {
            icw_coop_twist(mt, lane);
            idx = 0;
        }
        const int nw = 624 - idx, nl = nw + c, np = nl >> 1;
        for (int j = lane; j < nw; j += 64) tw[c + j] = icw_mt_temper(mt[idx + j]);
        if (lane == 0 && c) tw[0] = cword;
        __syncthreads();
        int nacc = 0;
        for (int p0 = 0; p0 < np; p0 += 64) {
            const int pp = p0 + lane;
            bool acc = false;
            double d = 0.0;
            if (pp < np) {
                const uint32_t ua = tw[2 * pp] >> 5, ub = tw[2 * pp + 1] >> 6;
                acc = !(ua == 0u && ub == 0u);                  /* dsopen rejects exactly -1.0 */
                d = ((ua * 67108864.0 + ub) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0;
            }
            const unsigned long long m = __ballot(acc);
            const int pos = nacc + __popcll(m & ((1ull << lane) - 1ull));
            if (acc) { vals[k + pos] = d; pidx[pos] = (short)pp; }
            nacc += __popcll(m);
        }
        __syncthreads();
        const int nv = k + nacc;
        const int ns = min(nv / V, T - t);
        for (int sm = lane; sm < ns; sm += 64) {
            const double *v = vals + sm * V;
            double rnd;
            if (RT == ICW_RENDER_RPDF) {
                rnd = v[0] / ICW_SQRT2;
            } else if (RT == ICW_RENDER_TPDF) {
                rnd = v[0];
                rnd += v[1];
                rnd /= 2.0;
            } else if (RT == ICW_RENDER_STPDF) {
                rnd = (v[0] - (sm == 0 ? prev_rnd : v[-1])) / 2.0;
            } else {
                rnd = v[0];
#pragma unroll
                for (int i = 1; i < 12; ++i) rnd += v[i];
                rnd /= (2.0 * ICW_SQRT6);
            }
            dd[(size_t)(t + sm) * dp] = rnd * dth_mul;
        }
        if (RT == ICW_RENDER_STPDF && ns > 0) prev_rnd = vals[ns - 1];
        t += ns;
        if (t >= T) {
            /* the block ends inside this window: consume exactly through its last value's pair */
            const int need = ns * V - k;                        /* >= 1: carried values are < V */
            const int plast = pidx[need - 1];
            idx += 2 * (plast + 1) - c;
            c = 0;
        } else {
            /* everything consumed; carry the partial sample's values and an odd last word */
            const int kn = nv - ns * V;
            __syncthreads();
            double cv = 0.0;
            if (lane < kn) cv = vals[ns * V + lane];
            __syncthreads();
            if (lane < kn) vals[lane] = cv;
            k = kn;
            if (nl & 1) { cword = tw[nl - 1]; c = 1; }
            else c = 0;
            idx = 624;
        }
        __syncthreads();
    }
    for (int i = lane; i < 624; i += 64) a.mt[(size_t)i * a.mt_pitch + g] = mt[i];
    if (lane == 0) {
        a.mt_idx[g] = idx;
        rs[0] = prev_rnd;
    }
}

/* ------------------------------------------------------ split dither generator (K3t/K3s/K3f) ---- */
/* The dither term of sound_render_value (sound_render.c:711-751) consumes the channel's MT19937 words
 * in a fixed order: sample t of a chunk takes words [W t, W t + W) after the chunk's starting
 * position (W = 2 V: V dsopen values of two words each, mt_jrnd.c:218-256) -- unless a pair is
 * rejected (exactly -1.0, probability 2^-53 per pair), which shifts every later sample.  So
 *   K3t  icw_dith_twist    one wave per generator: saves the starting state (the backup), then runs
 *                          the twists (mt_jrnd.c:99-124) and writes the chunk's W T tempered words,
 *                          coalesced, and the generator's state after them (mt, idx);
 *   K3s  icw_dith_samples  a thread per sample, frame-parallel: its W words -> the V values -> rnd *
 *                          dth_mul (STPDF: the previous sample's value, or the backup's prev_rnd);
 *                          a rejected pair flags the generator;
 *   K3f  icw_dith_fix      a wave per flagged generator only: the chunk again from the backup, the
 *                          sequential way (icw_dither_coop_body, rejections and all), output and state.
 * The serial part left is the twist chain itself; K3a did the windows' tempering, pairing, ballots and
 * samples on the same wave between twists.  Chunks of icw_dith_chunk_frames (icw_device.h) frames. */
__global__ __launch_bounds__(64) void icw_dith_twist(IcwK3Args a, int W)
{
    __shared__ uint32_t mt[624];
    const int lane = threadIdx.x, g = blockIdx.x;
    uint32_t *bk = a.dbk + (size_t)g * ICW_DBK;
    double *rs = a.rs + (size_t)g * ICW_RSTATE;
    for (int i = lane; i < 624; i += 64) {
        const uint32_t v = a.mt[(size_t)i * a.mt_pitch + g];
        mt[i] = v;
        bk[i] = v;
    }
    int idx = a.mt_idx[g];
    if (lane == 0) {
        bk[624] = (uint32_t)idx;
        *(double *)(bk + 626) = rs[0];
        a.dflag[g] = 0;
    }
    __syncthreads();
    uint32_t *wr = a.wbuf + (size_t)g * a.wpitch;
    const long long nw = (long long)W * a.T;
    long long pos = 0;
    bool twisted = false;
    while (pos < nw) {
        if (idx >= 624) {
            icw_coop_twist(mt, lane);
            idx = 0;
            twisted = true;
        }
        const int n = (int)min((long long)(624 - idx), nw - pos);
        for (int j = lane; j < n; j += 64) wr[pos + j] = icw_mt_temper(mt[idx + j]);
        pos += n;
        idx += n;
    }
    if (twisted)
        for (int i = lane; i < 624; i += 64) a.mt[(size_t)i * a.mt_pitch + g] = mt[i];
    if (lane == 0) a.mt_idx[g] = idx;
}

/* the dsopen value of a word pair (mt_jrnd.c:218-256); rej: the pair is the rejected -1.0 */
__device__ __forceinline__ double icw_dsopen_pair(uint32_t wa, uint32_t wb, bool &rej)
{
    const uint32_t ua = wa >> 5, ub = wb >> 6;
    rej |= ua == 0u && ub == 0u;
    return ((ua * 67108864.0 + ub) * (1.0 / 9007199254740992.0)) * 2.0 - 1.0;
}

/* gm: a thread per (generator, sample), samples fastest (generator-major rows, coalesced); tm: the
 * generators fastest (time-major rows, K3b / K3f) */
template <int RT>
__global__ __launch_bounds__(256) void icw_dith_samples(IcwK3Args a)
{
    constexpr int V = RT == ICW_RENDER_GAUSS ? 12 : (RT == ICW_RENDER_TPDF ? 2 : 1);
    constexpr int W = 2 * V;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long tot = (long long)a.n_gen * a.T;
    if (id >= tot) return;
    int g, t;
    if (a.dith_gm) { g = (int)(id / a.T); t = (int)(id - (long long)g * a.T); }
    else { t = (int)(id / a.n_gen); g = (int)(id - (long long)t * a.n_gen); }
    const uint32_t *w = a.wbuf + (size_t)g * a.wpitch + (size_t)t * W;
    uint32_t u[W];
    if constexpr (W % 4 == 0) {
#pragma unroll
        for (int i = 0; i < W; i += 4) {
            const uint4 q = *(const uint4 *)(w + i);
            u[i] = q.x; u[i + 1] = q.y; u[i + 2] = q.z; u[i + 3] = q.w;
        }
    } else {
        const uint2 q = *(const uint2 *)w;
        u[0] = q.x; u[1] = q.y;
    }
    bool rej = false;
    double rnd;
    if constexpr (RT == ICW_RENDER_RPDF) {
        rnd = icw_dsopen_pair(u[0], u[1], rej) / ICW_SQRT2;
    } else if constexpr (RT == ICW_RENDER_TPDF) {
        rnd = icw_dsopen_pair(u[0], u[1], rej);
        rnd += icw_dsopen_pair(u[2], u[3], rej);
        rnd /= 2.0;
    } else if constexpr (RT == ICW_RENDER_STPDF) {
        double prev;
        if (t == 0) {
            prev = *(const double *)(a.dbk + (size_t)g * ICW_DBK + 626);
        } else {
            bool r2 = false;               /* the previous sample's own pair is flagged by its thread */
            prev = icw_dsopen_pair(w[-2], w[-1], r2);
        }
        const double tr = icw_dsopen_pair(u[0], u[1], rej);
        rnd = (tr - prev) / 2.0;
        if (t == a.T - 1) a.rs[(size_t)g * ICW_RSTATE] = tr;     /* prev_rnd after the chunk */
    } else {
        rnd = icw_dsopen_pair(u[0], u[1], rej);
#pragma unroll
        for (int i = 1; i < 12; ++i) rnd += icw_dsopen_pair(u[2 * i], u[2 * i + 1], rej);
        rnd /= (2.0 * ICW_SQRT6);
    }
    const size_t o = a.dith_gm ? (size_t)g * a.dith_pitch + t : (size_t)t * a.dith_pitch + g;
    a.dith[o] = rnd * a.rk.dth_mul;
    if (rej) atomicOr(&a.dflag[g], 1);
}

template <int RT>
__global__ __launch_bounds__(64) void icw_dith_fix(IcwK3Args a)
{
    const int g = blockIdx.x;
    if (!a.dflag[g]) return;               /* wave-uniform: the usual case, no rejected pair */
    icw_dither_coop_body<RT>(a, g, a.dbk + (size_t)g * ICW_DBK);
    if (threadIdx.x == 0) a.dflag[g] = 0;
}

/* Shaper history as a ring of R values (R = ICW_MAX_NS_TAPS for the FIR shapers, 4 for the
 * order-4 IIR shapers; R divides the unroll length ICW_MAX_NS_TAPS): at unrolled step J the newest
 * value goes to slot J mod R, so age i lives in slot (J - i) mod R -- compile-time indices, no
 * register moves (the reference's ring with a decrementing write pointer, sound_render.c:403-489). */
template <int R>
__device__ __forceinline__ void icw_ring_rotate1(double (&X)[R])
{
    const double r0 = X[0];
#pragma unroll
    for (int k = 0; k < R - 1; ++k) X[k] = X[k + 1];
    X[R - 1] = r0;
}

/* One sample of sound_render_value after the dither term (sound_render.c:754-809).  NN is the
 * shaper's tap count (a template parameter: a runtime count would predicate all 20 taps). */
template <int KIND, int R, int NN, int J>
__device__ __forceinline__ int icw_render_step(double input, double d, double &prev_err, double (&E)[R],
                                               double (&O)[R], const IcwRenderK &k, const double (&cf)[2 * NN + 1],
                                               unsigned &clips, double &pk)
{
    input = (input * k.norm_mul) - prev_err;
    double q = input + d;
    int delta;
    q = icw_round_q(q, k.round_offset, k.sign_delta, delta);
    pk = fmax(pk, fabs(q));
    const int vc = icw_clamp_int(q, k, clips);    /* unconditional: a NaN counts no clip */
    int val = (isnan(q) ? (int)0x80000000 : vc) + delta;
    /* noise shaping for the next sample (ns_empty / ns_fir / ns_iir) */
    const double ev = (double)val - input;
    double res = 0.0;
    if (KIND == 1) {
        E[J % R] = ev;
#pragma unroll
        for (int i = 0; i < NN; ++i) res += cf[i] * E[(J - i + 2 * R) % R];
    } else if (KIND == 2) {
        E[J % R] = ev;
#pragma unroll
        for (int i = 0; i < NN; ++i) res += cf[i] * E[(J - i + 2 * R) % R] - cf[i + NN] * O[(J - 1 - i + 2 * R) % R];
        O[J % R] = res;
    }
    prev_err = res;
    return val << k.norm_shift;
}

template <int KIND, int R, int NN, int J0>
__device__ __forceinline__ void icw_render_block(const double (&xin)[ICW_MAX_NS_TAPS], const double (&dv)[ICW_MAX_NS_TAPS],
                                                 double &prev_err, double (&E)[R], double (&O)[R], const IcwRenderK &k,
                                                 const double (&cf)[2 * NN + 1], unsigned &clips, double &pk, int *vrow,
                                                 int lim)
{
    if constexpr (J0 < ICW_MAX_NS_TAPS) {
        if (J0 < lim) {
            vrow[J0] = icw_render_step<KIND, R, NN, J0>(xin[J0], dv[J0], prev_err, E, O, k, cf, clips, pk);
            icw_render_block<KIND, R, NN, J0 + 1>(xin, dv, prev_err, E, O, k, cf, clips, pk, vrow, lim);
        }
    }
}

/* a full block whose step J refills xin[J] / dv[J] with the next block's sample right after
 * consuming it, so the loads run a block ahead of use (clamped indices stay in bounds) */
template <int KIND, int R, int NN, int J0>
__device__ __forceinline__ void icw_render_block_pf(double (&xin)[ICW_MAX_NS_TAPS], double (&dv)[ICW_MAX_NS_TAPS],
                                                    double &prev_err, double (&E)[R], double (&O)[R],
                                                    const IcwRenderK &k, const double (&cf)[2 * NN + 1],
                                                    unsigned &clips, double &pk, int *vrow, const double *pp,
                                                    const double *dp, size_t dpitch, int tn, int tmax)
{
    if constexpr (J0 < ICW_MAX_NS_TAPS) {
        vrow[J0] = icw_render_step<KIND, R, NN, J0>(xin[J0], dv[J0], prev_err, E, O, k, cf, clips, pk);
        const int tj = min(tn + J0, tmax);
        xin[J0] = pp[(size_t)tj * 2];
        dv[J0] = dp ? dp[(size_t)tj * dpitch] : 0.0;
        icw_render_block_pf<KIND, R, NN, J0 + 1>(xin, dv, prev_err, E, O, k, cf, clips, pk, vrow, pp, dp, dpitch, tn,
                                                 tmax);
    }
}

/* Write frames [f0, f1) of a block: the lane pair (L = even lane, R = odd lane) of a stream owns
 * the interleaved L,R frames; values come from the pair's LDS rows.  16-bit frames are one dword;
 * 24-bit frames are three 16-bit words (2-byte aligned for every stride). */
__device__ __forceinline__ void icw_put_frames(const int *vl, const int *vr, unsigned char *o, int osz, int f0, int f1)
{
    if (osz == 2) {
        for (int f = f0; f < f1; ++f)
            *(uint32_t *)(o + (size_t)f * 4) = ((uint32_t)vl[f] & 0xffffu) | ((uint32_t)vr[f] << 16);
    } else {
        for (int f = f0; f < f1; ++f) {
            const uint32_t l = (uint32_t)vl[f], r = (uint32_t)vr[f];
            uint16_t *q = (uint16_t *)(o + (size_t)f * 6);
            q[0] = (uint16_t)(l & 0xffffu);
            q[1] = (uint16_t)(((l >> 16) & 0xffu) | ((r & 0xffu) << 8));
            q[2] = (uint16_t)((r >> 8) & 0xffffu);
        }
    }
}

/* Render (K3b): the serial remainder of sound_render_value -- scale, error feedback, rounding,
 * clips, peak, noise shaper -- with the dither term from K3a.  One lane per channel, samples in
 * blocks of ICW_MAX_NS_TAPS (a multiple of the ring period): the block's inputs are loaded
 * before use.  rs keeps the shaper history by age (0 = newest), 20 + 20 slots. */
template <int KIND, int R, int NN>
__global__ __launch_bounds__(64) void icw_render_serial(IcwK3Args a)
{
    constexpr int NM = ICW_MAX_NS_TAPS;
    static_assert(NM % R == 0, "ring period must divide the unroll");
    __shared__ int vals[64][NM + 1];    /* the block's rendered values, one row per lane */
    const int lane = threadIdx.x;
    const int g0 = blockIdx.x * 64 + lane;
    const bool valid = g0 < a.n_gen;
    const int g = valid ? g0 : a.n_gen - 1;
    const int s = g >> 1, ch = g & 1;
    double *rs = a.rs + (size_t)g * ICW_RSTATE;
    double prev_err = rs[1];
    double E[R], O[R];
    /* block start: age i sits in slot (-1 - i) mod R */
#pragma unroll
    for (int i = 0; i < R; ++i) { E[(R - 1 - i) % R] = rs[2 + i]; O[(R - 1 - i) % R] = rs[2 + NM + i]; }
    const IcwRenderK &k = a.rk;
    double cf[2 * NN + 1];                                    /* shaper coefficients in registers */
#pragma unroll
    for (int i = 0; i < 2 * NN; ++i) cf[i] = k.ns_c[i];
    cf[2 * NN] = 0.0;
    const int osz = k.is24 ? 3 : 2;
    const double *pp = a.pre + (size_t)s * a.pre_stride + ch;
    const double *dp = a.dith ? a.dith + g : nullptr;         /* time-major [t][dith_pitch] */
    const size_t dpitch = a.dith_pitch;
    unsigned char *op = a.out + (size_t)s * a.out_stride;     /* the stream's frames */
    int *vrow = vals[lane];
    const int *vl = vals[lane & ~1], *vr = vals[lane | 1];
    const int half = (lane & 1) * (NM / 2);
    unsigned clips = 0;
    double pk = 0.0;
    const int T = a.T;
    int t = 0;
    double xin[NM], dv[NM];
    if (T >= NM) {
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            xin[j] = pp[(size_t)j * 2];
            dv[j] = dp ? dp[(size_t)j * dpitch] : 0.0;         /* ROUND: rnd * dth_mul == 0.0 * dth_mul */
        }
    }
    for (; t + NM <= T; t += NM) {
        icw_render_block_pf<KIND, R, NN, 0>(xin, dv, prev_err, E, O, k, cf, clips, pk, vrow, pp, dp, dpitch, t + NM,
                                            T - 1);
        __builtin_amdgcn_wave_barrier();
        if (valid) icw_put_frames(vl, vr, op + (size_t)t * 2 * osz, osz, half, half + NM / 2);
        __builtin_amdgcn_wave_barrier();
    }
    const int rem = T - t;
    if (rem > 0) {
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            xin[j] = j < rem ? pp[(size_t)(t + j) * 2] : 0.0;
            dv[j] = (j < rem && dp) ? dp[(size_t)(t + j) * dpitch] : 0.0;
        }
        icw_render_block<KIND, R, NN, 0>(xin, dv, prev_err, E, O, k, cf, clips, pk, vrow, rem);
        __builtin_amdgcn_wave_barrier();
        const int h = (rem + 1) / 2;
        if (valid) icw_put_frames(vl, vr, op + (size_t)t * 2 * osz, osz, (lane & 1) ? h : 0, (lane & 1) ? rem : h);
        /* back to the block-start mapping: rotate left by rem mod R */
#pragma unroll
        for (int r = 1; r < NM; ++r)
            if (r <= rem) { icw_ring_rotate1<R>(E); icw_ring_rotate1<R>(O); }
    }
    if (!valid) return;
    rs[1] = prev_err;
#pragma unroll
    for (int i = 0; i < R; ++i) { rs[2 + i] = E[(R - 1 - i) % R]; rs[2 + NM + i] = O[(R - 1 - i) % R]; }
    if (clips) atomicAdd(&a.clips[g], clips);
    if (pk > 0.0) atomicMax(&a.peak_bits[g], (unsigned long long)__double_as_longlong(pk));
}

/* ------------------------------------------- render, row broadcast: the chain (K3c) ------- */
/* The serial render of K3b with one 16-lane DPP row per channel instead of one lane, built like the
 * IIR kernel K1r (icw_iir.hip): every lane of a row runs the channel's chain redundantly, so each
 * value is row-uniform, and what is not on the chain leaves the per-sample instruction stream --
 * K3b spends ~51 instructions per sample for a ~22-instruction dependent chain:
 *   - the shaper terms: right after the error ev of sample n is known, ONE lane-parallel multiply
 *     makes lane l hold cf[l+1] * ev (P2: cf[l+17]), term l+1 of sample n+l+1; the sum adds it
 *     from that lane with `v_fmac_f64_dpp ... row_newbcast` (icw_render_asm.inc).  The IIR shaper's
 *     term cf[i]*E - cf[i+NN]*O is formed the same way, three lane-parallel ops per sample;
 *   - clips and peak: each lane stages q in its own LDS slot; at the end of a 20-sample block lane
 *     l counts samples l and l+16 (every row holds all of them) -- ~0.5 instead of ~6 per sample;
 *   - the frames: the shifted values are staged alike and a block's frames are written by 40
 *     lanes at once.
 * Sums keep the reference's order (res = 0.0; res += t_0; res += t_1 ...), products are rounded
 * before they are added, so every value is the reference's (sound_render.c:754-809, ns_fir
 * :403-438, ns_iir :442-489).  Small batches (the host's choice): 4 channels per wave. */
__device__ __forceinline__ double icw_rmul(double a, double b)
{
    double r;
    asm volatile("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ double icw_rsub(double a, double b)
{
    double r;
    asm volatile("v_add_f64 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

#include "icw_render_asm.inc"

struct IcwRowNs {
    double c0, cN;      /* row-uniform: cf[0]; IIR: cf[NN] (the O term of t_0) */
    double pl, pl2;     /* per lane: FIR cf[l+1], cf[l+17]; IIR cf[l+1], cf[l+1+NN] (0 past the taps) */
    double one;
};

/* one sample at unroll step J (0..ICW_MAX_NS_TAPS-1); rings of R slots, the newest at J mod R.
 *
 * The integer never sits on the error-feedback chain.  The reference forms val = (int)q' + delta
 * (q' the clipped q, sound_render.c:782-797) and feeds back ev = (double)val - input (:800).  q' lies
 * in [lo + 1, hi - 1] (|q'| < 2^24) and delta is 0 or -1, so (double)val = trunc(q') + (double)delta
 * exactly -- an integer-valued sum of two integers, no rounding; the trunc of a negative q' in (-1, 0)
 * is -0.0, and -0.0 + 0.0 = +0.0 = (double)0, -0.0 + -1.0 = -1.0 = (double)-1.  A NaN q (only from a
 * NaN input, which makes ev NaN either way) clamps to a number here; its stored value is fixed up in
 * the flush from the staged q, as the reference's (int)NaN = INT_MIN (cvttsd2si) + delta 0.  The
 * double val (vst) is converted to the integer off the chain, in the flush.
 * MR: mid-riser (round_offset 0, sign_delta -1: sound_render_recalc, sound_render.c:527-540) -- the
 * rounding add q + (+-0.0) changes nothing but a -0.0 (to +0.0), which neither the clip stage, the
 * peak (fabs) nor trunc + delta can tell apart, so it is skipped and only delta's select remains,
 * beside the clamp.  Mid-tread (round_offset 0.5, sign_delta 0): q +- 0.5 by the sign of q, both
 * sums formed beside the compare, delta 0.
 * The FIR shaper's first term 0.0 + c0 * ev (ns_fir, sound_render.c:420-427: the sum starts at 0.0)
 * is one fma(c0, ev, +0.0): the exact product plus +0.0, rounded once, is round(c0 * ev) with an
 * exact zero's sign made +, what 0.0 + round(c0 * ev) gives -- except where c0 * ev is nonzero but
 * rounds to zero (|ev| below ~2^-1022 / |c0|: a subnormal input with vd = 0): the fma then gives the
 * product's sign, -0.0 for a negative one, where the reference's 0.0 + (-0.0) is +0.0.  Only the sign
 * of a zero differs, in res (prev_ns_err), and nothing downstream can see it: input = xs - res, then
 * q = input + d, differ at most in a zero's sign, which trunc + delta, the clip stage and the peak
 * (fabs) all map alike, so ev, the integer and the meters are the reference's (the saved prev_ns_err
 * of the state blob may hold -0.0 for its +0.0).  On the chain per sample: the input and q, clamp
 * (2), trunc, + delta, ev, the fma and the shaper's DPP sum -- 16 ops for MEW44 where the integer
 * round trip and the rounding's compare / select / add made it 23 (14 in a clamp-free block). */
/* qst: the lane's slot for sample 0 in the q stage qs[row][U / 2][16][2] -- samples 2i and 2i + 1 of a
 * lane side by side, written together by one ds_write_b128 at the odd sample (qh holds the even one) */
template <int KIND, int NN, int R, int J, bool MR, bool FAST>
__device__ __forceinline__ void icw_rrow_step(double xs, double d, double &prev_err, double (&E)[R], double (&O)[R],
                                              double (&P)[R], double (&P2)[R], const IcwRowNs &c,
                                              const IcwRenderK &k, double *qst, double &qh, double &mq)
{
    constexpr int S = J % R;
    const double input = xs - prev_err;                /* xs = x * norm_mul, formed in the staging */
    double q = input + d;
    double dd;                                         /* (double)delta */
    if constexpr (MR) {
        dd = q < 0.0 ? -1.0 : 0.0;
    } else {
        const double qa = q + 0.5, qb = q - 0.5;       /* q + round_offset, q - round_offset */
        q = q < 0.0 ? qb : qa;
        dd = 0.0;
    }
    /* the clip stage as it reaches the integer (icw_clamp_int); clips and peak from the staged q.  A
     * clamp-free block (FAST, icw_render_rowc) has lo < q < hi for every sample, where the reference's
     * clip stage changes nothing and trunc(q) is already in [lo + 1, hi - 1] */
    double vd;
    if constexpr (FAST) {
        vd = __builtin_trunc(q) + dd;
    } else {
        vd = __builtin_trunc(fmax(fmin(q, k.hi - 1.0), k.lo + 1.0)) + dd;
        mq = icw_vmax_abs(mq, q);       /* the block's largest |q| (icw_render_rowc's calm test; unused otherwise) */
    }
    if constexpr (J & 1) *(double2 *)(qst + (J >> 1) * 32) = make_double2(qh, q);   /* the integer is the flush's */
    else qh = q;
    const double ev = vd - input;
    double res = 0.0;
    /* the new products go out before this sample's sum, whose volatile fmac block then separates
     * them from their first DPP read in the next sample (a VALU write -> DPP read needs two
     * instructions in between, and the compiler does not look into the asm) */
    if constexpr (KIND == 1) {
        E[S] = ev;
        P[S] = icw_rmul(c.pl, ev);
        if constexpr (NN > 17) P2[S] = icw_rmul(c.pl2, ev);
        res = __builtin_fma(c.c0, ev, 0.0);
        res = icw_ns_row_sum<NN, R, S>(res, c.one, P, P2);
    } else if constexpr (KIND == 2) {
        E[S] = ev;
        const double op = O[(S + R - 1) % R];
        P[S] = icw_rsub(icw_rmul(c.pl, ev), icw_rmul(c.pl2, op));
        res = 0.0 + (c.c0 * ev - c.cN * op);
        res = icw_ns_row_sum<NN, R, S>(res, c.one, P, P2);
        O[S] = res;
    }
    prev_err = res;
}

/* look-ahead reads: the next block's inputs and dither values of the row's channel, staged in LDS
 * (icw_k3c_stage_*): sample J of this block reads sample J of the next -- a whole block ahead of
 * its use, at an immediate offset (no address arithmetic per sample, no wait on global memory) */
template <int KIND, int NN, int R, int J, bool MR, bool FAST>
__device__ __forceinline__ void icw_rrow_block(double (&xin)[ICW_MAX_NS_TAPS], double (&dv)[ICW_MAX_NS_TAPS],
                                               double &prev_err, double (&E)[R], double (&O)[R], double (&P)[R],
                                               double (&P2)[R], const IcwRowNs &c, const IcwRenderK &k, double *qst,
                                               const double *xn, const double *dn, double &mq)
{
    if constexpr (J < ICW_MAX_NS_TAPS) {
        /* the next block's samples J, J + 1 by one ds_read_b128 each for x and d (16-byte aligned rows) */
        double qh;
        icw_rrow_step<KIND, NN, R, J, MR, FAST>(xin[J], dv[J], prev_err, E, O, P, P2, c, k, qst, qh, mq);
        icw_rrow_step<KIND, NN, R, J + 1, MR, FAST>(xin[J + 1], dv[J + 1], prev_err, E, O, P, P2, c, k, qst, qh, mq);
        /* after both steps, so the 16 bytes land in the pair's own registers (no moves) */
        const double2 x2 = *(const double2 *)(xn + J), d2 = *(const double2 *)(dn + J);
        xin[J] = x2.x;
        xin[J + 1] = x2.y;
        dv[J] = d2.x;
        dv[J + 1] = d2.y;
        icw_rrow_block<KIND, NN, R, J + 2, MR, FAST>(xin, dv, prev_err, E, O, P, P2, c, k, qst, xn, dn, mq);
    }
}

template <int KIND, int NN, int R, int J, bool MR>
__device__ __forceinline__ void icw_rrow_block_lim(const double (&xin)[ICW_MAX_NS_TAPS], const double (&dv)[ICW_MAX_NS_TAPS],
                                                   double &prev_err, double (&E)[R], double (&O)[R], double (&P)[R],
                                                   double (&P2)[R], const IcwRowNs &c, const IcwRenderK &k, double *qst,
                                                   int lim, double &mq)
{
    if constexpr (J < ICW_MAX_NS_TAPS) {
        if (J < lim) {
            double qh;
            icw_rrow_step<KIND, NN, R, J, MR, false>(xin[J], dv[J], prev_err, E, O, P, P2, c, k, qst, qh, mq);
            if (J + 1 < lim) {
                icw_rrow_step<KIND, NN, R, J + 1, MR, false>(xin[J + 1], dv[J + 1], prev_err, E, O, P, P2, c, k, qst, qh, mq);
                icw_rrow_block_lim<KIND, NN, R, J + 2, MR>(xin, dv, prev_err, E, O, P, P2, c, k, qst, lim, mq);
            } else {
                qst[(J >> 1) * 32] = qh;                 /* the last sample, an even one, alone */
            }
        }
    }
}

/* What a lane holds of one block's staging between its global loads and its stores to LDS (frames
 * t0 .. t0 + U - 1 of the workgroup's two streams: lanes 0-19 / 32-51 frame i of stream A / B, L and R
 * in 16 bytes; its four channels' dither values: lanes 0-39 half a dither row each, 16 bytes).  The
 * loads run blocks ahead of the stores (icw_k3c_stage_*), so no per-sample wait reaches global memory. */
struct IcwRowStage {
    double2 x, d;
};

/* End of a block of nf samples: clips and peak of the staged q (lane l: samples l, l + 16 of its
 * row), then the block's frames -- lanes 0-31 write stream A's (rows 0, 1), 32-63 stream B's.  The
 * integer is the chain's trunc(q') + delta formed again from q, off the chain: the saturating
 * conversion, the clamp into [lo + 1, hi - 1] and the mid-riser's delta (q < 0); a NaN q gives
 * (int)NaN = INT_MIN (x86 cvttsd2si) with delta 0, as icw_render_round. */
template <bool MR>
__device__ __forceinline__ int icw_rrow_val(double q, int lo1, int hi1)
{
    const int v = icw_med3_i32(icw_cvt_sat_i32(q), lo1, hi1) + (MR && q < 0.0 ? -1 : 0);
    return q != q ? (int)0x80000000 : v;
}

/* (the exact form; returns, wave-uniform, whether every q of the block had |q| < clip_abs -- no clip,
 * so the next block may run clamp-free) */
template <bool MR>
__device__ __forceinline__ bool icw_rrow_flush(const double (*qs)[ICW_MAX_NS_TAPS / 2][16][2], int r, int lr, int lane,
                                               int nf, const IcwRenderK &k, unsigned &clips, double &pk,
                                               unsigned char *o0, unsigned char *o1, int osz)
{
    __builtin_amdgcn_wave_barrier();
    bool calm = true;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lr + 16 * h;
        if (j < nf) {
            const double q = qs[r][j >> 1][lr][j & 1];
            clips += (q >= k.hi ? 1u : 0u) + (q <= k.lo ? 1u : 0u);
            pk = fmax(pk, fabs(q));
            calm &= fabs(q) < k.clip_abs;
        }
    }
    calm = __all(calm);
    const int sb = lane >> 5, f = lane & 31;
    unsigned char *o = sb ? o1 : o0;
    if (o && f < nf) {
        const int lo1 = k.lo1, hi1 = k.hi1;
        const int vl = icw_rrow_val<MR>(qs[2 * sb][f >> 1][0][f & 1], lo1, hi1);
        const int vr = icw_rrow_val<MR>(qs[2 * sb + 1][f >> 1][0][f & 1], lo1, hi1);
        const uint32_t l = (uint32_t)(vl << k.norm_shift);
        const uint32_t rr = (uint32_t)(vr << k.norm_shift);
        if (osz == 2) {
            *(uint32_t *)(o + (size_t)f * 4) = (l & 0xffffu) | (rr << 16);
        } else {
            uint16_t *p = (uint16_t *)(o + (size_t)f * 6);
            p[0] = (uint16_t)(l & 0xffffu);
            p[1] = (uint16_t)(((l >> 16) & 0xffu) | ((rr & 0xffu) << 8));
            p[2] = (uint16_t)((rr >> 8) & 0xffffu);
        }
    }
    __builtin_amdgcn_wave_barrier();
    return calm;
}

/* ------------------------------------------- render, row broadcast + companion wave (K3c) ------ */
/* The row render with everything that is not the error-feedback chain on a second wave of the
 * workgroup, which the dispatcher puts on another SIMD of the CU.  A lone wave issues one FP64 op per
 * ~5 cycles, so on one wave every staging load, LDS store, integer conversion, meter update
 * and output store is issue time taken from the chain: 18.9 VALU + 2.5 SALU + 1.8 LDS per sample for a
 * 16-op chain (MEW44).  Here
 *   wave 0 (chain)      runs only the chain of sound_render.c:754-809 on its four channels: per sample
 *                       the row-uniform chain, one ds_read_b128 per two samples for x and for the
 *                       dither value (the next block, staged), one ds_write_b128 per two samples for q;
 *                       per block one counter read and one counter write;
 *   wave 1 (companion)  stages block n (global loads issued four blocks ahead, x * norm_mul, the
 *                       clamp-free input test) into staging buffer n mod 4 and publishes `staged`;
 *                       flushes block n - 4 once the chain has published it `done` (the exact flush of
 *                       icw_rrow_flush: integers, clips, peak, packed frames) and publishes `flushed`.
 * The hand-offs are LDS counters.  The LDS executes one wave's DS instructions in order, so a counter
 * written after a block's data is seen only once the data is there; the compiler is kept from
 * moving memory accesses across a counter access by a fence of its own.  The chain checks, at each
 * block start, the counters it read at the previous one (the companion runs a block ahead), so the
 * check costs no wait; it spins (s_sleep) only if the companion fell behind.  Every spin is bounded:
 * a hand-off that never comes flags a.err and the wave goes on, so the grid drains.
 * The clamp-free decision needs the block before to have been calm (no |q| >= clip_abs, no NaN):
 * the chain itself keeps max |q| in an exact block (one v_max_f64 per sample, only there); a NaN q
 * makes the chain's error, and so prev_ns_err, NaN for good (the shaper's sum of a NaN), which the
 * block-end test also sees; a FIR shaper's NaN is never self-clearing, a flat one has no history.
 * Every block goes through the same exact flush (a clamp-free block gives the same integers through
 * it: no clip, no NaN). */
#define ICW_K3C_NSB 4                  /* staging buffers (blocks) */
#define ICW_K3C_NQB 4                  /* q buffers (blocks) */
#define ICW_K3C_SPIN (1u << 24)        /* spin bound: ~2^24 s_sleep(1), far beyond any healthy wait */

__device__ __forceinline__ void icw_cfence() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ unsigned long long icw_lds_ld64(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int icw_lds_ld32(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void icw_lds_st32(int *p, int v)
{
    icw_cfence();
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* chain side: the counters (staged word | flushed << 32) once staged >= ns and flushed >= nf.  The
 * staged word is (blocks staged) << 4 | the clamp-free input tests of the last four staged blocks (bit
 * n mod 4 for block n), so one 64-bit read per block brings the chain both counters and block j + 1's
 * test (inline, as every hand-off here: a call would make the callee wait for all memory traffic) */
__device__ __forceinline__ unsigned long long icw_k3c_wait(const unsigned long long *sf, int ns, int nf, int32_t *err)
{
    unsigned long long v = icw_lds_ld64(sf);
    for (unsigned spin = 0;; ++spin) {
        const int st = __builtin_amdgcn_readfirstlane((int)(uint32_t)v) >> 4;
        const int fl = __builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
        if (st >= ns && fl >= nf) break;
        if (spin >= ICW_K3C_SPIN) {
            if (err && threadIdx.x == 0) atomicOr(err, 1);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
        v = icw_lds_ld64(sf);
    }
    icw_cfence();
    return v;
}

/* companion side: wait until the chain has published at least n blocks done */
__device__ __forceinline__ void icw_k3c_wait_done(const int *dn, int n, int32_t *err)
{
    for (unsigned spin = 0; __builtin_amdgcn_readfirstlane(icw_lds_ld32(dn)) < n; ++spin) {
        if (spin >= ICW_K3C_SPIN) {
            if (err && threadIdx.x == 64) atomicOr(err, 1);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    icw_cfence();
}

/* The companion's staging (generator-major dither rows).  Loads are issued by every lane from a
 * clamped, always valid address (the frame index held to T - 1, a spare lane on its row's first frame)
 * and the values a lane has no business loading are zeroed only at the store, four blocks later: a load
 * under a branch, or a select right after it, made the compiler wait for all memory traffic
 * (vmcnt(0)) every block.  A dither pair starting at the block's last, even frame reads the row's
 * padding (dith_pitch is T rounded up to even). */
struct IcwCompLane {
    const double *xr, *dr;       /* the lane's x row and dither row (frame 0; a spare lane: row 0 of the batch) */
    int xi, di;                  /* frame offsets in a block: x frame, first frame of the dither pair */
    bool xv, dvv;
    uint32_t xo, dof;            /* LDS byte offsets in a staging buffer */
};

__device__ __forceinline__ IcwCompLane icw_k3c_lane(const IcwK3Args &a, int lane)
{
    constexpr int U = ICW_MAX_NS_TAPS;
    IcwCompLane L;
    const int sb = lane >> 5, i = lane & 31;
    const int s = blockIdx.x * 2 + sb;
    L.xi = i < U ? i : 0;
    L.xv = i < U && 2 * s < a.n_gen;
    L.xr = L.xv ? a.pre + (size_t)s * a.pre_stride : a.pre;
    L.xo = (uint32_t)(((2 * sb) * U + L.xi) * sizeof(double));
    const int ld = lane < 2 * U ? lane : 0;
    const int ch = ld / (U / 2), p = ld % (U / 2);
    L.di = 2 * p;
    L.dvv = a.dith && lane < 2 * U && (int)blockIdx.x * 4 + ch < a.n_gen;
    L.dr = L.dvv ? a.dith + (size_t)(blockIdx.x * 4 + ch) * a.dith_pitch : a.pre;
    L.dof = (uint32_t)((ch * U + 2 * p) * sizeof(double));
    return L;
}

__device__ __forceinline__ void icw_k3c_stage_load(const IcwK3Args &a, const IcwCompLane &L, int t0, IcwRowStage &st)
{
    const int T1 = a.T - 1;
    const int fx = t0 + L.xi < T1 ? t0 + L.xi : T1;
    const int fd = t0 + L.di < T1 ? t0 + L.di : (T1 & ~1);
    st.x = *(const double2 *)(L.xr + (size_t)fx * 2);
    st.d = *(const double2 *)(L.dr + fd);
}

/* block t0's values to staging buffer (xs, ds); returns, wave-uniform, the clamp-free input test.
 * Branch-free: the lanes without a slot store into dum (a scratch area of 64 x 32 bytes), so every
 * loaded register is consumed on every path (a skipped store left its pending load's register free for
 * reuse, and the write to it waited for all memory traffic). */
__device__ __forceinline__ bool icw_k3c_stage_store(double (*xs)[ICW_MAX_NS_TAPS], double (*ds)[ICW_MAX_NS_TAPS], double *dum,
                                                    int lane, const IcwCompLane &L, const IcwRowStage &st, int t0, int T,
                                                    double nm, double thr)
{
    constexpr int U = ICW_MAX_NS_TAPS;
    const bool xl = (lane & 31) < U, dl = lane < 2 * U;
    const bool v = L.xv && t0 + L.xi < T;
    const double a = (v ? st.x.x : 0.0) * nm, b = (v ? st.x.y : 0.0) * nm;
    double *px = xl ? (double *)((char *)&xs[0][0] + L.xo) : dum + lane * 4;
    px[0] = a;
    px[xl ? U : 1] = b;
    const bool ok = !xl || (fabs(a) <= thr && fabs(b) <= thr);
    const bool v0 = L.dvv && t0 + L.di < T, v1 = L.dvv && t0 + L.di + 1 < T;
    double *pd = dl ? (double *)((char *)&ds[0][0] + L.dof) : dum + lane * 4 + 2;
    *(double2 *)pd = make_double2(v0 ? st.d.x : 0.0, v1 ? st.d.y : 0.0);
    return __all(ok);
}

template <int KIND, int NN, bool MR>
__global__ __launch_bounds__(128) void icw_render_rowc(IcwK3Args a)
{
    constexpr int U = ICW_MAX_NS_TAPS, NSB = ICW_K3C_NSB, NQB = ICW_K3C_NQB;
    constexpr int R = KIND == 1 ? U : (KIND == 2 ? 4 : 1);
    constexpr int QSTR = 4 * (U / 2) * 16 * 2;          /* doubles per q buffer */
    static_assert(U % R == 0, "ring period must divide the unroll");
    static_assert(U % 2 == 0, "samples go in pairs");
    static_assert(NSB == 4 && NQB == 4, "the companion's schedule below assumes four buffers of each");
    __shared__ __attribute__((aligned(16))) double qsb[NQB][4][U / 2][16][2];
    __shared__ __attribute__((aligned(16))) double xsl[NSB][4][U];
    __shared__ __attribute__((aligned(16))) double dsl[NSB][4][U];
    __shared__ __attribute__((aligned(8))) int cnt[4];  /* staged word (icw_k3c_wait), flushed, done (blocks) */
    __shared__ __attribute__((aligned(16))) double dum[64 * 4];   /* the companion's slotless stores */
    const int T = a.T;
    if (T <= 0) return;
    const int nbk = (T + U - 1) / U, nfull = T / U;
    const IcwRenderK &k = a.rk;
    const int osz = k.is24 ? 3 : 2;
    if (threadIdx.x == 0) { cnt[0] = 0; cnt[1] = 0; cnt[2] = 0; cnt[3] = 0; }
    __syncthreads();
    const unsigned long long *sfp = (const unsigned long long *)&cnt[0];
    if (threadIdx.x < 64) {
        /* ------------------------------------------------------------------ the chain ------ */
        const int lane = threadIdx.x, r = lane >> 4, lr = lane & 15;
        const int g0 = blockIdx.x * 4 + r;
        const bool valid = g0 < a.n_gen;
        const int g = valid ? g0 : a.n_gen - 1;
        double *rs = a.rs + (size_t)g * ICW_RSTATE;
        double prev_err = rs[1];
        double E[R], O[R], P[R], P2[R];
        IcwRowNs c;
        c.one = 1.0;
        c.c0 = k.ns_c[0];
        c.cN = KIND == 2 ? k.ns_c[NN] : 0.0;
        if constexpr (KIND == 2) {
            c.pl = lr + 1 < NN ? k.ns_c[lr + 1] : 0.0;
            c.pl2 = lr + 1 < NN ? k.ns_c[lr + 1 + NN] : 0.0;
        } else {
            c.pl = lr + 1 < NN ? k.ns_c[lr + 1] : 0.0;
            c.pl2 = lr + 17 < NN ? k.ns_c[lr + 17] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            E[(R - 1 - i) % R] = rs[2 + i];
            O[(R - 1 - i) % R] = rs[2 + U + i];
        }
        if constexpr (KIND == 1) {
#pragma unroll
            for (int m = 0; m < R; ++m) {
                P[m] = icw_rmul(c.pl, E[m]);
                if constexpr (NN > 17) P2[m] = icw_rmul(c.pl2, E[m]);
            }
        } else if constexpr (KIND == 2) {
#pragma unroll
            for (int m = 0; m < R; ++m) P[m] = icw_rsub(icw_rmul(c.pl, E[m]), icw_rmul(c.pl2, O[(m + R - 1) % R]));
        }
        asm volatile("s_nop 1");                       /* VALU write -> DPP read of P / P2 */
        double *const qst = &qsb[0][r][0][lr][0];
        /* blocks 0 and 1 staged: block 0 into registers, block 1 is read during block 0 */
        unsigned long long sf = icw_k3c_wait(sfp, nbk < 2 ? nbk : 2, 0, a.err);
        double xin[U], dv[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            xin[j] = xsl[0][r][j];
            dv[j] = dsl[0][r][j];
        }
        bool okn = (__builtin_amdgcn_readfirstlane((int)(uint32_t)sf) & 1) != 0;   /* block j's clamp-free input test */
        bool calm = false;                             /* the block before j clipped nowhere (no NaN) */
        int j = 0;
        auto step = [&](auto fast) {
            constexpr bool FAST = decltype(fast)::value;
            /* the counters read one block ago: block j + 1 staged, block j - NQB flushed */
            const int ns = j + 2 < nbk ? j + 2 : nbk, nf = j + 1 - NQB;
            if ((__builtin_amdgcn_readfirstlane((int)(uint32_t)sf) >> 4) < ns ||
                __builtin_amdgcn_readfirstlane((int)(uint32_t)(sf >> 32)) < nf)
                sf = icw_k3c_wait(sfp, ns, nf, a.err);
            icw_cfence();
            /* for the next block's check, and block j + 1's input test: staged then covers blocks up to
             * at most j + 3 (the companion stages block n after the chain's block n - 4), j + 1 among its
             * last four */
            sf = icw_lds_ld64(sfp);
            const int nb = (j + 1) & (NSB - 1);
            double mq = 0.0;
            icw_rrow_block<KIND, NN, R, 0, MR, FAST>(xin, dv, prev_err, E, O, P, P2, c, k, qst + (j & (NQB - 1)) * QSTR,
                                                     &xsl[nb][r][0], &dsl[nb][r][0], mq);
            if constexpr (!FAST) calm = __all(mq < k.clip_abs && prev_err == prev_err);
            icw_lds_st32(&cnt[2], j + 1);
            __builtin_amdgcn_sched_barrier(0);         /* the read of sf stays a block ahead of this use */
            okn = ((__builtin_amdgcn_readfirstlane((int)(uint32_t)sf) >> nb) & 1) != 0;
            ++j;
        };
        while (j < nfull) {
            while (j < nfull && !(KIND != 2 && calm && okn)) step(icw_ic<0>());
            if constexpr (KIND != 2) {
                while (j < nfull && okn) step(icw_ic<1>());
            }
        }
        const int rem = T - nfull * U;
        if (rem > 0) {
            const int nf = j + 1 - NQB;
            if (__builtin_amdgcn_readfirstlane((int)(uint32_t)(sf >> 32)) < nf) sf = icw_k3c_wait(sfp, nbk, nf, a.err);
            icw_cfence();
            double mq = 0.0;
            icw_rrow_block_lim<KIND, NN, R, 0, MR>(xin, dv, prev_err, E, O, P, P2, c, k, qst + (j & (NQB - 1)) * QSTR,
                                                   rem, mq);
            icw_lds_st32(&cnt[2], j + 1);
#pragma unroll
            for (int q = 1; q < U; ++q)
                if (q <= rem) { icw_ring_rotate1<R>(E); icw_ring_rotate1<R>(O); }
        }
        if (!valid || lr != 0) return;
        rs[1] = prev_err;
#pragma unroll
        for (int i = 0; i < R; ++i) { rs[2 + i] = E[(R - 1 - i) % R]; rs[2 + U + i] = O[(R - 1 - i) % R]; }
    } else {
        /* -------------------------------------------------------------- the companion ------ */
        const int lane = threadIdx.x - 64, r = lane >> 4, lr = lane & 15;
        const bool valid = (int)blockIdx.x * 4 + r < a.n_gen;
        const IcwCompLane sl = icw_k3c_lane(a, lane);
        const double nm = k.norm_mul, thr = k.spec_thr;
        const int sA = blockIdx.x * 2, sB = sA + 1;
        unsigned char *oA = 2 * sA < a.n_gen ? a.out + (size_t)sA * a.out_stride : nullptr;
        unsigned char *oB = 2 * sB < a.n_gen ? a.out + (size_t)sB * a.out_stride : nullptr;
        unsigned clips = 0;
        double pk = 0.0;
        IcwRowStage rg[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) icw_k3c_stage_load(a, sl, i * U, rg[i]);
        unsigned okm = 0;                              /* clamp-free input tests of the last four staged blocks */
        /* iteration n: flush block n - 4 (the chain has moved on to n - 3), then stage block n into
         * buffer n mod 4 (its last reader, block n - 5, is done) and send its registers for block n + 4 */
        auto iter = [&](int n, IcwRowStage &st) {
            if (n >= 4 && n - 4 < nbk) {
                const int jf = n - 4;
                icw_k3c_wait_done(&cnt[2], jf + 1, a.err);
                const int t = jf * U, nf = T - t < U ? T - t : U;
                (void)icw_rrow_flush<MR>(qsb[jf & (NQB - 1)], r, lr, lane, nf, k, clips, pk,
                                         oA ? oA + (size_t)t * 2 * osz : nullptr, oB ? oB + (size_t)t * 2 * osz : nullptr, osz);
                icw_lds_st32(&cnt[1], jf + 1);
            }
            /* unconditional, past the last block too (zeros into a buffer nobody reads any more, a
             * staged count past nbk): with the loads under a branch, the compiler's wait for a register
             * set assumed the path without the later loads and waited for everything */
            const int b = n & (NSB - 1);
            const bool ok = icw_k3c_stage_store(xsl[b], dsl[b], dum, lane, sl, st, n * U, T, nm, thr);
            okm = (okm & ~(1u << b)) | ((ok ? 1u : 0u) << b);
            icw_lds_st32(&cnt[0], (int)(((unsigned)(n + 1) << 4) | okm));
            icw_k3c_stage_load(a, sl, (n + 4) * U, st);
        };
        for (int n0 = 0; n0 < nbk + 4; n0 += 4) {
            iter(n0, rg[0]);
            iter(n0 + 1, rg[1]);
            iter(n0 + 2, rg[2]);
            iter(n0 + 3, rg[3]);
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            clips += __shfl_xor(clips, off);
            pk = fmax(pk, __shfl_xor(pk, off));
        }
        if (!valid || lr != 0) return;
        const int g = blockIdx.x * 4 + r;
        if (clips) atomicAdd(&a.clips[g], clips);
        if (pk > 0.0) atomicMax(&a.peak_bits[g], (unsigned long long)__double_as_longlong(pk));
    }
}

/* Render with FP_CHECK (K3f): sound_render_value's WITH FC CHECKS arithmetic (sound_render.c:
 * 857-903) and ns_fir / ns_iir's (428-433, 474-486), counting into the render census.  One lane per
 * channel like K3b, but compact (run-time loops, the reference's own decrementing ring in private
 * memory): a diagnostic mode.  The dither term comes from K3a; its FC() are identities (the sums of
 * dsopen values are multiples of 2^-56 below 12 in magnitude, never special). */
__global__ __launch_bounds__(64) void icw_render_fc(IcwK3Args a)
{
    constexpr int NM = ICW_MAX_NS_TAPS;
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= a.n_gen) return;
    const int s = g >> 1, ch = g & 1;
    const IcwRenderK &k = a.rk;
    const int n = k.ns_n;
    double *rs = a.rs + (size_t)g * ICW_RSTATE;
    double prev_err = rs[1];
    /* rs keeps the history by age (0 = newest); the reference ring: ebuf[(pos + age) mod n] */
    double E[NM], O[NM];
    int pos = 0;                                         /* E age j at slot (pos + j) mod n, O age j at (pos - 1 + j) */
#pragma unroll 1
    for (int i = 0; i < NM; ++i) E[i] = O[i] = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) { E[i] = rs[2 + i]; O[(i - 1 + n) % n] = rs[2 + NM + i]; }
    const double *pp = a.pre + (size_t)s * a.pre_stride + ch;
    const double *dp = a.dith ? a.dith + g : nullptr;
    unsigned char *op = a.out + (size_t)s * a.out_stride;
    const int osz = k.is24 ? 3 : 2;
    unsigned clips = 0;
    double pk = 0.0;
    IcwFes fe = {};
#pragma unroll 1
    for (int t = 0; t < a.T; ++t) {
        const double d = dp ? dp[(size_t)t * a.dith_pitch] : 0.0;
        const double input = icw_fc(icw_fc(pp[(size_t)t * 2] * k.norm_mul, fe) - prev_err, fe);
        int delta;
        double q = icw_fc(input + icw_fc(d, fe), fe);
        q = icw_fc(icw_round_q(q, k.round_offset, k.sign_delta, delta), fe);
        pk = fmax(pk, fabs(q));
        const int vc = icw_clamp_int(q, k, clips);
        const int val = (isnan(q) ? (int)0x80000000 : vc) + delta;
        const double ev = icw_fc((double)val - input, fe);
        double res = 0.0;
        if (k.ns_kind != 0) {
            pos = pos ? pos - 1 : n - 1;                 /* ns_ix_pos decrement (sound_render.c:410-413) */
            /* ages shift by one: the ring slot of age j is (pos + j) mod n */
            E[pos] = icw_fc(ev, fe);
            int ib = pos;
#pragma unroll 1
            for (int ic = 0; ic < n; ++ic) {
                if (k.ns_kind == 1) res = icw_fc(res + icw_fc(k.ns_c[ic] * E[ib], fe), fe);
                else res = icw_fc(res + icw_fc(icw_fc(k.ns_c[ic] * E[ib], fe) - icw_fc(k.ns_c[ic + n] * O[ib], fe), fe), fe);
                if (++ib >= n) ib = 0;
            }
            if (k.ns_kind == 2) O[(pos ? pos : n) - 1] = res;
        }
        prev_err = res;
        const int v = val << k.norm_shift;
        unsigned char *o = op + ((size_t)t * 2 + ch) * osz;
        o[0] = (unsigned char)v;
        o[1] = (unsigned char)(v >> 8);
        if (osz == 3) o[2] = (unsigned char)(v >> 16);
    }
    rs[1] = prev_err;
    /* back to the by-age layout: age j at slot (pos + j) mod n (E) and (pos - 1 + j) mod n (O: the
     * newest output sits one slot behind the newest error) */
    if (k.ns_kind != 0) {
        double e2[NM], o2[NM];
#pragma unroll 1
        for (int j = 0; j < n; ++j) { e2[j] = E[(pos + j) % n]; o2[j] = O[(pos - 1 + n + j) % n]; }
#pragma unroll 1
        for (int j = 0; j < n; ++j) { rs[2 + j] = e2[j]; rs[2 + NM + j] = o2[j]; }
    }
    if (clips) atomicAdd(&a.clips[g], clips);
    if (pk > 0.0) atomicMax(&a.peak_bits[g], (unsigned long long)__double_as_longlong(pk));
    icw_fes_flush(fe, a.fes + ((size_t)s * 4 + 2 + ch) * ICW_FES_PITCH);
}

/* ------------------------------------------------------ mixed render kernel (KR) -------- */
/* A call over streams with different renders (icw_set_stream_render): K2 ran with do_render 0 and left
 * every stream's pre-render doubles in the `pre` rows; the serial entries' streams go through K3b / K3c
 * run by run, and this kernel renders every stream whose entry is elementwise -- ROUND, or a dithered
 * render with the flat shaper from K3a's rows -- frame-parallel, a frame per thread, ICW_KR_TPW tiles of
 * 256 frames per workgroup.  One stream per workgroup row, so the entry is wave-uniform: it is read once
 * through the constant address space (scalar loads), and a workgroup of a serial entry's stream returns
 * at once.  The arithmetic is icw_render_round (icw_quant_dev.h), the steps K2's in-kernel render runs,
 * on the doubles K2 stored: the same bits.  Frames are packed at the stream's own size; a 6-byte row
 * beside 4-byte rows leaves rows that are not dword aligned, so 24-bit frames go out as bytes (K2's
 * icw_frame_store) and a 16-bit frame as one dword only where the row is aligned.  Meters: a wave
 * reduction, LDS, then one atomic per channel and workgroup, with K2's conditions. */
#define ICW_KR_TILE 256
#define ICW_KR_TPW  4
__global__ __launch_bounds__(ICW_KR_TILE) void icw_render_mixed(IcwKRArgs a)
{
    typedef const __attribute__((address_space(4))) IcwRenderEnt *EntP;
    typedef const __attribute__((address_space(4))) int32_t *IdxP;
    __shared__ unsigned red_clip[2][ICW_KR_TILE / 64];
    __shared__ double red_pk[2][ICW_KR_TILE / 64];
    const int tl = threadIdx.x, s = blockIdx.y;
    const EntP e = (EntP)a.tab + ((IdxP)a.ent)[s];
    if (e->serial) return;                            /* workgroup-uniform, before any barrier */
    IcwRenderK k;
    k.norm_mul = e->rk.norm_mul;
    k.hi = e->rk.hi;
    k.lo = e->rk.lo;
    k.round_offset = e->rk.round_offset;
    k.sign_delta = e->rk.sign_delta;
    k.norm_shift = e->rk.norm_shift;
    const bool is24 = e->rk.is24 != 0;
    const bool dith = e->dither != 0 && a.dith != nullptr;
    const int fsz = is24 ? 6 : 4;
    const int T = a.T;
    const double *pre = a.pre + (size_t)s * a.pre_stride;
    const double *dl = dith ? a.dith + (size_t)(2 * s) * a.dith_pitch : nullptr;
    unsigned char *o = a.out + (size_t)s * a.out_stride + (size_t)a.t0 * fsz;
    const bool pre16 = ((uintptr_t)pre & 15u) == 0u, out4 = ((uintptr_t)o & 3u) == 0u;
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    const int tw0 = blockIdx.x * ICW_KR_TILE * ICW_KR_TPW;
#pragma unroll
    for (int i = 0; i < ICW_KR_TPW; ++i) {
        const int t = tw0 + i * ICW_KR_TILE + tl;
        if (t >= T) break;
        double xl, xr;
        if (pre16) {
            const double2 p = *(const double2 *)(pre + (size_t)t * 2);
            xl = p.x; xr = p.y;
        } else {
            xl = pre[(size_t)t * 2]; xr = pre[(size_t)t * 2 + 1];
        }
        int vl, vr;
        if (dith) {
            const double d0 = dl[t], d1 = dl[a.dith_pitch + t];
            vl = icw_render_round<true>(xl, k, clip_l, pk_l, d0);
            vr = icw_render_round<true>(xr, k, clip_r, pk_r, d1);
        } else {
            vl = icw_render_round(xl, k, clip_l, pk_l);
            vr = icw_render_round(xr, k, clip_r, pk_r);
        }
        if (is24) {
            unsigned char *q = o + (size_t)t * 6;
            q[0] = (unsigned char)vl; q[1] = (unsigned char)(vl >> 8); q[2] = (unsigned char)(vl >> 16);
            q[3] = (unsigned char)vr; q[4] = (unsigned char)(vr >> 8); q[5] = (unsigned char)(vr >> 16);
        } else if (out4) {
            *(unsigned *)(o + (size_t)t * 4) = ((unsigned)vl & 0xffffu) | ((unsigned)vr << 16);
        } else {
            unsigned char *q = o + (size_t)t * 4;
            q[0] = (unsigned char)vl; q[1] = (unsigned char)(vl >> 8);
            q[2] = (unsigned char)vr; q[3] = (unsigned char)(vr >> 8);
        }
    }
    /* the peaks are maxima of |q| from +0.0, never a NaN: any order gives the same value */
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        clip_l += __shfl_xor(clip_l, m);
        clip_r += __shfl_xor(clip_r, m);
        pk_l = fmax(pk_l, __shfl_xor(pk_l, m));
        pk_r = fmax(pk_r, __shfl_xor(pk_r, m));
    }
    if ((tl & 63) == 0) {
        red_clip[0][tl >> 6] = clip_l; red_clip[1][tl >> 6] = clip_r;
        red_pk[0][tl >> 6] = pk_l; red_pk[1][tl >> 6] = pk_r;
    }
    __syncthreads();
    if (tl < 2) {
        unsigned cs = 0; double pm = 0.0;
        for (int i = 0; i < ICW_KR_TILE / 64; ++i) { cs += red_clip[tl][i]; pm = fmax(pm, red_pk[tl][i]); }
        if (cs) atomicAdd(&a.clips[s * 2 + tl], cs);
        if (pm > 0.0) atomicMax(&a.peak_bits[s * 2 + tl], (unsigned long long)__double_as_longlong(pm));
    }
}

/* ---------------------------------------------------------------- launch wrappers ------- */
extern "C" hipError_t icw_launch_render_mixed(const IcwKRArgs *a, hipStream_t st)
{
    if (a->T <= 0 || a->n_streams <= 0) return hipSuccess;
    if (!a->tab || !a->ent || !a->pre || !a->out) return hipErrorInvalidValue;
    const int per = ICW_KR_TILE * ICW_KR_TPW;
    hipLaunchKernelGGL(icw_render_mixed, dim3((unsigned)((a->T + per - 1) / per), (unsigned)a->n_streams), dim3(ICW_KR_TILE),
                       0, st, *a);
    return hipGetLastError();
}

template <int RT>
static hipError_t icw_launch_dither_t(const IcwK3Args *a, hipStream_t st)
{
    if (!a->wbuf) return hipErrorInvalidValue;
    constexpr int W = icw_dith_words(RT);
    const int chunk = icw_dith_chunk_frames(a->T, a->wcap, W);
    if (chunk <= 0) return hipErrorInvalidValue;
    for (int t0 = 0; t0 < a->T; t0 += chunk) {
        IcwK3Args c = *a;
        c.T = std::min(chunk, a->T - t0);
        c.dith = a->dith + (a->dith_gm ? (size_t)t0 : (size_t)t0 * a->dith_pitch);
        hipLaunchKernelGGL(icw_dith_twist, dim3(c.n_gen), dim3(64), 0, st, c, W);
        const long long tot = (long long)c.n_gen * c.T;
        hipLaunchKernelGGL(icw_dith_samples<RT>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, c);
        hipLaunchKernelGGL(icw_dith_fix<RT>, dim3(c.n_gen), dim3(64), 0, st, c);
    }
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_dither(const IcwK3Args *a, hipStream_t st)
{
    if (a->T <= 0) return hipSuccess;
    switch (a->rk.render_type) {
    case ICW_RENDER_RPDF: return icw_launch_dither_t<ICW_RENDER_RPDF>(a, st);
    case ICW_RENDER_TPDF: return icw_launch_dither_t<ICW_RENDER_TPDF>(a, st);
    case ICW_RENDER_STPDF: return icw_launch_dither_t<ICW_RENDER_STPDF>(a, st);
    case ICW_RENDER_GAUSS: return icw_launch_dither_t<ICW_RENDER_GAUSS>(a, st);
    default: return hipErrorInvalidValue;
    }
}

template <int KIND, int NN, bool MR>
static void icw_launch_rr(const IcwK3Args *a, int rb, hipStream_t st)
{
    /* K3c: a companion wave beside the chain, 128 threads */
    hipLaunchKernelGGL((icw_render_rowc<KIND, NN, MR>), dim3(rb), dim3(128), 0, st, *a);
}

template <bool MR>
static hipError_t icw_launch_render_row(const IcwK3Args *a, int rb, int nn, hipStream_t st)
{
    if (a->dith && !a->dith_gm) return hipErrorInvalidValue;   /* K3c stages generator-major rows */
    if (a->rk.ns_kind == 0) {
        icw_launch_rr<0, 0, MR>(a, rb, st);
    } else if (a->rk.ns_kind == 1) {
        switch (nn) {
        case 5: icw_launch_rr<1, 5, MR>(a, rb, st); break;
        case 9: icw_launch_rr<1, 9, MR>(a, rb, st); break;
        case 15: icw_launch_rr<1, 15, MR>(a, rb, st); break;
        case 16: icw_launch_rr<1, 16, MR>(a, rb, st); break;
        case 20: icw_launch_rr<1, 20, MR>(a, rb, st); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        if (nn != 4) return hipErrorInvalidValue;
        icw_launch_rr<2, 4, MR>(a, rb, st);
    }
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_render(const IcwK3Args *a, hipStream_t st)
{
    const int blocks = (a->n_gen + 63) / 64;
    if (a->fes) {
        hipLaunchKernelGGL(icw_render_fc, dim3(blocks), dim3(64), 0, st, *a);
        return hipGetLastError();
    }
    /* the tap counts of the canned shapers (sound_render.c:75-235): FIR 5, 9, 15, 16, 20; IIR 4 */
    const int nn = a->rk.ns_n;
    if (a->row) {
        const int rb = (a->n_gen + 3) / 4;          /* four channels (two streams) per wave */
        /* the quantiser as a template flag: mid-riser (sign_delta -1, round_offset 0) or mid-tread
         * (sign_delta 0, round_offset 0.5) -- render_consts gives no other pair */
        if (a->rk.sign_delta != 0 ? a->rk.round_offset != 0.0 : a->rk.round_offset != 0.5) return hipErrorInvalidValue;
        return a->rk.sign_delta ? icw_launch_render_row<true>(a, rb, nn, st) : icw_launch_render_row<false>(a, rb, nn, st);
    }
    if (a->rk.ns_kind == 0) {
        hipLaunchKernelGGL((icw_render_serial<0, 1, 0>), dim3(blocks), dim3(64), 0, st, *a);
    } else if (a->rk.ns_kind == 1) {
        switch (nn) {
        case 5: hipLaunchKernelGGL((icw_render_serial<1, ICW_MAX_NS_TAPS, 5>), dim3(blocks), dim3(64), 0, st, *a); break;
        case 9: hipLaunchKernelGGL((icw_render_serial<1, ICW_MAX_NS_TAPS, 9>), dim3(blocks), dim3(64), 0, st, *a); break;
        case 15: hipLaunchKernelGGL((icw_render_serial<1, ICW_MAX_NS_TAPS, 15>), dim3(blocks), dim3(64), 0, st, *a); break;
        case 16: hipLaunchKernelGGL((icw_render_serial<1, ICW_MAX_NS_TAPS, 16>), dim3(blocks), dim3(64), 0, st, *a); break;
        case 20: hipLaunchKernelGGL((icw_render_serial<1, ICW_MAX_NS_TAPS, 20>), dim3(blocks), dim3(64), 0, st, *a); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        if (nn != 4) return hipErrorInvalidValue;
        hipLaunchKernelGGL((icw_render_serial<2, 4, 4>), dim3(blocks), dim3(64), 0, st, *a);
    }
    return hipGetLastError();
}

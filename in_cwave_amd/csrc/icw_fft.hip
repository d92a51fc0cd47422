/*
 * icw_fft.hip -- gfx950 (CDNA4) kernel of the direct-FFT CWAVE encoder (include/icw_cwave.h:
 * icw_encode_cwave_fft, KX): the Hilbert transform of a whole track through a power-of-two FP64 FFT.
 *
 * Built like icw_kernels.hip (`-ffp-contract=off`, no fast-math).
 *
 * The transform.  P = 2^logP points per track, c[n] = x_L[n] + j x_R[n] (mono: a zero imaginary part), in
 * place in a workspace of P complex doubles.  It is the radix-2 decimation-in-frequency transform, whose
 * output is in bit-reversed order, cut into passes of l_0 + l_1 + .. = logP stages in its four-step form:
 * pass i works on blocks of M = 2^(l + logR) points (logR = the stages still to come), runs the 2^l-point
 * sub-transforms over the points n1 * 2^logR + n2 of a block, and multiplies the result k1 of column n2 by
 * the twiddle W_M^(n2 k1); the last pass (logR 0) has none.  The inverse is the mirror image: conjugate
 * twiddles, then the decimation-in-time sub-transforms from bit-reversed to natural order, without the
 * factors 1/2 (1/P is folded into the multiplier).  Nothing is ever transposed or reordered in memory: the
 * spectrum only exists in bit-reversed order, where the multiplier m is a function of the position p alone:
 * frequency 0 is p = 0 and P/2 is p = 1, a frequency below P/2 has an even p and one above it an odd p.
 *
 * One kernel, three kinds of pass (IcwFftArgs.kind):
 *   FWD  load, sub-transforms, twiddles, store;
 *   MID  load, the last forward sub-transforms, m / P, the first inverse sub-transforms, store: the spectrum
 *        never reaches memory;
 *   INV  load, conjugate twiddles, inverse sub-transforms, store.
 * The first pass of a track loads the PCM (icw_unpack, zero beyond the track's frames) instead of the
 * workspace; the last one reads I from the PCM again, takes Q from the transform and writes the file's
 * frames (icw_cwpack_dev.h), counting the clipped int16 samples.  A track of at most 2^ICW_FFT_PASS_LOG2
 * frames is one MID pass and touches no workspace.
 *
 * A workgroup of 256 lanes holds a tile of 2^l rows (the sub-transform's points) by 2^logC columns (adjacent
 * n2, or adjacent blocks where a block has fewer columns) as two planes of doubles with a row pitch of
 * 2^logC + 1.  Where 2^logR >= 2^logC a row of the tile is 2^logC adjacent points in memory, else the whole
 * tile is one contiguous run; either way consecutive lanes touch consecutive points.  A lane does up to
 * three stages on 8 points in registers between two LDS round trips.
 *
 * Twiddles.  Every twiddle is exp(-2 pi j t / M) for integers t < M = 2^k.  t / M is exact; it is reduced
 * to an octant exactly, the octant's angle pi/4 * r is formed as a double-double (one fma), and glibc's
 * do_sin / do_cos (icw_libm.h, under 0.55 ulp on x + dx) give the pair: none is a product of two others.
 * The sub-transforms' 2^(l-1) twiddles are computed once per workgroup into LDS.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/icw.h"
#include "icw_device.h"
#include "icw_fft.h"
#include "icw_launch.h"

#pragma clang fp contract(off)

#include "icw_unpack_dev.h"
#include "icw_libm.h"
#include "icw_cwpack_dev.h"

#define ICW_FFT_PIO4_HI 0x1.921fb54442d18p-1    /* pi/4 as a double-double */
#define ICW_FFT_PIO4_LO 0x1.1a62633145c07p-55

/* exp(-2 pi j t / 2^logM), 0 <= t < 2^logM <= 2^27 */
__device__ __forceinline__ void icw_fft_twiddle(uint32_t t, int logM, double &wr, double &wi)
{
    const double e = (double)t * __longlong_as_double((long long)(1023 + 3 - logM) << 52);   /* 8 t / M, exact */
    const int oct = (int)e;
    double r = e - (double)oct;                          /* exact, [0, 1) */
    if (oct & 1) r = 1.0 - r;                            /* exact: r has at most 27 bits */
    double c = 1.0, s = 0.0;
    if (r != 0.0) {
        const double hi = r * ICW_FFT_PIO4_HI;
        const double lo = __builtin_fma(r, ICW_FFT_PIO4_HI, -hi) + r * ICW_FFT_PIO4_LO;
        s = icw_lm_dosin(hi, lo);
        c = icw_lm_docos(hi, lo);
    }
    /* the angle is pi/4 (oct + r0): oct even x = pi/4 r0 above oct pi/4, oct odd x below (oct + 1) pi/4 */
    double cr, sr;
    switch (oct & 7) {
    case 0: cr = c; sr = s; break;
    case 1: cr = s; sr = c; break;
    case 2: cr = -s; sr = c; break;
    case 3: cr = -c; sr = s; break;
    case 4: cr = -c; sr = -s; break;
    case 5: cr = -s; sr = -c; break;
    case 6: cr = s; sr = -c; break;
    default: cr = c; sr = -s; break;
    }
    wr = cr;
    wi = -sr;
}

/* G stages (spans 2^(G + qlog) .. 2^(1 + qlog) rows) of the tile's sub-transforms on 2^G points per lane;
 * INV: the same stages backwards with conjugate twiddles, un-normalised */
template <int G, bool INV>
__device__ __forceinline__ void icw_fft_step(double *re, double *im, const double2 *tw, int l, int qlog, int logC, int tid)
{
    constexpr int N = 1 << G;
    const int PC = (1 << logC) + 1;
    const int nb = 1 << (l - G + logC);
    const int step = PC << qlog;
    for (int b = tid; b < nb; b += 256) {
        const int c = b & ((1 << logC) - 1), idx = b >> logC;
        const int r0 = idx & ((1 << qlog) - 1), hi = idx >> qlog;
        const int base = (((hi << G) << qlog) + r0) * PC + c;
        double vr[N], vi[N];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            vr[u] = re[base + u * step];
            vi[u] = im[base + u * step];
        }
#pragma unroll
        for (int s0 = 0; s0 < G; ++s0) {
            const int s = INV ? G - 1 - s0 : s0;
            const int half = 1 << (G - 1 - s);
            const int sh = l - 1 - (G - 1 - s) - qlog;   /* W_(2 half q)^e = W_S^(e << sh) */
#pragma unroll
            for (int u = 0; u < N; ++u) {
                if (u & half) continue;
                const double2 w = tw[(r0 + ((u & (half - 1)) << qlog)) << sh];
                if (!INV) {
                    const double ar = vr[u], ai = vi[u], br = vr[u + half], bi = vi[u + half];
                    const double dr = ar - br, di = ai - bi;
                    vr[u] = ar + br;
                    vi[u] = ai + bi;
                    vr[u + half] = dr * w.x - di * w.y;
                    vi[u + half] = dr * w.y + di * w.x;
                } else {
                    const double br = vr[u + half], bi = vi[u + half];
                    const double tr = br * w.x + bi * w.y, ti = bi * w.x - br * w.y;   /* b conj(w) */
                    const double ar = vr[u], ai = vi[u];
                    vr[u] = ar + tr;
                    vi[u] = ai + ti;
                    vr[u + half] = ar - tr;
                    vi[u + half] = ai - ti;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
            re[base + u * step] = vr[u];
            im[base + u * step] = vi[u];
        }
    }
}

template <bool INV>
__device__ __forceinline__ void icw_fft_group(int g, double *re, double *im, const double2 *tw, int l, int qlog, int logC, int tid)
{
    if (g == 3) icw_fft_step<3, INV>(re, im, tw, l, qlog, logC, tid);
    else if (g == 2) icw_fft_step<2, INV>(re, im, tw, l, qlog, logC, tid);
    else icw_fft_step<1, INV>(re, im, tw, l, qlog, logC, tid);
    __syncthreads();
}

/* the tile's sub-transforms: the stages in groups of three from the widest span down (forward), or the
 * same groups from the narrowest up (inverse) */
__device__ __forceinline__ void icw_fft_forward(double *re, double *im, const double2 *tw, int l, int logC, int tid)
{
    for (int rem = l; rem > 0;) {
        const int g = rem < 3 ? rem : 3;
        rem -= g;
        icw_fft_group<false>(g, re, im, tw, l, rem, logC, tid);
    }
}

__device__ __forceinline__ void icw_fft_inverse(double *re, double *im, const double2 *tw, int l, int logC, int tid)
{
    const int g0 = l % 3;                                /* the forward order's last, short group */
    int q = 0;
    if (g0) {
        icw_fft_group<true>(g0, re, im, tw, l, 0, logC, tid);
        q = g0;
    }
    for (; q < l; q += 3) icw_fft_group<true>(3, re, im, tw, l, q, logC, tid);
}

/* the tile's element e: its row, its column and its place in the track's transform */
struct IcwFftMap {
    int l, logR, logC;
    uint32_t tile;
    bool contig;
    __device__ __forceinline__ void operator()(int e, int &r, int &c, uint32_t &pos) const
    {
        if (contig) {                                    /* columns of several whole blocks: one run of memory */
            r = (e >> logR) & ((1 << l) - 1);
            c = ((e >> (logR + l)) << logR) | (e & ((1 << logR) - 1));
            pos = (tile << (l + logC)) + (uint32_t)e;
        } else {
            c = e & ((1 << logC) - 1);
            r = e >> logC;
            const uint32_t g = (tile << logC) + (uint32_t)c;
            pos = ((((g >> logR) << l) + (uint32_t)r) << logR) + (g & ((1u << logR) - 1u));
        }
    }
};

/* the last pass's store: frame pos < n of the track gets I from the PCM and Q from the tile */
template <int CWF, int NC>
__device__ __forceinline__ unsigned icw_fft_pack(const IcwFftArgs &a, const IcwFftTrack &tr, const IcwFftMap &map,
                                                 const double *re, const double *im, int npts, int PC, int tid)
{
    constexpr int FB = NC * icw_cw_bytes<CWF>::value;
    const uint32_t csz = a.fmt == ICW_FMT_U8 ? 1u : a.fmt == ICW_FMT_I16 ? 2u : a.fmt == ICW_FMT_I24 ? 3u : 4u;
    const size_t fsz = (size_t)csz * a.channels;
    unsigned clip = 0u;
    for (int e = tid; e < npts; e += 256) {
        int r, c;
        uint32_t pos;
        map(e, r, c, pos);
        if (pos >= tr.n) continue;
        const unsigned char *p = a.in + tr.in_off + (size_t)pos * fsz;
        double vi[NC], vq[NC];
        vi[0] = icw_unpack(p, a.fmt);
        vq[0] = re[r * PC + c];
        if constexpr (NC == 2) {
            vi[1] = icw_unpack(p + csz, a.fmt);
            vq[1] = im[r * PC + c];
        }
        icw_cw_frame_put<CWF, NC>(a.out + tr.out_off + (size_t)pos * FB, vi, vq, clip);
    }
    return clip;
}

__global__ __launch_bounds__(256) void icw_fft_pass(IcwFftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned nclip;
    const int l = a.l, logC = a.logC, logR = a.logR;
    const int S = 1 << l, PC = (1 << logC) + 1, npts = 1 << (l + logC);
    const int tid = threadIdx.x;
    double *re = lds, *im = lds + S * PC;
    double2 *tw = (double2 *)(lds + 2 * S * PC + ((2 * S * PC) & 1));   /* 16-byte aligned */
    const IcwFftTrack tr = a.tracks[blockIdx.y];
    double2 *ws = (double2 *)a.ws + tr.ws_off;
    const IcwFftMap map = {l, logR, logC, blockIdx.x, logR < logC};
    const uint32_t csz = a.fmt == ICW_FMT_U8 ? 1u : a.fmt == ICW_FMT_I16 ? 2u : a.fmt == ICW_FMT_I24 ? 3u : 4u;
    const size_t fsz = (size_t)csz * a.channels;

    if (tid == 0) nclip = 0u;
    for (int j = tid; j < (S >> 1); j += 256) {
        double wr, wi;
        icw_fft_twiddle((uint32_t)j, l, wr, wi);
        tw[j] = make_double2(wr, wi);
    }
    for (int e = tid; e < npts; e += 256) {
        int r, c;
        uint32_t pos;
        map(e, r, c, pos);
        double xr = 0.0, xi = 0.0;
        if (a.first) {
            if (pos < tr.n) {
                const unsigned char *p = a.in + tr.in_off + (size_t)pos * fsz;
                xr = icw_unpack(p, a.fmt);
                if (a.channels > 1) xi = icw_unpack(p + csz, a.fmt);
            }
        } else {
            const double2 v = ws[pos];
            xr = v.x;
            xi = v.y;
            if (a.kind == ICW_FFT_INV) {
                const uint32_t n2 = pos & ((1u << logR) - 1u), k1 = __brev((unsigned)r) >> (32 - l);
                if (n2 && k1) {
                    double wr, wi;
                    icw_fft_twiddle(n2 * k1, l + logR, wr, wi);
                    const double yr = xr * wr + xi * wi, yi = xi * wr - xr * wi;   /* v conj(w) */
                    xr = yr;
                    xi = yi;
                }
            }
        }
        re[r * PC + c] = xr;
        im[r * PC + c] = xi;
    }
    __syncthreads();

    if (a.kind != ICW_FFT_INV) icw_fft_forward(re, im, tw, l, logC, tid);
    if (a.kind == ICW_FFT_MID) {
        /* m / P at position pos of the bit-reversed spectrum: 0 at 0 (frequency 0) and 1 (P/2), -j at the
         * other even positions (below P/2), +j at the odd ones */
        const double sc = __longlong_as_double((long long)(1023 - a.logP) << 52);
        for (int e = tid; e < npts; e += 256) {
            int r, c;
            uint32_t pos;
            map(e, r, c, pos);
            const double xr = re[r * PC + c], xi = im[r * PC + c];
            double yr = 0.0, yi = 0.0;
            if (pos >= 2u) {
                if (pos & 1u) { yr = -(xi * sc); yi = xr * sc; }
                else { yr = xi * sc; yi = -(xr * sc); }
            }
            re[r * PC + c] = yr;
            im[r * PC + c] = yi;
        }
        __syncthreads();
    }
    if (a.kind != ICW_FFT_FWD) icw_fft_inverse(re, im, tw, l, logC, tid);

    if (!a.last) {
        for (int e = tid; e < npts; e += 256) {
            int r, c;
            uint32_t pos;
            map(e, r, c, pos);
            double xr = re[r * PC + c], xi = im[r * PC + c];
            if (a.kind == ICW_FFT_FWD) {
                const uint32_t n2 = pos & ((1u << logR) - 1u), k1 = __brev((unsigned)r) >> (32 - l);
                if (n2 && k1) {
                    double wr, wi;
                    icw_fft_twiddle(n2 * k1, l + logR, wr, wi);
                    const double yr = xr * wr - xi * wi, yi = xr * wi + xi * wr;
                    xr = yr;
                    xi = yi;
                }
            }
            ws[pos] = make_double2(xr, xi);
        }
        return;
    }
    unsigned clip = 0u;
    const bool st2 = a.channels > 1;
    switch (a.cwf) {
    case 0: clip = st2 ? icw_fft_pack<0, 2>(a, tr, map, re, im, npts, PC, tid) : icw_fft_pack<0, 1>(a, tr, map, re, im, npts, PC, tid); break;
    case 1: clip = st2 ? icw_fft_pack<1, 2>(a, tr, map, re, im, npts, PC, tid) : icw_fft_pack<1, 1>(a, tr, map, re, im, npts, PC, tid); break;
    case 2: clip = st2 ? icw_fft_pack<2, 2>(a, tr, map, re, im, npts, PC, tid) : icw_fft_pack<2, 1>(a, tr, map, re, im, npts, PC, tid); break;
    default: clip = st2 ? icw_fft_pack<3, 2>(a, tr, map, re, im, npts, PC, tid) : icw_fft_pack<3, 1>(a, tr, map, re, im, npts, PC, tid); break;
    }
    if (a.cwf == 1 || a.cwf == 2) {
        if (clip) atomicAdd(&nclip, clip);
        __syncthreads();
        if (tid == 0 && nclip) atomicAdd(a.clipped + blockIdx.y, (unsigned long long)nclip);
    }
}

/* ---------------------------------------------------------------- launch wrapper ------- */
/* one pass over n_tracks tracks of 2^logP points (a->tracks, a->clipped: the launch's first) */
extern "C" hipError_t icw_launch_fft_pass(const IcwFftArgs *a, int n_tracks, hipStream_t st)
{
    const int l = a->l, logC = a->logC, logR = a->logR, logP = a->logP;
    if (logP < 1 || logP > ICW_FFT_MAX_LOG2 || l < 1 || l > ICW_FFT_PASS_LOG2 || logR < 0 || l + logR > logP ||
        logC != icw_fft_logc(logP, l) || n_tracks < 1 || n_tracks > 65535 || a->cwf > 3u || a->fmt > ICW_FMT_F32 ||
        !a->channels || !a->tracks || !a->in || !a->out || !a->clipped || (a->kind != ICW_FFT_MID && logR == 0) ||
        (a->kind == ICW_FFT_MID && logR != 0) || (a->kind == ICW_FFT_FWD && a->last) || (a->kind == ICW_FFT_INV && a->first) ||
        (!(a->first && a->last) && (!a->ws || ((uintptr_t)a->ws & 15))))
        return hipErrorInvalidValue;
    const size_t S = (size_t)1 << l, PC = ((size_t)1 << logC) + 1;
    const size_t lds = (2 * S * PC + ((2 * S * PC) & 1) + (S > 2 ? S : 2)) * sizeof(double);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(icw_fft_pass, dim3(1u << (logP - l - logC), n_tracks), dim3(256), lds, st, *a);
    return hipGetLastError();
}

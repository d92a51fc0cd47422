/*
 * icw_encode.hip -- gfx950 (CDNA4) kernels of the CWAVE encoders: the FIR Hilbert converter's analytic
 * signal as the packed frames of a CWAVE file (include/icw_cwave.h: icw_encode_cwave, KFE), and the
 * packer that does the same to the quadrature IIR's (icw_encode_cwave_iir, KIP).
 *
 * Built like icw_kernels.hip (`-ffp-contract=off`, no fast-math).  The staging and the sums are the
 * converter's own (icw_fir_dev.h), so I and Q are bit for bit what KF / KF2 feed the graph.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/icw.h"
#include "icw_device.h"
#include "icw_launch.h"

#pragma clang fp contract(off)

#include "icw_unpack_dev.h"
#include "icw_fir_dev.h"
#include "icw_cwpack_dev.h"

/* KFE: the converter as a CWAVE encoder.  KF's staging and sums (so the same unpack, fades, I and Q,
 * bit for bit), written as the interleaved frames of a CWAVE file (cwave.h:74-81) instead of the I / Q
 * rows: per channel `Re Im` as double / int16 / int16 + float / float, stereo Re(L) Im(L) Re(R) Im(R),
 * mono input one channel.  One workgroup per 2048-frame tile of a stream; a lane converts both channels
 * of its 8 frames.
 *
 * Conversions (the file format has no reference writer; these are the project's definition):
 *   float   (float)v, round to nearest even;
 *   int16   rint(v) (ties to even) saturated to [-32768, 32767], NaN -> 0; every saturated or NaN sample
 *           of a frame inside the block counts in clipped[s];
 *   double  the bits.
 *
 * Byte assembly.  A lane's 8 frames are 8 FB contiguous file bytes (FB = 4 .. 32, always a whole number
 * CU = FB / 2 of 16-byte units), packed in registers and written over the staged inputs (all read by
 * then) with ds_write_b128.  Those stores go by groups of 8 consecutive lanes over 32 banks: a lane
 * stride of an odd number of units puts the 8 lanes on the 8 distinct slots, so an even CU gets one pad
 * unit per lane (physical unit j + j / CU) and the odd one (CU 3: the 6-byte frame) none.  The tile then
 * leaves as consecutive 16-byte units, one global_store_dwordx4 per lane and pass; a tile whose first
 * byte is not 16-byte aligned leaves as dwords funnelled from two LDS words, and only the at most two
 * partial dwords at its ends as bytes. */
/* A tile's byte image in LDS to its place dst in the file rows: consecutive 16-byte units where dst is
 * 16-byte aligned (the at most 14 bytes after the last whole unit of a short tile as halfwords), else dwords
 * funnelled from two LDS words with the at most two partial dwords at the ends as bytes.  PADU pad units
 * after every CU units of the image (KFE's lane stride, below; 0: the image is the tile's bytes).  The
 * caller's buffer reaches 16 bytes past the image's last byte: the funnel reads a second word there (its bits
 * are shifted out) -- KFE's staging area is larger, KIP declares the 16 spare bytes. */
template <int PADU, int CU>
__device__ __forceinline__ void icw_tile_out(unsigned char *dst, int nbytes, const void *lds_image, int tid)
{
    const uint4 *ob = (const uint4 *)lds_image;
    const uint32_t *ow = (const uint32_t *)lds_image;
    const unsigned char *oc = (const unsigned char *)lds_image;
    /* logical 16-byte unit / dword / byte of the tile -> its place in the padded image */
    auto pu = [](int j) { return j + PADU * (j / CU); };
    auto pw = [](int j) { return j + 4 * PADU * (j / (4 * CU)); };
    auto pb = [](int j) { return j + 16 * PADU * (j / (16 * CU)); };
    if (!((uintptr_t)dst & 15)) {
        const int nu = nbytes >> 4;
        uint4 *d4 = (uint4 *)dst;
        for (int j = tid; j < nu; j += 256) d4[j] = ob[pu(j)];
        const int rest = nbytes - 16 * nu;               /* < 16, even: the last frames of a short tile */
        if (tid < rest / 2) {
            const int j = 16 * nu + 2 * tid;
            *(unsigned short *)(dst + j) = *(const unsigned short *)(oc + pb(j));
        }
    } else {
        const int b = (int)((uintptr_t)dst & 3);
        unsigned char *d0 = dst - b;
        const int nd = (b + nbytes + 3) >> 2;
        for (int k = tid; k < nd; k += 256) {
            const int o = 4 * k - b;                     /* the dword's first byte in the tile */
            if (o >= 0 && o + 4 <= nbytes) {
                uint32_t v = ow[pw(k)];
                if (b) v = (ow[pw(k - 1)] >> (8 * (4 - b))) | (v << (8 * b));
                *(uint32_t *)(d0 + 4 * k) = v;
            } else {
                for (int i = 0; i < 4; ++i)
                    if (o + i >= 0 && o + i < nbytes) d0[4 * k + i] = oc[pb(o + i)];
            }
        }
    }
}

/* KFE's workgroup (icw_fir_encode_body.inc) for the per-stream kernel: the same text as the one-input
 * kernel's body, with the tile placed by the block offset */
template <int CWF, int NC>
__device__ __forceinline__ void icw_fir_encode_ps(const IcwEncArgs &e)
{
    constexpr bool PS = true;
#include "icw_fir_encode_body.inc"
}

template <int CWF, int NC>
__global__ __launch_bounds__(256) void icw_fir_encode(IcwEncArgs e)
{
    constexpr bool PS = false;
#include "icw_fir_encode_body.inc"
}

/* KFE over streams with different inputs (e.f.desc; the PS pattern of icw_fir.hip): the workgroup column is
 * one stream, whose format, sizes and channels come in by scalar loads through the constant address space
 * (icw_fir_own_input) and replace the launch's; the branch on its channels is wave-uniform, and either side
 * is the one-input kernel's body -- the same staging, sums, conversions and tile store, so a stream's bytes
 * are those of a one-input call.  e.out is the call's first frame: the tile goes to frame e.f.t0 + tt of
 * the stream's row at the stream's own FB, so a mono stream beside a stereo one starts tiles at addresses
 * that are not 16-byte aligned (icw_tile_out's funnel path).  Dynamic LDS is sized for the widest stream. */
template <int CWF>
__global__ __launch_bounds__(256) void icw_fir_encode_mixed(IcwEncArgs e)
{
    icw_fir_own_input(e.f, blockIdx.y);
    icw_fir_own_conv(e.f, blockIdx.y);
    if (e.f.nch > 1) icw_fir_encode_ps<CWF, 2>(e);
    else icw_fir_encode_ps<CWF, 1>(e);
}

/* KIP: the packer of the IIR encoder (icw_encode_cwave_iir).  The quadrature IIR's analytic signal of a
 * launch block is already in HBM, as the `in` rows K2 writes with iq_out set ([n_streams][T][4]: lI, lQ,
 * rI, rQ -- the bus-form hand-off); this kernel only converts and interleaves them into KFE's frame
 * layout with KFE's conversions (icw_enc_i16, icw_cw_bytes).  Mono input: the left converter's pair.
 *
 * One workgroup per tile of 1 024 frames of a stream; a lane converts frames tid, tid + 256, .. (its row
 * reads are two 16-byte loads, consecutive lanes consecutive rows) and writes each frame's FB bytes at
 * byte t * FB of an unpadded LDS image of the tile.  The image leaves as KFE's tiles do: 16-byte units
 * where the tile's first byte is 16-byte aligned, else dwords funnelled from two LDS words with the at
 * most two partial dwords at its ends as bytes.  The kernel runs once per block beside nothing it could
 * slow down (the recurrence bounds the call), so its LDS stores are left to conflict. */
#define ICW_PACK_R 4                                     /* frames per lane */
/* KIP's workgroup: tile blockIdx.x of stream blockIdx.y, NC channels per frame.  frame0: 0, or the
 * per-stream kernel's block offset (as PS in icw_fir_encode_body); that kernel's image is dynamic LDS,
 * sized by the launcher for the stereo frame, which holds the mono one. */
template <int CWF, int NC, bool PS>
__device__ __forceinline__ void icw_iq_pack_body(IcwPackArgs a, long long frame0)
{
    constexpr int CB = icw_cw_bytes<CWF>::value, FB = NC * CB;    /* bytes per channel, per frame */
    constexpr int TF = 256 * ICW_PACK_R;
    /* 16 spare bytes: the funnel's second word may lie past the tile's last byte (its bits are shifted out) */
    unsigned char *img;
    if constexpr (PS) {
        extern __shared__ __attribute__((aligned(16))) unsigned char img_dyn[];
        img = img_dyn;
    } else {
        __shared__ __attribute__((aligned(16))) unsigned char img_own[TF * FB + 16];
        img = img_own;
    }
    __shared__ unsigned nclip;
    const int s = blockIdx.y, tid = threadIdx.x;
    const int tt = blockIdx.x * TF;
    const int nf = min(TF, a.T - tt);
    if (tid == 0) nclip = 0u;
    const double *rows = a.iq + ((size_t)s * a.T + tt) * 4;
    unsigned clip = 0u;
#pragma unroll
    for (int r = 0; r < ICW_PACK_R; ++r) {
        const int t = r * 256 + tid;
        if (t < nf) {
            double v[2 * NC];
            const double2 l = *(const double2 *)(rows + (size_t)t * 4);
            v[0] = l.x;
            v[1] = l.y;
            if constexpr (NC == 2) {
                const double2 rr = *(const double2 *)(rows + (size_t)t * 4 + 2);
                v[2] = rr.x;
                v[3] = rr.y;
            }
            unsigned char *f = img + t * FB;             /* FB is even; a multiple of 4 but for the 6-byte frame */
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if constexpr (CWF == 0) {
                    *(double2 *)(f + 16 * k) = make_double2(v[2 * k], v[2 * k + 1]);
                } else if constexpr (CWF == 1) {
                    const uint32_t re = icw_enc_i16(v[2 * k], true, clip), im = icw_enc_i16(v[2 * k + 1], true, clip);
                    *(uint32_t *)(f + 4 * k) = re | (im << 16);
                } else if constexpr (CWF == 2) {
                    const uint32_t re = icw_enc_i16(v[2 * k], true, clip), im = __float_as_uint((float)v[2 * k + 1]);
                    unsigned short *h = (unsigned short *)(f + 6 * k);
                    h[0] = (unsigned short)re;
                    h[1] = (unsigned short)im;
                    h[2] = (unsigned short)(im >> 16);
                } else {
                    *(uint2 *)(f + 8 * k) = make_uint2(__float_as_uint((float)v[2 * k]), __float_as_uint((float)v[2 * k + 1]));
                }
            }
        }
    }
    __syncthreads();                                     /* the image is whole; nclip is zero */
    if (CWF == 1 || CWF == 2) {
        if (clip) atomicAdd(&nclip, clip);
    }
    unsigned char *dst = a.out + (size_t)s * a.out_stride + (size_t)tt * FB;
    if constexpr (PS) dst += (size_t)frame0 * FB;
    const int nbytes = nf * FB;
    icw_tile_out<0, 1>(dst, nbytes, img, tid);
    if (CWF == 1 || CWF == 2) {
        __syncthreads();
        if (tid == 0 && nclip) atomicAdd(a.clipped + s, (unsigned long long)nclip);
    }
}

template <int CWF, int NC>
__global__ __launch_bounds__(256) void icw_iq_pack(IcwPackArgs a)
{
    icw_iq_pack_body<CWF, NC, false>(a, 0);
}

/* KIP over streams with different inputs: the workgroup column's stream takes its channels from the table by a
 * scalar load and a wave-uniform branch to the one-input kernel's body; its tile goes to frame m.t0 + tt of
 * the stream's row at the stream's own FB (m.p.out is the call's first frame). */
template <int CWF>
__global__ __launch_bounds__(256) void icw_iq_pack_mixed(IcwPackMixArgs m)
{
    const __attribute__((address_space(4))) IcwInDesc *d = (const __attribute__((address_space(4))) IcwInDesc *)m.desc + blockIdx.y;
    if (d->nch > 1) icw_iq_pack_body<CWF, 2, true>(m.p, m.t0);
    else icw_iq_pack_body<CWF, 1, true>(m.p, m.t0);
}

/* the reader position and (IIR encoder; the FIR one passes no hq_phase) the Hilbert phases of the streams an
 * encode call covered: what icw_advance does to them, without its frame counter */
__global__ __launch_bounds__(64) void icw_enc_advance(long long *pos, uint32_t *hq_phase, int n_streams, long long n)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s < n_streams) {
        pos[s] += n;
        if (hq_phase) {
            hq_phase[s * 2 + 0] = (hq_phase[s * 2 + 0] + (unsigned)n) & 3u;
            hq_phase[s * 2 + 1] = (hq_phase[s * 2 + 1] + (unsigned)n) & 3u;
        }
    }
}

/* ---------------------------------------------------------------- launch wrappers ------- */
template <int CWF, int NC>
static hipError_t launch_fir_encode_t(const IcwEncArgs *e, hipStream_t st)
{
    constexpr int TF = 256 * ICW_FIR_R;
    constexpr int CU = NC * icw_cw_bytes<CWF>::value / 2, PADU = (CU & 1) ? 0 : 1;
    /* the staged channels, or the tile's padded frame image where that is larger (it takes their place) */
    const size_t lds = std::max((size_t)NC * icw_fir_px(e->f.M, TF) * sizeof(double), (size_t)256 * (CU + PADU) * 16);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    /* LDS above 64 KB per workgroup needs the kernel attribute (gfx950: 160 KB per CU) */
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void *)icw_fir_encode<CWF, NC>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((icw_fir_encode<CWF, NC>), dim3((e->f.T + TF - 1) / TF, e->f.n_streams), dim3(256), lds, st, *e);
    return hipGetLastError();
}

/* f(icw_ic<cwf>, icw_ic<channels>) for a CWAVE format cwf = cw_format - ICW_FMT_CW_F64 of 1 or 2 channels */
template <class F>
static hipError_t enc_dispatch(int cwf, bool st2, F &&f)
{
    switch (cwf) {
    case 0: return st2 ? f(icw_ic<0>{}, icw_ic<2>{}) : f(icw_ic<0>{}, icw_ic<1>{});
    case 1: return st2 ? f(icw_ic<1>{}, icw_ic<2>{}) : f(icw_ic<1>{}, icw_ic<1>{});
    case 2: return st2 ? f(icw_ic<2>{}, icw_ic<2>{}) : f(icw_ic<2>{}, icw_ic<1>{});
    case 3: return st2 ? f(icw_ic<3>{}, icw_ic<2>{}) : f(icw_ic<3>{}, icw_ic<1>{});
    }
    return hipErrorInvalidValue;
}

/* KFE of one launch block; cwf = cw_format - ICW_FMT_CW_F64 */
extern "C" hipError_t icw_launch_fir_encode(const IcwEncArgs *e, int cwf, hipStream_t st)
{
    const int M = e->f.M, nt = e->f.nt;
    if (M < 2 || M > ICW_FIR_MAX_M || (M & 1) || nt < 1 || 2 * nt - 1 > M / 2 || e->f.T <= 0) return hipErrorInvalidValue;
    return enc_dispatch(cwf, e->f.nch > 1, [&](auto fc, auto nc) {
        return launch_fir_encode_t<decltype(fc)::value, decltype(nc)::value>(e, st);
    });
}

/* KFE of one launch block over streams with different inputs (e->f.desc): LDS for the widest stream of the
 * call (e->f.nch), whose staged channels and frame image hold every narrower one's */
template <int CWF>
static hipError_t launch_fir_encode_mixed_t(const IcwEncArgs *e, hipStream_t st)
{
    constexpr int TF = 256 * ICW_FIR_R;
    const int nc = e->f.nch > 1 ? 2 : 1;
    const int cu = nc * icw_cw_bytes<CWF>::value / 2, padu = (cu & 1) ? 0 : 1;
    const size_t lds = std::max((size_t)nc * icw_fir_px(e->f.M, TF) * sizeof(double), (size_t)256 * (cu + padu) * 16);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void *)icw_fir_encode_mixed<CWF>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((icw_fir_encode_mixed<CWF>), dim3((e->f.T + TF - 1) / TF, e->f.n_streams), dim3(256), lds, st, *e);
    return hipGetLastError();
}

extern "C" hipError_t icw_launch_fir_encode_mixed(const IcwEncArgs *e, int cwf, hipStream_t st)
{
    const int M = e->f.M, nt = e->f.nt;
    if ((!e->f.desc && !e->f.conv) || !e->out || !e->clipped || e->f.n_streams <= 0) return hipErrorInvalidValue;
    if (M < 2 || M > ICW_FIR_MAX_M || (M & 1) || nt < 1 || 2 * nt - 1 > M / 2 || e->f.T <= 0) return hipErrorInvalidValue;
    switch (cwf) {
    case 0: return launch_fir_encode_mixed_t<0>(e, st);
    case 1: return launch_fir_encode_mixed_t<1>(e, st);
    case 2: return launch_fir_encode_mixed_t<2>(e, st);
    case 3: return launch_fir_encode_mixed_t<3>(e, st);
    }
    return hipErrorInvalidValue;
}

template <int CWF, int NC>
static hipError_t launch_iq_pack_t(const IcwPackArgs *a, hipStream_t st)
{
    constexpr int TF = 256 * ICW_PACK_R;
    hipLaunchKernelGGL((icw_iq_pack<CWF, NC>), dim3((a->T + TF - 1) / TF, a->n_streams), dim3(256), 0, st, *a);
    return hipGetLastError();
}

/* KIP of one launch block; cwf = cw_format - ICW_FMT_CW_F64, nc = channels of the file's frames (1 or 2) */
extern "C" hipError_t icw_launch_iq_pack(const IcwPackArgs *a, int cwf, int nc, hipStream_t st)
{
    if (a->T <= 0 || a->n_streams <= 0 || !a->iq || !a->out || !a->clipped || nc < 1 || nc > 2) return hipErrorInvalidValue;
    return enc_dispatch(cwf, nc > 1, [&](auto fc, auto ncc) {
        return launch_iq_pack_t<decltype(fc)::value, decltype(ncc)::value>(a, st);
    });
}

template <int CWF>
static hipError_t launch_iq_pack_mixed_t(const IcwPackMixArgs *a, hipStream_t st)
{
    constexpr int TF = 256 * ICW_PACK_R;
    /* the image of a stereo tile and the funnel's 16 spare bytes: at most 32 784 bytes */
    const size_t lds = (size_t)TF * 2 * icw_cw_bytes<CWF>::value + 16;
    hipLaunchKernelGGL((icw_iq_pack_mixed<CWF>), dim3((a->p.T + TF - 1) / TF, a->p.n_streams), dim3(256), lds, st, *a);
    return hipGetLastError();
}

/* KIP of one launch block over streams with different inputs (a->desc) */
extern "C" hipError_t icw_launch_iq_pack_mixed(const IcwPackMixArgs *a, int cwf, hipStream_t st)
{
    if (!a->desc || a->p.T <= 0 || a->p.n_streams <= 0 || !a->p.iq || !a->p.out || !a->p.clipped || a->t0 < 0)
        return hipErrorInvalidValue;
    switch (cwf) {
    case 0: return launch_iq_pack_mixed_t<0>(a, st);
    case 1: return launch_iq_pack_mixed_t<1>(a, st);
    case 2: return launch_iq_pack_mixed_t<2>(a, st);
    case 3: return launch_iq_pack_mixed_t<3>(a, st);
    }
    return hipErrorInvalidValue;
}

extern "C" hipError_t icw_launch_enc_advance(long long *pos, uint32_t *hq_phase, int n_streams, long long n, hipStream_t st)
{
    hipLaunchKernelGGL(icw_enc_advance, dim3((n_streams + 63) / 64), dim3(64), 0, st, pos, hq_phase, n_streams, n);
    return hipGetLastError();
}

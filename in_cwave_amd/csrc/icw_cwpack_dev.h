/*
 * icw_cwpack_dev.h -- device code shared by the CWAVE encoders (icw_encode.hip, icw_fft.hip): the bytes of
 * a channel's sample in every CWAVE format, the int16 conversion with its clip count, and one frame's
 * bytes to an address of any alignment.  Included after hip_runtime.h, inside `#pragma clang fp contract(off)`.
 *
 * Conversions (the file format has no reference writer; these are the project's definition):
 *   float   (float)v, round to nearest even;
 *   int16   rint(v) (ties to even) saturated to [-32768, 32767], NaN -> 0; every saturated or NaN sample
 *           of a live frame counts as clipped;
 *   double  the bits.
 */
#ifndef ICW_CWPACK_DEV_H_
#define ICW_CWPACK_DEV_H_

template <int CWF> struct icw_cw_bytes { static constexpr int value = CWF == 0 ? 16 : CWF == 1 ? 4 : CWF == 2 ? 6 : 8; };

__device__ __forceinline__ uint32_t icw_enc_i16(double v, bool live, unsigned &clip)
{
    const double r = __builtin_rint(v);
    if (r >= -32768.0 && r <= 32767.0) return (uint32_t)(int)r & 0xffffu;
    if (live) ++clip;
    return r != r ? 0u : (r < 0.0 ? 0x8000u : 0x7fffu);
}

/* One live frame of NC channels (vi[k], vq[k]: Re, Im of channel k) in format CWF to dst, whatever dst's
 * alignment: the frame is assembled as halfwords (every frame size is even) and leaves as dwords where
 * dst and the frame size allow, else as halfwords, else as bytes. */
template <int CWF, int NC>
__device__ __forceinline__ void icw_cw_frame_put(unsigned char *dst, const double (&vi)[NC], const double (&vq)[NC],
                                                 unsigned &clip)
{
    constexpr int CB = icw_cw_bytes<CWF>::value, FB = NC * CB, NH = FB / 2;
    uint32_t h[NH];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        constexpr int HC = CB / 2;
        if constexpr (CWF == 0) {
            const unsigned long long bi = (unsigned long long)__double_as_longlong(vi[k]);
            const unsigned long long bq = (unsigned long long)__double_as_longlong(vq[k]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h[HC * k + i] = (uint32_t)(bi >> (16 * i)) & 0xffffu;
                h[HC * k + 4 + i] = (uint32_t)(bq >> (16 * i)) & 0xffffu;
            }
        } else if constexpr (CWF == 1) {
            h[HC * k] = icw_enc_i16(vi[k], true, clip);
            h[HC * k + 1] = icw_enc_i16(vq[k], true, clip);
        } else if constexpr (CWF == 2) {
            const uint32_t im = __float_as_uint((float)vq[k]);
            h[HC * k] = icw_enc_i16(vi[k], true, clip);
            h[HC * k + 1] = im & 0xffffu;
            h[HC * k + 2] = im >> 16;
        } else {
            const uint32_t re = __float_as_uint((float)vi[k]), im = __float_as_uint((float)vq[k]);
            h[HC * k] = re & 0xffffu;
            h[HC * k + 1] = re >> 16;
            h[HC * k + 2] = im & 0xffffu;
            h[HC * k + 3] = im >> 16;
        }
    }
    const uintptr_t al = (uintptr_t)dst;
    if ((FB % 4) == 0 && !(al & 3)) {
#pragma unroll
        for (int i = 0; i < NH / 2; ++i) ((uint32_t *)dst)[i] = h[2 * i] | (h[2 * i + 1] << 16);
    } else if (!(al & 1)) {
#pragma unroll
        for (int i = 0; i < NH; ++i) ((unsigned short *)dst)[i] = (unsigned short)h[i];
    } else {
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            dst[2 * i] = (unsigned char)h[i];
            dst[2 * i + 1] = (unsigned char)(h[i] >> 8);
        }
    }
}

#endif /* ICW_CWPACK_DEV_H_ */

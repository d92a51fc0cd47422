/*
 * icw_unpack_dev.h -- device code shared by the kernel files: the input unpackers (little-endian,
 * exact conversions) and the fade of xwave_unpack_csample.  Included after hip_runtime.h, icw.h and
 * icw_device.h, inside `#pragma clang fp contract(off)`.
 */
#ifndef ICW_UNPACK_DEV_H_
#define ICW_UNPACK_DEV_H_

/* ------------------------------------------------------------------ input unpack --------- */
/* xwave_reader.c:205-239 + unpack_lsb.h:53-125 (little-endian, exact conversions) */
__device__ __forceinline__ double icw_unpack(const unsigned char *p, uint32_t fmt)
{
    switch (fmt) {
    case ICW_FMT_I16: {
        int v = (int)(short)((unsigned)p[0] | ((unsigned)p[1] << 8));
        return (double)v;
    }
    case ICW_FMT_U8:
        return 256.0 * (double)((signed char)(unsigned char)(p[0] - 0x80u));
    case ICW_FMT_I24: {
        int v = ((int)(((unsigned)p[0] << 8) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 24))) >> 8;
        return ((double)v) / 256.0;
    }
    case ICW_FMT_I32: {
        int v = (int)((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24));
        return ((double)v) / 65536.0;
    }
    default: {
        unsigned u = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        return 32768.0 * (double)__uint_as_float(u);
    }
    }
}

/* CWAVE unpackers (xwave_reader.c:171-200): no scaling, values already on the 16-bit scale */
__device__ __forceinline__ uint32_t icw_le32(const unsigned char *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void icw_unpack_iq(const unsigned char *p, uint32_t fmt, double &vI, double &vQ)
{
    switch (fmt) {
    case ICW_FMT_CW_F64: {
        const unsigned long long lo = icw_le32(p), hi = icw_le32(p + 4);
        const unsigned long long lo2 = icw_le32(p + 8), hi2 = icw_le32(p + 12);
        vI = __longlong_as_double((long long)(lo | (hi << 32)));
        vQ = __longlong_as_double((long long)(lo2 | (hi2 << 32)));
        break;
    }
    case ICW_FMT_CW_I16:
        vI = (double)(short)((unsigned)p[0] | ((unsigned)p[1] << 8));
        vQ = (double)(short)((unsigned)p[2] | ((unsigned)p[3] << 8));
        break;
    case ICW_FMT_CW_I16_F32:
        vI = (double)(short)((unsigned)p[0] | ((unsigned)p[1] << 8));
        vQ = (double)__uint_as_float(icw_le32(p + 2));
        break;
    default:
        vI = (double)__uint_as_float(icw_le32(p));
        vQ = (double)__uint_as_float(icw_le32(p + 4));
        break;
    }
}

/* one sample of format FMT; AL: the address is aligned to the sample's size, so one typed load
 * replaces the byte loads and their shifts */
template <int FMT, bool AL>
__device__ __forceinline__ double icw_unpack_f(const unsigned char *p)
{
    if constexpr (AL && FMT == ICW_FMT_I16) return (double)*(const short *)p;
    else if constexpr (AL && FMT == ICW_FMT_I32) return ((double)*(const int *)p) / 65536.0;
    else if constexpr (AL && FMT == ICW_FMT_F32) return 32768.0 * (double)*(const float *)p;
    else return icw_unpack(p, FMT);
}

template <int V> struct icw_ic { static constexpr int value = V; };

/* calls f(icw_ic<FMT>, icw_ic<AL>) for a uniform real format: the unpack specialised once per
 * workgroup instead of a format switch per sample.  al: the OR of the base address and the strides
 * the samples are read at (aligned when its low bits below the sample size are clear) */
template <typename F>
__device__ __forceinline__ void icw_fmt_dispatch(uint32_t fmt, uintptr_t al, F &&f)
{
    switch (fmt) {
    case ICW_FMT_I16:
        if (al & 1) f(icw_ic<ICW_FMT_I16>(), icw_ic<0>());
        else f(icw_ic<ICW_FMT_I16>(), icw_ic<1>());
        break;
    case ICW_FMT_U8: f(icw_ic<ICW_FMT_U8>(), icw_ic<0>()); break;
    case ICW_FMT_I24: f(icw_ic<ICW_FMT_I24>(), icw_ic<0>()); break;
    case ICW_FMT_I32:
        if (al & 3) f(icw_ic<ICW_FMT_I32>(), icw_ic<0>());
        else f(icw_ic<ICW_FMT_I32>(), icw_ic<1>());
        break;
    default:
        if (al & 3) f(icw_ic<ICW_FMT_F32>(), icw_ic<0>());
        else f(icw_ic<ICW_FMT_F32>(), icw_ic<1>());
        break;
    }
}

/* one I/Q pair of CWAVE format FMT; AL: the address is aligned to the pair's size, so one typed load
 * (16 bytes CW_F64, 8 CW_F32, 4 CW_I16) replaces the pair's byte loads.  The conversions are
 * icw_unpack_iq's, so the bits are.  CW_I16_F32 is a 6-byte pair whose float is 2-byte aligned at
 * best: always the byte form */
template <int FMT, bool AL>
__device__ __forceinline__ void icw_unpack_iq_f(const unsigned char *p, double &vI, double &vQ)
{
    if constexpr (AL && FMT == ICW_FMT_CW_F64) {
        const double2 v = *(const double2 *)p;
        vI = v.x;
        vQ = v.y;
    } else if constexpr (AL && FMT == ICW_FMT_CW_F32) {
        const float2 v = *(const float2 *)p;
        vI = (double)v.x;
        vQ = (double)v.y;
    } else if constexpr (AL && FMT == ICW_FMT_CW_I16) {
        const unsigned u = *(const unsigned *)p;
        vI = (double)(short)(u & 0xffffu);
        vQ = (double)(short)(u >> 16);
    } else {
        icw_unpack_iq(p, FMT, vI, vQ);
    }
}

/* calls f(icw_ic<FMT>, icw_ic<AL>) for a uniform CWAVE format, as icw_fmt_dispatch does for the real
 * ones.  al: the OR of the row's base address and the frame size (aligned when its low bits below the
 * pair's size are clear: the second channel's pair sits one pair further) */
template <typename F>
__device__ __forceinline__ void icw_cw_dispatch(uint32_t fmt, uintptr_t al, F &&f)
{
    switch (fmt) {
    case ICW_FMT_CW_F64:
        if (al & 15) f(icw_ic<ICW_FMT_CW_F64>(), icw_ic<0>());
        else f(icw_ic<ICW_FMT_CW_F64>(), icw_ic<1>());
        break;
    case ICW_FMT_CW_I16:
        if (al & 3) f(icw_ic<ICW_FMT_CW_I16>(), icw_ic<0>());
        else f(icw_ic<ICW_FMT_CW_I16>(), icw_ic<1>());
        break;
    case ICW_FMT_CW_I16_F32: f(icw_ic<ICW_FMT_CW_I16_F32>(), icw_ic<0>()); break;
    default:
        if (al & 7) f(icw_ic<ICW_FMT_CW_F32>(), icw_ic<0>());
        else f(icw_ic<ICW_FMT_CW_F32>(), icw_ic<1>());
        break;
    }
}

/* fade factor of xwave_unpack_csample (xwave_reader.c:918-936); < 0 means "no fade" */
__device__ __forceinline__ double icw_fade(long long ix, long long ns, long long fi, long long fo)
{
    double fade = -1.0;
    if (ix < fi)
        fade = ((double)ix) / ((double)fi);
    else if (ix > ns - fo && ix < ns)
        fade = ((double)(ns - ix)) / ((double)fo);
    return fade;
}

#endif /* ICW_UNPACK_DEV_H_ */

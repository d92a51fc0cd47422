"""Independent restatement of the CWAVE encoder (include/icw_cwave.h: icw_encode_cwave) in pure
Python, for the tests of the GPU kernel.

  unpack    the reader's exact sample conversions (xwave_reader.c:205-239), in numpy float64
  analytic  I[n] = x[n - k_M/2], Q[n] = fma over the odd taps in ascending order from +0.0, the taps
            from the oracle (oracle.fir_taps); the FMA is done exactly with fractions.Fraction and
            rounded once by float() (correctly rounded, ties to even) -- Python 3.10 has no math.fma
  frames    the file's interleaved frame layout (cwave.h:74-81) with the encoder's conversions:
            double = bits, float = astype(float32) (nearest even), int16 = rint (ties to even),
            NaN -> 0, clipped to [-32768, 32767]; and the count of clipped / NaN int16 samples

tests/test_cwave_encode_ref.py pins this file to the oracle's fir_process before a GPU test uses it.
"""
from fractions import Fraction

import numpy as np

from in_cwave_amd import abi

FRAME_DTYPES = {
    abi.FMT_CW_F64: np.dtype([("re", "<f8"), ("im", "<f8")]),
    abi.FMT_CW_I16: np.dtype([("re", "<i2"), ("im", "<i2")]),
    abi.FMT_CW_I16_F32: np.dtype([("re", "<i2"), ("im", "<f4")]),
    abi.FMT_CW_F32: np.dtype([("re", "<f4"), ("im", "<f4")]),
}


def unpack(raw, fmt, channels):
    """raw uint8 [n_frames * channels * sample bytes] -> float64 [n_frames, min(channels, 2)] on the
    16-bit scale"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if fmt == abi.FMT_U8:
        x = 256.0 * (raw.astype(np.int16) - 128).astype(np.float64)
    elif fmt == abi.FMT_I16:
        x = raw.view("<i2").astype(np.float64)
    elif fmt == abi.FMT_I24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = ((b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)) >> 8
        x = v.astype(np.float64) / 256.0
    elif fmt == abi.FMT_I32:
        x = raw.view("<i4").astype(np.float64) / 65536.0
    elif fmt == abi.FMT_F32:
        x = 32768.0 * raw.view("<f4").astype(np.float64)
    else:
        raise ValueError(fmt)
    return x.reshape(-1, channels)[:, :2].copy()


def analytic(x, k_M, g):
    """x float64 [T, nc] (zero history before it) -> (I, Q) float64 [T, nc]; g: the odd taps"""
    T, nc = x.shape
    c = k_M // 2
    xp = np.concatenate([np.zeros((k_M, nc)), x])          # xp[k_M + j] = x[j]
    I = xp[k_M - c:k_M - c + T].copy()
    Q = np.zeros((T, nc))
    gf = [Fraction(float(v)) for v in g]
    for ch in range(nc):
        col = xp[:, ch]
        # d[k][n] = x[n - c - m] - x[n - c + m], m = 2k + 1: one rounded double subtraction each
        d = [col[k_M - c - (2 * k + 1):k_M - c - (2 * k + 1) + T] - col[k_M - c + (2 * k + 1):k_M - c + (2 * k + 1) + T]
             for k in range(len(g))]
        for n in range(T):
            acc = 0.0
            for k in range(len(g)):
                dv = d[k][n]
                if dv != 0.0 or acc != 0.0:
                    acc = float(gf[k] * Fraction(float(dv)) + Fraction(acc))
            Q[n, ch] = acc
    return I, Q


def quant_i16(v):
    """(int16 values, number of clipped or NaN samples)"""
    r = np.rint(v)
    nan = np.isnan(r)
    bad = nan | (r > 32767.0) | (r < -32768.0)
    r = np.where(nan, 0.0, r)
    return np.clip(r, -32768.0, 32767.0).astype("<i2"), int(bad.sum())


def frames(I, Q, cw_format):
    """(uint8 [T * frame bytes], clipped int16 samples) of I, Q float64 [T, nc]"""
    rec = np.zeros(I.shape, dtype=FRAME_DTYPES[cw_format])
    clipped = 0
    with np.errstate(over="ignore", invalid="ignore"):
        if cw_format == abi.FMT_CW_F64:
            rec["re"], rec["im"] = I, Q
        elif cw_format == abi.FMT_CW_I16:
            rec["re"], a = quant_i16(I)
            rec["im"], b = quant_i16(Q)
            clipped = a + b
        elif cw_format == abi.FMT_CW_I16_F32:
            rec["re"], clipped = quant_i16(I)
            rec["im"] = Q.astype(np.float32)
        else:
            rec["re"], rec["im"] = I.astype(np.float32), Q.astype(np.float32)
    return rec.reshape(-1).view(np.uint8).copy(), clipped


def iq_of_f64_frames(data, nc):
    """(I, Q) float64 [T, nc] of ICW_FMT_CW_F64 frame bytes"""
    rec = np.ascontiguousarray(data, dtype=np.uint8).view(FRAME_DTYPES[abi.FMT_CW_F64]).reshape(-1, nc)
    return rec["re"].copy(), rec["im"].copy()


def encode(raw, fmt, channels, k_M, g, cw_format=abi.FMT_CW_F64):
    """one fresh stream: raw PCM bytes -> (CWAVE frame bytes, clipped)"""
    I, Q = analytic(unpack(raw, fmt, channels), k_M, g)
    return frames(I, Q, cw_format)

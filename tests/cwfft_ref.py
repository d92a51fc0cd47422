"""Independent restatement of the direct-FFT CWAVE converter (include/icw_cwave.h: icw_encode_cwave_fft) in
numpy longdouble / clongdouble, for the tests of the GPU kernel.

  fft_ld      a vectorised radix-2 decimation-in-time transform in clongdouble, twiddles from long-double
              cos / sin of 2 pi k / P (k / P exact, pi = 4 atan(1) in long double)
  hilbert_q   Q = Re( IDFT_P( m[k] DFT_P(x)[k] ) ), m = -j below P/2, +j above, 0 at 0 and P/2, x zero-padded
              to P = the smallest power of two >= max(N, 2); long double in, long double out
  hilbert_q_np the same formula through numpy.fft in float64: the yardstick of a float64 FFT's error
  tolerance   max(4 e_np, 2^-52 log2(P) max|reference|), e_np = max|numpy.fft float64 - long double|

Framing and quantising are cwenc_ref's (unpack, frames).  tests/test_cwave_fft_ref.py pins this file.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = 4 * np.arctan(LD(1))


def pad_len(n):
    p = 2
    while p < n:
        p *= 2
    return p


def _twiddles(p, sign):
    """exp(sign * 2 pi j k / p), k < p / 2, in clongdouble"""
    ang = 2 * PI * (np.arange(p // 2, dtype=LD) / LD(p))
    w = np.empty(p // 2, dtype=CLD)
    w.real = np.cos(ang)
    w.imag = sign * np.sin(ang)
    return w


def fft_ld(x, inverse=False):
    """DFT (inverse: without the factor 1 / P) of a power-of-two length array, in clongdouble"""
    x = np.asarray(x, dtype=CLD)
    p = x.size
    assert p & (p - 1) == 0 and p >= 1
    bits = p.bit_length() - 1
    idx = np.arange(p)
    rev = np.zeros(p, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    a = x[rev].copy()
    w_all = _twiddles(p, +1 if inverse else -1) if p > 1 else None
    half = 1
    while half < p:
        a = a.reshape(-1, 2, half)
        w = w_all[::p // (2 * half)]
        t = a[:, 1, :] * w
        a = np.stack([a[:, 0, :] + t, a[:, 0, :] - t], axis=1)
        half *= 2
    return a.reshape(-1)


def multiplier(p):
    m = np.zeros(p, dtype=CLD)
    m[1:p // 2] = -1j
    m[p // 2 + 1:] = 1j
    return m


def hilbert_q(x):
    """x float64 [N] -> Q longdouble [N]"""
    n = x.size
    p = pad_len(n)
    xp = np.zeros(p, dtype=CLD)
    xp[:n] = np.asarray(x, dtype=LD)
    y = fft_ld(multiplier(p) * fft_ld(xp), inverse=True) / LD(p)
    return y.real[:n].copy()


def hilbert_q_np(x):
    """the same formula through numpy.fft in float64"""
    n = x.size
    p = pad_len(n)
    xp = np.zeros(p, dtype=np.float64)
    xp[:n] = x
    m = multiplier(p).astype(np.complex128)
    return np.fft.ifft(m * np.fft.fft(xp)).real[:n].copy()


def tolerance(x, q_ref):
    """(bound, e_np) for one channel x float64 [N] and its long-double reference"""
    p = pad_len(x.size)
    e_np = float(np.max(np.abs(hilbert_q_np(x).astype(LD) - q_ref)))
    return max(4.0 * e_np, 2.0 ** -52 * np.log2(p) * float(np.max(np.abs(q_ref)))), e_np


def random_pcm16(rng, n, channels):
    """int16 PCM bytes of n frames, uniform in about +-30000"""
    return rng.integers(-30000, 30001, size=n * channels).astype("<i2").view(np.uint8).copy()

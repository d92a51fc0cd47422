"""Independent restatement of the direct-FFT CWAVE converter (include/icw_cwave.h: icw_encode_cwave_fft) in
numpy longdouble / clongdouble, for the tests of the GPU kernel.

  fft_ld      a vectorised radix-2 decimation-in-time transform in clongdouble, twiddles from long-double
              cos / sin of 2 pi k / P (k / P exact, pi = 4 atan(1) in long double)
  hilbert_q   Q = Re( IDFT_P( m[k] DFT_P(x)[k] ) ), m = -j below P/2, +j above, 0 at 0 and P/2, x zero-padded
              to P = the smallest power of two >= max(N, 2); long double in, long double out
  hilbert_q_np the same formula through numpy.fft in float64: the yardstick of a float64 FFT's error
  tolerance   max(4 e_np, 2^-52 log2(P) max|reference|), e_np = max|numpy.fft float64 - long double|
  impulse_q   the closed form of Q for a track that is zero but for K impulses, at chosen positions only: cost
              O(K x positions), so transform lengths far beyond fft_ld's reach have an exact reference
  impulse_tolerance   tolerance's formula with e_np taken over those positions

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


def multiplier(p, dtype=CLD):
    m = np.zeros(p, dtype=dtype)
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
    m = multiplier(p, np.complex128)                     # 0 and +-j: the same values in either width
    return np.fft.ifft(m * np.fft.fft(xp)).real[:n].copy()


def tolerance(x, q_ref):
    """(bound, e_np) for one channel x float64 [N] and its long-double reference"""
    p = pad_len(x.size)
    e_np = float(np.max(np.abs(hilbert_q_np(x).astype(LD) - q_ref)))
    return max(4.0 * e_np, 2.0 ** -52 * np.log2(p) * float(np.max(np.abs(q_ref)))), e_np


def impulse_track(n, pos, amp):
    """the float64 track of n frames that is zero but for amp[k] at frame pos[k] (pos pairwise different)"""
    x = np.zeros(n, dtype=np.float64)
    x[np.asarray(pos, dtype=np.int64)] = amp
    return x


def impulse_q(n, pos, amp, at):
    """Q longdouble [len(at)] of impulse_track(n, pos, amp) at the frames `at`, in closed form.

    The multiplier's kernel is h[d] = (2 / P) cot(pi d / P) for odd d and 0 for even d (d mod P, P = pad_len(n)):
    (1 / P) sum_k m[k] exp(2 pi j k d / P) = (2 / P) sum_{0 < k < P/2} sin(2 pi k d / P), which is that.  So
    Q[at] = sum_k amp[k] h[(at - pos[k]) mod P], exact and pointwise.  d / P is exact; d above P / 2 is folded
    to d - P so that the tangent's argument stays within +-pi/2; P = 2 has h = 0 (its d = 1 is P / 2)."""
    p = pad_len(n)
    at = np.asarray(at, dtype=np.int64)
    q = np.zeros(at.size, dtype=LD)
    for nk, ak in zip(np.asarray(pos, dtype=np.int64), np.asarray(amp, dtype=np.float64)):
        d = (at - nk) % p
        odd = ((d & 1) == 1) & (2 * d != p)
        d = d[odd]
        d = np.where(2 * d > p, d - p, d)
        q[odd] += LD(ak) * (LD(2) / LD(p)) / np.tan(PI * (d.astype(LD) / LD(p)))
    return q


def impulse_tolerance(n, pos, amp, at, q_ref, q_np=None):
    """(bound, e_np): tolerance's formula for impulse_track(n, pos, amp) with e_np taken over the frames `at`,
    q_ref = impulse_q(n, pos, amp, at).  q_np: hilbert_q_np of the track where the caller already has it."""
    p = pad_len(n)
    if q_np is None:
        q_np = hilbert_q_np(impulse_track(n, pos, amp))
    e_np = float(np.max(np.abs(q_np[np.asarray(at, dtype=np.int64)].astype(LD) - q_ref)))
    return max(4.0 * e_np, 2.0 ** -52 * np.log2(p) * float(np.max(np.abs(q_ref)))), e_np


def random_pcm16(rng, n, channels):
    """int16 PCM bytes of n frames, uniform in about +-30000"""
    return rng.integers(-30000, 30001, size=n * channels).astype("<i2").view(np.uint8).copy()

"""CPU: pins tests/cwfft_ref.py, the long-double restatement of the direct-FFT converter's definition
(include/icw_cwave.h: icw_encode_cwave_fft), before a GPU test uses it: against scipy.signal.hilbert, against
the same formula through numpy.fft in float64, and on a single-bin cosine.  The GPU tolerance is built on
numpy.fft's deviation from the long-double result, so that deviation is checked to be non-zero here.  The closed
form for sparse tracks (impulse_q, the reference of the lengths the long-double transform cannot reach) is pinned
to that transform within its own rounding, 2^-60 log2(P) max|Q|."""
import numpy as np
import pytest
from scipy.signal import hilbert as signal_hilbert

import cwfft_ref as R

# (N, P): the GPU accuracy test's lengths
SIZES = [(2, 2), (3, 4), (50, 64), (64, 64), (65, 128), (4096, 4096), (4097, 8192), (5000, 8192), (40000, 65536)]
EPS = float(np.finfo(np.longdouble).eps)


def signal(n, seed=7):
    return np.random.default_rng(seed).integers(-30000, 30001, size=n).astype(np.float64)


def test_long_double_is_wider_than_double():
    assert EPS < 2.0 ** -60


@pytest.mark.parametrize("n,p", SIZES)
def test_pad_len(n, p):
    assert R.pad_len(n) == p


@pytest.mark.parametrize("p", [1, 2, 8, 64])
def test_fft_ld_equals_the_dft_sum(p):
    rng = np.random.default_rng(p)
    x = rng.standard_normal(p) + 1j * rng.standard_normal(p)
    k = np.arange(p)
    dft = np.exp(-2j * np.pi * np.outer(k, k) / p) @ x
    assert np.max(np.abs(R.fft_ld(x).astype(np.complex128) - dft)) < 1e-12 * p
    back = R.fft_ld(R.fft_ld(x), inverse=True) / p
    assert np.max(np.abs(back.astype(np.complex128) - x)) < 1e-15


@pytest.mark.parametrize("n,p", SIZES)
def test_against_numpy_fft_and_scipy(n, p):
    x = signal(n)
    q = R.hilbert_q(x)
    assert q.dtype == np.longdouble and q.shape == (n,)
    q_np = R.hilbert_q_np(x)
    q_sp = signal_hilbert(x, p).imag[:n]
    scale = max(1.0, float(np.max(np.abs(q))))
    # two float64 FFTs against the long-double result: a few ulp of the largest value per stage
    bound = 2.0 ** -52 * 4 * max(1.0, np.log2(p)) * scale
    assert float(np.max(np.abs(q_np - q))) <= bound
    assert float(np.max(np.abs(q_sp - q))) <= bound
    if p >= 64:
        # the yardstick of the GPU tolerance: numpy.fft in float64 does deviate from the long-double result
        assert float(np.max(np.abs(q_np.astype(np.longdouble) - q))) > 0.0
        tol, e_np = R.tolerance(x, q)
        assert e_np > 0.0 and tol >= 4.0 * e_np


def _impulses(n, seed, k=16):
    rng = np.random.default_rng(seed)
    pos = rng.choice(n, size=min(k, n), replace=False)
    amp = rng.integers(-30000, 30001, size=pos.size).astype(np.float64)
    amp[amp == 0] = 1.0
    return pos, amp


@pytest.mark.parametrize("n", [3, 50, 1000, 1024, 4097])
def test_impulse_closed_form_equals_the_long_double_transform(n):
    """impulse_q at every frame against hilbert_q of the same sparse track, within the long-double transform's
    own rounding: 64-bit significands, log2(P) stages"""
    pos, amp = _impulses(n, 300 + n)
    x = R.impulse_track(n, pos, amp)
    assert np.count_nonzero(x) == pos.size
    q = R.hilbert_q(x)
    q_cf = R.impulse_q(n, pos, amp, np.arange(n))
    assert q_cf.dtype == np.longdouble and q_cf.shape == (n,)
    peak = float(np.max(np.abs(q)))
    assert peak > 0.0
    err = float(np.max(np.abs(q_cf - q)))
    assert err <= 2.0 ** -60 * np.log2(R.pad_len(n)) * peak, (err, peak)


def test_impulse_closed_form_two_points_is_zero():
    assert not R.impulse_q(2, [0, 1], [123.0, -77.0], [0, 1]).any()


def test_impulses_at_even_distances_contribute_exactly_nothing():
    n, probe = 1000, 333
    pos = np.array([333, 1, 335, 999, 331, 35])              # every distance to the probe is even (0 included)
    amp = np.array([30000.0, -30000.0, 12345.0, -1.0, 777.0, 29999.0])
    assert R.impulse_q(n, pos, amp, [probe])[0] == 0
    # across the wrap of the padded length: d = (2 - 998) mod 1024 = 28
    assert R.impulse_q(n, [998], [30000.0], [2])[0] == 0
    # and one odd distance does contribute, with the sign of cot: the frame after a positive impulse is positive
    assert R.impulse_q(n, pos, amp, [probe + 1])[0] != 0
    assert R.impulse_q(n, [10], [1.0], [11])[0] > 0 > R.impulse_q(n, [10], [1.0], [9])[0]


@pytest.mark.parametrize("n", [1000, 4097])
def test_impulse_tolerance_is_tolerance_over_the_probes(n):
    pos, amp = _impulses(n, 500 + n)
    x = R.impulse_track(n, pos, amp)
    at = np.arange(n)
    q_cf = R.impulse_q(n, pos, amp, at)
    bound, e_np = R.impulse_tolerance(n, pos, amp, at, q_cf)
    bound_fft, e_fft = R.tolerance(x, R.hilbert_q(x))
    # the two references agree to 2^-60 log2(P) max|Q|, far below e_np, so the two bounds agree to that
    slack = 4 * 2.0 ** -60 * np.log2(R.pad_len(n)) * float(np.max(np.abs(q_cf)))
    assert e_np > 0.0 and abs(e_np - e_fft) <= slack and abs(bound - bound_fft) <= 4 * slack
    assert bound == max(4.0 * e_np, 2.0 ** -52 * np.log2(R.pad_len(n)) * float(np.max(np.abs(q_cf))))
    # over a subset of the frames e_np can only shrink, and a precomputed numpy transform gives the same pair
    sub = at[::7]
    b2, e2 = R.impulse_tolerance(n, pos, amp, sub, q_cf[::7], q_np=R.hilbert_q_np(x))
    assert e2 <= e_np and (b2, e2) == R.impulse_tolerance(n, pos, amp, sub, q_cf[::7])


def test_two_frames_have_no_quadrature():
    assert not R.hilbert_q(np.array([123.0, -77.0])).any()


@pytest.mark.parametrize("p,k", [(64, 5), (4096, 37)])
def test_single_bin_cosine_gives_the_sine(p, k):
    n = np.arange(p)
    theta = 2 * R.PI * (np.asarray(n * k % p, dtype=np.longdouble) / p)
    x = (20000 * np.cos(theta)).astype(np.float64)
    q = R.hilbert_q(x)
    # x is the cosine rounded to double: its rounding error (half an ulp of 20000 per sample) passes through
    assert float(np.max(np.abs(q - 20000 * np.sin(theta)))) < 2.0 ** -52 * 20000 * np.log2(p)

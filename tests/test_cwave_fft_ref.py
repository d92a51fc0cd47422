"""CPU: pins tests/cwfft_ref.py, the long-double restatement of the direct-FFT converter's definition
(include/icw_cwave.h: icw_encode_cwave_fft), before a GPU test uses it: against scipy.signal.hilbert, against
the same formula through numpy.fft in float64, and on a single-bin cosine.  The GPU tolerance is built on
numpy.fft's deviation from the long-double result, so that deviation is checked to be non-zero here."""
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

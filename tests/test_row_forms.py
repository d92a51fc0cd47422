"""The row IIR's term blocks in the form the include carries them (in_cwave_amd/csrc/icw_row_asm.inc):
tools/gen_row_asm.py emits the compensation update NC = NC - D as the VOP2 `v_fmac_f64 NC, -1.0, D`
(tools/row_form_probe.hip, profiles/r15_row_form_probe.txt: the one encoding that makes the block
cheaper).  tests/test_row_asm.py interprets the generator's plain v_add_f64 lines; this file
interprets the emitted text of the include itself, every (order, first term) block of it:
  - against the plain Kahan sum of iir_rp_process_kahan (hblpf.c:1027-1044): equal up to the sign of
    an exact zero, and the same reject decision |S| < 1 (hblpf.c:1046);
  - against the generator's plain lines, register for register and bit for bit, zero signs included.
    The two interpreters differ where the forms differ: v_add_f64 is one IEEE addition, v_fmac_f64 is a
    fused multiply-add evaluated exactly in rationals and rounded once (_fma), with the zero-sign rules
    of IEEE 754 6.3 -- so the comparison fails if -1.0 * D + NC were not the rounding of NC - D.
Inputs: random terms; terms that make every compensation an exact zero, of either sign (integers,
+0.0 and -0.0 terms); sums that land one ulp under and over 1.0 only through the compensation."""
import functools
import importlib.util
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
INC = ROOT / "in_cwave_amd" / "csrc" / "icw_row_asm.inc"
ORDERS = (15, 18, 19, 20)


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("gen_row_asm", ROOT / "tools" / "gen_row_asm.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _blocks():
    """{(N, I0): asm lines} as the include carries them"""
    out, key = {}, None
    for ln in INC.read_text().splitlines():
        m = re.search(r"\(N == (\d+) && I0 == (\d+)\)", ln)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            out[key] = []
            continue
        m = re.match(r'\s+"(v_\S+ .*)\\n"$', ln)
        if m and key:
            out[key].append(m.group(1))
    return out


BLOCKS = _blocks()
F = np.float64


def _bits(v):
    return np.array([v], dtype=np.float64).view(np.uint64)[0]


def _fma(a, b, c):
    """round(a * b + c) with one rounding, finite operands: the exact rational result converted once
    (int / int true division rounds to nearest even); an exact zero takes IEEE 754's sign: the common
    sign when the product and the addend are zeros of one sign, else +0 (round to nearest)"""
    a, b, c = float(a), float(b), float(c)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact != 0:
        return F(exact.numerator / exact.denominator)
    prod_neg = (np.signbit(a) != np.signbit(b))
    if a * b == 0.0 and c == 0.0 and prod_neg == bool(np.signbit(c)):
        return F(-0.0) if prod_neg else F(0.0)
    return F(0.0)


def _interp(lines, i0, S, NC, T, prod_of):
    """operands %0 S, %1 NC, %2 T, %3 D, (I0 = 0) %4 R, then `one` and the products; returns the
    register file after every instruction (the trace) -- all arithmetic in IEEE double, one rounding
    per instruction"""
    one, base = (5, 6) if i0 == 0 else (4, 5)
    r = {0: F(S), 1: F(NC), 2: F(T), 3: F(0.0), one: F(1.0)}
    if i0 == 0:
        r[4] = F(0.0)
    trace = []
    for ln in lines:
        m = re.fullmatch(r"v_fmac_f64_dpp %(\d+), %(\d+), %(\d+) row_newbcast:(\d+) row_mask:0xf bank_mask:0xf", ln)
        if m:
            d, src, o, lane = (int(g) for g in m.groups())
            assert o == one and src >= base
            r[d] = _fma(prod_of(src - base, lane), 1.0, r[d])
        else:
            m = re.fullmatch(r"v_fmac_f64 %(\d+), -1\.0, %(\d+)", ln)
            if m:
                d, b = int(m.group(1)), int(m.group(2))
                r[d] = _fma(-1.0, r[b], r[d])
            else:
                m = re.fullmatch(r"v_add_f64 %(\d+), %(\d+), (-?)%(\d+)", ln)
                assert m, ln
                d, a, neg, b = int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4))
                r[d] = r[a] + (-r[b] if neg else r[b])
        trace.append((d, _bits(r[d])))
    return r, trace


def _kahan(x, t, i0):
    """hblpf.c:1027-1044; a zero-input step (I0 = 2) starts from S = t0, C = +0"""
    S, C = (F(x), F(0.0)) if i0 != 2 else (F(t[0]), F(0.0))
    for i in (range(0, len(t)) if i0 != 2 else range(1, len(t))):
        Y = F(t[i]) - C
        T = S + Y
        C = (T - S) - Y
        S = T
    return S


def _run(lines, n, i0, x, t):
    def prod(q, lane):
        i = q if i0 == 0 else (1 if i0 == 1 else 2) + q
        assert lane == ((n - 17) if i == 0 else (i - 1 if i - 1 < 16 else i - 17))
        return t[i]

    if i0 == 0:
        r, trace = _interp(lines, 0, x, 0.0, x, prod)
        return r[4], trace
    # the kernel's first step in plain code (icw_row_step), then the block from term I0
    S0, Y0 = (F(x), F(t[0])) if i0 == 1 else (F(t[0]), F(t[1]))
    T0 = S0 + Y0
    NC0 = Y0 - (T0 - S0)
    r, trace = _interp(lines, i0, T0, NC0, 0.0, prod)
    res = _gen().chain(n, i0)[2]
    return {"S": r[0], "T": r[2]}[res], trace


def _cases(n, rng):
    """(x, terms) lists: random; exact-zero compensations of both signs; sums around 1.0"""
    out = []
    for _ in range(40):
        out.append((rng.standard_normal() * 1e3, rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n))))
    # integers: every partial sum exact, every compensation +0
    out.append((3.0, rng.integers(-1000, 1000, n).astype(np.float64)))
    # zero terms of both signs between integers: Y = -0 + NC keeps a -0 compensation alive
    for sign in (0.0, -0.0):
        t = rng.integers(-50, 50, n).astype(np.float64)
        t[::2] = sign
        out.append((5.0, t))
        out.append((-0.0, np.full(n, sign)))            # a sum that stays zero
        out.append((0.0, np.full(n, sign)))
    t = np.zeros(n); t[1::3] = -0.0; t[2::3] = 7.0
    out.append((-7.0 * np.count_nonzero(t == 7.0), t))      # cancels to an exact zero at the end
    # one ulp over 1.0 only through the compensation (1 + 2^-53 + 2^-53), and one ulp under
    for tiny, start in ((2.0 ** -53, 1.0), (-(2.0 ** -54), 1.0), (2.0 ** -53, -1.0), (-(2.0 ** -54), -1.0)):
        for pos in ((1, 2), (n - 2, n - 1), (2, n - 1)):
            t = np.zeros(n); t[pos[0]] = tiny * np.sign(start); t[pos[1]] = tiny * np.sign(start)
            out.append((start, t))            # nonzero-input steps: x carries the 1.0
            t2 = t.copy(); t2[0] = start
            out.append((0.0, t2))             # zero-input steps: t0 carries it
    return out


@pytest.mark.parametrize("n", ORDERS)
def test_every_block_is_in_the_include(n):
    for i0 in ((0, 1, 2) if n > 17 else (1, 2)):
        lines = BLOCKS[(n, i0)]
        assert len(lines) == len(_gen().chain(n, i0)[0])
        # one VOP2 compensation update per full term, none of the VOP3 form left
        assert not [l for l in lines if re.fullmatch(r"v_add_f64 %1, %1, -%3", l)]
        assert sum(l.startswith("v_fmac_f64 ") for l in lines) == sum(
            l == "v_add_f64 %1, %1, -%3" for l in _gen().chain(n, i0)[0])
    assert sorted(k for k in BLOCKS if k[0] == n) == [(n, i0) for i0 in ((0, 1, 2) if n > 17 else (1, 2))]


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("i0", (0, 1, 2))
def test_emitted_block_equals_kahan_sum_and_plain_form(n, i0):
    if i0 == 0 and n <= 17:
        assert (n, 0) not in BLOCKS        # orders <= 17 have no spare product lane for t0
        return
    gen = _gen()
    plain = gen.chain(n, i0)[0]
    emitted = BLOCKS[(n, i0)]
    rng = np.random.default_rng(1000 * n + i0)
    seen_pos0 = seen_neg0 = seen_under = seen_over = False
    for x, t in _cases(n, rng):
        if i0 == 2:
            x = 0.0                         # zero-input parity: the literal +0.0 of hq_rp_process
        want = _kahan(x, t, i0)
        got, tr_e = _run(emitted, n, i0, x, t)
        got_p, tr_p = _run(plain, n, i0, x, t)
        assert got == want, (n, i0, x, t, got, want)            # == ignores only the sign of a zero
        assert (abs(got) < 1.0) == (abs(want) < 1.0)
        assert tr_e == tr_p, (n, i0, x, t)                      # every register write, bit for bit
        comp = [b for d, b in tr_e if d == 1]
        seen_pos0 |= any(b == 0 for b in comp)
        seen_neg0 |= any(b == 0x8000000000000000 for b in comp)
        seen_under |= 0.0 < abs(want) < 1.0 and abs(want) >= 1.0 - 2.0 ** -52
        seen_over |= 1.0 < abs(want) <= 1.0 + 2.0 ** -51
    # the inputs did what they were built for
    assert seen_pos0 and seen_neg0 and seen_under and seen_over

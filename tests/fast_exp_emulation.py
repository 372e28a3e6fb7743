"""Bit-level emulation of exp_nonpos_tab (tapir_amd/csrc/fast_exp.hpp) in Python, for tests that must know what the
kernel's exponential returns at a given argument: which branch lengths reach its edges, and that the clamp at -1e4
changes nothing above the band where the unclamped version wrapped.  Every fma is rounded once (exact rational
arithmetic, then one rounding to the nearest double), as v_fma_f64 does."""
import math
import struct
from fractions import Fraction

import mpmath

INV = 92.33248261689366
L_HI = 0.01083042469326756
L_LO = 2.9815858269852933e-12
SHIFT = 6755399441055744.0
C5, C4, C3 = 8.333333333333333e-03, 4.1666666666666664e-02, 1.6666666666666666e-01
CLAMP = -1.0e4
WRAP = -(2.0 ** 31) / INV     # below this the unclamped k = 64 n + j no longer fits 32 bits (-2.33e7)

with mpmath.workdps(40):
    TABLE = [float(mpmath.power(2, mpmath.mpf(j) / 64)) for j in range(64)]


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exp_nonpos_tab(x, clamp=True):
    """exp_nonpos_tab(x) as the kernel computes it; clamp=False: the version before the clamp (which returned +inf or 0
    in alternating bands below WRAP)."""
    if clamp:
        x = max(x, CLAMP)
    t = _fma(x, INV, SHIFT)
    kd = t - SHIFT
    r = _fma(-kd, L_HI, x)
    r = _fma(-kd, L_LO, r)
    k = struct.unpack("<q", struct.pack("<d", t))[0] & 0xFFFFFFFF
    k = k - (1 << 32) if k >= (1 << 31) else k           # the low 32 bits as a signed int
    T = TABLE[k & 63]
    q = _fma(r, C5, C4)
    q = _fma(q, r, C3)
    q = _fma(q, r, 0.5)
    q = _fma(q, r, 1.0)
    q = q * r
    p = _fma(T, q, T)
    try:
        return math.ldexp(p, k >> 6)
    except OverflowError:
        return math.inf

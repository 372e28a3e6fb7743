"""References for the exact quartet resolution probabilities.  Test helper, no GPU.

  window_rule     the smallest M in 16, 32, ..., cap whose Bernstein bound on the mass outside the windows meets the tolerance
  moments         the three means and variances of D1 = S - N1, D2 = S - N2, E = D2 - D1 (math.fsum)
  resolution      the numpy restatement of the formulas: the characteristic function on the M x M torus, summed against the
                  separable weights of the three regions (all M^2 frequencies, weights by direct summation: it shares
                  neither the half spectrum nor the closed-form weights of the kernels)
  windowed_dp     the dynamic programme of quartet_reference.exact_resolution on a moving window, for loci of any length;
                  returns the mass it lost
"""
import math

import numpy as np

MIN_WINDOW, MAX_WINDOW, DEFAULT_WINDOW, DEFAULT_TAIL = 16, 512, 128, 1e-12


def tail_bound(variances, M):
    """sum over the three variances of 2 exp(-t^2 / (2 (V + t / 3))), t = M / 2 - 1; a variance of 0 adds nothing"""
    t = M // 2 - 1
    return sum(2.0 * math.exp(-(t * t) / (2.0 * (v + t / 3.0))) for v in variances if v > 0.0)


def window_rule(variances, cap=DEFAULT_WINDOW, tol=DEFAULT_TAIL):
    """(M, bound): the smallest M in 16, 32, ..., cap with tail_bound <= tol; (0, the bound at the cap) when there is none"""
    M, b = MIN_WINDOW, 0.0
    while M <= cap:
        b = tail_bound(variances, M)
        if b <= tol:
            return M, b
        M *= 2
    return 0, b


def moments(y, x1, x2):
    """means (E D1, E D2, E E) and variances (Var D1, Var D2, Var E)"""
    y, x1, x2 = (np.asarray(v, dtype=np.float64) for v in (y, x1, x2))
    fs = lambda v: math.fsum(np.asarray(v).tolist())  # noqa: E731
    means = (fs(y - x1), fs(y - x2), fs(x1 - x2))
    var = tuple(fs(np.maximum(0.0, (p + m) - (p - m) ** 2)) for p, m in ((y, x1), (y, x2), (x1, x2)))
    return means, var


def _weights(c, M, positive):
    """w[k] = sum over d in [c - M/2, c + M/2) with d > 0 (or d < 0) of exp(-2 pi i k d / M), by direct summation"""
    d = np.arange(c - M // 2, c + M // 2)
    d = d[d > 0] if positive else d[d < 0]
    k = np.arange(M)
    ang = -2.0 * np.pi * ((k[:, None] * d[None, :]) % M) / M
    return np.exp(1j * ang).sum(axis=1) if d.size else np.zeros(M, dtype=np.complex128)


def resolution(y, x1, x2, cap=DEFAULT_WINDOW, tol=DEFAULT_TAIL):
    """(p_correct, p_ac, p_ad, p_polytomy, M, tail_bound); NaN probabilities and M = 0 when no window up to the cap will do"""
    y, x1, x2 = (np.asarray(v, dtype=np.float64) for v in (y, x1, x2))
    means, var = moments(y, x1, x2)
    M, bound = window_rule(var, cap, tol)
    if M == 0:
        return (math.nan,) * 4 + (0, bound)
    c1, c2, ce = (int(round(m)) for m in means)
    if var == (0.0, 0.0, 0.0):     # a point law: read off the centres
        pc, p1, p2 = float(c1 > 0 and c2 > 0), float(c1 < 0 and c1 < c2), float(c2 < 0 and c2 < c1)
        return pc, p1, p2, 1.0 - pc - p1 - p2, M, bound
    k = np.arange(M)
    z = np.exp(2j * np.pi * k / M)
    z1, z2 = z[:, None], z[None, :]
    phi = np.ones((M, M), dtype=np.complex128)
    for yi, ai, bi in zip(y.tolist(), x1.tolist(), x2.tolist()):
        if yi == 0.0 and ai == 0.0 and bi == 0.0:
            continue
        phi *= (1.0 - yi - ai - bi) + yi * z1 * z2 + ai * np.conj(z1) + bi * np.conj(z2)
    a1, a2 = _weights(c1, M, True), _weights(c2, M, True)
    b1, b2 = _weights(c1, M, False), _weights(c2, M, False)
    e, f = _weights(ce, M, True), _weights(-ce, M, True)
    j12 = (k[:, None] + k[None, :]) % M
    pc = float(np.sum(phi * a1[:, None] * a2[None, :]).real) / M ** 2
    p1 = float(np.sum(phi * b1[j12] * e[None, :]).real) / M ** 2
    p2 = float(np.sum(phi * b2[j12] * f[:, None]).real) / M ** 2
    pc, p1, p2 = (min(1.0, max(0.0, v)) for v in (pc, p1, p2))
    return pc, p1, p2, max(0.0, 1.0 - pc - p1 - p2), M, bound


def windowed_dp(y, x1, x2, half=96):
    """(p_correct, p_ac, p_ad, p_polytomy, lost): the law of (D1, D2) by dynamic programming on a (2 half + 1)^2 window that
    follows the running means; mass that steps over the window's edge, or is shifted out of it, is counted in `lost` (it
    belongs to no outcome, so every probability is low by at most `lost`).  p_polytomy is the mass on the ties."""
    y, x1, x2 = (np.asarray(v, dtype=np.float64) for v in (y, x1, x2))
    size = 2 * half + 1
    P = np.zeros((size, size))
    P[half, half] = 1.0
    o1 = o2 = 0                      # the window's centre: cell [i, j] is (D1, D2) = (o1 + i - half, o2 + j - half)
    m1 = m2 = 0.0
    for yi, ai, bi in zip(y.tolist(), x1.tolist(), x2.tolist()):
        Q = (1.0 - yi - ai - bi) * P
        Q[1:, 1:] += yi * P[:-1, :-1]
        Q[:-1, :] += ai * P[1:, :]
        Q[:, :-1] += bi * P[:, 1:]
        P = Q
        m1 += yi - ai
        m2 += yi - bi
        s1, s2 = int(round(m1)) - o1, int(round(m2)) - o2
        if s1 or s2:
            R = np.zeros_like(P)
            src1 = slice(max(0, s1), size + min(0, s1))
            dst1 = slice(max(0, -s1), size + min(0, -s1))
            src2 = slice(max(0, s2), size + min(0, s2))
            dst2 = slice(max(0, -s2), size + min(0, -s2))
            R[dst1, dst2] = P[src1, src2]
            P = R
            o1 += s1
            o2 += s2
    D1 = (o1 + np.arange(size) - half)[:, None]
    D2 = (o2 + np.arange(size) - half)[None, :]
    pc = float(P[(D1 > 0) & (D2 > 0)].sum())
    p1 = float(P[(D1 < 0) & (D1 < D2)].sum())
    p2 = float(P[(D2 < 0) & (D2 < D1)].sum())
    kept = float(P.sum())
    return pc, p1, p2, kept - pc - p1 - p2, max(0.0, 1.0 - kept)

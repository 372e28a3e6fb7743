"""References for quartet signal and noise with unequal tips.  Test helper, no GPU.

  twin_site          mpmath, good to 40 digits: the five matrices from mpmath.expm of Q r tau / kappa, (y, x1, x2) by brute-force
                     enumeration of all 256 tip patterns of ((a:Ta, b:Tb), (c:Tc, d:Td))
  site_values        the fp64 numpy restatement of the definition (the matrices of quartet_reference.transition), sums of
                     products of matrix entries only
  locus_sums         the nine sums with math.fsum
  bvn_upper,         the bivariate-normal rule of section 3.8: the integrand without cancellation where h != k, the clamps
  probabilities
  bvn_mp             mpmath's quadrature of the same integral at 30 digits
  exact_resolution   the exact distribution of (S - N1, S - N2) by dynamic programming with separate x1, x2, loci of at most
                     60 sites
"""
import math

import numpy as np

import quartet_reference as qr

SUMS = ("Y", "X1", "X2", "Yy", "X1x1", "X2x2", "YX1", "YX2", "X1X2")


# ---- the 40-digit twin ---------------------------------------------------------------------------------------------
def twin_site(Qhat, p, r, tips, internode):
    """(y, x1, x2) of one site at 40 digits: the probabilities of the tip patterns iijj, ijij and ijji (i != j), summed over
    all 256 patterns and both internal states."""
    import mpmath as mp
    r = mp.mpf(float(r))
    A, B, C, D = (mp.expm(Qhat * (r * mp.mpf(float(t)))) if t != 0 else mp.eye(4) for t in tips)
    N = mp.expm(Qhat * (r * mp.mpf(float(internode))))
    left = [[[A[u, a] * B[u, b] for b in range(4)] for a in range(4)] for u in range(4)]
    right = [[[sum(N[u, v] * C[v, c] * D[v, d] for v in range(4)) for d in range(4)] for c in range(4)] for u in range(4)]
    y = x1 = x2 = total = mp.mpf(0)
    for a in range(4):
        for b in range(4):
            for c in range(4):
                for d in range(4):
                    pr = sum(p[u] * left[u][a][b] * right[u][c][d] for u in range(4))
                    total += pr
                    if a == b and c == d and a != c:
                        y += pr
                    if a == c and b == d and a != b:
                        x1 += pr
                    if a == d and b == c and a != b:
                        x2 += pr
    assert abs(total - 1) < mp.mpf(10) ** -40
    return y, x1, x2


def twin_values(pi, exch, rates, tips, internode):
    """twin_site over a vector of final rates: three lists of mpf; a NaN or zero rate gives exact zeros.  Worked at 80 digits
    (as quartet_reference.twin_values)."""
    import mpmath as mp
    with mp.workdps(80):
        Qhat, p = qr.twin_generator(pi, exch)
        out = ([], [], [])
        for r in np.asarray(rates, dtype=np.float64).tolist():
            v = (mp.mpf(0),) * 3 if (not math.isfinite(r) or r == 0.0) else twin_site(Qhat, p, r, tips, internode)
            for o, w in zip(out, v):
                o.append(w)
        return out


# ---- the fp64 restatement ------------------------------------------------------------------------------------------
_NEQ = 1.0 - np.eye(4)


def site_values(model, pi, exch, rates, tips, internode):
    """(y [n], x1 [n], x2 [n]) in fp64 by the definition's formulas; NaN and zero rates give exactly 0."""
    r = np.asarray(rates, dtype=np.float64)
    live = np.isfinite(r) & (r != 0.0)
    y, x1, x2 = np.zeros(r.size), np.zeros(r.size), np.zeros(r.size)
    if live.any():
        p = np.asarray(pi, dtype=np.float64)
        p = p / p.sum()
        A, B, C, D = (qr.transition(model, pi, exch, r[live], t) for t in tips)
        N = qr.transition(model, pi, exch, r[live], internode)
        R = np.einsum("nuv,nvi,nvj->nuij", N, C, D)                       # R_u[i][j] = sum_v N_uv C_vi D_vj
        diag = np.einsum("nujj->nuj", R)
        y[live] = np.einsum("u,nui,nui,nuj,ij->n", p, A, B, diag, _NEQ)
        x1[live] = np.einsum("u,nui,nuj,nuij,ij->n", p, A, B, R, _NEQ)
        x2[live] = np.einsum("u,nui,nuj,nuji,ij->n", p, A, B, R, _NEQ)
    return y, x1, x2


def locus_sums(y, x1, x2):
    """[Y, X1, X2, Yy, X1x1, X2x2, YX1, YX2, X1X2] with math.fsum"""
    y, x1, x2 = (np.asarray(v, dtype=np.float64) for v in (y, x1, x2))
    return np.array([math.fsum(v.tolist()) for v in (y, x1, x2, y * y, x1 * x1, x2 * x2, y * x1, y * x2, x1 * x2)])


# ---- the probability rule ------------------------------------------------------------------------------------------
_GLX, _GLW = np.polynomial.legendre.leggauss(64)


def _bvn_integrand(h, k, theta):
    s = np.sin(theta)
    if h == k:
        return np.exp(-(k * k) / (1.0 + s))
    c = np.cos(theta)
    d = h - k
    return np.exp(-((d * d) / (2.0 * c * c) + (h * k) / (1.0 + s)))


def bvn_upper(h, k, rho):
    """B(h, k, rho) = P(Z1 > h, Z2 > k) by the 64-point Gauss-Legendre rule in theta; rho already clamped"""
    half = 0.5 * math.asin(rho)
    integral = half * float(np.sum(_GLW * _bvn_integrand(h, k, half + half * _GLX)))
    return max(0.0, qr._phi_upper(h) * qr._phi_upper(k) + integral / (2.0 * math.pi))


def bvn_mp(h, k, rho):
    """The same probability with mpmath's adaptive quadrature of the same integral at 30 digits."""
    import mpmath as mp
    with mp.workdps(30):
        h, k, rho = mp.mpf(float(h)), mp.mpf(float(k)), mp.mpf(float(rho))
        if h == k:
            f = lambda t: mp.exp(-(k * k) / (1 + mp.sin(t)))   # noqa: E731
        else:
            f = lambda t: mp.exp(-((h * h + k * k) - 2 * h * k * mp.sin(t)) / (2 * mp.cos(t) ** 2))   # noqa: E731
        a = mp.asin(rho)
        integral = mp.quad(f, mp.linspace(0, a, 9))
        return float(mp.ncdf(-h) * mp.ncdf(-k) + integral / (2 * mp.pi))


def clamp_rho(h, k, rho, cap):
    rho = min(1.0, max(-1.0, rho))
    if h != k:
        rho = min(cap, max(-0.999, rho))
    return rho


def _win_arguments(eW, eO1, eO2, vW, vO1, vO2, w_o1, w_o2, o1_o2, cap):
    """(h, k, rho~) of the probability that W ends ahead of O1 and O2, or None where it is 0 by definition"""
    s1 = (vW + vO1) + 2.0 * w_o1
    s2 = (vW + vO2) + 2.0 * w_o2
    if not s1 > 0.0 or not s2 > 0.0:
        return None
    h = (0.5 - (eW - eO1)) / math.sqrt(s1)
    k = (0.5 - (eW - eO2)) / math.sqrt(s2)
    rho = ((vW + (w_o1 + w_o2)) - o1_o2) / math.sqrt(s1 * s2)
    return h, k, clamp_rho(h, k, rho, cap)


def probability_arguments(sums):
    """The three (h, k, rho~) triples (or None) behind p_correct, p_ac, p_ad"""
    Y, X1, X2, Yy, X11, X22, YX1, YX2, X12 = (float(v) for v in sums)
    vS, v1, v2 = Y - Yy, X1 - X11, X2 - X22
    return [_win_arguments(Y, X1, X2, vS, v1, v2, YX1, YX2, X12, 0.999),
            _win_arguments(X1, Y, X2, v1, vS, v2, YX1, X12, YX2, 0.99) if X1 > 0.0 else None,
            _win_arguments(X2, Y, X1, v2, vS, v1, YX2, X12, YX1, 0.99) if X2 > 0.0 else None]


def probabilities(sums):
    """(p_correct, p_ac, p_ad, p_polytomy) from the nine sums"""
    pc, p1, p2 = (0.0 if a is None else bvn_upper(*a) for a in probability_arguments(sums))
    return pc, p1, p2, max(0.0, ((1.0 - pc) - p1) - p2)


def rows(model, pi, exch, rates, quartets):
    """[n_q, 13] rows of one locus by the restatement: the nine sums and the four probabilities."""
    quartets = np.asarray(quartets, dtype=np.float64).reshape(-1, 5)
    out = np.zeros((len(quartets), 13))
    for q, row in enumerate(quartets.tolist()):
        out[q, :9] = locus_sums(*site_values(model, pi, exch, rates, row[:4], row[4]))
        out[q, 9:] = probabilities(out[q, :9])
    return out


# ---- the exact distribution ----------------------------------------------------------------------------------------
def exact_resolution(y, x1, x2):
    """(p_correct, p_ac, p_ad, p_polytomy) exactly: every site is a signal site (y_i), a noise site of the first (x1_i) or
    of the second kind (x2_i) or none; D1 = S - N1, D2 = S - N2.  Correct: D1 > 0 and D2 > 0; ac: N1 strictly ahead of both
    others (D1 < 0 and D1 < D2); ad: N2 strictly ahead (D2 < 0 and D2 < D1); polytomy: the rest (ties)."""
    y, x1, x2 = (np.asarray(v, dtype=np.float64) for v in (y, x1, x2))
    n = y.size
    assert n <= 60
    size = 2 * n + 1
    P = np.zeros((size, size))
    P[n, n] = 1.0
    for yi, ai, bi in zip(y.tolist(), x1.tolist(), x2.tolist()):
        Q = (1.0 - yi - ai - bi) * P
        Q[1:, 1:] += yi * P[:-1, :-1]        # (+1, +1)
        Q[:-1, :] += ai * P[1:, :]           # (-1, 0)
        Q[:, :-1] += bi * P[:, 1:]           # (0, -1)
        P = Q
    d = np.arange(size) - n
    D1, D2 = d[:, None], d[None, :]
    pc = float(P[(D1 > 0) & (D2 > 0)].sum())
    p1 = float(P[(D1 < 0) & (D1 < D2)].sum())
    p2 = float(P[(D2 < 0) & (D2 < D1)].sum())
    return pc, p1, p2, 1.0 - pc - p1 - p2

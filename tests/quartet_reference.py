"""References for the quartet signal and noise stage.  Test helper, no GPU.

  twin_site          mpmath, good to 40 digits: M and N from mpmath.expm of Q r tau / kappa built from pi and the exchangeabilities
                     directly (no eigen-system), y and x by brute-force enumeration of all 256 tip patterns
  site_values        the fp64 numpy restatement of the definition: eigen-system from numpy.linalg.eigh on the symmetrised
                     generator, the expm1 form, sums of non-negative terms (F81: the closed form)
  locus_sums         the five sums with math.fsum
  bvn_upper,         the bivariate-normal approximation with continuity correction, 64-point Gauss-Legendre
  probabilities
  bvn_scipy, bvn_mp  the same probability from scipy.stats.multivariate_normal, and from mpmath's quadrature at 30 digits
  exact_resolution   the exact distribution of (S - N1, S - N2) by dynamic programming, loci of at most 60 sites
"""
import math

import numpy as np

PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]   # AC AG AT CG CT GT


# ---- the 40-digit twin ---------------------------------------------------------------------------------------------
def twin_generator(pi, exch):
    """Q / kappa as an mpmath matrix: Q_ij = r_ij pi_j, rows summing to zero, kappa = sum_i pi_i (-Q_ii); pi normalised."""
    import mpmath as mp
    p = [mp.mpf(float(v)) for v in pi]
    tot = sum(p)
    p = [v / tot for v in p]
    R = [[mp.mpf(0)] * 4 for _ in range(4)]
    for (i, j), e in zip(PAIRS, exch):
        R[i][j] = R[j][i] = mp.mpf(float(e))
    Q = mp.zeros(4, 4)
    for i in range(4):
        for j in range(4):
            if i != j:
                Q[i, j] = R[i][j] * p[j]
        Q[i, i] = -sum(Q[i, j] for j in range(4) if j != i)
    kappa = sum(p[i] * -Q[i, i] for i in range(4))
    return Q / kappa, p


def twin_site(Qhat, p, r, tip, internode):
    """(y, x_ijij, x_ijji) of one site at 40 digits: the probabilities of the tip patterns iijj, ijij and ijji (i != j) of
    ((a, b), (c, d)), summed over all 256 patterns and both internal states."""
    import mpmath as mp
    r = mp.mpf(float(r))
    M = mp.expm(Qhat * (r * mp.mpf(float(tip)))) if tip != 0 else mp.eye(4)
    N = mp.expm(Qhat * (r * mp.mpf(float(internode))))
    # P(a, b, c, d) = sum_u pi_u (M_ua M_ub) sum_v N_uv (M_vc M_vd): the two brackets once per (u, pair), then all 256 patterns
    left = [[[M[u, a] * M[u, b] for b in range(4)] for a in range(4)] for u in range(4)]
    right = [[[sum(N[u, v] * M[v, c] * M[v, d] for v in range(4)) for d in range(4)] for c in range(4)] for u in range(4)]
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
    assert abs(total - 1) < mp.mpf(10) ** -40          # the 256 patterns are a distribution, to the 40 digits promised
    return y, x1, x2


def twin_values(pi, exch, rates, tip, internode):
    """twin_site over a vector of final rates: three lists of mpf; a NaN or zero rate gives exact zeros.  Worked at 80
    digits so that 40 survive the squarings of expm at r tau up to 1e7 (twin_site checks that the patterns sum to 1)."""
    import mpmath as mp
    with mp.workdps(80):
        Qhat, p = twin_generator(pi, exch)
        out = ([], [], [])
        for r in np.asarray(rates, dtype=np.float64).tolist():
            v = (mp.mpf(0),) * 3 if (not math.isfinite(r) or r == 0.0) else twin_site(Qhat, p, r, tip, internode)
            for o, w in zip(out, v):
                o.append(w)
        return out


def relative_error(got, ref):
    """max |got - ref| / ref over the entries with ref != 0 (mpf arithmetic), and whether every ref == 0 entry came back 0."""
    import mpmath as mp
    worst, zeros_ok = 0.0, True
    with mp.workdps(40):
        for g, w in zip(np.asarray(got, dtype=np.float64).tolist(), ref):
            if w == 0:
                zeros_ok = zeros_ok and g == 0.0
            else:
                worst = max(worst, float(abs(mp.mpf(g) - w) / w))
    return worst, zeros_ok


# ---- the fp64 restatement ------------------------------------------------------------------------------------------
def eigen_system(pi, exch):
    """lam [3], U [4, 3], Ui [3, 4], pi [4] (normalised), kappa: the three non-zero eigen-pairs of Q through
    numpy.linalg.eigh on S = D^1/2 Q D^-1/2 (D = diag(pi))."""
    p = np.asarray(pi, dtype=np.float64)
    p = p / p.sum()
    R = np.zeros((4, 4))
    for (i, j), e in zip(PAIRS, exch):
        R[i, j] = R[j, i] = e
    Q = R * p[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    kappa = float(np.sum(p * -np.diag(Q)))
    sq = np.sqrt(p)
    S = sq[:, None] * Q / sq[None, :]
    S = 0.5 * (S + S.T)
    lam, V = np.linalg.eigh(S)
    keep = [k for k in range(4) if k != int(np.argmax(lam))]
    return lam[keep], (V / sq[:, None])[:, keep], (V * sq[:, None]).T[keep, :], p, kappa


def transition(model, pi, exch, rates, tau):
    """P(tau) per site, [n, 4, 4]: I + sum_k U[:,k] expm1(lam_k r tau / kappa) U^-1[k,:]; model "f81": e I + (1 - e) Pi with
    1 - e = -expm1(-r tau / kappa), kappa = 1 - sum pi^2."""
    r = np.asarray(rates, dtype=np.float64)
    if model == "f81":
        p = np.asarray(pi, dtype=np.float64)
        p = p / p.sum()
        kappa = 1.0 - float(np.sum(p * p))
        ome = -np.expm1(-(r * tau / kappa))
        return (1.0 - ome)[:, None, None] * np.eye(4)[None] + ome[:, None, None] * p[None, None, :]
    lam, U, Ui, p, kappa = eigen_system(pi, exch)
    em = np.expm1(lam[None, :] * (r * tau / kappa)[:, None])              # [n, 3]
    return np.eye(4)[None] + np.einsum("ik,nk,kj->nij", U, em, Ui)


_NEQ = 1.0 - np.eye(4)
_LT = np.triu(np.ones((4, 4)), 1)


def site_values(model, pi, exch, rates, tip, internode):
    """(y [n], x [n]) in fp64 by the definition's formulas; NaN and zero rates give exactly 0."""
    r = np.asarray(rates, dtype=np.float64)
    live = np.isfinite(r) & (r != 0.0)
    y, x = np.zeros(r.size), np.zeros(r.size)
    if live.any():
        p = np.asarray(pi, dtype=np.float64)
        p = p / p.sum()
        M = transition(model, pi, exch, r[live], tip)
        N = transition(model, pi, exch, r[live], internode)
        w = p[None, :, None] * N                                          # w_xy = pi_x N_xy
        M2 = M * M
        y[live] = np.einsum("nxy,nxi,nyj,ij->n", w, M2, M2, _NEQ)
        c = M[:, :, None, :] * M[:, None, :, :]                           # c[n, x, y, i] = M_xi M_yi
        x[live] = 2.0 * np.einsum("nxy,nxyi,nxyj,ij->n", w, c, c, _LT)
    return y, x


def locus_sums(y, x):
    """[Y, X, Yy, Xx, XY] with math.fsum"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.array([math.fsum(y.tolist()), math.fsum(x.tolist()), math.fsum((y * y).tolist()), math.fsum((x * x).tolist()),
                     math.fsum((x * y).tolist())])


_GLX, _GLW = np.polynomial.legendre.leggauss(64)


def _bvn_integrand(h, k, theta):
    s = np.sin(theta)
    if h == k:
        return np.exp(-(k * k) / (1.0 + s))
    c = np.cos(theta)
    return np.exp(-((h * h + k * k) - 2.0 * h * k * s) / (2.0 * c * c))


def _phi_upper(h):
    return 0.5 * math.erfc(h / math.sqrt(2.0))


def bvn_upper(h, k, rho):
    """B(h, k, rho) = P(Z1 > h, Z2 > k) = Phi(-h) Phi(-k) + (1 / 2 pi) int_0^{asin rho} ..., 64-point Gauss-Legendre in theta"""
    half = 0.5 * math.asin(min(1.0, max(-1.0, rho)))
    integral = half * float(np.sum(_GLW * _bvn_integrand(h, k, half + half * _GLX)))
    return max(0.0, _phi_upper(h) * _phi_upper(k) + integral / (2.0 * math.pi))   # (rho < 0: the two terms cancel; never below 0)


def bvn_scipy(h, k, rho):
    """The same probability from scipy (rho = 1: the distribution is singular, P(Z > max(h, k))).  Not for 1 - 1e-9 < |rho| < 1:
    scipy refuses such a matrix, or with allow_singular answers for |rho| = 1 (2e-7 away at rho = 1 - 1e-12): bvn_reference
    takes mpmath there."""
    from scipy.stats import multivariate_normal
    if rho >= 1.0:
        return _phi_upper(max(h, k))
    return float(multivariate_normal(mean=[0.0, 0.0], cov=[[1.0, rho], [rho, 1.0]]).cdf([-h, -k]))


def bvn_mp(h, k, rho):
    """The same probability with mpmath's adaptive quadrature of the same integral at 30 digits: a check of the 64-point rule
    that shares neither its nodes nor its arithmetic."""
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


def bvn_reference(h, k, rho):
    """scipy where it can be trusted, mpmath in the sliver next to |rho| = 1 where it cannot"""
    return bvn_mp(h, k, rho) if 1.0 - 1e-9 < abs(rho) < 1.0 else bvn_scipy(h, k, rho)


def probabilities(sums):
    """(p_correct, p_incorrect, p_polytomy) from [Y, X, Yy, Xx, XY]"""
    Y, X, Yy, Xx, XY = (float(v) for v in sums)
    var_s, var_n = Y - Yy, X - Xx
    sigma2 = (var_s + var_n) + 2.0 * XY
    if not sigma2 > 0.0:
        return 0.0, 0.0, 1.0
    sigma = math.sqrt(sigma2)
    k = (0.5 - (Y - X)) / sigma
    pc = bvn_upper(k, k, ((var_s + 2.0 * XY) - Xx) / sigma2)
    pw = 0.0
    if X > 0.0:
        pw = 2.0 * bvn_upper((0.5 - (X - Y)) / sigma, 0.5 / math.sqrt(2.0 * X), min(math.sqrt(X / 2.0) / sigma, 0.99))
    return pc, pw, max(0.0, (1.0 - pc) - pw)


def probability_arguments(sums):
    """The (h, k, rho) triples `probabilities` evaluates B at: [(k, k, rho_D)] and, when X > 0, the p_incorrect triple."""
    Y, X, Yy, Xx, XY = (float(v) for v in sums)
    var_s, var_n = Y - Yy, X - Xx
    sigma2 = (var_s + var_n) + 2.0 * XY
    if not sigma2 > 0.0:
        return []
    sigma = math.sqrt(sigma2)
    k = (0.5 - (Y - X)) / sigma
    out = [(k, k, min(1.0, max(-1.0, ((var_s + 2.0 * XY) - Xx) / sigma2)))]
    if X > 0.0:
        out.append(((0.5 - (X - Y)) / sigma, 0.5 / math.sqrt(2.0 * X), min(math.sqrt(X / 2.0) / sigma, 0.99)))
    return out


def rows(model, pi, exch, rates, quartets):
    """[n_q, 8] rows of one locus by the restatement: the five sums and the three probabilities."""
    out = np.zeros((len(quartets), 8))
    for q, (tip, internode) in enumerate(quartets):
        y, x = site_values(model, pi, exch, rates, tip, internode)
        out[q, :5] = locus_sums(y, x)
        out[q, 5:] = probabilities(out[q, :5])
    return out


# ---- the exact distribution ----------------------------------------------------------------------------------------
def exact_resolution(y, x):
    """(p_correct, p_incorrect, p_polytomy) exactly: every site is a signal site (probability y_i), a noise site for the one
    or for the other wrong topology (x_i each) or none; D1 = S - N1, D2 = S - N2.  Correct: D1 > 0 and D2 > 0; incorrect:
    one wrong topology strictly ahead of both others; polytomy: the rest (ties)."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n = y.size
    assert n <= 60
    size = 2 * n + 1
    P = np.zeros((size, size))
    P[n, n] = 1.0
    for yi, xi in zip(y.tolist(), x.tolist()):
        Q = (1.0 - yi - 2.0 * xi) * P
        Q[1:, 1:] += yi * P[:-1, :-1]        # (+1, +1)
        Q[:-1, :] += xi * P[1:, :]           # (-1, 0)
        Q[:, :-1] += xi * P[:, 1:]           # (0, -1)
        P = Q
    d = np.arange(size) - n
    D1, D2 = d[:, None], d[None, :]
    pc = float(P[(D1 > 0) & (D2 > 0)].sum())
    pw = float(P[(D1 < 0) & (D1 < D2)].sum() + P[(D2 < 0) & (D2 < D1)].sum())
    return pc, pw, 1.0 - pc - pw

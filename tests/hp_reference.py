"""Plain high-precision references for the site-likelihood and PI kernels (test helper, not a conftest).

Everything here is restated from the mathematics alone, in mpmath at DPS decimal digits.  It shares no code and no
formula arrangement with the kernels or with oracle/tapir_oracle.c: no Jacobi iteration, no rescaling, no rounding of
intermediate results to fp64, no QUADPACK restatement (the QUADPACK reference is scipy.integrate.quad itself, which is
what the reference program calls).

* Column log-likelihood f(u) = log L(s = e^u) of one alignment column, with g = df/du and h = d2f/du2, under GTR in
  HyPhy's parametrisation (Q_ij = r_ij pi_j for i != j, rows summing to 0, not normalised; the reported rate is
  kappa * s with kappa = sum_i pi_i (-Q_ii)) and under F81 (r_ij = 1, P(tau) = e I + (1 - e) Pi in closed form).
  P(tau) comes from mpmath's symmetric eigen-solver applied to D^1/2 Q D^-1/2, and the derivatives are analytic:
  d/du P(t e^u) = (Q tau) P, d2/du2 = (Q tau + (Q tau)^2) P.  Pruning is plain (mpmath's exponent range makes
  rescaling unnecessary).
* Whole-locus log-likelihood lnL = sum_c w_c log L_c at site rate 1 (stage 1's objective) with d lnL / d log t_b and
  d2 lnL / d (log t_b)^2 of any branch, analytic (the same three matrices, carried from the branch to the root past the stored
  sibling messages), and d lnL / d r_q of the six exchangeabilities by central differences inside mpmath at 60 digits with a
  relative step of 1e-18 (truncation and rounding both below 1e-30).
* One rate-class model of stage 1, phi(theta) = lnL(exch(theta), t = b / totalFactor(exch(theta))), with gradient and Hessian in the free
  log class rates by central differences at 60 digits (class_model_reference), and the 203 partitions, totalFactor and the Akaike
  weights written out from their definitions (rate_partitions, partition_classes, total_factor, akaike_weights).
* PI(t) = 16 r^2 t exp(-4 r t) and its exact integral G(4rb) - G(4ra), G(x) = -(1+x) exp(-x).
"""
import math

import mpmath
import numpy as np
from scipy import integrate

DPS = 40
mp = mpmath.mp
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))   # exchangeability order AC, AG, AT, CG, CT, GT
# A base composition far from uniform, shared by the deep-tree tests: a saturated rare base costs a partial 5.6 bits per tip.
SKEW_PI = [0.02, 0.02, 0.02, 0.94]
SKEW_EXCH = [1.0, 2.0, 0.5, 1.5, 3.0, 1.0]


def floored_pi(pi, floor=1e-12):
    """pi as a GTR plan floors it (an absent base gets floor * sum) and renormalised."""
    pi = np.asarray(pi, np.float64)
    p = np.maximum(pi, floor * pi.sum())
    return p / p.sum()


def rate_matrix(pi, exch, dps=None):
    """HyPhy's unnormalised GTR generator (mpmath matrix) and kappa.  Exchangeabilities that are already mpf are taken as
    they are (a relative step of 1e-18 must survive); anything else goes through float."""
    with mp.workdps(dps or DPS):
        pi = [mpmath.mpf(float(x)) for x in pi]
        tot = mpmath.fsum(pi)
        pi = [x / tot for x in pi]
        Q = mpmath.zeros(4, 4)
        for (i, j), r in zip(PAIRS, exch):
            r = r if isinstance(r, mpmath.mpf) else mpmath.mpf(float(r))
            Q[i, j] = r * pi[j]
            Q[j, i] = r * pi[i]
        for i in range(4):
            Q[i, i] = -mpmath.fsum(Q[i, j] for j in range(4) if j != i)
        kappa = -mpmath.fsum(pi[i] * Q[i, i] for i in range(4))
        return Q, pi, kappa


class _Model:
    """Transition matrices P(tau), dP/du, d2P/du2 (tau = t e^u) as 4x4 object arrays of mpf."""

    def __init__(self, pi, exch, model, dps=None):
        self.model = model
        self.dps = dps or DPS
        with mp.workdps(self.dps):
            if model == "f81":
                p = [mpmath.mpf(float(x)) for x in pi]
                tot = mpmath.fsum(p)
                self.pi = [x / tot for x in p]
                self.kappa = 1 - mpmath.fsum(x * x for x in self.pi)
            else:
                Q, self.pi, self.kappa = rate_matrix(pi, exch, self.dps)
                sq = [mpmath.sqrt(x) for x in self.pi]
                S = mpmath.zeros(4, 4)
                for i in range(4):
                    for j in range(4):
                        S[i, j] = sq[i] * Q[i, j] / sq[j]
                S = (S + S.T) / 2
                lam, V = mpmath.eigsy(S)
                self.lam = [lam[k] for k in range(4)]
                # P_ij(tau) = sqrt(pi_j / pi_i) sum_k V_ik V_jk exp(lam_k tau)
                self.B = [[[V[i, k] * V[j, k] * sq[j] / sq[i] for j in range(4)] for i in range(4)] for k in range(4)]

    def matrices(self, tau, derivs=True):
        """derivs=False: P alone (the other two are None), a third of the work."""
        with mp.workdps(self.dps):
            P = np.empty((4, 4), object)
            P1 = np.empty((4, 4), object)
            P2 = np.empty((4, 4), object)
            if self.model == "f81":
                e = mpmath.exp(-tau)
                e1, e2 = -tau * e, (tau * tau - tau) * e
                for i in range(4):
                    for j in range(4):
                        d = 1 if i == j else 0
                        P[i, j] = e * d + (1 - e) * self.pi[j]
                        P1[i, j] = e1 * (d - self.pi[j])
                        P2[i, j] = e2 * (d - self.pi[j])
                return P, P1, P2
            terms = []
            for k in range(4):
                x = self.lam[k] * tau
                e = mpmath.exp(x)
                terms.append((e, x * e, (x + x * x) * e))
            for i in range(4):
                for j in range(4):
                    P[i, j] = mpmath.fsum(terms[k][0] * self.B[k][i][j] for k in range(4))
                    if not derivs:
                        continue
                    P1[i, j] = mpmath.fsum(terms[k][1] * self.B[k][i][j] for k in range(4))
                    P2[i, j] = mpmath.fsum(terms[k][2] * self.B[k][i][j] for k in range(4))
            return (P, P1, P2) if derivs else (P, None, None)


def kappa(pi, exch=None, model="gtr"):
    return float(_Model(pi, exch, model).kappa)


def column_curves(states, parent, blen, leaf_taxon, pi, exch, u, model="gtr", small_nodes=False):
    """f, g, h of every column of `states` (uint8 masks [ntaxa, ncols]) at every u: float arrays [len(u), ncols].
    parent / blen / leaf_taxon: post-order tree arrays (root last), as the engine takes them.  pi is used as given
    (normalised to sum 1): a GTR plan floors absent bases first, see floored_pi.
    small_nodes=True appends two int arrays [len(u), ncols]: the number of non-root nodes whose (unscaled) partial has its
    largest component below 2^-256, and below 2^-512.  The kernels rescale a running partial below 2^-256 before it goes up
    a branch, so a pair with a count of 0 is evaluated without rescaling and one with a node below 2^-512 rescales more
    than once; the root's partial goes up no branch and is not counted."""
    states = np.asarray(states, np.uint8)
    ntaxa, ncols = states.shape
    parent = np.asarray(parent)
    blen = np.asarray(blen, np.float64)
    leaf_taxon = np.asarray(leaf_taxon)
    M = _Model(pi, exch, model)
    nn = len(parent)
    children = [[] for _ in range(nn)]
    for n in range(nn):
        if parent[n] >= 0:
            children[parent[n]].append(n)
    one, zero = mpmath.mpf(1), mpmath.mpf(0)
    tips = {}
    for n in range(nn):
        if leaf_taxon[n] >= 0:
            m = states[leaf_taxon[n]] & 15
            tips[n] = np.array([[one if (int(c) >> i) & 1 else zero for c in m] for i in range(4)], object)
    F = np.empty((len(u), ncols))
    G = np.empty_like(F)
    H = np.empty_like(F)
    below = np.zeros((2, len(u), ncols), np.int64)
    with mp.workdps(DPS):
        limits = (mpmath.ldexp(one, -256), mpmath.ldexp(one, -512))
        for iu, uu in enumerate(u):
            s = mpmath.exp(mpmath.mpf(float(uu)))
            part = [None] * nn
            for n in range(nn):          # post-order: children first
                if leaf_taxon[n] >= 0:
                    v, d1, d2 = tips[n], None, None
                else:
                    v = d1 = d2 = None
                    for c in children[n]:
                        mv, m1, m2 = part[c]
                        if v is None:
                            v, d1, d2 = mv, m1, m2
                        else:
                            v, d1, d2 = v * mv, d1 * mv + v * m1, d2 * mv + 2 * d1 * m1 + v * m2
                if parent[n] < 0:
                    part[n] = (v, d1, d2)
                    continue
                if small_nodes and d1 is not None:     # (a tip's largest component is 1)
                    for c in range(ncols):
                        top = max(v[:, c])
                        below[0, iu, c] += top < limits[0]
                        below[1, iu, c] += top < limits[1]
                P, P1, P2 = M.matrices(mpmath.mpf(float(blen[n])) * s)
                if d1 is None:           # a tip: its vector does not depend on u
                    part[n] = (P.dot(v), P1.dot(v), P2.dot(v))
                else:
                    part[n] = (P.dot(v), P1.dot(v) + P.dot(d1), P2.dot(v) + 2 * P1.dot(d1) + P.dot(d2))
            v, d1, d2 = part[nn - 1]
            pi_r = np.array(M.pi, object)
            L, L1, L2 = pi_r.dot(v), pi_r.dot(d1), pi_r.dot(d2)
            for c in range(ncols):
                g = L1[c] / L[c]
                F[iu, c] = float(mpmath.log(L[c]))
                G[iu, c] = float(g)
                H[iu, c] = float(L2[c] / L[c] - g * g)
    if small_nodes:
        return F, G, H, below[0], below[1]
    return F, G, H


# ---- whole-locus log-likelihood (stage 1) -----------------------------------------------------------------------------

def _locus_sweep(M, states, parent, blen, leaf_taxon, branches, want_derivs):
    """Plain pruning of every column at once (object arrays [4, ncols] of mpf), no rescaling.  Returns per column log L_c
    and, per requested branch, g_c = L'/L and h_c = L''/L - g_c^2 in log t_b: with only t_b moving, L is linear in P_b, so
    L' = pi . (path to the root applied to (Q t) P l_b) and L'' the same with (Q t + (Q t)^2) P.  Every branch's message is
    computed once; a derivative climbs from its branch to the root past the stored sibling messages."""
    states = np.asarray(states, np.uint8)
    ntaxa, ncols = states.shape
    parent = np.asarray(parent)
    leaf_taxon = np.asarray(leaf_taxon)
    nn = len(parent)
    children = [[] for _ in range(nn)]
    for n in range(nn):
        if parent[n] >= 0:
            children[parent[n]].append(n)
    one, zero = mpmath.mpf(1), mpmath.mpf(0)
    mats, part, msg = [None] * nn, [None] * nn, [None] * nn
    for n in range(nn):                  # post-order: children first
        if leaf_taxon[n] >= 0:
            m = states[leaf_taxon[n]] & 15
            m = np.where(m == 0, 15, m)  # a zero byte is read as a gap
            v = np.array([[one if (int(c) >> i) & 1 else zero for c in m] for i in range(4)], object).reshape(4, ncols)
        else:
            v = None
            for c in children[n]:
                v = msg[c] if v is None else v * msg[c]
        part[n] = v
        if parent[n] >= 0:
            # (a length that is already mpf is taken as it is: class_model_reference moves it by 1e-15 of itself)
            mats[n] = M.matrices(blen[n] if isinstance(blen[n], mpmath.mpf) else mpmath.mpf(float(blen[n])), want_derivs)
            if leaf_taxon[n] >= 0:       # P v for a 0/1 vector: the sum of the mask's columns of P, once per mask
                tab = np.empty((4, 16), object)
                for mask in set(int(x) for x in m):
                    tab[:, mask] = np.sum([mats[n][0][:, i] for i in range(4) if (mask >> i) & 1], axis=0)
                msg[n] = tab[:, m.astype(int)]
            else:
                msg[n] = mats[n][0].dot(v)
    roots = [n for n in range(nn) if parent[n] < 0]
    assert roots == [nn - 1]
    pi_r = np.array(M.pi, object)
    L = pi_r.dot(part[nn - 1])
    logl = np.array([mpmath.log(x) for x in L], object)
    g, h = {}, {}
    if not want_derivs:
        return logl, g, h
    if branches is None:
        branches = [n for n in range(nn) if parent[n] >= 0]
    for b in branches:
        b = int(b)
        assert parent[b] >= 0
        a1, a2 = mats[b][1].dot(part[b]), mats[b][2].dot(part[b])
        n = b
        while True:
            p = int(parent[n])
            for s in children[p]:
                if s != n:
                    a1, a2 = a1 * msg[s], a2 * msg[s]
            if parent[p] < 0:
                break
            a1, a2 = mats[p][0].dot(a1), mats[p][0].dot(a2)
            n = p
        g[b] = pi_r.dot(a1) / L
        h[b] = pi_r.dot(a2) / L - g[b] * g[b]
    return logl, g, h


def _wsum(weights, vals):
    if weights is None:
        return mpmath.fsum(vals)
    return mpmath.fsum(mpmath.mpf(float(w)) * v for w, v in zip(weights, vals))


def locus_reference_columns(states, parent, blen, leaf, pi, exch, branches=None, dps=None):
    """Per column (mpf object arrays): log L_c, and dicts branch -> L'/L and branch -> L''/L - (L'/L)^2 in log t_b.  A locus
    made of these columns with weights w has lnL = sum w_c log L_c and the same sums for its derivatives."""
    dps = dps or DPS
    with mp.workdps(dps):
        want = branches is None or len(branches) > 0      # branches=[]: the values alone, a third of the matrix work
        return _locus_sweep(_Model(floored_pi(pi), exch, "gtr", dps), states, parent, blen, leaf, branches, want)


def locus_reference(states, weights, parent, blen, leaf, pi, exch, branches=None, dps=None, as_float=True):
    """lnL = sum_c w_c log L_c of a locus at site rate 1 under GTR, and for every branch in `branches` (default: all)
    d lnL / d log t_b and d2 lnL / d (log t_b)^2, analytic, at dps digits (default DPS).  states: uint8 masks
    [ntaxa, ncols] (0 is read as 15); weights: per column or None; parent / blen / leaf: post-order arrays, root last; pi is
    floored as a GTR plan floors it.  Returns (lnl, dlogt, d2logt): floats and arrays over all nodes (NaN where not
    requested), or with as_float=False an mpf and two dicts branch -> mpf."""
    dps = dps or DPS
    with mp.workdps(dps):
        logl, g, h = locus_reference_columns(states, parent, blen, leaf, pi, exch, branches, dps)
        lnl = _wsum(weights, logl)
        d1 = {b: _wsum(weights, g[b]) for b in g}
        d2 = {b: _wsum(weights, h[b]) for b in h}
        if not as_float:
            return lnl, d1, d2
        ga, ha = np.full(len(parent), np.nan), np.full(len(parent), np.nan)
        for b in d1:
            ga[b], ha[b] = float(d1[b]), float(d2[b])
        return float(lnl), ga, ha


def locus_dexch_reference_columns(states, parent, blen, leaf, pi, exch, dps=60, step=1e-18):
    """Per column d log L_c / d r_q at fixed branch lengths, [6, ncols] of mpf: central differences of log L_c with a relative
    step of `step`, evaluated at `dps` digits (truncation ~ step^2, rounding ~ 10^-dps / step: both below 1e-30)."""
    ncols = np.asarray(states).shape[1]
    out = np.empty((6, ncols), object)
    with mp.workdps(dps):
        hh = mpmath.mpf(step)
        base = [mpmath.mpf(float(r)) for r in exch]
        pif = floored_pi(pi)
        for q in range(6):
            f = []
            for sgn in (1, -1):
                e = list(base)
                e[q] = base[q] * (1 + sgn * hh)
                f.append(_locus_sweep(_Model(pif, e, "gtr", dps), states, parent, blen, leaf, None, False)[0])
            out[q] = (f[0] - f[1]) / (2 * hh * base[q])
    return out


def locus_dexch_reference(states, weights, parent, blen, leaf, pi, exch, dps=60, step=1e-18, as_float=True):
    """d lnL / d r_q at fixed branch lengths for the six exchangeabilities (see locus_dexch_reference_columns)."""
    with mp.workdps(dps):
        cols = locus_dexch_reference_columns(states, parent, blen, leaf, pi, exch, dps, step)
        out = [_wsum(weights, cols[q]) for q in range(6)]
        return np.array([float(x) for x in out]) if as_float else out


# ---- the rate-class models of stage 1 ------------------------------------------------------------------------------

def rate_partitions():
    """The 203 partitions of the six rates (AC, AG, AT, CG, CT, GT) into classes as restricted growth strings (the first rate
    is in class 0, every later one in a class seen before or in the next new one): the general model "012345" first, the
    other 202 in lexicographic order, which is the order the engine documents (include/tphip.h, stage1_driver.hip)."""
    import itertools
    out = []
    for tail in itertools.product(range(6), repeat=5):       # (lexicographic already)
        s = (0,) + tail
        if all(s[i] <= max(s[:i]) + 1 for i in range(1, 6)):
            out.append("".join(str(c) for c in s))
    out.remove("012345")
    return ["012345"] + out


def partition_classes(partition):
    """(class of each of the six rates, k): -1 on the class that contains AG (fixed at 1), the k free classes numbered
    0..k-1 in order of first appearance."""
    ag, free = partition[1], []
    for c in partition:
        if c != ag and c not in free:
            free.append(c)
    return [-1 if c == ag else free.index(c) for c in partition], len(free)


def total_factor(pi, exch, dps=None):
    """HyPhy's totalFactor = sum over the six pairs of r_ij 2 pi_i pi_j: the expected substitutions per unit of branch length
    of the unnormalised generator, so that t = b / totalFactor turns a length b in expected substitutions into the
    generator's time (mpf; pi is normalised to sum 1 first; mpf exchangeabilities are taken as they are)."""
    with mp.workdps(dps or DPS):
        p = [mpmath.mpf(float(x)) for x in pi]
        tot = mpmath.fsum(p)
        return mpmath.fsum((r if isinstance(r, mpmath.mpf) else mpmath.mpf(float(r))) * 2 * p[i] * p[j] / (tot * tot)
                           for (i, j), r in zip(PAIRS, exch))


def akaike_weights(lnl, nfree, dps=None):
    """w_m = exp(lnL_m - k_m) / sum_n exp(lnL_n - k_n) (mpf list): mpmath's exponent range needs no shift by the maximum."""
    with mp.workdps(dps or DPS):
        e = [mpmath.exp(mpmath.mpf(float(a)) - int(k)) for a, k in zip(lnl, nfree)]
        tot = mpmath.fsum(e)
        return [x / tot for x in e]


def class_model_reference(states, weights, parent, b, leaf, pi, partition, theta, order=2, dps=60, step=1e-15):
    """One rate-class model of stage 1 on one locus: phi(theta) = lnL(exch(theta), t = b / totalFactor(exch(theta))), where
    exch_q = 1 on the class of AG and exp(theta_c) on free class c (partition_classes), b are the stashed branch lengths in
    expected substitutions and pi is floored as a GTR plan floors it.  Returns (phi, gradient [k], Hessian [k][k]) as mpf
    (order = 0: phi only, 1: no Hessian; the entries not asked for are None); k = 0 has a value only.

    Derivatives are central differences of phi in theta with an ABSOLUTE step h = `step` at `dps` digits, from one stencil:
    g_a = (f(+a) - f(-a)) / 2h, H_aa = (f(+a) - 2 f(0) + f(-a)) / h^2, H_ab = (f(+a+b) + f(-a-b) - f(+a) - f(-a) - f(+b) - f(-b)
    + 2 f(0)) / 2h^2: 1 + 2k + k(k-1) values.  Choice of h: the truncation terms are h^2 f'''/6, h^2 f''''/12 and, for H_ab, h^2 times
    a sum of fourth derivatives of the same size; the rounding terms are u |f| c / h for g and 4 u |f| c / h^2 for H, where
    u = 10^-dps and c is the number of roundings one evaluation accumulates (measured: c is about 3).  phi is a sum over a few hundred columns of
    logarithms that move by less than one per unit of theta each, so |f| and its derivatives of every order stay below ~10^3
    on the loci of the tests (80 to 100 columns).  With h = 1e-15 and 60 digits: truncation <= 1e-30 * 10^3 = 1e-27, rounding of
    H <= 4e-60 * 10^3 * 10^3 / 1e-30 = 4e-24 at the pessimistic c and 4e-27 at c = 1; rounding of g <= 1e-39.  All below 1e-25 for
    c < 25, and test_class_model_reference_does_not_depend_on_its_precision measures it against 120 digits and h = 1e-17
    (which cuts truncation by 10^4 and rounding by 10^56): nothing moves at 1e-25."""
    cls, k = partition_classes(partition)
    assert len(theta) == k
    pif = floored_pi(pi)
    with mp.workdps(dps):
        h = mpmath.mpf(step)
        th0 = [x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x)) for x in theta]
        bb = [x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x)) for x in b]

        def phi(shift):
            th = [x + s * h for x, s in zip(th0, shift)]
            exch = [mpmath.mpf(1) if c < 0 else mpmath.exp(th[c]) for c in cls]
            tf = total_factor(pif, exch, dps)
            t = [x / tf for x in bb]
            logl = _locus_sweep(_Model(pif, exch, "gtr", dps), states, parent, t, leaf, None, False)[0]
            return _wsum(weights, logl)

        def unit(*idx, sign=1):
            return [sign if a in idx else 0 for a in range(k)]

        f0 = phi([0] * k)
        if order == 0 or k == 0:
            return f0, None, None
        fp = [phi(unit(a)) for a in range(k)]
        fm = [phi(unit(a, sign=-1)) for a in range(k)]
        g = [(fp[a] - fm[a]) / (2 * h) for a in range(k)]
        if order == 1:
            return f0, g, None
        H = [[None] * k for _ in range(k)]
        for a in range(k):
            H[a][a] = (fp[a] - 2 * f0 + fm[a]) / (h * h)
            for c in range(a + 1, k):
                both = phi(unit(a, c)) + phi(unit(a, c, sign=-1))
                H[a][c] = H[c][a] = (both - fp[a] - fm[a] - fp[c] - fm[c] + 2 * f0) / (2 * h * h)
        return f0, g, H


def newton_gain(g, H, coords=None, dps=None):
    """(1/2 g' (-H)^-1 g, smallest eigenvalue of -H) on the coordinates `coords` (default: all) as floats: what a Newton step
    would still gain in phi from a point with gradient g and Hessian H, and whether -H is positive definite there."""
    coords = list(range(len(g))) if coords is None else list(coords)
    if not coords:
        return 0.0, math.inf
    with mp.workdps(dps or 60):
        A = mpmath.matrix([[-H[a][c] for c in coords] for a in coords])
        gv = mpmath.matrix([g[a] for a in coords])
        lam = mpmath.eigsy(A, eigvals_only=True)
        x = mpmath.lu_solve(A, gv)
        return float((gv.T * x)[0] / 2), float(min(lam))


# ---- PI ------------------------------------------------------------------------------------------------------------

def finalize_rates(rates, round_decimals=4, correction=1.0, nres=None, threshold=3):
    """What the PI stage does to a raw rate: HyPhy's 4-decimal print and parse, / correction, NaN below threshold."""
    r = np.array([float("%.*f" % (round_decimals, v)) if (round_decimals >= 0 and np.isfinite(v)) else v
                  for v in np.asarray(rates, np.float64)])
    r = r / correction
    if nres is not None:
        r[np.asarray(nres) < threshold] = np.nan
    return r


def net_pi(rates, T):
    """nansum over sites of 16 r^2 t exp(-4 r t), t = 0..T-1: math.fsum of per-term doubles (every term is >= 0)."""
    r = np.asarray(rates, np.float64)
    r = r[np.isfinite(r)]
    out = np.empty(T)
    for t in range(T):
        out[t] = math.fsum((16.0 * r * r * t) * np.exp(-4.0 * r * t))
    return out


def integral_exact(a, b, r):
    """int_a^b 16 r^2 t exp(-4 r t) dt = G(4rb) - G(4ra), G(x) = -(1+x) exp(-x), at DPS digits (mpf)."""
    with mp.workdps(DPS):
        r = mpmath.mpf(float(r))
        xa, xb = 4 * r * int(a), 4 * r * int(b)
        return (1 + xa) * mpmath.exp(-xa) - (1 + xb) * mpmath.exp(-xb)


def net_integrals_exact(rates, intervals):
    """Per interval: math.fsum over the finite rates of the exact integrals (rounded to fp64 one by one)."""
    r = np.asarray(rates, np.float64)
    r = r[np.isfinite(r) & (r != 0.0)]
    out = []
    for a, b in intervals:
        out.append(math.fsum(float(integral_exact(a, b, x)) for x in r))
    return np.array(out)


def townsend_pi(t, r):
    return 16 * (r ** 2) * t * np.exp(-(4 * r * t))


def quad(a, b, r):
    """scipy.integrate.quad as the reference calls it (tapir/compute.py:50-52): (integral, abserr)."""
    return integrate.quad(townsend_pi, a, b, args=(r,))


def net_integrals_quad(rates, intervals):
    """Per interval: math.fsum of the scipy integrals and of their abserr over the finite rates."""
    r = np.asarray(rates, np.float64)
    r = r[np.isfinite(r)]
    si, se = [], []
    for a, b in intervals:
        q = [quad(float(a), float(b), float(x)) for x in r]
        si.append(math.fsum(v for v, _ in q))
        se.append(math.fsum(e for _, e in q))
    return np.array(si), np.array(se)

"""Plain reference for the empirical-Bayes site rates (test helper, not a conftest).

The model, restated from its definition with numpy / scipy and nothing of tapir_amd/eb.py or the kernels' optimiser:

* site rate s = mu rho, rho in K equiprobable categories of Gamma(alpha, alpha) represented by their means
  (compute.discrete_gamma), w_k = 1 / K;
* column likelihood L_c(s) = exp(f) of the one-category site-rate stage: `oracle.column_curve` (fp64, the kernels' forms)
  or, for small cases, `hp_reference.column_curves` (40 digits, plain pruning);
* marginal m_c = sum_k w_k L_c(mu rho_k); locus objective l(mu, alpha) = sum_c n_c log m_c over site patterns;
* posterior p_ck = w_k L_c(mu rho_k) / m_c; rate = kappa mu sum_k p_ck rho_k, sd = kappa mu sqrt(var_p rho), ll = log m_c;
* a category with log(mu rho_k) < U_MIN is evaluated at U_MIN (the documented approximation).

The fits are bounded scalar searches on the objective's VALUES only (no derivatives): a coarse grid that brackets the
maximum, then scipy.optimize.minimize_scalar(method="bounded") inside the bracket.
"""
import math

import numpy as np
from scipy import optimize

from oracle import oracle as orc
from tapir_amd import compute

U_MIN = math.log(1e-10)
U_MAX = math.log(1e4)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def kappa(pi, exch):
    pi = np.asarray(pi, np.float64)
    pi = pi / pi.sum()
    return 2.0 * sum(pi[i] * pi[j] * r for (i, j), r in zip(PAIRS, exch))


def patterns(states):
    """Unique columns (masks normalised 0 -> 15), their counts, and the column -> pattern map."""
    s = np.asarray(states, np.uint8) & 15
    s = np.where(s == 0, 15, s).astype(np.uint8)
    pat, inverse, counts = np.unique(s, axis=1, return_inverse=True, return_counts=True)
    return pat, counts.astype(np.float64), np.asarray(inverse).reshape(-1)


class Locus:
    """One locus: tree arrays as the engine takes them, model (pi, exch; exch of ones = F81), alignment columns."""

    def __init__(self, states, parent, blen, leaf, pi, exch, hp_model=None):
        self.states = np.asarray(states, np.uint8)
        self.parent, self.blen, self.leaf = np.asarray(parent, np.int32), np.asarray(blen, np.float64), np.asarray(leaf, np.int32)
        self.pi = np.asarray(pi, np.float64) / np.sum(pi)
        self.exch = np.ones(6) if exch is None else np.asarray(exch, np.float64)
        self.kappa = kappa(self.pi, self.exch)
        self.pat, self.count, self.inverse = patterns(self.states)
        self.hp_model = hp_model     # None: oracle curves (fp64); "gtr" / "f81": 40-digit curves of hp_reference

    def pattern_logliks(self, u):
        """f[K, npatterns] = log L_c(exp(u_k))."""
        u = np.asarray(u, np.float64)
        if self.hp_model is not None:
            import hp_reference as hp
            F, _, _ = hp.column_curves(self.pat, self.parent, self.blen, self.leaf, self.pi,
                                       None if self.hp_model == "f81" else self.exch, u, model=self.hp_model)
            return F
        out = np.empty((len(u), self.pat.shape[1]))
        for c in range(self.pat.shape[1]):
            out[:, c] = orc.column_curve(self.pat, self.parent, self.blen, self.leaf, self.pi, self.exch, c, u)[0]
        return out

    def mixture(self, log_mu, alpha, ncat):
        """log m_c [npatterns], posterior weights p[K, npatterns], rho[K], category log-likelihoods f[K, npatterns]."""
        rho, w = compute.discrete_gamma(alpha, ncat)
        return self.mixture_of(log_mu, rho, w)

    def mixture_of(self, log_mu, rho, w):
        """mixture() for a given category table (rho[K], w[K])."""
        rho, w = np.asarray(rho, np.float64), np.asarray(w, np.float64)
        f = self.pattern_logliks(np.maximum(log_mu + np.log(rho), U_MIN))
        a = f + np.log(w)[:, None]
        top = a.max(axis=0)
        e = np.exp(a - top)
        z = e.sum(axis=0)
        return top + np.log(z), e / z, rho, f

    def objective(self, log_mu, alpha, ncat):
        logm = self.mixture(log_mu, alpha, ncat)[0]
        return float(np.dot(self.count, logm))

    def objective_of(self, log_mu, rho, w):
        return float(np.dot(self.count, self.mixture_of(log_mu, rho, w)[0]))

    def posterior(self, log_mu, alpha, ncat):
        """Per COLUMN: rate, sd, ll, the moments mean / second of rho behind them, the posterior weights [K, ncols] and
        fmax = max_k |f_k| (the scale of the kernels' error bound)."""
        rho, w = compute.discrete_gamma(alpha, ncat)
        return self.posterior_of(log_mu, rho, w)

    def posterior_of(self, log_mu, rho, w):
        logm, p, rho, f = self.mixture_of(log_mu, rho, w)
        mean = (p * rho[:, None]).sum(axis=0)
        second = (p * (rho ** 2)[:, None]).sum(axis=0)
        km = self.kappa * math.exp(log_mu)
        sd = km * np.sqrt(np.maximum(second - mean ** 2, 0.0))
        m = self.inverse
        return dict(rate=(km * mean)[m], sd=sd[m], ll=logm[m], mean=mean[m], second=second[m], weights=p[:, m],
                    fmax=np.abs(f).max(axis=0)[m])

    def fit_scale(self, alpha, ncat, grid=97):
        """argmax over log mu of the objective at fixed alpha: (log_mu, objective)."""
        rho, w = compute.discrete_gamma(alpha, ncat)
        return self.fit_scale_of(rho, w, grid)

    def fit_scale_of(self, rho, w, grid=97):
        us = np.linspace(U_MIN, U_MAX, grid)
        vals = np.array([self.objective_of(u, rho, w) for u in us])
        i = int(np.argmax(vals))        # the first of equal maxima: the near side of the plateau at large mu
        lo, hi = us[max(i - 1, 0)], us[min(i + 1, grid - 1)]
        r = optimize.minimize_scalar(lambda u: -self.objective_of(u, rho, w), bounds=(lo, hi), method="bounded",
                                     options=dict(xatol=1e-11, maxiter=200))
        if -r.fun >= vals[i]:
            return float(r.x), float(-r.fun)
        return float(us[i]), float(vals[i])

    def fit(self, ncat, alpha_bounds=(0.2, 50.0), grid=9):
        """argmax over (log mu, alpha), alpha within bounds: (log_mu, alpha, objective)."""
        la = np.linspace(math.log(alpha_bounds[0]), math.log(alpha_bounds[1]), grid)
        prof = [self.fit_scale(math.exp(x), ncat) for x in la]
        i = int(np.argmax([p[1] for p in prof]))
        lo, hi = la[max(i - 1, 0)], la[min(i + 1, grid - 1)]
        r = optimize.minimize_scalar(lambda x: -self.fit_scale(math.exp(x), ncat)[1], bounds=(lo, hi), method="bounded",
                                     options=dict(xatol=1e-6, maxiter=100))
        best = (la[i], prof[i][1])
        if -r.fun >= best[1]:
            best = (float(r.x), float(-r.fun))
        alpha = math.exp(best[0])
        u, val = self.fit_scale(alpha, ncat)
        return u, alpha, val

    def profile(self, ncat, log_alphas, grid=33):
        """max over log mu of the objective at each log alpha."""
        return np.array([self.fit_scale(math.exp(x), ncat, grid=grid)[1] for x in log_alphas])

"""Empirical-Bayes site rates under a discrete-gamma prior: the outer search.

Per locus the site rate is s = mu rho with rho ~ Gamma(alpha, alpha) in K equiprobable categories (Yang 1994), and the
rate reported for a column is the posterior mean kappa mu E[rho | column] at the locus' fitted (mu, alpha).  The engine
owns everything per column and the fit of mu at given categories (Plan.eb_fit_scale: Newton in log mu on the device,
Plan.eb_posterior); this module owns the categories and the search over alpha: a golden-section search over log alpha
in [alpha_min, alpha_max], run for all loci of a batch in lockstep -- every round is one vectorised discrete-gamma table
for all loci on the host (the incomplete-gamma inverse stays in scipy), one eb_fit_scale call warm-started from each
locus' best scale so far, and a numpy update of each locus' bracket.
"""
import math

import numpy as np

ALPHA_BOUNDS = (0.2, 50.0)   # design parameters (section 3.4): at K = 16, alpha = 0.2 the lowest category sits 14.5 log-units under mu
DEFAULT_CATEGORIES = 8
MIN_CATEGORIES, MAX_CATEGORIES = 2, 16
LOG_ALPHA_TOL = 1e-4         # width of the final bracket in log alpha
_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


class EbError(ValueError):
    """Invalid empirical-Bayes settings."""


def gamma_tables(alpha, ncat):
    """Yang's discrete gamma for a vector of shapes: (rates[L][K], weights[L][K]); row l equals compute.discrete_gamma(alpha[l], K)."""
    from scipy.special import gammainc, gammaincinv
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    ncat = int(ncat)
    if not MIN_CATEGORIES <= ncat <= MAX_CATEGORIES:
        raise EbError("the number of gamma categories must be in %d..%d" % (MIN_CATEGORIES, MAX_CATEGORIES))
    if not np.all(alpha > 0):
        raise EbError("alpha must be positive")
    a = alpha[:, None]
    cuts = gammaincinv(a, np.arange(1, ncat)[None, :] / ncat)
    inner = gammainc(a + 1.0, cuts)
    upper = np.concatenate([inner, np.ones((len(alpha), 1))], axis=1)
    lower = np.concatenate([np.zeros((len(alpha), 1)), inner], axis=1)
    return ncat * (upper - lower), np.full((len(alpha), ncat), 1.0 / ncat)


def parsimony_changes(states, parent, leaf_taxon):
    """Fitch's minimum number of changes of every column on the tree (post-order arrays, root last); gaps / N join anything."""
    states = np.asarray(states, np.uint8)
    parent = np.asarray(parent)
    leaf_taxon = np.asarray(leaf_taxon)
    ncols = states.shape[1]
    sets = [None] * len(parent)
    changes = np.zeros(ncols, np.int64)
    for n in range(len(parent)):                      # children come before their parent
        if leaf_taxon[n] >= 0:
            m = states[leaf_taxon[n]] & 15
            sets[n] = np.where(m == 0, 15, m).astype(np.uint8)
        p = parent[n]
        if p < 0:
            continue
        if sets[p] is None:
            sets[p] = sets[n]
        else:
            both = sets[p] & sets[n]
            empty = both == 0
            changes += empty
            sets[p] = np.where(empty, sets[p] | sets[n], both).astype(np.uint8)
        sets[n] = None
    return changes


def start_scales(states, locus_offsets, parent, branch_len, leaf_taxon):
    """A host-side start for the fit of mu: the locus' mean parsimony rate (changes per column / tree length), which lies
    below the maximum (parsimony undercounts), or 1 / tree length for a locus without a change.  The pipeline does not use it
    (estimate() takes the engine's Plan.eb_start_scale, computed on the device from the same Fitch pass); it is for callers that
    want a start without an engine call, and for tests and tools that need a sensible scale to evaluate at."""
    off = np.asarray(locus_offsets, np.int64)
    blen = np.asarray(branch_len, np.float64)
    length = float(blen[np.asarray(parent) >= 0].sum())
    if not length > 0:
        raise EbError("the tree has no length")
    ch = parsimony_changes(states, parent, leaf_taxon)
    csum = np.concatenate([[0], np.cumsum(ch)])
    n = np.maximum(off[1:] - off[:-1], 1)
    mean = (csum[off[1:]] - csum[off[:-1]]) / n
    return np.where(mean > 0, mean, 1.0) / length


class _Calls:
    """The engine calls of one search, with the alignment kept on the device between rounds when the engine can."""

    def __init__(self, plan, states, use_patterns):
        self.plan, self.states, self.use_patterns = plan, np.ascontiguousarray(states, np.uint8), use_patterns
        self.d_states = None
        if hasattr(plan, "eb_fit_scale_dev"):
            import torch
            self.d_states = torch.from_numpy(self.states).to("cuda:%d" % getattr(plan, "device", 0))
        self.rounds = 0
        self.evaluations = 0

    def start(self):
        if self.d_states is not None:
            return self.plan.eb_start_scale_dev(self.d_states)
        return self.plan.eb_start_scale(self.states)

    def posterior(self, alpha, ncat, scale):
        rates, weights = gamma_tables(alpha, ncat)
        if self.d_states is None:
            return self.plan.eb_posterior(self.states, rates, weights, scale, use_patterns=self.use_patterns)
        import torch
        dev, n = self.d_states.device, self.states.shape[1]
        out = {k: torch.empty(n, dtype=torch.float64, device=dev) for k in ("rate", "sd", "lnl")}
        out["nres"] = torch.empty(n, dtype=torch.int32, device=dev)
        self.plan.eb_posterior_dev(self.d_states, rates, weights, scale, out["rate"], out["sd"], out["lnl"], out["nres"],
                                   use_patterns=self.use_patterns)
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def posterior_table(self, alpha, ncat, scale):
        """posterior() with the category posterior p[K, ncols] besides ("post"); it stays on the device (a torch tensor, with
        "nres_dev" beside it) when the engine works on device pointers, for posterior_pi below."""
        rates, weights = gamma_tables(alpha, ncat)
        if self.d_states is None:
            return self.plan.eb_posterior_table(self.states, rates, weights, scale, use_patterns=self.use_patterns)
        import torch
        dev, n = self.d_states.device, self.states.shape[1]
        out = {k: torch.empty(n, dtype=torch.float64, device=dev) for k in ("rate", "sd", "lnl")}
        out["nres"] = torch.empty(n, dtype=torch.int32, device=dev)
        post = torch.empty((int(ncat), n), dtype=torch.float64, device=dev)
        self.plan.eb_posterior_table_dev(self.d_states, rates, weights, scale, post, out["rate"], out["sd"], out["lnl"], out["nres"],
                                         use_patterns=self.use_patterns)
        torch.cuda.synchronize(dev)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        host["post"], host["nres_dev"] = post, out["nres"]
        return host

    def fit_scale(self, alpha, ncat, scale):
        rates, weights = gamma_tables(alpha, ncat)
        if self.d_states is not None:
            r = self.plan.eb_fit_scale_dev(self.d_states, rates, weights, scale, use_patterns=self.use_patterns)
        else:
            r = self.plan.eb_fit_scale(self.states, rates, weights, scale, use_patterns=self.use_patterns)
        self.rounds += 1
        self.evaluations += int(np.abs(r["iters"]).max(initial=0)) * ncat
        return r


def fit(plan, states, start=None, ncat=DEFAULT_CATEGORIES, alpha=None, alpha_bounds=ALPHA_BOUNDS, use_patterns=True, calls=None):
    """(mu, alpha) per locus of `plan`.  alpha: a fixed shape for every locus (no search), or None to estimate it per locus
    within alpha_bounds.  start[L]: initial scales (None: the engine's Plan.eb_start_scale).
    Returns dict(alpha[L], scale[L], locus_lnl[L], iters[L], rounds, evaluations): rounds = eb_fit_scale calls,
    evaluations = likelihood evaluations per column over the whole search (sum over rounds of slowest locus' iterations x K)."""
    lo, hi = float(alpha_bounds[0]), float(alpha_bounds[1])
    if not 0 < lo < hi:
        raise EbError("alpha bounds must satisfy 0 < low < high")
    L = int(plan.nloci)
    calls = calls or _Calls(plan, states, use_patterns)
    start = np.asarray(calls.start() if start is None else start, np.float64).reshape(L)
    if alpha is not None:
        a = np.full(L, float(alpha))
        r = calls.fit_scale(a, ncat, start)
        return dict(alpha=a, scale=r["scale"], locus_lnl=r["locus_lnl"], iters=r["iters"], rounds=calls.rounds,
                    evaluations=calls.evaluations)
    # golden section on x = log alpha, all loci in lockstep: bracket [a, b], interior points x1 < x2 with values f1, f2
    a, b = np.full(L, math.log(lo)), np.full(L, math.log(hi))
    x1, x2 = b - _GOLD * (b - a), a + _GOLD * (b - a)
    r1 = calls.fit_scale(np.exp(x1), ncat, start)
    r2 = calls.fit_scale(np.exp(x2), ncat, r1["scale"])
    f1, f2, s1, s2 = r1["locus_lnl"], r2["locus_lnl"], r1["scale"], r2["scale"]
    while np.max(b - a) > LOG_ALPHA_TOL:
        left = f1 >= f2                                    # the maximum lies in [a, x2]; otherwise in [x1, b]
        b = np.where(left, x2, b)
        a = np.where(left, a, x1)
        xn = np.where(left, b - _GOLD * (b - a), a + _GOLD * (b - a))    # the one new interior point of each locus
        rn = calls.fit_scale(np.exp(xn), ncat, np.where(left, s1, s2))  # warm start: the scale of the neighbouring point
        fn, sn = rn["locus_lnl"], rn["scale"]
        x1, x2, f1, f2, s1, s2 = (np.where(left, xn, x2), np.where(left, x1, xn), np.where(left, fn, f2), np.where(left, f1, fn),
                                  np.where(left, sn, s2), np.where(left, s1, sn))
    # the ends of the search interval are candidates too (a profile that still rises at alpha_max: no rate variation to find)
    best_x, best_f, best_s = np.where(f1 >= f2, x1, x2), np.maximum(f1, f2), np.where(f1 >= f2, s1, s2)
    for end in (math.log(lo), math.log(hi)):
        near = (np.abs(best_x - end) < 10 * LOG_ALPHA_TOL)
        if near.any():
            re = calls.fit_scale(np.where(near, math.exp(end), np.exp(best_x)), ncat, best_s)
            take = near & (re["locus_lnl"] >= best_f)
            best_x, best_f, best_s = np.where(take, end, best_x), np.where(take, re["locus_lnl"], best_f), np.where(take, re["scale"], best_s)
    final = calls.fit_scale(np.exp(best_x), ncat, best_s)
    return dict(alpha=np.exp(best_x), scale=final["scale"], locus_lnl=final["locus_lnl"], iters=final["iters"], rounds=calls.rounds,
                evaluations=calls.evaluations)


def posterior_table(plan, states, alpha, scale, ncat=DEFAULT_CATEGORIES, use_patterns=True):
    """The per-column posterior at given (alpha[L], scale[L]) with the category posterior p[K, ncols] as "post" (DESIGN section
    3.10); "post" is a device tensor when the engine works on device pointers (see posterior_pi)."""
    return _Calls(plan, states, use_patterns).posterior_table(np.asarray(alpha, np.float64).reshape(-1), ncat, scale)


def posterior_pi(plan, table, alpha, scale, replicates, seed=1, level=0.95, locus_ids=None):
    """The rate posterior of posterior_table / estimate(table=True) carried into the PI rows (Plan.posterior_pi; conditional on
    the fitted alpha and scale): dict(analytic [L, 2, Wb], expected_counts [L, K], summary [L, 4, Wb]).  A table on the device
    is read where it lies; only the small per-locus results come back."""
    post = table["post"]
    K = int(post.shape[0])
    rho, _ = gamma_tables(alpha, K)
    if isinstance(post, np.ndarray):
        return plan.posterior_pi(post, table["nres"], scale, rho, replicates=replicates, seed=seed, level=level, locus_ids=locus_ids)
    import torch
    dev, L, Wb = post.device, int(plan.nloci), int(plan.bootstrap_width)
    out = dict(analytic=torch.zeros((L, 2, Wb), dtype=torch.float64, device=dev),
               expected_counts=torch.zeros((L, K), dtype=torch.float64, device=dev),
               summary=torch.zeros((L, 4, Wb), dtype=torch.float64, device=dev))
    ws = torch.empty(plan.posterior_pi_workspace_bytes(K, replicates, seed, level)[1], dtype=torch.uint8, device=dev)
    d_scale = torch.from_numpy(np.ascontiguousarray(scale, np.float64)).to(dev)
    d_rho = torch.from_numpy(np.ascontiguousarray(rho, np.float64)).to(dev)
    plan.posterior_pi_dev(post, table["nres_dev"], d_scale, d_rho, K, out["analytic"], out["expected_counts"], out["summary"], None,
                          None, ws, replicates, seed=seed, level=level, locus_ids=locus_ids)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def estimate(plan, states, ncat=DEFAULT_CATEGORIES, alpha=None, alpha_bounds=ALPHA_BOUNDS, use_patterns=True, table=False):
    """The whole estimator for the loci of `plan`: the engine's start scales, the fit of (mu, alpha) per locus, then the
    per-column posterior; the alignment is uploaded once.
    Returns dict(rate, sd, lnl, nres [ncols]; alpha, scale, locus_lnl [L]; rounds, evaluations); with table=True also
    "post", the category posterior p[K, ncols] (kept on the device when the engine can: see posterior_table)."""
    calls = _Calls(plan, states, use_patterns)
    f = fit(plan, states, None, ncat=ncat, alpha=alpha, alpha_bounds=alpha_bounds, use_patterns=use_patterns, calls=calls)
    post = calls.posterior_table(f["alpha"], ncat, f["scale"]) if table else calls.posterior(f["alpha"], ncat, f["scale"])
    out = dict(rate=post["rate"], sd=post["sd"], lnl=post["lnl"], nres=post["nres"])
    if table:
        out.update({k: post[k] for k in ("post", "nres_dev") if k in post})
    out.update(alpha=f["alpha"], scale=f["scale"], locus_lnl=f["locus_lnl"], rounds=f["rounds"], evaluations=f["evaluations"],
               categories=int(ncat))
    return out

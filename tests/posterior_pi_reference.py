"""CPU reference of the empirical-Bayes rate posterior carried into the PI rows (test helper, not a conftest).

Restated from the definitions of DESIGN.md section 3.10 alone, sharing no code with csrc/posterior_pi_kernels.hpp:

* the draw rule in numpy, bit-exact given a table p[K, n]: Philox4x32-10 (the restatement of tests/bootstrap_reference.py),
  key = (seed & 0xffffffff, seed >> 32), counter = (j, b, locus_id lo, locus_id hi), word i of block j for the column
  4j + i of the locus, culled or not; with c_k the fp64 running sum p_0 + ... + p_k added in that order the category is the
  number of k <= K - 2 with (x + 0.5) 2^-32 >= c_k ((x + 0.5) 2^-32 is exact in fp64); N_b[k] counts the live columns;
* the analytic moments in numpy's extended precision (longdouble), the variance in the centred form;
* the exact Poisson-binomial law of N_1 for K = 2 by dynamic programming;
* the category rates and rows P[k][w] in fp64 numpy / scipy (the stand-in engine's values).
"""
import numpy as np

import bootstrap_reference as bsr
import hp_reference as hp


def words(seed, locus_id, B, n):
    """uint32 [B, n]: the word that serves column i of the locus in replicate b."""
    seed, locus_id, B, n = int(seed), int(locus_id), int(B), int(n)
    J = (n + 3) // 4
    if J == 0 or B == 0:
        return np.zeros((B, 0), np.uint32)
    ctr = np.empty((B, J, 4), np.uint64)
    ctr[:, :, 0] = np.arange(J, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[:, :, 2] = locus_id & 0xFFFFFFFF
    ctr[:, :, 3] = (locus_id >> 32) & 0xFFFFFFFF
    x = bsr.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    return x.reshape(B, 4 * J)[:, :n]


def categories(p, x):
    """p [K, n] fp64, x uint32 [B, n] -> drawn category int [B, n] by the rule above."""
    p = np.asarray(p, np.float64)
    K = p.shape[0]
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32          # exact: 33 significant bits
    c = np.add.accumulate(p[:K - 1], axis=0)               # c_k = (..(p_0 + p_1) + ..) + p_k
    cat = np.zeros(x.shape, np.int64)
    for k in range(K - 1):
        cat += u >= c[k][None, :]
    return cat


def counts(p, live, seed, locus_id, B):
    """int32 [B, K]: N_b[k] = the live columns of the locus drawn into category k in replicate b."""
    p = np.asarray(p, np.float64)
    K, n = p.shape
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    cat = categories(p, words(seed, locus_id, B, n))
    out = np.zeros((int(B), K), np.int32)
    for k in range(K):
        out[:, k] = ((cat == k) & live[None, :]).sum(axis=1)
    return out


def rows_from_counts(cnt, P):
    """[B, Wb] longdouble: sum_k N_b[k] P[k][w]."""
    return np.asarray(cnt).astype(np.longdouble) @ np.asarray(P, np.longdouble)


def analytic(p, live, P):
    """(expected_counts [K], mean [Wb], sd [Wb]) in longdouble from p [K, n], live [n] and the category rows P [K, Wb]."""
    p = np.asarray(p, np.float64).astype(np.longdouble)
    P = np.asarray(P).astype(np.longdouble)
    live = np.ones(p.shape[1], bool) if live is None else np.asarray(live, bool)
    q = p[:, live]                                         # [K, n_live]
    nk = q.sum(axis=1)
    mean = nk @ P
    a = q.T @ P                                            # [n_live, Wb] each site's own mean row
    var = np.zeros(P.shape[1], np.longdouble)
    for k in range(P.shape[0]):
        var += (q[k][:, None] * (P[k][None, :] - a) ** 2).sum(axis=0)
    return nk, mean, np.sqrt(var)


def poisson_binomial(p1):
    """Exact law of the number of successes of independent trials with probabilities p1 [n]: float64 [n + 1]."""
    law = np.zeros(len(p1) + 1, np.longdouble)
    law[0] = 1.0
    for i, q in enumerate(np.asarray(p1, np.float64).astype(np.longdouble)):
        law[1:i + 2] = law[1:i + 2] * (1 - q) + law[0:i + 1] * q
        law[0] *= 1 - q
    return law.astype(np.float64)


def category_rates(kappa, scale, rho, round_decimals, correction):
    """r_lk [K]: the plan's finalisation of the raw rate (kappa mu) rho_k (the round trip, then / correction)."""
    raw = (float(kappa) * float(scale)) * np.asarray(rho, np.float64)
    return hp.finalize_rates(raw, round_decimals, correction, None, 0)


def category_rows(rates, T, intervals, exact=False):
    """P [K, T + n_i] in fp64: 16 r^2 t exp(-4 r t) at t = 0..T-1, then the interval integrals (scipy's quad, or the exact
    antiderivative); an all-zero row for a non-finite or zero rate."""
    r = np.asarray(rates, np.float64)
    P = np.zeros((r.size, T + len(intervals)))
    t = np.arange(T, dtype=np.float64)
    ok = np.isfinite(r) & (r != 0.0)
    rr = r[ok][:, None]
    P[ok, :T] = 16.0 * rr * rr * t[None, :] * np.exp(-4.0 * rr * t[None, :])
    if len(intervals):
        P[:, T:] = bsr.site_integrals(r, [list(map(int, iv)) for iv in intervals], exact=exact)
    return P

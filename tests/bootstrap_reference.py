"""CPU reference of the site bootstrap of the PI rows (test helper, not a conftest).

Restated from the definition in DESIGN.md section 3.5 alone, sharing no code with csrc/bootstrap_kernels.hpp:

* Philox4x32-10 in numpy (Salmon, Moraes, Dror, Shaw 2011: multipliers 0xD2511F53 / 0xCD9E8D57, key increments
  0x9E3779B9 / 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (j, b, locus_id & 0xffffffff, locus_id >> 32);
  draw 2j = ((x1 2^32 + x0) n) >> 64, draw 2j + 1 the same from (x3, x2), the last draw of an odd n discarded.
* Site rows p_i[w]: 16 r^2 t exp(-4 r t) for t = 0..T-1 in mpmath (tests/hp_reference.py's precision), then one integral
  per interval (scipy.integrate.quad, what the reference program calls, or the exact antiderivative); all zero for a NaN
  or zero rate.  Rounded to numpy's extended precision (two-double split), so a replicate row sum_i c_i p_i accumulated in
  longdouble carries an error far below the fp64 bounds of the tests.
* Summary: mean, sd (ddof = 1), numpy's default quantiles at (1 - level) / 2 and 1 - (1 - level) / 2.
"""
import mpmath
import numpy as np

import hp_reference as hp

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint array [..., 4], key: uint array [..., 2] (broadcastable) -> output words uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def draws(seed, locus_id, b, n):
    """The n column indices replicate b of a locus of n columns draws (Python integers: the 128-bit product is exact)."""
    seed, locus_id, n = int(seed), int(locus_id), int(n)
    calls = (n + 1) // 2
    if calls == 0:
        return []
    ctr = np.empty((calls, 4), np.uint64)
    ctr[:, 0] = np.arange(calls, dtype=np.uint64)
    ctr[:, 1] = int(b)
    ctr[:, 2] = locus_id & 0xFFFFFFFF
    ctr[:, 3] = (locus_id >> 32) & 0xFFFFFFFF
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)).tolist()
    out = []
    for x0, x1, x2, x3 in x:
        out.append((((x1 << 32) | x0) * n) >> 64)
        out.append((((x3 << 32) | x2) * n) >> 64)
    return out[:n]


def counts(seed, locus_id, n, rep0, nrep):
    """uint16 [nrep, n]: how often each column is drawn in replicates rep0 .. rep0 + nrep - 1."""
    out = np.zeros((int(nrep), int(n)), np.int64)
    for k in range(int(nrep)):
        np.add.at(out[k], np.asarray(draws(seed, locus_id, rep0 + k, n), dtype=np.int64), 1)
    assert out.max(initial=0) < 65536
    return out.astype(np.uint16)


def _to_longdouble(x):
    """mpf -> numpy longdouble by a two-double split (exact to ~2^-105, then rounded once to the longdouble format)."""
    hi = float(x)
    lo = float(x - mpmath.mpf(hi))
    return np.longdouble(hi) + np.longdouble(lo)


def site_net(final_rates, T):
    """[n, T] longdouble: 16 r^2 t exp(-4 r t) per site at t = 0..T-1 from mpmath; zero rows for NaN / zero rates."""
    r = np.asarray(final_rates, np.float64)
    out = np.zeros((r.size, T), np.longdouble)
    with mpmath.mp.workdps(hp.DPS):
        for i, v in enumerate(r):
            if not np.isfinite(v) or v == 0.0:
                continue
            x = mpmath.mpf(float(v))
            c, q, p = 16 * x * x, mpmath.exp(-4 * x), mpmath.mpf(1)
            for t in range(T):
                out[i, t] = _to_longdouble(c * t * p)
                p *= q
    return out


def site_integrals(final_rates, intervals, exact=False):
    """[n, n_i] float64 per-site integrals: scipy.integrate.quad (exact=False) or the antiderivative in mpmath."""
    r = np.asarray(final_rates, np.float64)
    out = np.zeros((r.size, len(intervals)))
    for i, v in enumerate(r):
        if not np.isfinite(v) or v == 0.0:
            continue
        for k, (a, b) in enumerate(intervals):
            out[i, k] = float(hp.integral_exact(a, b, v)) if exact else hp.quad(float(a), float(b), float(v))[0]
    return out


def rows_from_counts(cnt, site_values):
    """[nrep, W] longdouble: sum_i cnt[b, i] * site_values[i, w] accumulated in extended precision."""
    c = np.asarray(cnt).astype(np.longdouble)
    return c @ np.asarray(site_values, np.longdouble)


def summarize(rows, level):
    """rows [B, W] float64 -> [4, W]: mean, sd (ddof = 1), quantiles at (1 - level) / 2 and 1 - (1 - level) / 2."""
    rows = np.asarray(rows, np.float64)
    q = np.quantile(rows, [(1 - level) / 2, 1 - (1 - level) / 2], axis=0)
    return np.stack([rows.mean(axis=0), rows.std(axis=0, ddof=1), q[0], q[1]])

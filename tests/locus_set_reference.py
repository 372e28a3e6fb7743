"""References for the locus-set accumulation curves.  Test helper, no GPU.

  normal_rows     the definition of the normal rows: np.cumsum over the gathered per-locus rows' sums, in the order given, and
                  the family's restated probability rule (quartet_reference / unequal_quartet_reference) on those sums
  exact_rows      the numpy mirror of the exact rows of one quartet at a forced M: the per-locus moments of
                  exact_quartet_reference.moments added left to right, the head rule by its tail_bound at M, the
                  characteristic function of the concatenation on the whole M x M torus (no half spectrum), the weights of
                  its _weights by direct summation
  concatenated    the planes of the first k loci of an order as one long locus: what windowed_dp is applied to
  default_order   the ranking rule: a stable argsort of -p_correct per quartet
  k_needed        the smallest k whose p_correct reaches the target, or None
"""
import math

import numpy as np

import exact_quartet_reference as er
import quartet_reference as qr
import unequal_quartet_reference as ur


def normal_rows(locus_rows, order):
    """locus_rows [L, n_q, 8 or 13], order [n_q, K] -> [n_q, K, 8 or 13]"""
    locus_rows, order = np.asarray(locus_rows, np.float64), np.asarray(order)
    width = locus_rows.shape[2]
    nsum, rule = (5, qr.probabilities) if width == 8 else (9, ur.probabilities)
    out = np.zeros(order.shape + (width,))
    for q in range(order.shape[0]):
        out[q, :, :nsum] = np.cumsum(locus_rows[order[q], q, :nsum], axis=0)
        for k in range(order.shape[1]):
            out[q, k, nsum:] = rule(out[q, k, :nsum])
    return out


def concatenated(planes, off, order_q, k):
    """planes: (y, x1, x2) of one quartet, each [ncols]; the columns of loci order_q[:k] one after the other"""
    cols = np.concatenate([np.arange(off[l], off[l + 1]) for l in order_q[:k]] + [np.zeros(0, np.int64)]).astype(np.int64)
    return tuple(np.asarray(p, np.float64)[cols] for p in planes)


def exact_rows(planes, off, order_q, M=er.DEFAULT_WINDOW, tol=er.DEFAULT_TAIL, n_head=0):
    """[K, 6] rows p_correct, p_ac, p_ad, p_polytomy, window, tail_bound of one quartet's prefixes, all on the M x M torus"""
    y, x1, x2 = (np.asarray(p, np.float64) for p in planes)
    K = len(order_q)
    n_head = n_head or K
    rows = np.zeros((K, 6))
    means, var = np.zeros(3), np.zeros(3)
    k_ = np.arange(M)
    z = np.exp(2j * np.pi * k_ / M)
    z1, z2 = z[:, None], z[None, :]
    j12 = (k_[:, None] + k_[None, :]) % M
    phi = np.ones((M, M), dtype=np.complex128)
    is_open = True
    for k, l in enumerate(order_q):
        sl = slice(int(off[l]), int(off[l + 1]))
        m, v = er.moments(y[sl], x1[sl], x2[sl])
        means, var = means + np.array(m), var + np.array(v)          # left to right
        finite = bool(np.all(np.isfinite(means)) and np.all(np.isfinite(var)))
        bound = er.tail_bound(tuple(var.tolist()), M) if finite else math.nan
        is_open = is_open and finite and bound <= tol and k < n_head
        if not is_open:
            rows[k] = (math.nan,) * 4 + (0, bound)
            continue
        for yi, ai, bi in zip(y[sl].tolist(), x1[sl].tolist(), x2[sl].tolist()):
            if yi == 0.0 and ai == 0.0 and bi == 0.0:
                continue
            phi *= (1.0 - yi - ai - bi) + yi * z1 * z2 + ai * np.conj(z1) + bi * np.conj(z2)
        c1, c2, ce = (int(round(v)) for v in means.tolist())
        if not var.any():              # a point law: read off the centres
            pc, p1, p2 = float(c1 > 0 and c2 > 0), float(c1 < 0 and c1 < c2), float(c2 < 0 and c2 < c1)
            rows[k] = (pc, p1, p2, 1.0 - pc - p1 - p2, M, bound)
            continue
        a1, a2 = er._weights(c1, M, True), er._weights(c2, M, True)
        b1, b2 = er._weights(c1, M, False), er._weights(c2, M, False)
        e, f = er._weights(ce, M, True), er._weights(-ce, M, True)
        pc = float(np.sum(phi * a1[:, None] * a2[None, :]).real) / M ** 2
        p1 = float(np.sum(phi * b1[j12] * e[None, :]).real) / M ** 2
        p2 = float(np.sum(phi * b2[j12] * f[:, None]).real) / M ** 2
        pc, p1, p2 = (min(1.0, max(0.0, v)) for v in (pc, p1, p2))
        rows[k] = (pc, p1, p2, max(0.0, 1.0 - pc - p1 - p2), M, bound)
    return rows


def default_order(p_correct):
    """p_correct [L, n_q] (the per-locus normal approximation) -> [n_q, L]: descending, ties by ascending locus index"""
    return np.argsort(-np.asarray(p_correct, np.float64).T, axis=1, kind="stable")


def k_needed(p_correct, target):
    """p_correct [K] of the sets of size 1..K: the smallest k with p_correct >= target (NaN never is), or None"""
    hit = np.flatnonzero(np.asarray(p_correct, np.float64) >= target)
    return int(hit[0]) + 1 if hit.size else None

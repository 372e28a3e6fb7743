"""CPU mirror of the column simulation of the parametric bootstrap (test helper, not a conftest).

Restated from the definition in DESIGN.md section 3.7 alone, sharing no code with csrc/simulate_kernels.hpp:

* draw d belongs to the node with post-order index d; Philox4x32-10 (bootstrap_reference.philox4x32_10) with key
  ((seed & 0xffffffff) ^ 0x73696D75, seed >> 32) and counter (i, b | ((d >> 1) << 16), id & 0xffffffff, id >> 32);
  u = (((x1 << 32) | x0) >> 11) 2^-53 for an even d, the same from (x3, x2) for an odd one;
* selection: p clamped at >= 0, c0 = p0, c1 = c0 + p1, c2 = c1 + p2, c3 = c2 + p3, v = u c3, state = (v >= c0) + (v >= c1) +
  (v >= c2);
* root: p = pi; a node with parent state x and branch length t: row x of exp(Q r t / kappa) = I + U expm1(lam r t / kappa)
  U^-1 from a numpy eigen-system (F81: (1 - w) I + w Pi with w = -expm1(-r t / kappa));
* a NaN, infinite or negative rate gives a column of 15s; with a mask (0 read as 15) a cell that is not one of 1, 2, 4, 8 is
  copied through.

The GPU's expm1 and eigen-system differ from numpy's in the last bits, so a draw that falls within 1e-12 c3 of a boundary
c_k is *undecided*: the mirror reports, per cell, whether every draw on the path from the root was decided.

simulate() goes locus by locus; simulate_all_loci() is the same definition with all loci advanced together, for large trees.
"""
import numpy as np

import bootstrap_reference as bsr

KEY_TAG = 0x73696D75
DECIDED = 1e-12


def eigen_system(pi, exch):
    """pi [4] (normalised here), exch [6] AC, AG, AT, CG, CT, GT -> dict(pi, lam [4], U [4, 4], Ui [4, 4], kappa, Q)."""
    pi = np.asarray(pi, np.float64)
    pi = pi / pi.sum()
    R = np.zeros((4, 4))
    for k, (i, j) in enumerate([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]):
        R[i, j] = R[j, i] = exch[k]
    Q = R * pi[None, :]
    Q[range(4), range(4)] = -Q.sum(axis=1)
    kappa = float(-(pi * np.diag(Q)).sum())
    sq = np.sqrt(pi)
    S = sq[:, None] * Q / sq[None, :]
    lam, V = np.linalg.eigh(0.5 * (S + S.T))
    lam[-1] = 0.0   # the stationary eigenvalue (eigh: ascending) is 0 exactly; left at 1e-17 it would grow with s
    return dict(pi=pi, lam=lam, U=V / sq[:, None], Ui=V.T * sq[None, :], kappa=kappa, Q=Q, f81=False)


def f81_system(pi):
    pi = np.asarray(pi, np.float64)
    pi = pi / pi.sum()
    Q = np.tile(pi, (4, 1)) - np.eye(4)
    return dict(pi=pi, kappa=float(1.0 - (pi * pi).sum()), Q=Q, f81=True)


def transition_rows(model, x, s):
    """rows x[c] of exp(Q s[c]) (Q normalised to one substitution is model Q / kappa; s = r t / kappa): [n, 4]"""
    n = len(x)
    if model["f81"]:
        w = -np.expm1(-s)
        p = w[:, None] * model["pi"][None, :]
        p[np.arange(n), x] += 1.0 - w
        return p
    E = np.expm1(np.outer(s, model["lam"]))             # [n, 4]; the zero eigenvalue gives exactly 0
    p = (model["U"][x] * E) @ model["Ui"]
    p[np.arange(n), x] += 1.0
    return p


def uniforms(seed, stream_id, b, d, n):
    """u of node d for the columns 0..n-1 of a locus"""
    seed, stream_id = int(seed), int(stream_id)
    ctr = np.empty((n, 4), np.uint64)
    ctr[:, 0] = np.arange(n, dtype=np.uint64)
    ctr[:, 1] = int(b) | ((int(d) >> 1) << 16)
    ctr[:, 2] = stream_id & 0xFFFFFFFF
    ctr[:, 3] = (stream_id >> 32) & 0xFFFFFFFF
    key = np.array([(seed & 0xFFFFFFFF) ^ KEY_TAG, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    x = bsr.philox4x32_10(ctr, key).astype(np.uint64)
    lo, hi = (x[:, 2], x[:, 3]) if d & 1 else (x[:, 0], x[:, 1])
    bits = (hi << np.uint64(32)) | lo
    return (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def select(p, u):
    """(state [n], decided [n])"""
    c = np.cumsum(np.maximum(p, 0.0), axis=1)
    v = u * c[:, 3]
    state = (v >= c[:, 0]).astype(np.int64) + (v >= c[:, 1]) + (v >= c[:, 2])
    decided = np.all(np.abs(v[:, None] - c) > DECIDED * c[:, 3:4], axis=1)
    return state, decided


def simulate_locus(parent, blen, leaf, ntaxa, model, rates, stream_id, b=0, seed=1, mask=None):
    """One locus: rates [n] raw rates (kappa * s), mask [ntaxa, n] or None.
    Returns dict(states uint8 [ntaxa, n], sure bool [ntaxa, n] (the cell does not hang on an undecided draw), draws, undecided)."""
    parent, leaf = np.asarray(parent), np.asarray(leaf)
    blen = np.asarray(blen, np.float64)
    rates = np.asarray(rates, np.float64)
    n, nn = rates.size, len(parent)
    bad = ~(rates >= 0.0) | np.isinf(rates)
    r = np.where(bad, 0.0, rates)
    node_state, node_sure = {}, {}
    states = np.empty((ntaxa, n), np.uint8)
    sure = np.ones((ntaxa, n), bool)
    undecided = 0
    for d in range(nn - 1, -1, -1):
        u = uniforms(seed, stream_id, b, d, n)
        if parent[d] < 0:
            p = np.tile(model["pi"], (n, 1))
            up = np.ones(n, bool)
        else:
            s = r * blen[d] / model["kappa"]
            p = transition_rows(model, node_state[parent[d]], s)
            up = node_sure[parent[d]]
        st, dec = select(p, u)
        undecided += int((~dec).sum())
        node_state[d], node_sure[d] = st, up & dec
        if leaf[d] >= 0:
            cell = (1 << st).astype(np.uint8)
            ok = node_sure[d].copy()
            if mask is not None:
                m = np.where(mask[leaf[d]] == 0, 15, mask[leaf[d]]).astype(np.uint8)
                through = ~np.isin(m, [1, 2, 4, 8])
                cell = np.where(through, m, cell)
                ok |= through
            states[leaf[d]] = np.where(bad, 15, cell)
            sure[leaf[d]] = ok | bad
    return dict(states=states, sure=sure, draws=nn * n, undecided=undecided)


def simulate(parent, blen, leaf, ntaxa, offsets, models, rates, locus_ids=None, b=0, seed=1, mask=None):
    """A plan's worth of loci: offsets [L + 1], models a list of L systems.  Same keys as simulate_locus."""
    L = len(offsets) - 1
    parts = []
    for l in range(L):
        a, e = int(offsets[l]), int(offsets[l + 1])
        parts.append(simulate_locus(parent, blen, leaf, ntaxa, models[l], rates[a:e], l if locus_ids is None else locus_ids[l],
                                    b=b, seed=seed, mask=None if mask is None else mask[:, a:e]))
    return dict(states=np.concatenate([p["states"] for p in parts], axis=1), sure=np.concatenate([p["sure"] for p in parts], axis=1),
                draws=sum(p["draws"] for p in parts), undecided=sum(p["undecided"] for p in parts))


def simulate_all_loci(parent, blen, leaf, ntaxa, offsets, models, rates, locus_ids=None, b=0, seed=1, mask=None):
    """simulate() with every locus advanced together, one pass over the tree for the whole plan and one Philox call per pair of
    nodes: for trees of thousands of nodes, where simulate()'s per-locus, per-node calls take minutes.  The same definition
    and the same keys; the GTR row is summed by einsum instead of a matrix product, which may move a probability by an ulp
    and with it only a draw that is undecided anyway (tests/test_simulate.py holds the two functions to each other)."""
    parent, leaf = np.asarray(parent), np.asarray(leaf)
    blen = np.asarray(blen, np.float64)
    rates = np.asarray(rates, np.float64)
    offsets = np.asarray(offsets, np.int64)
    L, n, nn = len(offsets) - 1, rates.size, len(parent)
    loc = np.repeat(np.arange(L), np.diff(offsets))
    ids = np.arange(L) if locus_ids is None else np.array([int(v) for v in locus_ids], object)
    f81 = models[0]["f81"]
    pi = np.stack([m["pi"] for m in models])[loc]
    kappa = np.array([m["kappa"] for m in models])[loc]
    if not f81:
        lam = np.stack([m["lam"] for m in models])[loc]
        U = np.stack([m["U"] for m in models])[loc]
        Ui = np.stack([m["Ui"] for m in models])[loc]
    ctr = np.empty((n, 4), np.uint64)
    ctr[:, 0] = np.arange(n) - offsets[loc]
    ctr[:, 2] = np.array([int(v) & 0xFFFFFFFF for v in ids], np.uint64)[loc]
    ctr[:, 3] = np.array([(int(v) >> 32) & 0xFFFFFFFF for v in ids], np.uint64)[loc]
    key = np.array([(int(seed) & 0xFFFFFFFF) ^ KEY_TAG, (int(seed) >> 32) & 0xFFFFFFFF], np.uint64)
    bad = ~(rates >= 0.0) | np.isinf(rates)
    r = np.where(bad, 0.0, rates)
    cols = np.arange(n)
    node_state, node_sure = {}, {}
    states = np.empty((ntaxa, n), np.uint8)
    sure = np.ones((ntaxa, n), bool)
    undecided, x, x_of = 0, None, -1
    for d in range(nn - 1, -1, -1):
        if x_of != d >> 1:
            ctr[:, 1] = int(b) | ((d >> 1) << 16)
            x, x_of = bsr.philox4x32_10(ctr, key).astype(np.uint64), d >> 1
        lo, hi = (x[:, 2], x[:, 3]) if d & 1 else (x[:, 0], x[:, 1])
        u = (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        if parent[d] < 0:
            p, up = pi, np.ones(n, bool)
        else:
            s = r * blen[d] / kappa
            px = node_state[parent[d]]
            up = node_sure[parent[d]]
            if f81:
                w = -np.expm1(-s)
                p = w[:, None] * pi
                p[cols, px] += 1.0 - w
            else:
                p = np.einsum("nk,nkj->nj", U[cols, px] * np.expm1(s[:, None] * lam), Ui)
                p[cols, px] += 1.0
        st, dec = select(p, u)
        undecided += int((~dec).sum())
        if leaf[d] < 0:
            node_state[d], node_sure[d] = st.astype(np.int8), up & dec
            continue
        cell = (1 << st).astype(np.uint8)
        ok = up & dec
        if mask is not None:
            m = np.where(mask[leaf[d]] == 0, 15, mask[leaf[d]]).astype(np.uint8)
            through = ~np.isin(m, [1, 2, 4, 8])
            cell = np.where(through, m, cell)
            ok |= through
        states[leaf[d]] = np.where(bad, 15, cell)
        sure[leaf[d]] = ok | bad
    return dict(states=states, sure=sure, draws=nn * n, undecided=undecided)


def caterpillar(ntaxa):
    """((((t0, t1), t2), t3) ...): post-order arrays with 2 ntaxa - 1 nodes"""
    parent, blen, leaf = [], [], []
    # nodes: t0, t1, i0, t2, i1, t3, i2 ...
    parent += [2, 2]
    leaf += [0, 1]
    blen += [0.3, 0.2]
    last = 2
    for k in range(2, ntaxa):
        parent.append(last + 2)   # internal node `last` hangs under the next internal node
        leaf.append(-1)
        blen.append(0.1 + 0.01 * k)
        parent.append(last + 2)
        leaf.append(k)
        blen.append(0.25)
        last += 2
    parent.append(-1)
    leaf.append(-1)
    blen.append(0.0)
    return parent, blen, leaf


def joint_z(states, model, s2):
    """max |z| of the 16 joint frequencies of a two-taxon alignment (rows 0 and 1, single-base cells) against
    pi_x P_xy(s2), P = exp(Q s2 / kappa) by scipy's Pade expm -- not the eigen-form the simulation used."""
    from scipy.linalg import expm
    P = expm(model["Q"] * (s2 / model["kappa"]))
    expect = model["pi"][:, None] * P
    code = {1: 0, 2: 1, 4: 2, 8: 3}
    a = np.array([code[int(v)] for v in states[0]])
    c = np.array([code[int(v)] for v in states[1]])
    N = a.size
    counts = np.zeros((4, 4))
    np.add.at(counts, (a, c), 1)
    z = (counts - N * expect) / np.sqrt(N * expect * (1.0 - expect))
    return float(np.abs(z).max()), counts, expect

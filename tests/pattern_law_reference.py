"""The exact law of fully resolved alignment columns on a small tree (test helper, not a conftest), and the statistics that hold
simulated columns to it.

Nothing here comes from the column simulation (tapir_amd/csrc/simulate_kernels.hpp) or from its mirror
(tests/simulate_reference.py): no random numbers, no inversion, no top-down pass.  A column's probability is its likelihood,
computed bottom-up by plain pruning in mpmath at hp_reference.DPS (40) digits with hp_reference's transition matrices -- the
quantity whose logarithm hp_reference.column_curves returns as F (tests/test_pattern_law.py holds the two to each other).

* pattern_probabilities  the 4^n probabilities of an n-taxon tree, n <= 5; column k has taxon j in state (k // 4^j) % 4
* pair_joint             pi_x P_xy(d rate / kappa) by mpmath's expm of hp_reference.rate_matrix (GTR) or in closed form (F81)
* pooled_chi2, pair_cells, tip_pairs, path_lengths, first_leaf: what the tests of both the mirror and the GPU score with
"""
import mpmath
import numpy as np

import hp_reference as hp

mp = mpmath.mp
CODE = np.zeros(16, np.int64)
CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]


def all_columns(n):
    """uint8 masks [n, 4^n]: column k has taxon j in state (k // 4^j) % 4"""
    k = np.arange(4 ** n)
    return np.stack([(1 << ((k // 4 ** j) % 4)).astype(np.uint8) for j in range(n)])


def column_index(states):
    """the column number of all_columns for every column of `states` (single-base masks [n, N])"""
    states = np.asarray(states)
    assert np.all(np.isin(states, [1, 2, 4, 8]))
    return sum(CODE[states[j]] * 4 ** j for j in range(states.shape[0]))


def pattern_probabilities(parent, blen, leaf, pi, exch, rate, model, as_mpf=False):
    """Probability of each of the 4^n fully resolved columns (order: all_columns) at raw rate `rate` (kappa * s): floats, or
    the mpf values themselves with as_mpf=True.  pi is used as given, normalised to sum 1."""
    parent, leaf = np.asarray(parent), np.asarray(leaf)
    n = int((leaf >= 0).sum())
    assert n <= 5
    cols = all_columns(n)
    M = hp._Model(pi, exch, model)
    nn = len(parent)
    with mp.workdps(hp.DPS):
        s = mpmath.mpf(float(rate)) / M.kappa
        one, zero = mpmath.mpf(1), mpmath.mpf(0)
        msg = [None] * nn
        for d in range(nn):                                  # post-order: children first
            if leaf[d] >= 0:
                v = np.array([[one if (int(c) >> i) & 1 else zero for c in cols[leaf[d]]] for i in range(4)], object)
            else:
                v = None
                for c in np.flatnonzero(parent == d):
                    v = msg[c] if v is None else v * msg[c]
            if parent[d] < 0:
                L = np.array(M.pi, object).dot(v)
            else:
                msg[d] = M.matrices(mpmath.mpf(float(blen[d])) * s, derivs=False)[0].dot(v)
        return list(L) if as_mpf else np.array([float(x) for x in L])


def _mpf(x):
    return x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x))


def pair_joint(pi, exch, rate, model, d, as_mpf=False):
    """pi_x P_xy(d rate / kappa), [4, 4]: two tips a path of length d (a float or an mpf) apart (reversibility).  GTR: mpmath's expm (Pade) of
    hp_reference.rate_matrix; F81: P = e I + (1 - e) Pi with e = exp(-d rate / kappa), kappa = 1 - sum pi^2."""
    with mp.workdps(hp.DPS):
        if model == "f81":
            p = [mpmath.mpf(float(x)) for x in pi]
            tot = mpmath.fsum(p)
            p = [x / tot for x in p]
            kappa = 1 - mpmath.fsum(x * x for x in p)
            e = mpmath.exp(-_mpf(d) * mpmath.mpf(float(rate)) / kappa)
            J = [[p[x] * ((e if x == y else 0) + (1 - e) * p[y]) for y in range(4)] for x in range(4)]
        else:
            Q, p, kappa = hp.rate_matrix(pi, exch)
            P = mpmath.expm(Q * (_mpf(d) * mpmath.mpf(float(rate)) / kappa), method="pade")
            J = [[p[x] * P[x, y] for y in range(4)] for x in range(4)]
        if as_mpf:
            return J
        return np.array([[float(v) for v in row] for row in J])


def pooled_chi2(counts, prob, min_expected=5.0):
    """Pearson X^2 of `counts` against N prob with every cell whose expected count is below min_expected pooled into one:
    (X^2, df = cells - 1)."""
    counts = np.asarray(counts, np.float64)
    expect = counts.sum() * np.asarray(prob, np.float64)
    small = expect < min_expected
    o, e = counts[~small], expect[~small]
    if small.any():
        o, e = np.append(o, counts[small].sum()), np.append(e, expect[small].sum())
    return float(((o - e) ** 2 / e).sum()), len(e) - 1


def chi2_bound(df, sigmas):
    return df + sigmas * np.sqrt(2.0 * df)


def pattern_counts(states):
    n = np.asarray(states).shape[0]
    return np.bincount(column_index(states), minlength=4 ** n)


# ---- tip pairs of deeper trees ---------------------------------------------------------------------------------------

def first_leaf(parent, leaf):
    """per node: the taxon of the first leaf below it (the node of lowest index among its descendants that is a leaf)"""
    nn = len(parent)
    kids = [[] for _ in range(nn)]
    for d in range(nn):
        if parent[d] >= 0:
            kids[parent[d]].append(d)
    first = [-1] * nn
    for d in range(nn):                       # post-order: children first
        first[d] = leaf[d] if leaf[d] >= 0 else first[kids[d][0]]
    return first, kids


def tip_pairs(parent, leaf):
    """One (internal node v, taxon a, taxon b) per internal node: the first leaf under v's first child and under its second,
    so that v is the most recent common ancestor of a and b."""
    first, kids = first_leaf(parent, leaf)
    return [(v, first[kids[v][0]], first[kids[v][1]]) for v in range(len(parent)) if leaf[v] < 0]


def path_lengths(parent, blen, leaf, pairs):
    """the path length between the two taxa of every pair, through their most recent common ancestor under `parent`"""
    node_of = {int(t): d for d, t in enumerate(leaf) if t >= 0}
    out = []
    for _, a, b in pairs:
        up = {}
        d, acc = node_of[a], 0.0
        while d >= 0:
            up[d] = acc
            acc += blen[d]
            d = parent[d]
        d, acc = node_of[b], 0.0
        while d not in up:
            acc += blen[d]
            d = parent[d]
        out.append(acc + up[d])
    return np.array(out)


def pair_counts(states, pairs):
    """[len(pairs), 16] joint counts, cell 4 x + y for taxon a in state x and taxon b in state y"""
    code = CODE[np.asarray(states)]
    return np.stack([np.bincount(4 * code[a] + code[b], minlength=16) for _, a, b in pairs])


def pair_z(counts, expect_prob, N, min_expected=50.0):
    """z = (count - E) / sqrt(E (1 - E / N)) of every cell of every pair, cells with E < min_expected pooled into one per pair:
    (max |z|, number of cells)."""
    worst, cells = 0.0, 0
    for c, p in zip(np.asarray(counts, np.float64), np.asarray(expect_prob, np.float64)):
        e = N * p
        small = e < min_expected
        o, e2 = c[~small], e[~small]
        if small.any():
            o, e2 = np.append(o, c[small].sum()), np.append(e2, e[small].sum())
        z = (o - e2) / np.sqrt(e2 * (1.0 - e2 / N))
        worst = max(worst, float(np.abs(z).max()))
        cells += len(e2)
    return worst, cells


def redirect_to_grandparent(parent, v):
    """`parent` with node v hung under its grandparent"""
    out = list(parent)
    assert parent[v] >= 0 and parent[parent[v]] >= 0
    out[v] = parent[parent[v]]
    return out


# ---- the two 5-taxon trees and their near-miss laws -------------------------------------------------------------------
PI5 = np.array([0.10, 0.35, 0.15, 0.40])
EXCH5 = np.array([1.3, 1.0, 0.6, 0.9, 2.1, 0.7])
# post-order arrays, root last.  "nested": ((0:.3,1:.8):.25,((2:.1,3:.6):.4,4:.9)) -- the group ((2,3),4) is written without
# a length, which is a branch of length 0 above node 7: an internal node under an internal node under the root, and a
# transition over a zero branch.  "polytomies": (0:.3,(2:.1,3:.6,1:.8):.4,4:.9) -- three children at the root, three inside.
TREES5 = {
    "nested": dict(parent=[2, 2, 8, 5, 5, 7, 7, 8, -1], blen=[0.3, 0.8, 0.25, 0.1, 0.6, 0.4, 0.9, 0.0, 0.0],
                   leaf=[0, 1, -1, 2, 3, -1, 4, -1, -1], node_of_tip={0: 0, 1: 1, 2: 3, 3: 4, 4: 6}, above_23=5),
    "polytomies": dict(parent=[6, 4, 4, 4, 6, 6, -1], blen=[0.3, 0.1, 0.6, 0.8, 0.4, 0.9, 0.0],
                       leaf=[0, 2, 3, 1, -1, 4, -1], node_of_tip={0: 0, 2: 1, 3: 2, 1: 3, 4: 5}, above_23=4),
}
NEAR_MISSES = ("cherry (2,3) swapped", "branch above (2,3) x 1.25", "tips 1 and 4 exchanged", "every branch x 1.05")


def near_miss(tree, which):
    """(blen, leaf) of the near-miss law `which` (an index into NEAR_MISSES) of a TREES5 entry"""
    blen, leaf, at = list(tree["blen"]), list(tree["leaf"]), tree["node_of_tip"]
    if which == 0:
        blen[at[2]], blen[at[3]] = blen[at[3]], blen[at[2]]
    elif which == 1:
        blen[tree["above_23"]] *= 1.25
    elif which == 2:
        leaf[at[1]], leaf[at[4]] = 4, 1
    else:
        blen = [1.05 * b for b in blen]
    return blen, leaf


def laws5(tree_name, model, rate_over_kappa=0.8):
    """(rate, [truth, near-miss 0..3]) as float probability arrays over the 1024 patterns"""
    tree = TREES5[tree_name]
    exch = None if model == "f81" else EXCH5
    rate = rate_over_kappa * hp.kappa(PI5, exch, model)
    laws = [pattern_probabilities(tree["parent"], tree["blen"], tree["leaf"], PI5, exch, rate, model)]
    for w in range(4):
        blen, leaf = near_miss(tree, w)
        laws.append(pattern_probabilities(tree["parent"], blen, leaf, PI5, exch, rate, model))
    return rate, laws


N5 = 2 ** 19      # how it was chosen: the docstring of tests/test_pattern_law.py
CASES5 = [(t, k) for t in ("nested", "polytomies") for k in ("gtr", "f81")]


def score5(counts, laws):
    """[(X^2, df)] of the counts against the truth and the four near-misses"""
    return [pooled_chi2(counts, p) for p in laws]


def check5(name, counts, laws):
    """prints X^2 / df of the truth and the four near-misses and asserts the acceptance and the power"""
    scores = score5(counts, laws)
    x2, df = scores[0]
    print("%s: N = %d, truth X^2 / df = %.3f (df %d, accepted up to %.3f)" % (name, counts.sum(), x2 / df, df, chi2_bound(df, 5) / df))
    for label, (x, d) in zip(NEAR_MISSES, scores[1:]):
        print("    %-28s X^2 / df = %8.3f (df %d, rejected above %.3f)" % (label, x / d, d, chi2_bound(d, 10) / d))
    assert x2 <= chi2_bound(df, 5)
    for x, d in scores[1:]:
        assert x > chi2_bound(d, 10)


# ---- one tip pair per internal node of a deeper tree ---------------------------------------------------------------------
def pair_joint_many(pi, exch, rate, model, lengths):
    """pair_joint for many path lengths, [len, 16] floats: the same matrices from hp_reference's 40-digit eigen-form, which
    costs a fortieth of mpmath's expm per length (tests/test_pattern_law.py holds the two to each other)."""
    M = hp._Model(pi, exch, model)
    out = np.empty((len(lengths), 16))
    with mp.workdps(hp.DPS):
        s = mpmath.mpf(float(rate)) / M.kappa
        for k, d in enumerate(lengths):
            P = M.matrices(_mpf(d) * s, derivs=False)[0]
            out[k] = [float(M.pi[x] * P[x, y]) for x in range(4) for y in range(4)]
    return out


def node_levels(parent):
    """edges between every node and the root (post-order arrays: a parent has a higher index than its children)"""
    lev = [0] * len(parent)
    for d in range(len(parent) - 2, -1, -1):
        lev[d] = lev[parent[d]] + 1
    return lev


def tree_height(parent, blen):
    h = [0.0] * len(parent)
    for d in range(len(parent) - 2, -1, -1):
        h[d] = h[parent[d]] + blen[d]
    return max(h)


def mid_depth_node(parent, blen, leaf):
    """The internal node to hang under its grandparent: among the internal nodes with a grandparent whose level lies in the
    middle third of the tree's levels, the one under the longest parent branch (the first of them).  Redirecting it moves the
    path of every pair that runs through that branch by the branch's length, so the longest branch is the clearest near-miss;
    the choice reads the tree alone."""
    lev = node_levels(parent)
    top = max(lev)
    cand = [v for v in range(len(parent)) if leaf[v] < 0 and parent[v] >= 0 and parent[parent[v]] >= 0
            and top / 3.0 <= lev[v] <= 2.0 * top / 3.0]
    return max(cand, key=lambda v: (blen[parent[v]], -v))


def pair_case(parent, blen, leaf, model, tau=0.5):
    """What the pair tests need of one tree and model: the pairs, the raw rate at which height x rate / kappa = tau, the 16
    joint probabilities of every pair under the tree and under the tree with mid_depth_node hung under its grandparent."""
    exch = None if model == "f81" else EXCH5
    rate = tau / tree_height(parent, blen) * hp.kappa(PI5, exch, model)
    pairs = tip_pairs(parent, leaf)
    v = mid_depth_node(parent, blen, leaf)
    truth = pair_joint_many(PI5, exch, rate, model, path_lengths(parent, blen, leaf, pairs))
    moved = path_lengths(redirect_to_grandparent(parent, v), blen, leaf, pairs)
    return dict(pairs=pairs, rate=rate, node=v, truth=truth, redirected=pair_joint_many(PI5, exch, rate, model, moved))


def separation(case, N, min_expected=50.0):
    """max |z| that counts equal to their expectation under the truth would score against the redirected tree: what the
    near-miss is worth at N columns without any noise"""
    return pair_z(N * case["truth"], case["redirected"], N, min_expected)[0]


def deep_tree(name):
    """(ntaxa, parent, blen, leaf) as lists: the trees of tests/test_gpu_simulate.py (the caterpillar's arrays are the ones that
    file uses; nothing else of simulate_reference is read here) and a Yule tree of 2562 taxa"""
    if name == "caterpillar17":
        import simulate_reference
        return (17,) + simulate_reference.caterpillar(17)
    from tapir_amd import synth
    ntaxa = {"yule70": 70, "yule2562": 2562}[name]
    root, names = synth.yule_tree(ntaxa, 4)
    pin = synth.plan_inputs(root, names)
    return ntaxa, [int(v) for v in pin["parent"]], [float(v) for v in pin["blen"]], [int(v) for v in pin["leaf"]]

"""Brute-force reference of the site concordance counts and a plain-loop mirror of the rows rule.
The counts enumerate every quartet of A x B x C x D explicitly, per column, and classify it by comparing its four cells: no
closed form.  Counts are Python ints.  Test helper."""
import itertools
import math

import numpy as np

ONE_BASE = (1, 2, 4, 8)


def classify(a, b, c, d):
    """0, 1, 2 for a decisive quartet column supporting ab|cd, ac|bd, ad|bc; None otherwise (a cell that is not exactly one
    base, all four alike, or three or more different bases in a way that pairs nothing)."""
    if a not in ONE_BASE or b not in ONE_BASE or c not in ONE_BASE or d not in ONE_BASE:
        return None
    if a == b and c == d and a != c:
        return 0
    if a == c and b == d and a != b:
        return 1
    if a == d and b == c and a != b:
        return 2
    return None


def split_sets(group_offsets, group_taxa):
    """[(A, B, C, D)] as lists of taxon rows, from the CSR tables."""
    goff = [int(v) for v in group_offsets]
    taxa = [int(v) for v in group_taxa]
    assert len(goff) % 4 == 1
    return [tuple(taxa[goff[4 * s + g]:goff[4 * s + g + 1]] for g in range(4)) for s in range(len(goff) // 4)]


def counts(states, locus_offsets, group_offsets, group_taxa):
    """[L][n_sets][3] Python ints: every quartet, every column, one comparison at a time."""
    states = np.asarray(states)
    sets = split_sets(group_offsets, group_taxa)
    off = [int(v) for v in locus_offsets]
    out = []
    for l in range(len(off) - 1):
        cols = [[int(v) for v in states[:, c]] for c in range(off[l], off[l + 1])]
        per_set = []
        for A, B, C, D in sets:
            n = [0, 0, 0]
            for col in cols:
                for a, b, c, d in itertools.product(A, B, C, D):
                    k = classify(col[a], col[b], col[c], col[d])
                    if k is not None:
                        n[k] += 1
            per_set.append(n)
        out.append(per_set)
    return out


def counts_np(states, locus_offsets, group_offsets, group_taxa, chunk=4096):
    """counts() with the columns of a chunk of quartets compared at once by numpy: still every quartet of A x B x C x D listed
    and classified cell by cell (the same three comparisons), for shapes the Python loops are too slow for.  uint64
    [L, n_sets, 3] (the sums of a locus must stay below 2^63)."""
    states = np.asarray(states, dtype=np.uint8)
    sets = split_sets(group_offsets, group_taxa)
    off = np.asarray(locus_offsets, dtype=np.int64)
    out = np.zeros((len(off) - 1, len(sets), 3), dtype=np.uint64)
    one = np.isin(states, ONE_BASE)
    for s, (A, B, C, D) in enumerate(sets):
        per_col = np.zeros((3, states.shape[1]), dtype=np.int64)
        quartets = itertools.product(A, B, C, D)
        while True:
            idx = np.array(list(itertools.islice(quartets, chunk)), dtype=np.int64).reshape(-1, 4)
            if len(idx) == 0:
                break
            a, b, c, d = (states[idx[:, g]] for g in range(4))
            ok = one[idx[:, 0]] & one[idx[:, 1]] & one[idx[:, 2]] & one[idx[:, 3]]
            per_col[0] += (ok & (a == b) & (c == d) & (a != c)).sum(axis=0)
            per_col[1] += (ok & (a == c) & (b == d) & (a != b)).sum(axis=0)
            per_col[2] += (ok & (a == d) & (b == c) & (a != b)).sum(axis=0)
        for l in range(len(off) - 1):
            out[l, s] = per_col[:, off[l]:off[l + 1]].sum(axis=1).astype(np.uint64)
    return out


def closed_form(column, A, B, C, D):
    """(conc, disc1, disc2) of one column from the groups' base counts -- the formula the kernel uses, held against the
    enumeration by tests/test_concordance.py."""
    def base_counts(G):
        return [sum(1 for t in G if int(column[t]) == m) for m in ONE_BASE]
    a, b, c, d = (base_counts(G) for G in (A, B, C, D))
    dot = lambda u, v: sum(x * y for x, y in zip(u, v))   # noqa: E731
    every = sum(a[x] * b[x] * c[x] * d[x] for x in range(4))
    return (dot(a, b) * dot(c, d) - every, dot(a, c) * dot(b, d) - every, dot(a, d) * dot(b, c) - every)


def rows(counts_, node_sets):
    """The rows rule in plain loops: counts_ [L][n_sets][3] integers -> float64 [L, n_nodes, 12]."""
    nodes = [int(v) for v in node_sets]
    L = len(counts_)
    out = np.zeros((L, len(nodes) - 1, 12))
    for l in range(L):
        for i in range(len(nodes) - 1):
            s0, s1 = nodes[i], nodes[i + 1]
            row = [float(int(v)) for v in counts_[l][s0]] + [float(int(v)) for v in counts_[l][s0 + 1]]
            f = [0.0, 0.0, 0.0]
            n, decisive = 0.0, 0
            for s in range(s0 + 2, s1):
                k = [float(int(v)) for v in counts_[l][s]]
                dec = k[0] + k[1] + k[2]
                if dec > 0.0:
                    for j in range(3):
                        f[j] = f[j] + k[j] / dec
                    n = n + dec
                    decisive += 1
            means = [v / float(decisive) for v in f + [n]] if decisive else [math.nan] * 4
            out[l, i] = row + means + [float(decisive), float(s1 - s0 - 2)]
    return out


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------
def csr(sets):
    """[(A, B, C, D)] -> (group_offsets, group_taxa)"""
    sizes = [len(g) for groups in sets for g in groups]
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
            np.array([t for groups in sets for g in groups for t in g], dtype=np.int32))


def shaped_sets(rng, ntaxa, shapes):
    """One set per shape (|A|, |B|, |C|, |D|): taxa drawn without replacement, in no order; what is left belongs to no group."""
    out = []
    for shape in shapes:
        pick = rng.permutation(ntaxa)[:sum(shape)].tolist()
        cuts = np.cumsum((0,) + tuple(shape))
        out.append(tuple(pick[cuts[g]:cuts[g + 1]] for g in range(4)))
    return out


SHAPES = [(1, 1, 1, 1), (1, 1, 1, 6), (2, 3, 1, 3)]


def stored(row):
    """A row of 12 as the file stores it (15 values)."""
    pooled = [int(v) for v in row[:3]]
    total = sum(pooled)
    return (pooled + [p / total if total else None for p in pooled] + [int(v) for v in row[3:6]]
            + [None if math.isnan(v) else v for v in row[6:10]] + [int(row[10]), int(row[11])])

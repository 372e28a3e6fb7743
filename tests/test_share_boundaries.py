"""The share boundaries by predicted work and compact_kernel's reserve rule, in their numpy restatement (tools/share_replay.py:
reserve_split, class_prefixes, work_shares -- the integer arithmetic of site_rate_kernel.hpp / site_rate_params.hpp), on
random per-locus class counts including zeros."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import share_replay as rp  # noqa: E402

W_SLOW, W_EASY = rp.fixed(2.9, rp.WEIGHT_SHIFT), rp.fixed(2.04, rp.WEIGHT_SHIFT)


def _counts(rng, nloci):
    """Class counts of `nloci` loci: a third of the loci have no slow, no easy or no column at all."""
    n_slow = rng.integers(0, 400, size=nloci)
    n_easy = rng.integers(0, 1500, size=nloci)
    kind = rng.integers(0, 9, size=nloci)
    n_slow[(kind == 0) | (kind == 2)] = 0
    n_easy[(kind == 1) | (kind == 2)] = 0
    n_easy[kind == 3] = rng.integers(1, 4, size=int((kind == 3).sum()))     # fewer easy columns than a reserve takes one of
    return n_slow, n_easy


def _marks(rng, n_slow, n_easy):
    m = np.zeros(n_slow + n_easy, dtype=bool)
    m[rng.permutation(n_slow + n_easy)[:n_slow]] = True
    return m


CASES = [(seed, nloci, frac, main, nshares) for seed, (nloci, frac, main, nshares) in enumerate([
    (1, 0.25, 16, 48), (7, 0.25, 16, 48), (40, 0.4, 5, 35), (3, 0.1, 37, 74), (12, 1.0, 16, 48), (9, 0.0, 48, 48), (2, 0.25, 300, 2100)])]


@pytest.mark.parametrize("seed,nloci,frac,main,nshares", CASES)
def test_shares_partition_the_list_and_are_balanced(seed, nloci, frac, main, nshares):
    rng = np.random.default_rng(100 + seed)
    n_slow, n_easy = _counts(rng, nloci)
    q = rp.fixed(frac, rp.RESERVE_SHIFT)
    shares, mpre, tpre = rp.work_shares(n_slow, n_easy, q, W_SLOW, W_EASY, main, nshares)
    assert len(shares) == nshares
    tail = rp.reserved_before(n_easy, q)
    assert np.array_equal(np.diff(tpre), tail) and np.array_equal(np.diff(mpre), n_slow + n_easy - tail)
    # (1) the main shares tile [0, main columns), the tail shares [0, tail columns): nothing lost, nothing twice
    for in_tail, total in ((False, int(mpre[-1])), (True, int(tpre[-1]))):
        part = [(g0, g1) for t, g0, g1 in shares if t == in_tail]
        if not part:
            assert total == 0
            continue
        assert part[0][0] == 0 and part[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(part, part[1:])) and all(g0 <= g1 for g0, g1 in part)
    assert [t for t, _, _ in shares] == [False] * main + [True] * (nshares - main)
    # (2) predicted work of the main shares, in the measure the boundaries are cut in: the class COUNTS of a locus, its work
    # spread evenly over its columns (so the interpolation inside a locus is exact by definition, and what is bounded is the
    # rounding of the cuts to whole columns).  Where the slow columns of a locus actually lie does not enter the boundaries and
    # is not tested here: two shares of one locus differ in true predicted work by however unevenly its marks are spread.
    # A cut falls on a whole column of its locus: below the exact cut by less than one
    # column, whose weight depends on where the locus' slow columns lie -- the prediction smears them evenly (work of the locus
    # / its columns per column).  So two shares differ by at most one column's (largest) weight at either end in that even
    # measure, plus 1 for the floor of the target.
    _, wpre, _ = rp.class_prefixes(n_slow, n_easy, q, W_SLOW, W_EASY)
    nm, ww = np.diff(mpre), np.diff(wpre)

    def even_work(g):   # predicted work of the first g main columns, the locus' work spread evenly over its columns
        l = int(np.searchsorted(mpre, g, side="right")) - 1
        l = min(l, len(nm) - 1)
        return float(wpre[l]) + (float(ww[l]) * (g - int(mpre[l])) / float(nm[l]) if nm[l] else 0.0)

    work = np.array([even_work(g1) - even_work(g0) for t, g0, g1 in shares if not t])
    if int(wpre[-1]) > 0:
        assert work.max() - work.min() <= 2 * max(W_SLOW, W_EASY) + 2, (work.max(), work.min())
        assert abs(work.sum() - float(wpre[-1])) < 1e-6 * float(wpre[-1]) + 1
    # (3) the tail shares' column counts differ by at most 1
    tails = np.array([g1 - g0 for t, g0, g1 in shares if t])
    if len(tails):
        assert tails.max() - tails.min() <= 1 and tails.sum() == int(tpre[-1])


@pytest.mark.parametrize("frac", [0.0, 0.1, 0.25, 0.5, 1.0])
def test_reserve_rule_sees_its_locus_only(frac):
    """The reserve set of a locus is a function of the locus' own marks: main part and tail are a stable partition of its list,
    the tail holds floor(frac * easy) easy columns spread over the locus, and other loci do not enter (reserve_split takes one
    locus; the per-locus prefixes only shift when loci are added or removed)."""
    rng = np.random.default_rng(7)
    q = rp.fixed(frac, rp.RESERVE_SHIFT)
    loci = [_marks(rng, s, e) for s, e in ((0, 0), (5, 0), (0, 3), (0, 1), (17, 400), (300, 299), (1, 1000))]
    split = [rp.reserve_split(m, q) for m in loci]
    for m, (mi, ti) in zip(loci, split):
        n_easy = int((~m).sum())
        assert len(ti) == int(rp.reserved_before(n_easy, q)) and not m[ti].any()
        assert np.array_equal(np.sort(np.concatenate([mi, ti])), np.arange(len(m)))      # a partition ...
        assert np.all(np.diff(mi) > 0) and np.all(np.diff(ti) > 0)                       # ... in list order
        if frac == 0.0:
            assert len(ti) == 0 and np.array_equal(mi, np.arange(len(m)))                # the old list, entry for entry
        if len(ti) > 1:   # every k-th easy column: the ranks of the reserved ones are evenly spaced
            rank = (np.cumsum(~m) - 1)[ti]
            assert np.diff(rank).max() - np.diff(rank).min() <= 1
    # The rule as the kernel applies it, on whole batches (reserve_batch: loci concatenated, ranks counted from each locus'
    # offset): a locus' reserved columns are the same whichever loci stand before or after it -- alone, reordered, with loci
    # removed -- and the per-locus prefixes are those of its own counts.
    for keep in ([4], [6, 4, 2], [0, 1, 4, 5], [5, 3, 6, 0, 4, 1, 2], list(range(7))):
        marks = np.concatenate([loci[i] for i in keep]) if keep else np.zeros(0, dtype=bool)
        woff = np.concatenate([[0], np.cumsum([len(loci[i]) for i in keep])])
        res = rp.reserve_batch(marks, woff, q)
        n_slow = [int(loci[i].sum()) for i in keep]
        n_easy = [int((~loci[i]).sum()) for i in keep]
        mpre, _, tpre = rp.class_prefixes(n_slow, n_easy, q, W_SLOW, W_EASY)
        for k, i in enumerate(keep):
            mine = res[woff[k]:woff[k + 1]]
            assert np.array_equal(np.flatnonzero(mine), split[i][1]), (keep, i)
            assert np.array_equal(np.flatnonzero(~mine), split[i][0]), (keep, i)
            assert tpre[k + 1] - tpre[k] == mine.sum() and mpre[k + 1] - mpre[k] == len(mine) - mine.sum()

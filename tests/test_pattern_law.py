"""The exact site-pattern law (tests/pattern_law_reference.py) held to itself, and the CPU mirror of the column simulation
(tests/simulate_reference.py) held to it, without a GPU.  tests/test_gpu_simulate_law.py asks the same of the kernel.  Every test
prints its figures before it asserts.

The law itself: the 4^n probabilities sum to 1 within 1e-30, the two-taxon law is pair_joint (mpmath's expm, not the
eigen-form), summing a tip out gives the law of the pruned tree (a branch of length a + b for the two it merges), and the
probabilities are exp(F) of hp_reference.column_curves.

Full pattern law on two 5-taxon trees (pattern_law_reference.TREES5), GTR and F81, rate 0.8 kappa, one locus of N columns with
stream id 0, replicate 0, seed 1, no mask.  Pearson X^2 over the 1024 patterns, cells with an expected count below 5 pooled into
one, df = cells - 1.  The truth is accepted at X^2 <= df + 5 sqrt(2 df) (Z_BOUND = 5 of test_simulate.py); each of four
near-miss laws must give X^2 > df + 10 sqrt(2 df) on the same counts.

N = 2^19: the smallest power of two in 2^16..2^20 at which the mirror, with seed 1, accepts the truth and rejects all four
near-misses in all four cases (the x 1.05 near-miss is the last to fall: at 2^18 it scores 1.377 against 1.446 on nested/gtr).
Seed 1 was the first and only seed tried.  The mirror's X^2 / df at N = 2^19 (acceptance at about 1.22, rejection above about
1.44; near-misses in the order of pattern_law_reference.NEAR_MISSES):

                      truth   cherry swapped   above (2,3) x 1.25   tips 1, 4 exchanged   all x 1.05
  nested      gtr     0.936       131.386             2.486                41.489             1.859
  nested      f81     0.923       165.347             2.793                50.918             2.068
  polytomies  gtr     0.955       260.650             3.194               191.807             1.974
  polytomies  f81     0.986       321.622             3.452               222.457             2.032

One tip pair per internal node (pattern_law_reference.tip_pairs; height x rate / kappa = 0.5, 16 joint frequencies per pair
against pair_joint of the path length, cells with an expected count below 50 pooled, z = (count - E) / sqrt(E (1 - E / N))): the
mirror on caterpillar17 and yule70 at 65 536 columns, max |z| <= 5.  Seed 1 was the only seed tried.  The mirror's max |z|:
caterpillar17 gtr 3.17, f81 3.42 (256 cells); yule70 gtr 3.57, f81 3.18 (1103 cells).  On the 2562-taxon tree at 16 384 columns
the mirror, run once by hand (25 s per model: too long for this suite), gave 4.28 (gtr, 38 726 cells) and 4.17 (f81, 38 926
cells) against the bound of 6, and 31.51 and 24.70 against the tree with node 4063 under its grandparent.

The power of the pair statistic is a property of the two laws and N, printed as "without noise": the max |z| that counts equal
to their expectation would score against the redirected tree.  On the two Yule trees it is 24 to 31.  On caterpillar17 no node
reaches 10 at 65 536 columns: redirecting a node moves paths by one internal branch, at most 8 % of the height, which is worth
5.58 at the best node and 4.36 to 4.89 at the mid-depth one.  The GPU test therefore asks the factor of 10 of caterpillar17 on
2^20 columns (16 times the columns, 4 times the separation: 17.4 to 19.6), where it also repeats the acceptance.
"""
import mpmath
import numpy as np
import pytest

import hp_reference as hp
import pattern_law_reference as plr
import simulate_reference as sim

N5, CASES5, check5, deep_tree = plr.N5, plr.CASES5, plr.check5, plr.deep_tree


def mirror_model(kind, pi=plr.PI5):
    return sim.eigen_system(pi, plr.EXCH5) if kind == "gtr" else sim.f81_system(pi)


# ---- the law against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree, kind", CASES5)
def test_probabilities_sum_to_one(tree, kind):
    t = plr.TREES5[tree]
    exch = None if kind == "f81" else plr.EXCH5
    p = plr.pattern_probabilities(t["parent"], t["blen"], t["leaf"], plr.PI5, exch, 0.8 * hp.kappa(plr.PI5, exch, kind), kind, as_mpf=True)
    with mpmath.mp.workdps(hp.DPS):
        off = abs(mpmath.fsum(p) - 1)
        print("%s %s: |sum - 1| = %s, smallest probability %s" % (tree, kind, mpmath.nstr(off, 3), mpmath.nstr(min(p), 3)))
        assert len(p) == 1024 and min(p) > 0 and off <= mpmath.mpf("1e-30")


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_two_taxa_equal_pair_joint(kind):
    exch = None if kind == "f81" else plr.EXCH5
    rate = 0.8 * hp.kappa(plr.PI5, exch, kind)
    p = plr.pattern_probabilities([2, 2, -1], [0.7, 0.4, 0.0], [0, 1, -1], plr.PI5, exch, rate, kind, as_mpf=True)
    with mpmath.mp.workdps(hp.DPS):
        d = mpmath.mpf(0.7) + mpmath.mpf(0.4)         # the sum of the two fp64 lengths, which is not the fp64 number 1.1
    J = plr.pair_joint(plr.PI5, exch, rate, kind, d, as_mpf=True)
    many = plr.pair_joint_many(plr.PI5, exch, rate, kind, [d])[0]
    with mpmath.mp.workdps(hp.DPS):
        worst = max(abs(p[x + 4 * y] - J[x][y]) for x in range(4) for y in range(4))     # taxon 0 in x, taxon 1 in y
        print("%s: worst |pattern law - pair_joint| = %s" % (kind, mpmath.nstr(worst, 3)))
        assert worst <= mpmath.mpf("1e-30")
        assert all(many[4 * x + y] == float(J[x][y]) for x in range(4) for y in range(4))
    # the joint law is not symmetric under GTR's pi but is under exchange of the tips (reversibility)
    assert max(abs(J[x][y] - J[y][x]) for x in range(4) for y in range(4)) <= mpmath.mpf("1e-30")


@pytest.mark.parametrize("tree, kind", CASES5)
def test_summing_out_a_tip_gives_the_pruned_tree(tree, kind):
    """nested without tip 4: node 7 keeps one child, so (2,3) hangs on the root by 0.4 + 0.  polytomies without tip 1: the
    inner trifurcation becomes the cherry (2,3).  Tip 4 (tip 1) is the slowest (second) digit of the pattern number."""
    exch = None if kind == "f81" else plr.EXCH5
    rate = 0.8 * hp.kappa(plr.PI5, exch, kind)
    t = plr.TREES5[tree]
    full = np.array(plr.pattern_probabilities(t["parent"], t["blen"], t["leaf"], plr.PI5, exch, rate, kind, as_mpf=True), object)
    if tree == "nested":
        pruned = plr.pattern_probabilities([2, 2, 6, 5, 5, 6, -1], [0.3, 0.8, 0.25, 0.1, 0.6, 0.4 + 0.0, 0.0], [0, 1, -1, 2, 3, -1, -1],
                                           plr.PI5, exch, rate, kind, as_mpf=True)
        with mpmath.mp.workdps(hp.DPS):
            summed = full.reshape(4, 256).sum(axis=0)                                    # taxa 0..3 keep their digits
    else:
        pruned = plr.pattern_probabilities([5, 3, 3, 5, 5, -1], [0.3, 0.1, 0.6, 0.4, 0.9, 0.0], [0, 1, 2, -1, 3, -1],
                                           plr.PI5, exch, rate, kind, as_mpf=True)     # taxa 0, 2, 3, 4 renumbered 0, 1, 2, 3
        with mpmath.mp.workdps(hp.DPS):
            summed = full.reshape(64, 4, 4).sum(axis=1).reshape(256)
    with mpmath.mp.workdps(hp.DPS):
        worst = max(abs(a - b) for a, b in zip(summed, pruned))
        print("%s %s: worst |marginal - pruned tree| = %s" % (tree, kind, mpmath.nstr(worst, 3)))
        assert worst <= mpmath.mpf("1e-30")


def test_probabilities_are_exp_of_column_curves():
    t = plr.TREES5["nested"]
    for kind in ("gtr", "f81"):
        exch = None if kind == "f81" else plr.EXCH5
        kappa = hp.kappa(plr.PI5, exch, kind)
        p = plr.pattern_probabilities(t["parent"], t["blen"], t["leaf"], plr.PI5, exch, 0.8 * kappa, kind)
        cols = plr.all_columns(5)[:, ::37]
        F = hp.column_curves(cols, t["parent"], t["blen"], t["leaf"], plr.PI5, exch, [np.log(0.8 * kappa / kappa)], model=kind)[0][0]
        worst = float(np.max(np.abs(np.exp(F) / p[::37] - 1.0)))
        print("%s: worst |exp(F) / p - 1| over %d patterns = %.3g" % (kind, cols.shape[1], worst))
        assert worst <= 1e-13     # F rounded to fp64 (|F| < 16: 16 x 2^-53), u rounded to fp64, exp's own ulp


# ---- the mirror against the law: 5-taxon trees ------------------------------------------------------------------------
@pytest.mark.parametrize("tree, kind", CASES5)
def test_mirror_draws_the_pattern_law(tree, kind):
    t = plr.TREES5[tree]
    rate, laws = plr.laws5(tree, kind)
    out = sim.simulate_locus(t["parent"], t["blen"], t["leaf"], 5, mirror_model(kind), np.full(N5, rate), stream_id=0, b=0, seed=1)
    assert out["undecided"] == 0
    check5("mirror %s %s" % (tree, kind), plr.pattern_counts(out["states"]), laws)


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_mirror_never_draws_an_absent_base(kind):
    """pi_T = 0 (F81: exactly; GTR: floored at 1e-12 as a plan floors it, 9 x 65 536 x 1e-12 expected draws): no cell is T."""
    t = plr.TREES5["nested"]
    pi = np.array([0.3, 0.3, 0.4, 0.0])
    model = mirror_model(kind, hp.floored_pi(pi) if kind == "gtr" else pi)
    out = sim.simulate_locus(t["parent"], t["blen"], t["leaf"], 5, model, np.full(65536, 0.8 * model["kappa"]), stream_id=0, b=0, seed=1)
    seen = sorted(set(out["states"].ravel().tolist()))
    print("%s: cell values seen %s" % (kind, seen))
    assert seen == [1, 2, 4]


# ---- pairs: one tip pair per internal node ----------------------------------------------------------------------------
def test_every_internal_node_has_its_pair():
    for name in ("caterpillar17", "yule70", "yule2562"):
        ntaxa, parent, blen, leaf = deep_tree(name)
        pairs = plr.tip_pairs(parent, leaf)
        assert [v for v, _, _ in pairs] == [v for v in range(len(parent)) if leaf[v] < 0] and len(pairs) == ntaxa - 1
        node_of = {t: d for d, t in enumerate(leaf) if t >= 0}
        for v, a, b in pairs[::max(1, len(pairs) // 40)]:          # v is the first node the two tips' paths to the root share
            up = set()
            d = node_of[a]
            while d >= 0:
                up.add(d)
                d = parent[d]
            d = node_of[b]
            while d not in up:
                d = parent[d]
            assert d == v


@pytest.mark.parametrize("kind", ["gtr", "f81"])
@pytest.mark.parametrize("name", ["caterpillar17", "yule70"])
def test_mirror_pair_frequencies(name, kind):
    ntaxa, parent, blen, leaf = deep_tree(name)
    c = plr.pair_case(parent, blen, leaf, kind)
    N = 65536
    out = sim.simulate_locus(parent, blen, leaf, ntaxa, mirror_model(kind), np.full(N, c["rate"]), stream_id=0, b=0, seed=1)
    counts = plr.pair_counts(out["states"], c["pairs"])
    z, cells = plr.pair_z(counts, c["truth"], N)
    z_alt, _ = plr.pair_z(counts, c["redirected"], N)
    print("mirror %s %s: max |z| = %.2f over %d cells of %d pairs; node %d under its grandparent: %.2f (without noise %.2f)"
          % (name, kind, z, cells, len(c["pairs"]), c["node"], z_alt, plr.separation(c, N)))
    assert out["undecided"] == 0
    assert cells < 10000 and z <= 5.0


def test_pair_joint_many_is_pair_joint():
    """The eigen-form the long pair lists use against mpmath's expm, on eight path lengths of the 2562-taxon tree."""
    ntaxa, parent, blen, leaf = deep_tree("yule2562")
    pairs = plr.tip_pairs(parent, leaf)
    lengths = plr.path_lengths(parent, blen, leaf, pairs)[::330]
    rate = 0.5 / plr.tree_height(parent, blen) * hp.kappa(plr.PI5, plr.EXCH5, "gtr")
    many = plr.pair_joint_many(plr.PI5, plr.EXCH5, rate, "gtr", lengths)
    worst = max(float(np.max(np.abs(many[k] - plr.pair_joint(plr.PI5, plr.EXCH5, rate, "gtr", d).ravel()))) for k, d in enumerate(lengths))
    print("worst |eigen-form - expm| over %d lengths: %.3g" % (len(lengths), worst))
    assert len(lengths) == 8 and worst <= 2.0 ** -53

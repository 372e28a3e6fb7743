"""simulate_columns_kernel against the mathematics on trees with internal structure (run with -m gpu on the MI355X box).  Nothing
here compares bytes with the mirror (tests/test_gpu_simulate.py does); every reference is the exact law of
tests/pattern_law_reference.py or the plan's own likelihood kernels.  Every test prints its figures before it asserts.

1. Full pattern law on the two 5-taxon trees of pattern_law_reference.TREES5 (an internal node under an internal node over a
   zero branch; trifurcations at the root and inside), GTR and F81, rate 0.8 kappa, one locus of N = 2^19 columns, replicate 0,
   seed 1, no mask.  Pearson X^2 over the 1024 patterns, cells with an expected count below 5 pooled, df = cells - 1: the truth
   is accepted at X^2 <= df + 5 sqrt(2 df), and each of four near-miss laws (the cherry's two lengths swapped, the branch above
   it x 1.25, tips 1 and 4 exchanged, every branch x 1.05) must give X^2 > df + 10 sqrt(2 df) on the same counts.  N and the
   mirror's eight X^2 / df per case are in tests/test_pattern_law.py, which asks the same of the mirror; seed 1 was the first and
   only seed tried.  With pi_T = 0 no simulated cell is T.

2. One tip pair per internal node of caterpillar17, yule70 and a Yule tree of 2562 taxa (2561 internal nodes: 161 packed
   words, block of 128 threads, 82 432 bytes of LDS): the first leaf under the node's first child and under its second, so every
   slot of every packed word decides a pair.  Height x rate / kappa = 0.5; N = 65 536, 65 536 and 16 384.  Per pair the 16 joint
   frequencies against pair_joint of the path length, cells with an expected count below 50 pooled, z = (count - E) /
   sqrt(E (1 - E / N)); max |z| <= 5 with fewer than 10 000 cells and 6 above.  The same counts against the tree with one
   mid-depth internal node (pattern_law_reference.mid_depth_node) hung under its grandparent must give max |z| > 10.  The mirror's
   figures are in tests/test_pattern_law.py; of the 2562-taxon tree this suite runs the kernel only (the mirror was run once by
   hand).  caterpillar17's internal branches are at most 8 % of its height, which no node's redirection turns into a max |z| of
   10 at 65 536 columns (5.58 without noise at the best node); it is accepted at 65 536 columns as stated and, for the factor
   of 10, simulated once more at 2^20 columns, where the acceptance is asserted again.

3. The simulator against the likelihood kernels: 65 536 columns of caterpillar17 and of yule70 at one rate r0, (f, g, h) =
   eval_columns at u0 = log(r0 / kappa).  Under the truth the score g has mean 0 and variance minus the mean curvature:
   |mean g| <= 5 sd(g) / sqrt(N) and |mean(g^2 + h)| <= 5 sd(g^2 + h) / sqrt(N) (sample sds); at u0 + 0.1 the first fails by a
   factor of 2 or more.  Neither the mirror nor mpmath takes part: kappa is sum_i pi_i (-Q_ii) in numpy.

Figures on the MI355X are in DESIGN.md section 5.
"""
import functools

import numpy as np
import pytest

import pattern_law_reference as plr
from pattern_law_reference import N5, CASES5, check5, deep_tree

pytestmark = pytest.mark.gpu


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def simulate(engine, ntaxa, parent, blen, leaf, kind, rate, n, pi=plr.PI5):
    """one locus of n columns at one rate, replicate 0, seed 1, no mask"""
    plan = engine.Plan(ntaxa, parent, blen, leaf, [0, n], [pi], None if kind == "f81" else [plr.EXCH5], 5, [], [], model=kind)
    try:
        return plan.simulate_columns(np.full(n, rate), replicate=0, seed=1)
    finally:
        plan.close()


# ---- 1. the full pattern law -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree, kind", CASES5)
def test_kernel_draws_the_pattern_law(tree, kind):
    engine = _engine()
    t = plr.TREES5[tree]
    rate, laws = plr.laws5(tree, kind)
    got = simulate(engine, 5, t["parent"], t["blen"], t["leaf"], kind, rate, N5)
    check5("GPU %s %s" % (tree, kind), plr.pattern_counts(got), laws)


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_kernel_never_draws_an_absent_base(kind):
    engine = _engine()
    t = plr.TREES5["nested"]
    pi = np.array([0.3, 0.3, 0.4, 0.0])
    kappa = numpy_kappa(kind, pi)
    got = simulate(engine, 5, t["parent"], t["blen"], t["leaf"], kind, 0.8 * kappa, 65536, pi=pi)
    seen = sorted(set(got.ravel().tolist()))
    print("GPU %s, pi_T = 0: cell values seen %s" % (kind, seen))
    assert seen == [1, 2, 4]


# ---- 2. one tip pair per internal node ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_case(name, kind):
    ntaxa, parent, blen, leaf = deep_tree(name)
    return (ntaxa, parent, blen, leaf), plr.pair_case(parent, blen, leaf, kind)


def pair_scores(engine, name, kind, n):
    (ntaxa, parent, blen, leaf), c = pair_case(name, kind)
    got = simulate(engine, ntaxa, parent, blen, leaf, kind, c["rate"], n)
    counts = plr.pair_counts(got, c["pairs"])
    z, cells = plr.pair_z(counts, c["truth"], n)
    z_alt, _ = plr.pair_z(counts, c["redirected"], n)
    print("GPU %s %s, N = %d: max |z| = %.2f over %d cells of %d pairs; node %d under its grandparent: %.2f (without noise %.2f)"
          % (name, kind, n, z, cells, len(c["pairs"]), c["node"], z_alt, plr.separation(c, n)))
    return z, cells, z_alt


@pytest.mark.parametrize("kind", ["gtr", "f81"])
@pytest.mark.parametrize("name, n", [("caterpillar17", 65536), ("yule70", 65536), ("yule2562", 16384)])
def test_every_internal_node_decides_its_pair(name, n, kind):
    engine = _engine()
    z, cells, z_alt = pair_scores(engine, name, kind, n)
    assert z <= (5.0 if cells < 10000 else 6.0)
    if name == "caterpillar17":       # see the module docstring: the factor of 10 needs 2^20 columns on this tree
        z, cells, z_alt = pair_scores(engine, name, kind, 2 ** 20)
        assert cells < 10000 and z <= 5.0
    assert z_alt > 10.0


# ---- 3. the simulator against the likelihood kernels ---------------------------------------------------------------------
def numpy_kappa(kind, pi=plr.PI5):
    pi = np.asarray(pi, np.float64) / np.sum(pi)
    if kind == "f81":
        return float(1.0 - (pi * pi).sum())
    R = np.zeros((4, 4))
    for k, (i, j) in enumerate([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]):
        R[i, j] = R[j, i] = plr.EXCH5[k]
    Q = R * pi[None, :]
    return float((pi * Q.sum(axis=1)).sum())      # sum_i pi_i (-Q_ii), Q_ii = -sum_j Q_ij


@pytest.mark.parametrize("kind", ["gtr", "f81"])
@pytest.mark.parametrize("name", ["caterpillar17", "yule70"])
def test_score_of_simulated_columns_under_the_likelihood_kernels(name, kind):
    engine = _engine()
    ntaxa, parent, blen, leaf = deep_tree(name)
    n = 65536
    kappa = numpy_kappa(kind)
    r0 = 0.5 / plr.tree_height(parent, blen) * kappa
    plan = engine.Plan(ntaxa, parent, blen, leaf, [0, n], [plr.PI5], None if kind == "f81" else [plr.EXCH5], 5, [], [], model=kind)
    try:
        st = plan.simulate_columns(np.full(n, r0), replicate=0, seed=1)
        u0 = np.log(r0 / kappa)
        f, g, h = plan.eval_columns(st, np.full(n, u0))
        _, g1, _ = plan.eval_columns(st, np.full(n, u0 + 0.1))
        plan_kappa = float(plan.models()[3][0])
    finally:
        plan.close()
    info = g * g + h
    b_g, b_i, b_1 = (5.0 * float(np.std(v, ddof=1)) / np.sqrt(n) for v in (g, info, g1))
    print("GPU %s %s: kappa %.6f (plan %.6f), mean g = %+.5f (bound %.5f), mean(g^2 + h) = %+.5f (bound %.5f), at u0 + 0.1 mean g = "
          "%+.5f (bound %.5f: %.1f x)" % (name, kind, kappa, plan_kappa, g.mean(), b_g, info.mean(), b_i, g1.mean(), b_1, abs(g1.mean()) / b_1))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g)) and np.all(np.isfinite(h))
    assert abs(g.mean()) <= b_g
    assert abs(info.mean()) <= b_i
    assert abs(g1.mean()) > 2.0 * b_1

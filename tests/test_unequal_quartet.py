"""Quartet signal and noise with unequal tips, without a GPU: the definition
(tests/unequal_quartet_reference.py: the fp64 restatement against the 40-digit twin, the symmetries, the probability rule
against mpmath, the normal approximation against the exact distribution), compute.tree_quartets, and the host layers above
the engine -- pipeline.unequal_quartet_tables, the --unequal-quartets / --tree-quartets flags and the third sqlite file -- on
the CPU stand-in engine (tests/unequal_quartet_engine.py).

Bounds:
  restatement against the twin   64 * 2^-52 relative.  y, x1 and x2 are sums of non-negative products of five matrix entries
                                 and a frequency; an entry carries a few units (eigh's backward error on a well-separated
                                 4 x 4 spectrum, an expm1, a three-term sum), five entries per product, and the sums of
                                 non-negative terms add at most their length in units to a term's error but no more than the
                                 largest term error to the relative error of the sum.  A reference of exactly 0 must be 0.
  B against mpmath               1e-13 absolute at |rho| <= 0.999 (section 3.8's table: 2.3e-15 measured)
  normal against exact           0.05 where the largest expected count is at least 1 (section 3.6's documented largest gap)
"""
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import quartet_reference as qr
import unequal_quartet_engine
import unequal_quartet_reference as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52

GTR = dict(model="gtr", pi=[0.31, 0.19, 0.27, 0.23], exch=[1.0, 2.7, 0.6, 1.2, 3.1, 0.9])
F81 = dict(model="f81", pi=[0.4, 0.0, 0.35, 0.25], exch=[1.0] * 6)          # one absent base
JC = dict(model="f81", pi=[0.25] * 4, exch=[1.0] * 6)
# all tips 0; equal tips; Ta != Tb only; the long-branch case and its mirror; one tip 0; t_o from 1e-3 to 50; tips of 300
QUARTETS = [((0.0, 0.0, 0.0, 0.0), 1e-3), ((20.0, 20.0, 20.0, 20.0), 5.0), ((20.0, 35.0, 27.0, 27.0), 5.0),
            ((100.0, 5.0, 100.0, 5.0), 2.0), ((100.0, 5.0, 5.0, 100.0), 2.0), ((0.0, 12.0, 7.5, 30.0), 3.0),
            ((1.0, 2.0, 3.0, 4.0), 50.0), ((300.0, 300.0, 300.0, 300.0), 0.5), ((300.0, 1e-2, 64.0, 3.0), 1e-3)]


def _rates():
    rng = np.random.default_rng(20261019)
    return np.concatenate([10.0 ** rng.uniform(-9, 3, 6), [0.0, np.nan, 1e4, 1e-9]])


# ---- the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, m", [("gtr", GTR), ("f81", F81), ("jc", JC)])
def test_restatement_against_the_40_digit_twin(name, m):
    rates = _rates()
    worst = 0.0
    for tips, internode in QUARTETS:
        twin = ur.twin_values(m["pi"], m["exch"], rates, tips, internode)
        got = ur.site_values(m["model"], m["pi"], m["exch"], rates, tips, internode)
        errs = []
        for g, t in zip(got, twin):
            e, zeros_ok = qr.relative_error(g, t)
            assert zeros_ok                                # culled and zero rates, and the noise at all tips 0: exactly 0
            assert g[6] == 0.0 and g[7] == 0.0
            errs.append(e)
        print("%s tips=%s to=%g: relative error of y %.2e, x1 %.2e, x2 %.2e (bound %.2e)" % ((name, tips, internode) + tuple(errs) + (64 * U,)))
        if not any(tips):
            assert np.all(got[1] == 0.0) and np.all(got[2] == 0.0) and all(v == 0 for v in twin[1]) and all(v == 0 for v in twin[2])
        worst = max(worst, *errs)
        assert max(errs) <= 64 * U
    print("%s: largest relative error of the restatement %.2e = %.1f * 2^-52" % (name, worst, worst / U))


def test_symmetries_of_the_restatement_and_of_the_twin():
    import mpmath as mp
    rates = np.array([1e-3, 0.04, 2.0])
    tiny = mp.mpf(10) ** -35
    for m in (GTR, F81):
        args = (m["pi"], m["exch"], rates)
        for (ta, tb, tc, td), to in (((100.0, 5.0, 60.0, 9.0), 2.0), ((3.0, 40.0, 0.0, 17.0), 11.0)):
            base_t = ur.twin_values(*args, (ta, tb, tc, td), to)
            swap_t = ur.twin_values(*args, (tb, ta, tc, td), to)          # a <-> b: x1 and x2 change places, y stays
            pair_t = ur.twin_values(*args, (tc, td, ta, tb), to)          # (a, b) <-> (c, d): all three stay
            base = ur.site_values(m["model"], *args, (ta, tb, tc, td), to)
            swap = ur.site_values(m["model"], *args, (tb, ta, tc, td), to)
            pair = ur.site_values(m["model"], *args, (tc, td, ta, tb), to)
            for k in range(3):
                assert abs(base_t[0][k] - swap_t[0][k]) <= tiny and abs(base_t[1][k] - swap_t[2][k]) <= tiny
                assert abs(base_t[2][k] - swap_t[1][k]) <= tiny
                assert all(abs(base_t[w][k] - pair_t[w][k]) <= tiny for w in range(3))
                assert base_t[1][k] != base_t[2][k]
            for a, b in ((base[0], swap[0]), (base[1], swap[2]), (base[2], swap[1]), (base[0], pair[0]), (base[1], pair[1]),
                         (base[2], pair[2])):
                assert np.max(np.abs(a / b - 1)) <= 128 * U               # each within 64 * 2^-52 of the same number
        # Ta = Tb: the two noise patterns have the same probability
        _, x1, x2 = ur.twin_values(*args, (30.0, 30.0, 45.0, 70.0), 10.0)
        assert all(a > 0 and abs(a - b) <= tiny * a for a, b in zip(x1, x2))
        _, r1, r2 = ur.site_values(m["model"], *args, (30.0, 30.0, 45.0, 70.0), 10.0)
        assert np.max(np.abs(r1 / r2 - 1)) <= 128 * U
        # equal tips: section 3.6's values
        y, x1, x2 = ur.site_values(m["model"], *args, (20.0,) * 4, 5.0)
        y0, x0 = qr.site_values(m["model"], *args, 20.0, 5.0)
        assert max(np.max(np.abs(y / y0 - 1)), np.max(np.abs(x1 / x0 - 1)), np.max(np.abs(x2 / x0 - 1))) <= (64 + 128) * U


def _locus(n, lo, hi, seed):
    return 10.0 ** np.random.default_rng(seed).uniform(lo, hi, n)


def test_long_branch_attraction():
    """Two long and two short tips: the wrong grouping of the two long branches collects more sites than the right one, and
    the locus is more likely to resolve ac|bd than ab|cd (Su & Townsend 2015); its mirror favours ad|bc."""
    r = _locus(300, -3.0, -1.5, 11)
    row = ur.rows("gtr", GTR["pi"], GTR["exch"], r, [(100, 5, 100, 5, 2)])[0]
    mirror = ur.rows("gtr", GTR["pi"], GTR["exch"], r, [(100, 5, 5, 100, 2)])[0]
    print("(100,5,100,5):2 Y %.3f X1 %.3f X2 %.3f: p_correct %.4f p_ac %.4f p_ad %.4f p_polytomy %.4f" % (tuple(row[:3]) + tuple(row[9:])))
    assert row[1] > row[0] > row[2] and row[10] > row[9] > row[11]
    assert mirror[2] > mirror[0] > mirror[1] and mirror[11] > mirror[9] > mirror[10]
    assert abs(mirror[11] - row[10]) <= 1e-12 and abs(mirror[9] - row[9]) <= 1e-12


# ---- the probability rule ------------------------------------------------------------------------------------------
def _test_loci():
    out = []
    for k, (n, lo, hi) in enumerate(((400, -3.5, -1.0), (60, -3, -1), (30, -2, 0), (5, -4, -3), (200, -1, 1), (1, -2, -2))):
        out.append(_locus(n, lo, hi, 70 + k))
    return out


PROB_QUARTETS = [(30, 30, 30, 30, 4), (100, 5, 100, 5, 2), (5, 9, 20, 31, 20), (0, 0, 0, 0, 2), (37, 37, 93, 107, 56), (0, 50, 3, 3, 1)]


def _grid():
    """64 (h, k) pairs with |h|, |k| <= 5, pairs 1e-12 to 1e-2 apart among them"""
    rng = np.random.default_rng(2)
    pairs = [(h, h + d) for h in (-3.0, -0.4, 0.0, 0.7, 2.5) for d in (1e-12, 1e-9, 1e-6, 1e-4, 1e-2)]
    pairs += [(h, h) for h in (-2.0, 0.0, 0.3, 1.9)]
    pairs += [tuple(v) for v in rng.uniform(-5, 5, (64 - len(pairs), 2)).tolist()]
    return pairs


def test_bivariate_normal_against_mpmath():
    triples = set()
    for m in (GTR, F81):
        for r in _test_loci():
            for row in ur.rows(m["model"], m["pi"], m["exch"], r, PROB_QUARTETS):
                triples.update(a for a in ur.probability_arguments(row[:9]) if a is not None)
    reached = len(triples)
    for h, k in _grid():
        for rho in (-0.999, 0.6, 0.999):
            triples.add((h, k, ur.clamp_rho(h, k, rho, 0.999)))
        if h == k:
            triples.add((h, k, 1.0))
    worst = 0.0
    for h, k, rho in sorted(triples):
        assert abs(rho) <= 0.999 or h == k                          # the rule never integrates unequal arguments past the clamp
        err = abs(ur.bvn_upper(h, k, rho) - ur.bvn_mp(h, k, rho))
        worst = max(worst, err)
        assert err <= 1e-13, (h, k, rho, err)
    print("B against mpmath at 30 digits on %d triples (%d reached by the test loci): largest difference %.2e" % (len(triples), reached, worst))


def test_equal_tip_sums_reproduce_section_3_6():
    for m in (GTR, F81):
        for r in _test_loci() + [_locus(20, -3.0, -1.0, 4)]:
            for tip, internode in ((30.0, 4.0), (5.0, 20.0), (100.0, 0.5), (0.0, 2.0), (20.0, 5.0)):
                y, x = qr.site_values(m["model"], m["pi"], m["exch"], r, tip, internode)
                Y, X, Yy, Xx, XY = qr.locus_sums(y, x)
                pc0, pw0, pp0 = qr.probabilities([Y, X, Yy, Xx, XY])
                args = ur.probability_arguments([Y, X, X, Yy, Xx, Xx, XY, XY, Xx])
                assert args[0] is None or args[0][0] == args[0][1]                      # h == k, bit for bit
                pc, p1, p2, pp = ur.probabilities([Y, X, X, Yy, Xx, Xx, XY, XY, Xx])
                assert abs(pc - pc0) <= 1e-12 and abs((p1 + p2) - pw0) <= 1e-12 and abs(pp - pp0) <= 1e-12 and p1 == p2


def test_probabilities_lie_in_the_unit_interval_and_sum_to_one():
    for m in (GTR, F81):
        for r in _test_loci():
            for row in ur.rows(m["model"], m["pi"], m["exch"], r, PROB_QUARTETS):
                p = row[9:]
                assert np.all(p >= 0.0) and np.all(p <= 1.0)
                if p[3] > 0.0:                                                         # (not clipped)
                    assert abs(p.sum() - 1.0) <= 1e-15, row
                else:
                    assert p[:3].sum() >= 1.0
                assert np.all(row[:3] >= row[3:6]) and np.all(row[3:9] >= 0)
    assert ur.probabilities([0] * 9) == (0.0, 0.0, 0.0, 1.0)
    empty = ur.rows("gtr", GTR["pi"], GTR["exch"], np.array([np.nan, 0.0]), [(10, 12, 3, 4, 1)])[0]
    assert np.array_equal(empty, [0] * 12 + [1])
    assert np.array_equal(ur.rows("gtr", GTR["pi"], GTR["exch"], np.zeros(0), [(10, 12, 3, 4, 1)])[0], [0] * 12 + [1])
    p = ur.probabilities([3.0, 0.0, 0.4, 0.5, 0.0, 0.1, 0.0, 0.2, 0.0])
    assert p[1] == 0.0 and p[2] > 0.0                                                  # E N1 = 0: nothing can favour ac|bd


EXACT_LOCI = [(60, -3.0, -1.0, (30, 30, 45, 70, 10)), (60, -2.5, -1.5, (100, 5, 100, 5, 2)), (40, -3.0, -1.0, (20, 35, 27, 27, 5)),
              (60, -2.0, -1.0, (100, 5, 5, 100, 2)), (20, -2.0, -1.0, (5, 9, 20, 31, 20)), (60, -2.0, -1.0, (37, 37, 93, 107, 56)),
              (60, -4.0, -2.0, (20, 20, 30, 40, 5)), (30, -3.5, -2.5, (0, 12, 7.5, 30, 3))]


def test_normal_approximation_against_the_exact_distribution():
    """Every gap is printed (recorded in DESIGN.md section 3.8); asserted at 0.05 where the largest expected count is at
    least 1, the regime in which section 3.6 documents that gap; the loci with every count under 1 are recorded only."""
    worst_big, worst_small = 0.0, 0.0
    for k, (n, lo, hi, quartet) in enumerate(EXACT_LOCI):
        r = _locus(n, lo, hi, 30 + k)
        y, x1, x2 = ur.site_values("gtr", GTR["pi"], GTR["exch"], r, quartet[:4], quartet[4])
        s = ur.locus_sums(y, x1, x2)
        approx, exact = ur.probabilities(s), ur.exact_resolution(y, x1, x2)
        gap = max(abs(a - b) for a, b in zip(approx, exact))
        big = max(s[:3]) >= 1.0
        print("n=%d %s: Y=%.3f X1=%.3f X2=%.3f normal %.4f / %.4f / %.4f / %.4f, exact %.4f / %.4f / %.4f / %.4f, largest gap %.4f%s"
              % ((n, quartet, s[0], s[1], s[2]) + approx + exact + (gap, "" if big else "  (every count under 1: recorded only)")))
        assert abs(sum(exact) - 1.0) < 1e-12 and min(exact) >= -1e-15
        if big:
            worst_big = max(worst_big, gap)
            assert gap <= 0.05
        else:
            worst_small = max(worst_small, gap)
    print("largest gap: %.4f with a count of at least 1, %.4f with every count under 1" % (worst_big, worst_small))
    assert worst_big > 0.0                                        # some locus is in the asserted regime


def test_exact_distribution_on_a_case_done_by_hand():
    pc, p1, p2, pp = ur.exact_resolution([0.3], [0.1], [0.25])
    assert abs(pc - 0.3) < 1e-15 and abs(p1 - 0.1) < 1e-15 and abs(p2 - 0.25) < 1e-15 and abs(pp - 0.35) < 1e-15
    # two sites, y = 0.5, x1 = 0.3, x2 = 0.2 each: SS correct; N1N1 ac; N2N2 ad; every mixed pair is a tie
    pc, p1, p2, pp = ur.exact_resolution([0.5, 0.5], [0.3, 0.3], [0.2, 0.2])
    assert abs(pc - 0.25) < 1e-15 and abs(p1 - 0.09) < 1e-15 and abs(p2 - 0.04) < 1e-15 and abs(pp - 0.62) < 1e-15
    a = ur.exact_resolution([0.2, 0.1, 0.3], [0.05, 0.2, 0.1], [0.05, 0.2, 0.1])       # x1 = x2: section 3.6's distribution
    b = qr.exact_resolution([0.2, 0.1, 0.3], [0.05, 0.2, 0.1])
    assert abs(a[0] - b[0]) < 1e-15 and abs(a[1] + a[2] - b[1]) < 1e-15 and a[1] == a[2]


# ---- the quartets of a tree ----------------------------------------------------------------------------------------
def _tq(text):
    from tapir_amd import compute, newick
    return compute.tree_quartets(newick.parse(text))


def test_tree_quartets_worked_example():
    assert _tq("((A:1,B:1):2,(C:2,(D:1,E:1):1):1);") == [("node1", ["A", "B"], 1.0, 1.0, 2.0, 2.0, 3.0),
                                                         ("node2", ["D", "E"], 1.0, 1.0, 2.0, 4.0, 1.0)]


def test_tree_quartets_star_caterpillar_trifurcation_and_zero_length():
    assert _tq("(A:1,B:1,C:1,D:1);") == [] and _tq("(A:1,B:2);") == [] and _tq("((A:1,B:1):1,C:2);") == []
    cat = _tq("(((((A:1,B:1):1,C:2):1,D:3):1,E:4):1,F:5);")       # the root's edges join; F is a leaf: no quartet there
    assert cat == [("node1", ["A", "B"], 1.0, 1.0, 2.0, 4.0, 1.0), ("node2", ["A", "B", "C"], 2.0, 2.0, 3.0, 5.0, 1.0),
                   ("node3", ["A", "B", "C", "D"], 3.0, 3.0, 4.0, 6.0, 1.0)]
    tri = _tq("((A:1,B:2):1,(C:1,D:1):1,(E:3,F:4):2);")           # a trifurcating root stays; lineages through it go down again
    assert tri == [("node1", ["A", "B"], 1.0, 2.0, 2.0, 5.0, 1.0), ("node2", ["C", "D"], 1.0, 1.0, 2.0, 5.0, 1.0),
                   ("node3", ["E", "F"], 3.0, 4.0, 2.0, 2.0, 2.0)]
    assert _tq("((A:1,B:1):0,(C:1,D:1):1,E:1);") == [("node1", ["C", "D"], 1.0, 1.0, 1.0, 1.0, 1.0)]   # the zero-length edge is skipped
    three = _tq("((A:1,B:2,C:3):1,(D:1,E:1):1);")                 # more than two lineages: the two shortest
    assert three == [("node1", ["A", "B", "C"], 1.0, 2.0, 1.0, 1.0, 2.0)]
    no_lengths = _tq("((A,B),(C,D));")                            # no lengths: the internode is 0 and is skipped
    assert no_lengths == []


def test_tree_quartets_of_the_bundled_tree(golden_dir):
    from tapir_amd import compute, newick
    root = newick.read_tree(os.path.join(golden_dir, "Euteleost.tree"))
    quartets = compute.tree_quartets(root)
    n = len(newick.leaves(root))
    depth = newick.distance_from_tip(root)
    assert len(quartets) == n - 3 and [q[0] for q in quartets] == ["node%d" % (k + 1) for k in range(n - 3)]
    for label, clade, ta, tb, tc, td, to in quartets:
        assert ta == tb and tc <= td and to > 0 and ta + to <= depth      # ultrametric: Ta = Tb = the clade's age
        assert td <= 2 * depth and len(clade) >= 2


# ---- pipeline and command line on the stand-in engine ------------------------------------------------------------
TREE3 = dict(leaf_names=["a", "b", "c"], parent=[3, 3, 4, 4, -1], blen=[0.1, 0.1, 0.2, 0.1, 0.0], leaf=[0, 1, 2, -1, -1])


def test_unequal_quartet_tables_do_not_depend_on_the_shard_or_on_the_list():
    from tapir_amd import pipeline
    rng = np.random.default_rng(5)
    per_locus = [rng.uniform(0.001, 0.2, n) for n in (30, 1, 17, 0, 64)]
    per_locus[0][3] = np.nan
    per_locus[2][:5] = 0.0
    pi = rng.dirichlet([5] * 4, 5)
    exch = rng.uniform(0.5, 3, (5, 6))
    t = TREE3
    quartets = [(20.0, 25.0, 30.0, 35.0, 5.0), (100.0, 5.0, 100.0, 5.0, 2.0)]
    args = (pipeline.Run(t["leaf_names"], t["parent"], t["blen"], t["leaf"], 12, [], [], device=0),)
    full = pipeline.unequal_quartet_tables(unequal_quartet_engine, per_locus, pi, exch, *args, quartets)
    assert full.shape == (5, 2, 13)
    for ids in ([0, 2, 4], [1, 3], [4]):
        part = pipeline.unequal_quartet_tables(unequal_quartet_engine, [per_locus[i] for i in ids], pi[ids], exch[ids], *args, quartets)
        assert np.array_equal(part, full[ids])
    assert np.array_equal(full[3], [[0] * 12 + [1]] * 2)                               # the empty locus
    for l in range(5):
        assert np.array_equal(full[l], ur.rows("gtr", pi[l], exch[l], per_locus[l], quartets))
    f81 = pipeline.unequal_quartet_tables(unequal_quartet_engine, per_locus, pi, None, *args, quartets, model="f81")
    assert np.array_equal(f81[0], ur.rows("f81", pi[0], None, per_locus[0], quartets))
    assert pipeline.unequal_quartet_tables(unequal_quartet_engine, [], pi[:0], exch[:0], *args, quartets).shape == (0, 2, 13)
    # a list longer than 256 goes through in several calls; a row does not depend on the list
    del unequal_quartet_engine.CALLS[:]
    long_list = [quartets[k % 2] for k in range(300)]
    rows = pipeline.unequal_quartet_tables(unequal_quartet_engine, per_locus[1:3], pi[1:3], exch[1:3], *args, long_list)
    assert [len(c[2]) for c in unequal_quartet_engine.CALLS] == [256, 44] and rows.shape == (2, 300, 13)
    assert np.array_equal(rows[:, 298], full[1:3, 0]) and np.array_equal(rows[:, 299], full[1:3, 1])


def _synthetic_dir(tmp_path, nloci=4):
    from tapir_amd import synth
    d = synth.simulate(nloci, 40, 5, 3)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    return str(aln), str(tmp_path / "tree.newick")


BASE = ["--times", "10,30", "--intervals", "5-15,20-40", "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"]
UFLAG = ["--unequal-quartets", "100/5/100/5:2,20/20.5/30/1e1:0.25"]
UNAME = "phylogenetic-informativeness-unequal-quartets.sqlite"
COLUMNS = ["id", "quartet", "tip_a", "tip_b", "tip_c", "tip_d", "internode", "signal", "noise_ac", "noise_ad", "p_correct", "p_ac",
           "p_ad", "p_polytomy"]


def _run(tmp_path, name, aln, tree, extra, base=BASE):
    from tapir_amd import cli
    out = tmp_path / name
    out.mkdir()
    return cli.main([aln, tree, "--output", str(out)] + base + extra, engine_mod=unequal_quartet_engine)


def _rows(path):
    con = sqlite3.connect(path)
    rows = con.execute("select l.locus, q.quartet, q.tip_a, q.tip_b, q.tip_c, q.tip_d, q.internode, q.signal, q.noise_ac, q.noise_ad, "
                       "q.p_correct, q.p_ac, q.p_ad, q.p_polytomy from loci l join quartet q on q.id = l.id order by l.id, q.rowid").fetchall()
    meta = dict(con.execute("select key, value from meta"))
    clades = con.execute("select quartet, ntaxa, taxa from clade order by rowid").fetchall()
    con.close()
    return rows, meta, clades


def test_cli_writes_the_third_database_and_nothing_else_changes(tmp_path):
    import json
    from tapir_amd import compute, newick, nexus
    aln, tree = _synthetic_dir(tmp_path)
    plain = _run(tmp_path, "plain", aln, tree, ["--quartets", "20:5"])
    del unequal_quartet_engine.CALLS[:]
    both = _run(tmp_path, "both", aln, tree, ["--quartets", "20:5", "--tree-quartets"] + UFLAG)
    of_tree = compute.tree_quartets(newick.read_tree(tree))
    assert len(of_tree) == 5 - 3
    typed = [[100.0, 5.0, 100.0, 5.0, 2.0], [20.0, 20.5, 30.0, 10.0, 0.25]]
    quartets = typed + [list(q[2:]) for q in of_tree]
    assert unequal_quartet_engine.CALLS == [("unequal_quartets", "gtr", quartets, 4)]     # typed rows first, then the tree's
    assert sorted(os.listdir(both)) == sorted(os.listdir(plain) + [UNAME])
    for f in os.listdir(plain):                                   # the main database, the .rates files, the --quartets file
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(both, f), "rb").read(), f
    con = sqlite3.connect(os.path.join(both, UNAME))
    main = sqlite3.connect(os.path.join(both, "phylogenetic-informativeness.sqlite"))
    tables = {r[0] for r in con.execute("select name from sqlite_master where type = 'table'")} - {"sqlite_sequence"}
    assert tables == {"loci", "quartet", "clade", "meta"}
    cols = lambda t: [r[1] for r in con.execute("pragma table_info(%s)" % t)]  # noqa: E731
    assert cols("loci") == ["id", "locus"] and cols("meta") == ["key", "value"] and cols("clade") == ["quartet", "ntaxa", "taxa"]
    assert cols("quartet") == COLUMNS
    loci = con.execute("select * from loci order by id").fetchall()
    assert loci == main.execute("select * from loci order by id").fetchall() and len(loci) == 4
    con.close()
    main.close()
    rows, meta, clades = _rows(os.path.join(both, UNAME))
    labels = ["100/5/100/5:2", "20/20.5/30/1e1:0.25", "node1", "node2"]
    assert meta["quartets"] == ",".join(labels) and meta["model"] == "gtr"
    assert len(rows) == 4 * (2 + len(of_tree)) and [r[1] for r in rows[:4]] == labels          # as typed, then the tree's
    assert [list(r[2:7]) for r in rows[:4]] == quartets
    assert clades == [(q[0], len(q[1]), ",".join(q[1])) for q in of_tree]
    for l, (_, name) in enumerate(loci):
        doc = json.load(open(os.path.join(both, name + ".nex.rates")))["sites"]
        r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
        _, st = nexus.read_states(os.path.join(aln, name + ".nex"))
        r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
        pi = [doc["freqs"][k] for k in "ACGT"]
        exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
        want = ur.rows("gtr", pi, exch, r, quartets)
        got = np.array([row[7:] for row in rows[4 * l:4 * l + 4]])
        assert np.array_equal(got, want[:, [0, 1, 2, 9, 10, 11, 12]]), name
    # either flag alone
    only_tree = _run(tmp_path, "tree", aln, tree, ["--tree-quartets"])
    rows_t, meta_t, clades_t = _rows(os.path.join(only_tree, UNAME))
    assert len(rows_t) == 4 * len(of_tree) and meta_t["quartets"] == "node1,node2" and clades_t == clades
    assert [r[7:] for r in rows_t[:2]] == [r[7:] for r in rows[2:4]]
    only_typed = _run(tmp_path, "typed", aln, tree, UFLAG)
    rows_u, _, clades_u = _rows(os.path.join(only_typed, UNAME))
    assert len(rows_u) == 8 and clades_u == [] and rows_u[:2] == rows[:2]
    assert "phylogenetic-informativeness-quartets.sqlite" not in os.listdir(only_typed)


def test_cli_unequal_quartets_from_rate_files(tmp_path):
    """--site-rates reads rates only: the model comes from --site-model (with the frequencies of the .rates documents), as
    for --quartets, and the rows are those of the run that wrote the files."""
    aln, tree = _synthetic_dir(tmp_path)
    base = ["--times", "10,30", "--intervals", "5-15,20-40", "--threshold", "0"]
    first = _run(tmp_path, "first", aln, tree, ["--site-model", "f81", "--tree-quartets"] + UFLAG, base=base)
    rows1, meta1, _ = _rows(os.path.join(first, UNAME))
    assert meta1["model"] == "f81"
    rates = tmp_path / "rates"
    rates.mkdir()
    for f in os.listdir(first):
        if f.endswith(".rates"):
            shutil.copy(os.path.join(first, f), rates)
    second = _run(tmp_path, "second", str(rates), tree, ["--site-rates", "--site-model", "f81", "--tree-quartets"] + UFLAG, base=base)
    rows2, meta2, _ = _rows(os.path.join(second, UNAME))
    assert meta2["model"] == "f81" and len(rows2) == len(rows1) == 16
    by_name = {(r[0].replace(".nex", ""), r[1]): r for r in rows2}
    for a in rows1:
        assert a[2:] == by_name[(a[0], a[1])][2:]


def _argv(tmp_path, golden_dir, *extra):
    return [str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10"] + list(extra)


@pytest.mark.parametrize("value, message", [
    ("20:5", "Cannot convert quartet '20:5' to Ta/Tb/Tc/Td:to"),
    ("1/2/3:5", "Cannot convert quartet '1/2/3:5' to Ta/Tb/Tc/Td:to"),
    ("1/2/3/4/5:5", "Cannot convert quartet '1/2/3/4/5:5' to Ta/Tb/Tc/Td:to"),
    ("1/2/3/4", "Cannot convert quartet '1/2/3/4' to Ta/Tb/Tc/Td:to"),
    ("1/a/3/4:5", "Cannot convert quartet '1/a/3/4:5' to Ta/Tb/Tc/Td:to"),
    ("1/2/3/4:0", "the internode length to must be positive"),
    ("1/2/3/4:-1", "the internode length to must be positive"),
    ("-1/2/3/4:5", "the tip length Ta must not be negative"),
    ("1/2/3/-4:5", "the tip length Td must not be negative"),
    ("1/2/3/4:5,,1/2/3/4:1", "Cannot convert quartet '' to Ta/Tb/Tc/Td:to"),
    ("1/nan/3/4:5", "Ta, Tb, Tc, Td and to must be finite"),
    ("1/2/3/4:inf", "Ta, Tb, Tc, Td and to must be finite"),
    (",".join(["1/2/3/4:1"] * 257), "--unequal-quartets takes 1..256 quartets"),
])
def test_cli_refuses_bad_unequal_quartets(tmp_path, golden_dir, value, message, capsys):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args(_argv(tmp_path, golden_dir, "--unequal-quartets=" + value))
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err and "unrecognized arguments" not in err


def test_cli_flags_parse_and_need_a_model_with_site_rates(tmp_path, golden_dir, capsys):
    from tapir_amd import cli
    a = cli.get_args(_argv(tmp_path, golden_dir))
    assert a.unequal_quartets is None and a.tree_quartets is False
    a = cli.get_args(_argv(tmp_path, golden_dir, "--tree-quartets", "--unequal-quartets", "100/5/100/5:2, 0/1.5/2e1/3:0.5"))
    assert a.tree_quartets and a.unequal_quartets == [("100/5/100/5:2", 100.0, 5.0, 100.0, 5.0, 2.0), ("0/1.5/2e1/3:0.5", 0.0, 1.5, 20.0, 3.0, 0.5)]
    # no depth check: a lineage through the parent can be nearly twice the tree's depth
    assert cli.get_args(_argv(tmp_path, golden_dir, "--unequal-quartets", "1e5/1/1/1:1")).unequal_quartets[0][1] == 1e5
    for flags in (["--tree-quartets"], ["--unequal-quartets", "1/2/3/4:5"]):
        with pytest.raises(SystemExit):
            cli.get_args(_argv(tmp_path, golden_dir, "--site-rates", *flags))
        err = capsys.readouterr().err
        assert flags[0] + " needs the loci's substitution model" in err and "--site-model jc, --site-model f81 or --exchangeabilities" in err
        for model in (["--site-model", "jc"], ["--site-model", "f81"], ["--exchangeabilities", "1,2,1,1,2,1"]):
            assert cli.get_args(_argv(tmp_path, golden_dir, "--site-rates", *flags, *model)).site_rates


_CLI_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import unequal_quartet_engine
from tapir_amd import cli
cli.main(%(argv)r, engine_mod=unequal_quartet_engine)
'''


def test_cli_two_ranks_gloo_matches_single_process(tmp_path):
    """Five files on two ranks (ragged shards): the gathered rows equal the single-process run's, row for row."""
    import torch  # noqa: F401
    from tapir_amd import cli
    aln, tree = _synthetic_dir(tmp_path, nloci=5)
    outs = []
    for name in ("single", "multi"):
        out = tmp_path / name
        out.mkdir()
        outs.append(out)
    argv = [aln, tree] + BASE + UFLAG + ["--tree-quartets", "--output"]
    single = cli.main(argv + [str(outs[0])], engine_mod=unequal_quartet_engine)
    script = tmp_path / "w.py"
    script.write_text(_CLI_WORKER % {"root": ROOT, "argv": argv + [str(outs[1])]})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29549")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29549", str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = _rows(os.path.join(single, UNAME)), _rows(os.path.join(str(outs[1]), UNAME))
    assert a == b and len(a[0]) == 5 * 4


def test_engine_and_header_declare_the_entry_points():
    """The binding lists the new C entry points with the header's signatures (the struct's layout included)."""
    import ctypes
    from tapir_amd import engine
    names = {s[0] for s in engine.SYMBOLS}
    entry = {"tphip_unequal_quartet_workspace_bytes", "tphip_unequal_quartet_tables", "tphip_unequal_quartet_tables_dev",
             "tphip_unequal_quartet_sites", "tphip_unequal_quartet_sites_dev"}
    assert entry <= names
    assert ctypes.sizeof(engine.UnequalQuartetOpts) == 24 and engine.UnequalQuartetOpts.tips.offset == 8
    for m in ("unequal_quartet_tables", "unequal_quartet_sites", "unequal_quartet_tables_dev", "unequal_quartet_sites_dev",
              "unequal_quartet_workspace_bytes"):
        assert hasattr(engine.Plan, m)
    header = open(os.path.join(ROOT, "include", "tphip.h")).read()
    assert "#define TPHIP_VERSION 110" in header and "tphip_unequal_quartet_opts" in header
    for name in entry:
        assert "int %s(" % name in header
    assert os.path.exists(os.path.join(ROOT, "tapir_amd", "csrc", "unequal_quartet_driver.hip"))

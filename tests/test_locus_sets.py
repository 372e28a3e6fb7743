"""Locus-set accumulation curves without a GPU: the numpy mirror of the exact rows
(tests/locus_set_reference.py) against the dynamic programme on the concatenated planes, the head rule, the ranking rule and
the order file, the tables and the command line through the CPU stand-in engine (tests/locus_set_engine.py).

Bounds: the exact mirror against exact_quartet_reference.windowed_dp within 1e-10 (section 3.9's derivation, which holds up to
2048 live sites: every set here is shorter) plus the mass the programme reports lost plus the prefix's own tail_bound."""
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import exact_quartet_reference as er
import locus_set_engine
import locus_set_reference as lr
import quartet_reference as qr
import unequal_quartet_reference as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def _planes(rng, n, scale):
    """y, x1, x2 of n sites with y + x1 + x2 <= 0.95"""
    y, x1, x2 = rng.gamma(1.0, scale, n), rng.gamma(1.0, 0.4 * scale, n), rng.gamma(1.0, 0.3 * scale, n)
    f = np.minimum(1.0, 0.95 / (y + x1 + x2))
    return np.stack([y * f, x1 * f, x2 * f])


def _batch(rng, sizes, scales):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    planes = np.concatenate([_planes(rng, n, s) for n, s in zip(sizes, scales)], axis=1)
    return off, planes


# ---- the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [128, 256])
def test_mirror_against_the_dp_on_the_concatenation_for_every_prefix_of_two_orders(M):
    rng = np.random.default_rng(5 + M)
    off, planes = _batch(rng, [30, 0, 200, 64, 150], [0.05, 0.0, 0.03, 0.1, 0.02])
    planes[:, off[2] + 10:off[2] + 40] = 0.0                      # dead sites
    assert int(off[-1]) <= 2048
    for order in ([2, 0, 4, 1, 3], [3, 1, 4, 0, 2]):
        rows = lr.exact_rows(planes, off, order, M)
        worst = 0.0
        for k in range(5):
            want = er.windowed_dp(*lr.concatenated(planes, off, order, k + 1))
            assert rows[k, 4] == M and 0 <= rows[k, 5] <= 1e-12, (order, k, rows[k])
            worst = max(worst, np.abs(rows[k, :4] - want[:4]).max() - want[4] - rows[k, 5])
            assert abs(rows[k, :4].sum() - 1) <= 1e-12
        print("M = %d, order %s: against the DP beyond lost mass and tail bound %.2e (allowed %.0e)" % (M, order, worst, TOL))
        assert worst <= TOL
    # k = 1 is the per-locus law on the same torus; the rows do not depend on what follows in the order
    a, b = lr.exact_rows(planes, off, [2, 0, 4, 1, 3], M), lr.exact_rows(planes, off, [2, 0, 4], M)
    assert np.array_equal(a[:3], b)
    one = er.resolution(*planes[:, off[2]:off[3]], cap=M)
    assert np.abs(a[0, :4] - np.array(one[:4])).max() <= TOL + a[0, 5] + one[5]


def test_head_rule_prefixes_one_and_two_fit_a_cap_of_64_and_three_does_not():
    rng = np.random.default_rng(12)
    off, planes = _batch(rng, [30, 30, 60, 20], [0.05, 0.05, 0.2, 0.01])
    order = [0, 1, 2, 3]
    fits = []
    for k in range(4):                                            # the reference's window rule alone says so
        _, var = er.moments(*lr.concatenated(planes, off, order, k + 1))
        fits.append(er.window_rule(var, cap=64)[0] != 0)
    assert fits == [True, True, False, False]
    rows = lr.exact_rows(planes, off, order, 64)
    assert np.all(rows[:2, 4] == 64) and np.all(rows[:2, 5] <= 1e-12) and np.all(np.isfinite(rows[:2, :4]))
    for k in (2, 3):
        _, var = er.moments(*lr.concatenated(planes, off, order, k + 1))
        assert np.all(np.isnan(rows[k, :4])) and rows[k, 4] == 0
        assert abs(rows[k, 5] / er.tail_bound(var, 64) - 1) <= 1e-12 and rows[k, 5] > 1e-12
    # at 128 every prefix fits; with n_head = 1 only the first is computed, and it is the same row
    full, cut = lr.exact_rows(planes, off, order, 128), lr.exact_rows(planes, off, order, 128, n_head=1)
    assert np.all(full[:, 4] == 128) and np.array_equal(cut[0], full[0]) and np.all(cut[1:, 4] == 0) and np.all(np.isnan(cut[1:, :4]))
    assert np.array_equal(cut[1:, 5], full[1:, 5])


def test_point_law_and_a_locus_without_a_live_site_in_the_middle():
    rng = np.random.default_rng(2)
    off, planes = _batch(rng, [3, 25, 40], [0.0, 0.0, 0.05])
    planes[:, off[0]:off[1]] = np.array([[1.0, 0, 1.0], [0, 0, 0], [0, 0, 0]])       # S = 2 for certain
    rows = lr.exact_rows(planes, off, [0, 1, 2], 64)
    assert np.array_equal(rows[0], [1, 0, 0, 0, 64, 0]) and np.array_equal(rows[1], rows[0])   # the culled locus adds nothing
    want = er.windowed_dp(*lr.concatenated(planes, off, [0, 1, 2], 3))
    assert np.abs(rows[2, :4] - want[:4]).max() <= TOL + want[4] + rows[2, 5]
    mid = lr.exact_rows(planes, off, [2, 1, 0], 64)                                  # ... also after a law that is no point
    assert np.array_equal(mid[1, :4], mid[0, :4]) and np.abs(mid[2, :4] - rows[2, :4]).max() <= TOL
    wrong = planes.copy()
    wrong[:, off[0]:off[1]] = np.array([[0, 0, 0], [1.0, 0, 1.0], [0, 0, 0]])        # N1 = 2 for certain
    assert np.array_equal(lr.exact_rows(wrong, off, [0], 64)[0], [0, 1, 0, 0, 64, 0])


# ---- the order ----------------------------------------------------------------------------------------------------------
def _rows8(p_correct):
    """per-locus rows [L, n_q, 8] with these p_correct [L, n_q]"""
    p = np.asarray(p_correct, np.float64)
    rows = np.zeros(p.shape + (8,))
    rows[..., 5] = p
    return rows


def test_ranking_rule_ties_order_file_and_max_k(tmp_path):
    from tapir_amd import pipeline
    names = ["a", "b", "c", "d"]
    p = [[0.5, 0.1], [0.9, 0.1], [0.5, 0.7], [0.9, 0.1]]
    order = pipeline.locus_set_order(_rows8(p), names)
    assert order.dtype == np.int32 and order.tolist() == [[1, 3, 0, 2], [2, 0, 1, 3]]      # descending, ties by ascending index
    assert np.array_equal(order, lr.default_order(p))
    rows13 = np.zeros((4, 2, 13))
    rows13[..., 9] = p
    assert np.array_equal(pipeline.locus_set_order(rows13, names), order)
    assert pipeline.locus_set_order(_rows8(p), names, max_k=2).tolist() == [[1, 3], [2, 0]]
    assert pipeline.locus_set_order(_rows8(p), names, max_k=9).tolist() == order.tolist()
    f = tmp_path / "order.txt"
    f.write_text("c\n\n  a  \nd\n")
    assert pipeline.locus_set_order(_rows8(p), names, str(f)).tolist() == [[2, 0, 3]] * 2  # b is left out
    assert pipeline.locus_set_order(_rows8(p), names, str(f), max_k=1).tolist() == [[2]] * 2
    for text, message in (("c\nx\n", "unknown locus 'x'"), ("c\na\nc\n", "named more than once"), ("\n", "names no locus")):
        f.write_text(text)
        with pytest.raises(pipeline.PipelineError, match=message):
            pipeline.locus_set_order(_rows8(p), names, str(f))
    with pytest.raises(pipeline.PipelineError, match="max_k must be at least 1"):
        pipeline.locus_set_order(_rows8(p), names, max_k=0)
    with pytest.raises(pipeline.PipelineError, match="not distinct"):
        f.write_text("a\n")
        pipeline.locus_set_order(_rows8(p), ["a", "a", "c", "d"], str(f))


def test_tiles_and_n_head_keep_planes_and_workspace_within_the_bound():
    from tapir_amd import pipeline
    B = pipeline.EXACT_QUARTET_BYTES
    tile, n_head = pipeline.locus_set_tile(1000, 500000, 100, 1000, 2, 128)
    assert tile == 33 and 8 * 2 * 33 * 500000 <= B < 8 * 2 * 34 * 500000 and n_head == 1000        # the planes bind
    tile, n_head = pipeline.locus_set_tile(1000, 5000, 100, 1000, 2, 512)
    assert tile == 100 and 1 <= n_head < 1000 and tile * (48 * 1000 + 36 * 1000 + 2048 + 6168 * n_head) <= B
    assert tile * (48 * 1000 + 36 * 1000 + 2048 + 6168 * (n_head + 1)) > B                          # 257 tiles x 24 bytes a prefix
    assert pipeline.locus_set_tile(3, 10 ** 9, 5, 3, 3, 128) == (1, 3)                              # at least one quartet
    assert pipeline.locus_set_tile(10, 600, 300, 10, 3, 128) == (256, 10)                           # the engine's limit


def test_tiled_rows_equal_untiled_rows_and_a_sub_batch_gives_the_same_rows(monkeypatch):
    from tapir_amd import pipeline
    rng = np.random.default_rng(4)
    per_locus = [10.0 ** rng.uniform(-3, -1, n) for n in (7, 30, 1, 19)]
    per_locus[1][3] = np.nan
    pi = rng.dirichlet([5.0] * 4, 4)
    exch = rng.uniform(0.5, 2.0, (4, 6))
    tree = ([3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1])
    run = pipeline.Run(["a", "b", "c"], *tree, 8, [], [], device=0)
    q2 = np.array([[20.0, 5.0], [0.0, 3.0], [35.0, 1.0], [7.0, 7.0], [50.0, 0.5]])
    q5 = np.array([[20.0, 22.0, 25.0, 30.0, 5.0], [1.0, 0.0, 3.0, 40.0, 2.0], [9.0, 9.0, 9.0, 9.0, 4.0]])
    o2 = np.array([[3, 1, 0], [0, 1, 2], [1, 3, 0], [3, 0, 1], [1, 0, 3]])
    o5 = o2[:3]
    call = lambda **kw: (pipeline.exact_locus_set_tables(locus_set_engine, per_locus, pi, exch, run, q2, o2, **kw),   # noqa: E731
                         pipeline.exact_locus_set_tables(locus_set_engine, per_locus, pi, exch, run, q5, o5, unequal=True, **kw))
    whole = call()
    assert whole[0].shape == (5, 3, 6) and whole[1].shape == (3, 3, 6) and np.all(whole[0][..., 4] == 128)
    del locus_set_engine.CALLS[:]
    monkeypatch.setattr(pipeline, "EXACT_QUARTET_BYTES", 2 * (48 * 4 + 36 * 3 + 2048 + 24 * 17 * 3))   # two quartets, n_head = 3
    tiled = call()
    assert [c[1][0] for c in locus_set_engine.CALLS] == [2, 2, 1, 2, 1] and {c[3] for c in locus_set_engine.CALLS} == {3}
    assert np.array_equal(whole[0], tiled[0]) and np.array_equal(whole[1], tiled[1])
    # less room: one quartet a tile and two prefixes of it; the rows k <= 2 are the same, the third is reported as not computed
    monkeypatch.setattr(pipeline, "EXACT_QUARTET_BYTES", 48 * 4 + 36 * 3 + 2048 + 24 * 17 * 2)
    cut = call()
    assert np.array_equal(cut[0][:, :2], whole[0][:, :2]) and np.all(cut[0][:, 2, 4] == 0) and np.all(np.isnan(cut[0][:, 2, :4]))
    # locus 2 is named by no order: without it (what travels to rank 0 of a several-rank run) the rows are the same
    monkeypatch.undo()
    keep = [0, 1, 3]
    sub = pipeline.exact_locus_set_tables(locus_set_engine, [per_locus[l] for l in keep], pi[keep], exch[keep], run, q2,
                                          np.searchsorted(keep, o2))
    assert np.array_equal(sub[[0, 2, 3, 4]], whole[0][[0, 2, 3, 4]])
    assert pipeline.exact_locus_set_tables(locus_set_engine, [], pi[:0], exch[:0], run, q2, np.zeros((5, 0), np.int32)).shape == (5, 0, 6)
    # the normal rows: the engine's call on all loci's rows
    rows = pipeline.quartet_tables(locus_set_engine, per_locus, pi, exch, run, q2)
    got = pipeline.locus_set_tables(locus_set_engine, rows, o2)
    assert np.array_equal(got, lr.normal_rows(rows, o2)) and np.array_equal(got[:, 0], rows[o2[:, 0], np.arange(5)])


def test_a_quartet_list_longer_than_256_goes_through_in_several_calls():
    """--tree-quartets on a tree with more than 256 internodes: the engine takes at most 256 quartets (and 2^24 pairs) a call."""
    from tapir_amd import pipeline
    rng = np.random.default_rng(8)
    per_locus = [10.0 ** rng.uniform(-3, -1, n) for n in (9, 14, 5)]
    pi = rng.dirichlet([5.0] * 4, 3)
    exch = rng.uniform(0.5, 2.0, (3, 6))
    tree = ([3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1])
    run = pipeline.Run(["a", "b", "c"], *tree, 8, [], [], device=0)
    two = np.array([[20.0, 22.0, 25.0, 30.0, 5.0], [9.0, 8.0, 7.0, 6.0, 4.0]])
    long_list = two[np.arange(300) % 2]
    rows = pipeline.unequal_quartet_tables(locus_set_engine, per_locus, pi, exch, run, long_list)
    order = pipeline.locus_set_order(rows, ["a", "b", "c"])
    assert order.shape == (300, 3)
    del locus_set_engine.CALLS[:]
    got = pipeline.locus_set_tables(locus_set_engine, rows, order)
    assert [c[2][0] for c in locus_set_engine.CALLS if c[0] == "locus_set_rows"] == [256, 44] and got.shape == (300, 3, 13)
    short = pipeline.locus_set_tables(locus_set_engine, rows[:, :2], order[:2])
    assert np.array_equal(got[298:], short) and np.array_equal(got[:2], short)      # a quartet's rows do not depend on the list
    del locus_set_engine.CALLS[:]
    exact = pipeline.exact_locus_set_tables(locus_set_engine, per_locus, pi, exch, run, long_list, order, unequal=True)
    assert [c[1][0] for c in locus_set_engine.CALLS if c[0] == "locus_set_exact"] == [256, 44] and exact.shape == (300, 3, 6)
    assert np.array_equal(exact[298:], exact[:2]) and np.all(exact[..., 4] == 128)
    # many loci: slices of 2^24 // L quartets
    calls = []
    stub = type("Stub", (), {"locus_set_rows": staticmethod(lambda r, o, device=0: calls.append(r.shape) or np.zeros(o.shape + (8,)))})
    big = np.broadcast_to(np.zeros((1, 1, 8)), (200000, 100, 8))
    assert pipeline.locus_set_tables(stub, big, np.zeros((100, 1), np.int32)).shape == (100, 1, 8)
    assert calls == [(200000, 83, 8), (200000, 17, 8)] and 200000 * 83 <= 1 << 24 < 200000 * 84


# ---- the tables ---------------------------------------------------------------------------------------------------------
def _table(con, name):
    return con.execute("select * from %s order by rowid" % name).fetchall()


def test_k_needed_is_three_on_one_curve_and_null_on_another(tmp_path):
    from tapir_amd import db
    name = str(tmp_path / "q.sqlite")
    files = ["l%d.nex" % i for i in range(4)]
    db.write_quartet_db(name, files, np.zeros((4, 2, 8)), ["20:5", "0:3"], [[20, 5], [0, 3]], "gtr")
    rows = np.zeros((2, 4, 8))
    rows[0, :, 5] = [0.5, 0.9, 0.96, 0.99]
    rows[1, :, 5] = [0.1, 0.2, 0.3, 0.4]
    exact = np.zeros((2, 4, 6))
    exact[0, :, 0] = [0.6, 0.97, np.nan, np.nan]                   # the head ends at 2 and reaches the target there
    exact[0, :, 4] = [128, 128, 0, 0]
    exact[1, :, 0] = [0.1, 0.2, np.nan, np.nan]                    # no computed prefix reaches it
    exact[1, :, 4] = [128, 128, 0, 0]
    order = np.array([[3, 1, 0, 2], [0, 1, 2, 3]])
    db.add_locus_set_tables(name, rows, order, ["20:5", "0:3"], 0.95, "p_correct", None, exact=exact, window_cap=128)
    con = sqlite3.connect(name)
    assert [r[1] for r in con.execute("pragma table_info(locus_set_summary)")] == ["quartet", "target", "k_needed", "p_correct_all",
                                                                                   "k_needed_exact"]
    assert _table(con, "locus_set_summary") == [("20:5", 0.95, 3, 0.99, 2), ("0:3", 0.95, None, 0.4, None)]
    assert lr.k_needed(rows[0, :, 5], 0.95) == 3 and lr.k_needed(rows[1, :, 5], 0.95) is None
    got = _table(con, "locus_set")
    assert [(r[0], r[1], r[2]) for r in got[:4]] == [("20:5", 1, 4), ("20:5", 2, 2), ("20:5", 3, 1), ("20:5", 4, 3)]   # ids are 1-based
    ex = _table(con, "locus_set_exact")
    assert ex[2] == ("20:5", 3, None, None, None, 0, 0.0) and ex[1][:3] == ("20:5", 2, 0.97)
    meta = dict(_table(con, "meta"))
    assert meta["locus_sets_order"] == "p_correct" and meta["locus_sets_max"] == "all" and meta["locus_sets_target"] == "0.95"
    assert meta["locus_sets_window_cap"] == "128"
    con.close()


# ---- the command line ---------------------------------------------------------------------------------------------------
def _synthetic_dir(tmp_path, nloci=4):
    from tapir_amd import synth
    d = synth.simulate(nloci, 40, 5, 3)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    return str(aln), str(tmp_path / "tree.newick")


BASE = ["--times", "10,30", "--intervals", "5-15,20-40", "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"]
QFLAGS = ["--quartets", "20:5,0:3", "--unequal-quartets", "100/5/100/5:2", "--tree-quartets"]
QNAME = "phylogenetic-informativeness-quartets.sqlite"
UNAME = "phylogenetic-informativeness-unequal-quartets.sqlite"


def _run(tmp_path, name, aln, tree, extra):
    from tapir_amd import cli
    out = tmp_path / name
    out.mkdir()
    return cli.main([aln, tree, "--output", str(out)] + BASE + extra, engine_mod=locus_set_engine)


def _tables(con):
    return {r[0] for r in con.execute("select name from sqlite_master where type = 'table'")} - {"sqlite_sequence"}


def test_cli_adds_the_tables_for_the_three_quartet_flags_and_changes_nothing_else(tmp_path):
    import json
    from tapir_amd import compute, newick, nexus
    aln, tree = _synthetic_dir(tmp_path)
    plain = _run(tmp_path, "plain", aln, tree, QFLAGS + ["--exact-quartets"])
    sets = _run(tmp_path, "sets", aln, tree, QFLAGS + ["--exact-quartets", "--locus-sets", "--locus-sets-target", "0.5"])
    normal = _run(tmp_path, "normal", aln, tree, QFLAGS + ["--locus-sets", "--locus-sets-max", "2"])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(sets))
    for f in os.listdir(plain):
        same = open(os.path.join(plain, f), "rb").read() == open(os.path.join(sets, f), "rb").read()
        assert same == (f not in (QNAME, UNAME)), f               # every other output: byte for byte
    of_tree = compute.tree_quartets(newick.read_tree(tree))
    for name, unequal in ((QNAME, False), (UNAME, True)):
        old, new, cut = (sqlite3.connect(os.path.join(d, name)) for d in (plain, sets, normal))
        assert _tables(new) == _tables(old) | {"locus_set", "locus_set_summary", "locus_set_exact"}
        assert _tables(cut) == _tables(old) - {"quartet_exact"} | {"locus_set", "locus_set_summary"}
        for t in _tables(old) - {"meta"}:                         # what the file holds without the flag is still there, unchanged
            assert _table(old, t) == _table(new, t), t
        meta_old, meta_new, meta_cut = dict(_table(old, "meta")), dict(_table(new, "meta")), dict(_table(cut, "meta"))
        assert {k: meta_new[k] for k in meta_old} == meta_old
        assert set(meta_new) - set(meta_old) == {"locus_sets_order", "locus_sets_max", "locus_sets_target", "locus_sets_window_cap"}
        assert (meta_new["locus_sets_order"], meta_new["locus_sets_max"], meta_new["locus_sets_target"],
                meta_new["locus_sets_window_cap"]) == ("p_correct", "all", "0.5", "128")
        assert meta_cut["locus_sets_max"] == "2" and meta_cut["locus_sets_target"] == "0.95" and "locus_sets_window_cap" not in meta_cut
        nsum, p_col = (9, 10) if unequal else (5, 6)              # columns of the per-locus table `quartet`
        sums = list(ur.SUMS) if unequal else ["Y", "X", "Yy", "Xx", "XY"]
        wrong = ["p_ac", "p_ad"] if unequal else ["p_incorrect"]
        assert [r[1] for r in new.execute("pragma table_info(locus_set)")] == ["quartet", "k", "id"] + sums + ["p_correct"] + wrong + ["p_polytomy"]
        assert [r[1] for r in new.execute("pragma table_info(locus_set_exact)")] == ["quartet", "k", "p_correct"] + wrong + [
            "p_polytomy", "window", "tail_bound"]
        assert [r[1] for r in cut.execute("pragma table_info(locus_set_summary)")] == ["quartet", "target", "k_needed", "p_correct_all"]
        labels = ["100/5/100/5:2"] + [q[0] for q in of_tree] if unequal else ["20:5", "0:3"]
        lengths = [[100.0, 5.0, 100.0, 5.0, 2.0]] + [list(q[2:]) for q in of_tree] if unequal else [[20.0, 5.0], [0.0, 3.0]]
        loci = _table(new, "loci")
        L = len(loci)
        per_locus = _table(new, "quartet")
        got, got_exact, summary = _table(new, "locus_set"), _table(new, "locus_set_exact"), _table(new, "locus_set_summary")
        assert len(got) == len(got_exact) == L * len(labels) and [r[0] for r in summary] == labels
        assert len(_table(cut, "locus_set")) == 2 * len(labels)
        sites = []                                                # per locus: rates and model, read back from the run's own files
        for key, locus in loci:
            doc = json.load(open(os.path.join(sets, locus + ".nex.rates")))["sites"]
            r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
            _, st = nexus.read_states(os.path.join(aln, locus + ".nex"))
            r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
            sites.append((r, [doc["freqs"][k] for k in "ACGT"], [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]))
        worst = 0.0
        for q, lab in enumerate(labels):
            mine = got[q * L:(q + 1) * L]
            assert [(r[0], r[1]) for r in mine] == [(lab, k + 1) for k in range(L)]
            p_locus = np.array([per_locus[l * len(labels) + q][p_col] for l in range(L)])
            order = np.argsort(-p_locus, kind="stable")
            assert [r[2] for r in mine] == [loci[l][0] for l in order]                              # the ranking rule
            assert [r[:3] for r in _table(cut, "locus_set")[2 * q:2 * q + 2]] == [r[:3] for r in mine[:2]]
            signal = np.array([per_locus[l * len(labels) + q][7 if unequal else 4] for l in order])
            assert [r[3] for r in mine] == np.cumsum(signal).tolist()                                # the sums add, left to right
            first = per_locus[order[0] * len(labels) + q]
            assert mine[0][3 + nsum:] == first[(10 if unequal else 6):]                              # k = 1: the per-locus row
            for r in mine:
                want = (ur.probabilities if unequal else qr.probabilities)(r[3:3 + nsum])
                assert max(abs(a - b) for a, b in zip(r[3 + nsum:], want)) <= 1e-13
            p_set = [r[3 + nsum] for r in mine]
            assert summary[q][1:4] == (0.5, lr.k_needed(p_set, 0.5), p_set[-1])
            planes = []
            for r, pi, exch in (sites[l] for l in order):
                row = lengths[q]
                if unequal:
                    planes.append(np.stack(ur.site_values("gtr", pi, exch, r, row[:4], row[4])))
                else:
                    y, x = qr.site_values("gtr", pi, exch, r, row[0], row[1])
                    planes.append(np.stack([y, x, x]))
            p_exact = []
            for k in range(L):
                e = got_exact[q * L + k]
                assert e[:2] == (lab, k + 1)
                p_exact.append(np.nan if e[2] is None else e[2])
                if e[-2] == 0:                                    # does not fit 128: never truncated
                    assert all(v is None for v in e[2:-2]) and e[-1] > 1e-12
                    continue
                assert e[-2] == 128 and e[-1] <= 1e-12
                want = er.windowed_dp(*np.nan_to_num(np.concatenate(planes[:k + 1], axis=1)))
                lost = want[4]
                want = want[:4] if unequal else (want[0], want[1] + want[2], want[3])
                worst = max(worst, max(abs(a - b) for a, b in zip(e[2:-2], want)) - lost - e[-1])
            assert summary[q][4] == lr.k_needed(p_exact, 0.5)
        print("%s: exact set rows against the DP on the concatenated site values beyond lost mass and tail bound %.2e" % (name, worst))
        assert worst <= TOL
        for con in (old, new, cut):
            con.close()
    # an order file: the same loci for every quartet, in the file's order; one kind of quartet alone
    f = tmp_path / "order.txt"
    f.write_text("locus00002\nlocus00000\n")
    only = _run(tmp_path, "only", aln, tree, ["--tree-quartets", "--locus-sets", "--locus-sets-order", str(f)])
    assert QNAME not in os.listdir(only)
    con = sqlite3.connect(os.path.join(only, UNAME))
    names = dict((v, k) for k, v in _table(con, "loci"))
    assert [r[2] for r in _table(con, "locus_set")] == [names["locus00002"], names["locus00000"]] * len(of_tree)
    assert dict(_table(con, "meta"))["locus_sets_order"] == "file:order.txt"
    con.close()
    f.write_text("locus00002\nnobody\n")
    from tapir_amd import pipeline
    with pytest.raises(pipeline.PipelineError, match="unknown locus 'nobody'"):
        _run(tmp_path, "bad", aln, tree, ["--tree-quartets", "--locus-sets", "--locus-sets-order", str(f)])


def _argv(tmp_path, golden_dir, *extra):
    return [str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10"] + list(extra)


def test_cli_flags_parse_and_argument_errors_fire_before_any_work(tmp_path, golden_dir, capsys):
    from tapir_amd import cli
    a = cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5"))
    assert a.locus_sets is False and a.locus_sets_order is None and a.locus_sets_max is None and a.locus_sets_target is None
    for flags in (["--quartets", "20:5"], ["--unequal-quartets", "1/2/3/4:5"], ["--tree-quartets"]):
        a = cli.get_args(_argv(tmp_path, golden_dir, "--locus-sets", *flags))
        assert a.locus_sets is True and a.locus_sets_target == 0.95 and a.locus_sets_max is None
    a = cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5", "--locus-sets", "--locus-sets-max", "7", "--locus-sets-target", "0.8",
                           "--locus-sets-order", "some/file"))
    assert a.locus_sets_max == 7 and a.locus_sets_target == 0.8 and os.path.isabs(a.locus_sets_order)
    q = ["--quartets", "20:5"]
    for extra, message in ((["--locus-sets"], "--locus-sets needs --quartets, --unequal-quartets or --tree-quartets"),
                           (["--bootstrap", "10", "--locus-sets"], "--locus-sets needs --quartets"),
                           (q + ["--locus-sets-order", "f"], "--locus-sets-order needs --locus-sets"),
                           (q + ["--locus-sets-max", "3"], "--locus-sets-max needs --locus-sets"),
                           (q + ["--locus-sets-target", "0.9"], "--locus-sets-target needs --locus-sets"),
                           (q + ["--locus-sets", "--locus-sets-max", "0"], "--locus-sets-max must be at least 1"),
                           (q + ["--locus-sets", "--locus-sets-max", "x"], "invalid int value"),
                           (q + ["--locus-sets", "--locus-sets-target", "0"], "--locus-sets-target must be in (0, 1)"),
                           (q + ["--locus-sets", "--locus-sets-target", "1"], "--locus-sets-target must be in (0, 1)"),
                           (q + ["--locus-sets", "--locus-sets-target", "nan"], "--locus-sets-target must be in (0, 1)")):
        with pytest.raises(SystemExit) as e:
            cli.get_args(_argv(tmp_path, golden_dir, *extra))
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err, (extra, err)


_CLI_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import locus_set_engine
from tapir_amd import cli
cli.main(%(argv)r, engine_mod=locus_set_engine)
'''


def test_cli_two_ranks_gloo_matches_single_process(tmp_path):
    """Five files on two ranks (ragged shards): the set tables equal the single-process run's bit for bit -- the exact rows
    too, whose rates and models travel to rank 0."""
    import torch  # noqa: F401
    from tapir_amd import cli
    aln, tree = _synthetic_dir(tmp_path, nloci=5)
    outs = []
    for name in ("single", "multi"):
        out = tmp_path / name
        out.mkdir()
        outs.append(out)
    argv = [aln, tree] + BASE + QFLAGS + ["--exact-quartets", "--locus-sets", "--locus-sets-max", "4", "--output"]
    single = cli.main(argv + [str(outs[0])], engine_mod=locus_set_engine)
    script = tmp_path / "w.py"
    script.write_text(_CLI_WORKER % {"root": ROOT, "argv": argv + [str(outs[1])]})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29553")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29553", str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in (QNAME, UNAME):
        a, b = sqlite3.connect(os.path.join(single, name)), sqlite3.connect(os.path.join(str(outs[1]), name))
        for t in ("locus_set", "locus_set_summary", "locus_set_exact", "meta"):
            assert _table(a, t) == _table(b, t), (name, t)
        assert len(_table(a, "locus_set")) == 4 * len(_table(a, "locus_set_summary"))
        a.close()
        b.close()


def test_engine_and_header_declare_the_entry_points():
    import ctypes
    from tapir_amd import engine
    names = {s[0] for s in engine.SYMBOLS}
    entry = {"tphip_locus_set_rows_dev", "tphip_locus_set_rows", "tphip_locus_set_exact_workspace_bytes", "tphip_locus_set_exact_dev",
             "tphip_locus_set_exact"}
    assert entry <= names
    o = engine.LocusSetOpts
    assert ctypes.sizeof(o) == 48 and (o.n_q.offset, o.n_k.offset, o.family.offset, o.window_cap.offset, o.tail_tolerance.offset,
                                       o.n_head.offset, o.order.offset) == (4, 8, 12, 16, 24, 32, 40)
    for m in ("locus_set_exact", "locus_set_exact_dev", "locus_set_exact_workspace_bytes"):
        assert hasattr(engine.Plan, m)
    assert callable(engine.locus_set_rows) and callable(engine.locus_set_rows_dev)
    header = open(os.path.join(ROOT, "include", "tphip.h")).read()
    assert "tphip_locus_set_opts" in header
    for name in entry:
        assert "int %s(" % name in header
    import __graft_entry__ as ge
    unit = {u["src"]: u for u in ge.HIP_UNITS}
    assert unit["locus_set_driver.hip"]["flags"] == unit["exact_quartet_driver.hip"]["flags"]      # the shared device functions round the same
    assert "locus_set_kernels.hpp" in unit["locus_set_driver.hip"]["deps"]
    for f in ("locus_set_driver.hip", "locus_set_kernels.hpp", "quartet_probabilities.hpp", "unequal_quartet_probabilities.hpp"):
        assert os.path.exists(os.path.join(ROOT, "tapir_amd", "csrc", f))
    # the order is validated before any device is touched
    ge.build()
    rows8 = np.zeros((4, 2, 8))
    for order, message in (([[0, 0], [1, 2]], "repeated"), ([[0, 4], [1, 2]], "out of range"), ([[0, -1], [1, 2]], "out of range"),
                           (np.zeros((2, 5), np.int32), "n_k must be in 1..nloci")):
        with pytest.raises(engine.TphipError, match=message):
            engine.locus_set_rows(rows8, order)

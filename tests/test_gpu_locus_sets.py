"""Locus-set accumulation curves on the GPU (tphip_locus_set_rows, tphip_locus_set_exact and their _dev twins; DESIGN.md
section 3.11) against tests/locus_set_reference.py and the dynamic programme of tests/exact_quartet_reference.py applied to
the concatenated planes.  Run with -m gpu on the MI355X box.  Every test prints its figures before it asserts.

Bounds (stated by the definition, none tuned to the kernels):
  exact rows      1e-10 absolute (section 3.9's derivation: at most 2048 live factors at a few ulp each, times the weights'
                  1-norm; the largest set here has 467 columns) plus the mass the windowed programme reports lost plus the
                  prefix's own tail_bound, against the programme and against the numpy mirror at the same M.
  k = 1           against tphip_quartet_exact's row of the first locus: 1e-10 plus both rows' tail bounds (the two calls may
                  use different windows).
  normal rows     the sums bit-equal to np.cumsum of the engine's own per-locus rows; k = 1 bit-equal to the per-locus row;
                  the probabilities within 1e-13 of the restated rule on the engine's sums (the bound of the per-locus tests).
  bit identity    twice; loci appended; permuted and longer quartet lists; another quartet's order changed; a larger
                  workspace; a smaller n_head (rows k <= n_head); _dev against the host twin.
"""
import numpy as np
import pytest

import exact_quartet_reference as er
import locus_set_reference as lr
import quartet_reference as qr
import unequal_quartet_reference as ur

pytestmark = pytest.mark.gpu

TOL = 1e-10
# a five-taxon tree ((A, B), (C, D), E): the exact stage never looks at it
PARENT, BLEN, LEAF = [2, 2, 7, 5, 5, 7, 7, -1], [0.1, 0.1, 0.05, 0.1, 0.1, 0.05, 0.2, 0.0], [0, 1, -1, 2, 3, -1, 4, -1]
SIZES = [0, 1, 37, 64, 65, 300]          # an empty locus, one column, less than a wave, a wave, a wave + 1, an LDS tile + 44
ORDERS = np.array([[2, 0, 3, 5, 1, 4],
                   [1, 0, 2, 4, 3, 5],   # quartet 1: a point law, the empty locus, a locus culled entirely, then the rest
                   [5, 4, 3, 2, 1, 0]], np.int32)


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _planes(rng, n, scale):
    y, x1, x2 = rng.gamma(1.0, scale, n), rng.gamma(1.0, 0.4 * scale, n), rng.gamma(1.0, 0.3 * scale, n)
    f = np.minimum(1.0, 0.95 / (y + x1 + x2))
    return np.stack([y * f, x1 * f, x2 * f])


def _synthetic():
    """Planes [3][n_q = 3][467] and, per (quartet, k), the dynamic programme on the concatenation of the first k loci of the
    quartet's order.  Quartet 0: variances of about 0.07 a site (every prefix fits 128, the first few fit 64); quartet 1 the
    same scale, its one-column locus the point law y = 1 and its 37-column locus dead; quartet 2 about 0.25 a site (the long
    prefixes need 256)."""
    rng = np.random.default_rng(311)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(off[-1])
    planes = np.stack([_planes(rng, n, s) for s in (0.05, 0.05, 0.2)], axis=1)
    dead = np.zeros(n, bool)
    dead[off[3] + 5:off[3] + 9] = True
    dead[off[5] + 250:off[5] + 262] = True            # across the LDS tile's edge of the long locus
    dead[off[4]] = dead[off[5] - 1] = True
    planes[:, :, dead] = 0.0
    planes[:, 1, off[1]] = (1.0, 0.0, 0.0)            # quartet 1: a certain signal site
    planes[:, 1, off[2]:off[3]] = 0.0                 # ... and a locus without a live site
    dp = np.zeros((3, 6, 5))
    for q in range(3):
        for k in range(6):
            dp[q, k] = er.windowed_dp(*lr.concatenated(planes[:, q], off, ORDERS[q], k + 1))
    mirror = {cap: np.stack([lr.exact_rows(planes[:, q], off, ORDERS[q], cap) for q in range(3)]) for cap in (64, 128)}
    mirror[256] = lr.exact_rows(planes[:, 2], off, ORDERS[2], 256)[None]
    return dict(off=off, planes=planes, dp=dp, mirror=mirror)


@pytest.fixture(scope="module")
def synthetic():
    """Planes and CPU references, computed once and left unchanged."""
    return _synthetic()


def _synthetic_plan(engine, off):
    L = len(off) - 1
    return engine.Plan(5, PARENT, BLEN, LEAF, off, np.full((L, 4), 0.25), None, 8, [], [], correction=1.0, threshold=0, round_decimals=-1,
                       model="f81")


def _check_against(rows, dp, mirror, cap, label):
    """rows, mirror [n_q][K][6], dp [n_q][K][5]; the computed prefixes form a head, the others are NaN / 0 / the bound"""
    worst_dp = worst_m = 0.0
    for q in range(rows.shape[0]):
        computed = rows[q, :, 4] != 0
        assert np.array_equal(computed, mirror[q, :, 4] != 0), (label, q, rows[q, :, 4], mirror[q, :, 4])
        assert np.array_equal(computed, np.arange(rows.shape[1]) < computed.sum())                     # a head
        for k in range(rows.shape[1]):
            g = rows[q, k]
            assert abs(g[5] - mirror[q, k, 5]) <= 1e-9 * mirror[q, k, 5], (label, q, k, g[5], mirror[q, k, 5])
            if not computed[k]:
                assert np.all(np.isnan(g[:4])) and g[4] == 0 and g[5] > 1e-12
                continue
            assert g[4] == cap and 0.0 <= g[5] <= 1e-12
            assert g[:4].min() >= 0.0 and g[:4].max() <= 1.0 and abs(g[:4].sum() - 1.0) <= 1e-12
            d_dp = np.abs(g[:4] - dp[q, k, :4]).max() - dp[q, k, 4] - g[5]
            d_m = np.abs(g[:4] - mirror[q, k, :4]).max() - g[5]
            worst_dp, worst_m = max(worst_dp, d_dp), max(worst_m, d_m)
    print("%s cap %d: heads %s; beyond lost mass and tail bound, against the DP %.2e, against the mirror %.2e (allowed %.0e)"
          % (label, cap, (rows[..., 4] != 0).sum(axis=1).tolist(), worst_dp, worst_m, TOL))
    assert worst_dp <= TOL and worst_m <= TOL


# ---- 1. synthetic planes: the exact rows ------------------------------------------------------------------------------
def test_exact_rows_against_the_dp_and_the_mirror(synthetic):
    engine = _engine()
    s = synthetic
    y, x1, x2 = s["planes"]
    plan = _synthetic_plan(engine, s["off"])
    try:
        got = {cap: plan.locus_set_exact(y, x1, x2, ORDERS, window_cap=cap) for cap in (64, 128)}
        got[256] = plan.locus_set_exact(y[2:], x1[2:], x2[2:], ORDERS[2:], window_cap=256)
        per_locus = {cap: plan.quartet_exact(y, x1, x2, window_cap=cap) for cap in (64, 128)}
    finally:
        plan.close()
    _check_against(got[64], s["dp"], s["mirror"][64], 64, "three quartets")
    _check_against(got[128], s["dp"], s["mirror"][128], 128, "three quartets")
    _check_against(got[256], s["dp"][2:], s["mirror"][256], 256, "quartet 2 alone")
    # the head rule, by the reference's window rule alone: quartet 0 at 64 stops inside its order, at 128 it does not;
    # quartet 2 needs 256 for its long prefixes
    heads = {cap: (got[cap][..., 4] != 0).sum(axis=1).tolist() for cap in got}
    for cap, rows, quartets in ((64, got[64], range(3)), (128, got[128], range(3)), (256, got[256], [2])):
        for i, q in enumerate(quartets):
            for k in range(6):
                _, var = er.moments(*lr.concatenated(s["planes"][:, q], s["off"], ORDERS[q], k + 1))
                M, bound = er.window_rule(var, cap)
                want = (M != 0)                                        # some window up to the cap holds the prefix
                assert (rows[i, k, 4] != 0) == want, (cap, q, k, var, bound, rows[i, k])
                assert abs(rows[i, k, 5] - er.tail_bound(var, cap)) <= 1e-9 * er.tail_bound(var, cap)
    assert 0 < heads[64][0] < 6 and heads[128][0] == 6 and heads[128][2] < 6 and heads[256] == [6], heads
    # quartet 1: a point law (read off the centres, also after the empty locus), then a locus without a live site
    for cap in (64, 128):
        assert np.array_equal(got[cap][1, 0], [1, 0, 0, 0, cap, 0]) and np.array_equal(got[cap][1, 1], got[cap][1, 0])
        assert np.array_equal(got[cap][1, 2], got[cap][1, 0])
    assert np.array_equal(got[128][0, 1, :4], got[128][0, 0, :4])      # quartet 0: the empty locus adds nothing
    # k = 1 against the per-locus exact rows
    worst = 0.0
    for cap in (64, 128):
        for q in range(3):
            a, b = got[cap][q, 0], per_locus[cap][ORDERS[q, 0], q]
            assert (a[4] != 0) == (b[4] != 0)
            if a[4] != 0:
                worst = max(worst, np.abs(a[:4] - b[:4]).max() - a[5] - b[5])
    print("k = 1 against tphip_quartet_exact beyond both tail bounds: %.2e (allowed %.0e)" % (worst, TOL))
    assert worst <= TOL


def test_exact_rows_are_bit_identical_whatever_surrounds_them(synthetic):
    import torch
    engine = _engine()
    s = synthetic
    y, x1, x2 = s["planes"]
    plan = _synthetic_plan(engine, s["off"])
    try:
        first = plan.locus_set_exact(y, x1, x2, ORDERS)
        again = plan.locus_set_exact(y, x1, x2, ORDERS)
        short = plan.locus_set_exact(y, x1, x2, ORDERS[:, :4])
        perm = [2, 0, 1]
        permuted = plan.locus_set_exact(*[np.ascontiguousarray(p[perm]) for p in (y, x1, x2)], ORDERS[perm])
        longer = [1, 0, 1, 2, 0]
        other = ORDERS[longer].copy()
        other[2] = other[2][::-1]                                       # quartet 1 a second time, its order reversed
        wide = plan.locus_set_exact(*[np.ascontiguousarray(p[longer]) for p in (y, x1, x2)], other)
        changed = ORDERS.copy()
        changed[1] = [5, 4, 3, 2, 1, 0]
        around = plan.locus_set_exact(y, x1, x2, changed)
        cut = plan.locus_set_exact(y, x1, x2, ORDERS, n_head=3)
        d_planes = torch.from_numpy(np.ascontiguousarray(s["planes"])).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        dev = []
        need = plan.locus_set_exact_workspace_bytes(3, 6)
        for extra in (0, 4096):
            ws = torch.empty(need + extra, dtype=torch.uint8, device="cuda")
            d_rows = torch.zeros((3, 6, 6), dtype=torch.float64, device="cuda")
            plan.locus_set_exact_dev(d_planes[0], d_planes[1], d_planes[2], ORDERS, d_rows, ws, stream=stream)
            torch.cuda.synchronize()
            dev.append(d_rows.cpu().numpy())
        assert plan.locus_set_exact_workspace_bytes(3, 6, n_head=2) < need
    finally:
        plan.close()
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)   # noqa: E731
    assert same(first, again)
    assert same(short, first[:, :4])                                    # loci appended to the order
    assert same(permuted, first[perm])
    assert same(wide[[0, 1, 3, 4]], first[[1, 0, 2, 0]])
    assert same(around[[0, 2]], first[[0, 2]])                          # another quartet's order changed
    assert same(dev[0], first) and same(dev[1], first)                  # _dev, and a larger workspace
    assert same(cut[:, :3], first[:, :3])
    assert np.all(np.isnan(cut[:, 3:, :4])) and np.all(cut[:, 3:, 4] == 0) and same(cut[:, 3:, 5], first[:, 3:, 5])
    print("exact rows bit-identical: twice, loci appended, permuted / longer quartet list, another order changed, _dev, "
          "a larger workspace, n_head = 3 for k <= 3")


def test_bad_options_are_rejected(synthetic):
    import torch
    engine = _engine()
    s = synthetic
    y, x1, x2 = s["planes"]
    plan = _synthetic_plan(engine, s["off"])
    try:
        for order, message in ((np.array([[0, 1, 1]] * 3), "repeated"), (np.array([[0, 1, 6]] * 3), "out of range"),
                               (np.array([[0, -1, 2]] * 3), "out of range"), (np.zeros((3, 7), np.int32), "n_k must be in 1..nloci"),
                               (np.zeros((3, 0), np.int32), "n_k must be in 1..nloci")):
            with pytest.raises(engine.TphipError, match=message):
                plan.locus_set_exact(y, x1, x2, order)
        for bad, message in ((dict(window_cap=48), "window_cap must be a power of two"), (dict(window_cap=1024), "window_cap must be"),
                             (dict(tail_tolerance=2.0), "tail_tolerance must be in"), (dict(n_head=7), "n_head must be in"),
                             (dict(n_head=-1), "n_head must be in")):
            with pytest.raises(engine.TphipError, match=message):
                plan.locus_set_exact(y, x1, x2, ORDERS, **bad)
        with pytest.raises(engine.TphipError, match="one row per quartet"):
            plan.locus_set_exact(y, x1, x2, ORDERS[:2])
        d_planes = torch.from_numpy(np.ascontiguousarray(s["planes"])).cuda()
        d_rows = torch.zeros((3, 6, 6), dtype=torch.float64, device="cuda")
        ws = torch.empty(plan.locus_set_exact_workspace_bytes(3, 6), dtype=torch.uint8, device="cuda")
        with pytest.raises(engine.TphipError, match="libtphip error 1: ws_bytes: workspace smaller"):
            plan.locus_set_exact_dev(d_planes[0], d_planes[1], d_planes[2], ORDERS, d_rows, ws[:-256])
    finally:
        plan.close()
    rows8 = np.zeros((6, 3, 8))
    with pytest.raises(engine.TphipError, match="repeated"):
        engine.locus_set_rows(rows8, np.array([[0, 0]] * 3))
    with pytest.raises(engine.TphipError, match="out of range"):
        engine.locus_set_rows(rows8, np.array([[0, 6]] * 3))
    with pytest.raises(engine.TphipError, match="must be \\[L, n_q, 8\\]"):
        engine.locus_set_rows(np.zeros((6, 3, 9)), np.array([[0, 1]] * 3))


def test_the_pipelines_tiles_keep_the_engines_own_workspace_within_the_bound(synthetic):
    """pipeline.locus_set_tile estimates the workspace; the engine states it (tphip_locus_set_exact_workspace_bytes).  Whatever
    (tile, n_head) the pipeline picks keeps the real figure within the bound, on few and on many loci, unless not even one
    quartet with one prefix fits."""
    engine = _engine()
    s = synthetic
    from tapir_amd import pipeline
    old = pipeline.EXACT_QUARTET_BYTES
    many = _synthetic_plan(engine, np.arange(3001, dtype=np.int64))
    try:
        for plan_, L in ((_synthetic_plan(engine, s["off"]), 6), (many, 3000)):
            for bound in (1 << 14, 1 << 18, 1 << 22, 1 << 26):
                for cap in (64, 128, 512):
                    for n_q, n_k in ((3, L), (200, min(L, 500)), (256, 1)):
                        pipeline.EXACT_QUARTET_BYTES = bound
                        tile, n_head = pipeline.locus_set_tile(L, 3000, n_q, n_k, 3, cap)
                        need = plan_.locus_set_exact_workspace_bytes(tile, n_k, cap, n_head)
                        assert need <= bound or (tile == 1 and n_head == 1), (L, bound, cap, n_q, n_k, tile, n_head, need)
            if plan_ is not many:
                plan_.close()
    finally:
        pipeline.EXACT_QUARTET_BYTES = old
        many.close()


# ---- 2. through the real path -----------------------------------------------------------------------------------------
REAL_SIZES = [20, 33, 60]
Q3 = [(20.0, 5.0), (7.0, 7.0), (50.0, 0.5)]                                                        # (T, t_o)
U3 = [(20.0, 22.0, 25.0, 30.0, 5.0), (100.0, 5.0, 90.0, 6.0, 2.0), (9.0, 8.0, 7.0, 6.0, 4.0)]     # four distinct tips each
REAL_ORDERS = np.array([[2, 0, 1], [1, 2, 0], [0, 1, 2]], np.int32)


def _real_case(kind):
    rng = np.random.default_rng(20261021 + (kind == "f81"))
    off = np.concatenate([[0], np.cumsum(REAL_SIZES)]).astype(np.int64)
    n = int(off[-1])
    rates = 10.0 ** rng.uniform(-3.5, -1.0, n)
    nres = np.full(n, 5, np.int32)
    nres[off[1] + 4:off[1] + 30:3] = 2                         # a locus with culled columns
    rates[off[2] + 7] = 0.0                                    # a zero rate
    pi = rng.dirichlet([6.0] * 4, len(REAL_SIZES))
    exch = rng.uniform(0.3, 4.0, (len(REAL_SIZES), 6)) if kind == "gtr" else None
    return dict(kind=kind, off=off, rates=rates, nres=nres, pi=pi, exch=exch)


def _real_plan(engine, c):
    return engine.Plan(5, PARENT, BLEN, LEAF, c["off"], c["pi"], c["exch"], 8, [], [], correction=1.0, threshold=3, round_decimals=-1,
                       model=c["kind"])


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_real_path_exact_and_normal_rows(kind):
    """*_quartet_sites_dev -> locus_set_exact_dev on the buffer where it lies; the normal rows from the engine's own per-locus
    rows."""
    import torch
    engine = _engine()
    c = _real_case(kind)
    plan = _real_plan(engine, c)
    try:
        d_r, d_n = torch.from_numpy(c["rates"]).cuda(), torch.from_numpy(c["nres"]).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        ws = torch.empty(plan.locus_set_exact_workspace_bytes(3, 3), dtype=torch.uint8, device="cuda")
        d_eq = torch.zeros((2, 3, len(c["rates"])), dtype=torch.float64, device="cuda")
        d_un = torch.zeros((3, 3, len(c["rates"])), dtype=torch.float64, device="cuda")
        d_eq_rows = torch.zeros((3, 3, 6), dtype=torch.float64, device="cuda")
        d_un_rows = torch.zeros((3, 3, 6), dtype=torch.float64, device="cuda")
        plan.quartet_sites_dev(d_r, d_n, Q3, d_eq, stream)
        plan.locus_set_exact_dev(d_eq[0], d_eq[1], d_eq[1], REAL_ORDERS, d_eq_rows, ws, stream=stream)
        plan.unequal_quartet_sites_dev(d_r, d_n, U3, d_un, stream)
        plan.locus_set_exact_dev(d_un[0], d_un[1], d_un[2], REAL_ORDERS, d_un_rows, ws, stream=stream)
        torch.cuda.synchronize()
        eq_sites, un_sites = d_eq.cpu().numpy(), d_un.cpu().numpy()
        eq_exact, un_exact = d_eq_rows.cpu().numpy(), d_un_rows.cpu().numpy()
        host_exact = plan.locus_set_exact(un_sites[0], un_sites[1], un_sites[2], REAL_ORDERS)
        eq_locus = plan.quartet_tables(c["rates"], c["nres"], Q3)
        un_locus = plan.unequal_quartet_tables(c["rates"], c["nres"], U3)
    finally:
        plan.close()
    assert np.array_equal(host_exact, un_exact)
    worst = 0.0
    for exact, planes in ((eq_exact, (eq_sites[0], eq_sites[1], eq_sites[1])), (un_exact, tuple(un_sites))):
        assert np.all(exact[..., 4] == 128) and np.all(exact[..., 5] <= 1e-12)
        for q in range(3):
            for k in range(3):
                want = er.windowed_dp(*lr.concatenated([p[q] for p in planes], c["off"], REAL_ORDERS[q], k + 1))
                worst = max(worst, np.abs(exact[q, k, :4] - want[:4]).max() - want[4] - exact[q, k, 5])
    print("%s: exact rows from the engine's own site values against the DP beyond lost mass and tail bound %.2e (allowed %.0e)"
          % (kind, worst, TOL))
    assert worst <= TOL
    worst_p = 0.0
    for locus_rows, nsum, rule in ((eq_locus, 5, qr.probabilities), (un_locus, 9, ur.probabilities)):
        rows = engine.locus_set_rows(locus_rows, REAL_ORDERS)
        assert rows.shape == (3, 3, locus_rows.shape[2])
        d_in, d_out = torch.from_numpy(locus_rows).cuda(), torch.zeros(rows.shape, dtype=torch.float64, device="cuda")
        engine.locus_set_rows_dev(d_in, 3, REAL_ORDERS, d_out, family=int(nsum == 9))
        assert np.array_equal(d_out.cpu().numpy(), rows)
        for q in range(3):
            assert np.array_equal(rows[q, :, :nsum], np.cumsum(locus_rows[REAL_ORDERS[q], q, :nsum], axis=0))
            assert np.array_equal(rows[q, 0], locus_rows[REAL_ORDERS[q, 0], q])                       # k = 1: the per-locus row
            for k in range(3):
                worst_p = max(worst_p, max(abs(a - b) for a, b in zip(rows[q, k, nsum:], rule(rows[q, k, :nsum]))))
        assert np.array_equal(engine.locus_set_rows(locus_rows, REAL_ORDERS[:, :2]), rows[:, :2])
        assert np.array_equal(engine.locus_set_rows(locus_rows[:, ::-1], REAL_ORDERS[::-1]), rows[::-1])
    print("%s: normal rows' sums bit-equal to np.cumsum, k = 1 to the per-locus rows; probabilities against the restatement %.2e "
          "(allowed 1e-13)" % (kind, worst_p))
    assert worst_p <= 1e-13


# ---- 3. the command line ----------------------------------------------------------------------------------------------
def test_cli_locus_sets_on_the_bundled_loci(tmp_path, golden_dir):
    """chr1_918.nex under two names plus informativeness_cutoff.nex (its four columns under the tree's taxon names: the file's
    own tax1 .. tax5 are not in Euteleost.tree): the two copies tie in every p_correct, so file order decides between them, and
    the sums of the set of both are twice the one's."""
    import json
    import os
    import shutil
    import sqlite3
    engine = _engine()
    from tapir_amd import cli, compute, newick, nexus
    aln = tmp_path / "aln"
    aln.mkdir()
    for name in ("a_918.nex", "b_918.nex"):
        shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln / name)
    taxa, _ = nexus.read_states(os.path.join(golden_dir, "chr1_918.nex"))
    text = open(os.path.join(golden_dir, "informativeness_cutoff.nex")).read()
    for i, taxon in enumerate(taxa):
        text = text.replace("tax%d " % (i + 1), "%s " % taxon)
    (aln / "informativeness_cutoff.nex").write_text(text)
    tree = os.path.join(golden_dir, "Euteleost.tree")
    out = tmp_path / "out"
    out.mkdir()
    run = cli.main([str(aln), tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                    "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1", "--quartets", "30:4", "--unequal-quartets", "30/28/25/31:4",
                    "--exact-quartets", "--exact-quartets-window", "256", "--locus-sets", "--locus-sets-target", "0.9"])
    T = int(compute.correct_tree(newick.read_tree(tree))[0])
    for name, unequal, quartet in (("phylogenetic-informativeness-quartets.sqlite", False, (30.0, 4.0)),
                                   ("phylogenetic-informativeness-unequal-quartets.sqlite", True, (30.0, 28.0, 25.0, 31.0, 4.0))):
        con = sqlite3.connect(os.path.join(run, name))
        loci = con.execute("select id, locus from loci order by id").fetchall()
        per_locus = con.execute("select * from quartet order by id").fetchall()
        sets = con.execute("select * from locus_set order by k").fetchall()
        exact = con.execute("select * from locus_set_exact order by k").fetchall()
        summary = con.execute("select * from locus_set_summary").fetchall()
        meta = dict(con.execute("select key, value from meta"))
        con.close()
        names = [l[1] for l in loci]                                            # file order: whatever the directory gives
        assert sorted(names) == ["a_918", "b_918", "informativeness_cutoff"] and len(sets) == len(exact) == 3
        first, second = sorted((names.index("a_918"), names.index("b_918")))
        nsum, p_col = (9, 10) if unequal else (5, 6)
        p_locus = np.array([r[p_col] for r in per_locus])
        order = np.argsort(-p_locus, kind="stable")
        assert p_locus[first] == p_locus[second] and list(order).index(first) + 1 == list(order).index(second)   # the tie: file order
        assert [r[2] for r in sets] == [loci[l][0] for l in order]
        assert meta["locus_sets_order"] == "p_correct" and meta["locus_sets_target"] == "0.9" and meta["locus_sets_window_cap"] == "256"
        assert sets[0][3 + nsum:] == per_locus[order[0]][p_col:]                # k = 1: the per-locus row
        ka = list(order).index(first)                                           # the step that adds the first copy
        before = [0.0] * nsum if ka == 0 else list(sets[ka - 1][3:3 + nsum])
        one = [sets[ka][3 + m] - before[m] for m in range(nsum)]
        if ka == 0:                                                             # the same locus twice: the sums double
            assert [sets[1][3 + m] for m in range(nsum)] == [2 * v for v in one]
        rule = ur.probabilities if unequal else qr.probabilities
        for r in sets:
            assert max(abs(a - b) for a, b in zip(r[3 + nsum:], rule(r[3:3 + nsum]))) <= 1e-13
        p_set = [r[3 + nsum] for r in sets]
        assert summary[0][:4] == (sets[0][0], 0.9, lr.k_needed(p_set, 0.9), p_set[-1])
        planes = []
        for key, locus in (loci[l] for l in order):
            doc = json.load(open(os.path.join(run, locus + ".nex.rates")))["sites"]
            r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
            _, st = nexus.read_states(os.path.join(str(aln), locus + ".nex"))
            r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
            pi = [doc["freqs"][k] for k in "ACGT"]
            exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
            plan = engine.Plan(3, [3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1], [0, r.size], [pi], [exch], T, [], [],
                               correction=1.0, threshold=0, round_decimals=-1)
            try:
                s = plan.unequal_quartet_sites(r, None, [quartet]) if unequal else plan.quartet_sites(r, None, [quartet])
            finally:
                plan.close()
            planes.append(np.stack([s[0, 0], s[1, 0], s[-1, 0]]))
        worst, p_exact = 0.0, []
        for k in range(3):
            e = exact[k]
            assert e[1] == k + 1 and e[-2] == 256 and 0 <= e[-1] <= 1e-12      # (variances below about 230)
            want = er.windowed_dp(*np.concatenate(planes[:k + 1], axis=1))
            ref = want[:4] if unequal else (want[0], want[1] + want[2], want[3])
            worst = max(worst, max(abs(a - b) for a, b in zip(e[2:-2], ref)) - want[4] - e[-1])
            p_exact.append(e[2])
        print("%s: order %s (per-locus p_correct %s); exact p_correct of the sets %s, normal %s; against the windowed DP beyond lost "
              "mass and tail bound %.2e (allowed %.0e); k_needed %s, exact %s"
              % (name, [loci[l][1] for l in order], p_locus.tolist(), p_exact, p_set, worst, TOL, summary[0][2], summary[0][4]))
        assert worst <= TOL
        assert summary[0][4] == lr.k_needed(p_exact, 0.9)

"""The exact quartet resolution probabilities on the GPU (tphip_quartet_exact, tphip_quartet_exact_dev, --exact-quartets;
DESIGN.md section 3.9) against the dynamic programmes of tests/quartet_reference.py, tests/unequal_quartet_reference.py and
tests/exact_quartet_reference.py.  Run with -m gpu on the MI355X box.  Every test prints its figures before it asserts.

Bounds (stated by the definition, none tuned to the kernels):
  probabilities   1e-10 absolute against the dynamic programme applied to the very planes the kernels read (plus the mass a
                  windowed programme reports lost): at most 2048 factors at a few ulp each, times the weights' 1-norm, which
                  grows with log M.  The numpy restatement measured 7e-15.
  tail_bound      every row comes back computed with tail_bound <= 1e-12 at the default cap of 128 (the variances stay
                  below 51); which of two windows is picked at a tie of the bound with the tolerance is not asserted.
  rows            every computed row lies in [0, 1] and sums to 1 within 1e-12.
  bit identity    two calls; a permuted quartet list; a locus alone against inside the batch; host against _dev.
"""
import json
import os
import sqlite3

import numpy as np
import pytest

import exact_quartet_reference as er
import quartet_reference as qr
import unequal_quartet_reference as ur

pytestmark = pytest.mark.gpu

TOL = 1e-10
# a five-taxon tree ((A, B), (C, D), E): this stage never looks at it
PARENT, BLEN, LEAF = [2, 2, 7, 5, 5, 7, 7, -1], [0.1, 0.1, 0.05, 0.1, 0.1, 0.05, 0.2, 0.0], [0, 1, -1, 2, 3, -1, 4, -1]
SIZES = [1, 20, 33, 60, 60, 33, 20, 1]
Q6 = [(0.0, 3.0), (20.0, 5.0), (35.0, 1.0), (7.0, 7.0), (50.0, 0.5), (12.0, 40.0)]                 # (T, t_o); one with T = 0
U6 = [(20.0, 22.0, 25.0, 30.0, 5.0), (1.0, 0.0, 3.0, 40.0, 2.0), (100.0, 5.0, 90.0, 6.0, 2.0), (100.0, 5.0, 6.0, 90.0, 2.0),
      (9.0, 8.0, 7.0, 6.0, 4.0), (30.0, 31.0, 45.0, 70.0, 10.0)]                                   # four distinct tips each


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _check_rows(rows):
    """every row computed, in [0, 1], summing to 1"""
    assert np.all(np.isfinite(rows))
    assert np.all(np.isin(rows[..., 4], [16, 32, 64, 128, 256, 512])) and np.all(rows[..., 5] <= 1e-12) and np.all(rows[..., 5] >= 0)
    assert rows[..., :4].min() >= 0.0 and rows[..., :4].max() <= 1.0
    assert np.max(np.abs(rows[..., :4].sum(axis=-1) - 1.0)) <= 1e-12


# ---- 1. through the real path ---------------------------------------------------------------------------------------
def _real_case(kind):
    rng = np.random.default_rng(20261020 + (kind == "f81"))
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(off[-1])
    rates = 10.0 ** rng.uniform(-3.5, -1.0, n)
    nres = np.full(n, 5, np.int32)
    nres[off[3] + 4:off[3] + 30:3] = 2                         # a locus with culled columns
    rates[off[4] + 7] = 0.0                                    # a zero rate
    nres[off[6]:off[7]] = 0                                    # a locus culled entirely
    pi = rng.dirichlet([6.0] * 4, len(SIZES))
    exch = rng.uniform(0.3, 4.0, (len(SIZES), 6)) if kind == "gtr" else None
    return dict(kind=kind, off=off, rates=rates, nres=nres, pi=pi, exch=exch)


def _real_plan(engine, c):
    return engine.Plan(5, PARENT, BLEN, LEAF, c["off"], c["pi"], c["exch"], 8, [], [], correction=1.0, threshold=3, round_decimals=-1,
                       model=c["kind"])


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_rows_against_the_dp_on_the_engines_own_site_values(kind):
    engine = _engine()
    c = _real_case(kind)
    plan = _real_plan(engine, c)
    try:
        eq_sites = plan.quartet_sites(c["rates"], c["nres"], Q6)
        un_sites = plan.unequal_quartet_sites(c["rates"], c["nres"], U6)
        eq_rows = plan.quartet_exact(eq_sites[0], eq_sites[1], eq_sites[1])
        un_rows = plan.quartet_exact(un_sites[0], un_sites[1], un_sites[2])
    finally:
        plan.close()
    assert eq_rows.shape == un_rows.shape == (len(SIZES), 6, 6)
    _check_rows(eq_rows)
    _check_rows(un_rows)
    worst_eq = worst_un = 0.0
    for l in range(len(SIZES)):
        sl = slice(int(c["off"][l]), int(c["off"][l + 1]))
        for q in range(6):
            pc, pw, pp = qr.exact_resolution(eq_sites[0, q, sl], eq_sites[1, q, sl])
            g = eq_rows[l, q]
            worst_eq = max(worst_eq, abs(g[0] - pc), abs(g[1] + g[2] - pw), abs(g[3] - pp), abs(g[1] - g[2]))
            want = ur.exact_resolution(un_sites[0, q, sl], un_sites[1, q, sl], un_sites[2, q, sl])
            worst_un = max(worst_un, max(abs(a - b) for a, b in zip(un_rows[l, q, :4], want)))
    print("%s: 8 loci x 6 quartets; against the DPs %.2e (equal tips) %.2e (unequal), allowed %.0e; windows %s; largest tail bound %.1e"
          % (kind, worst_eq, worst_un, TOL, sorted(set(eq_rows[..., 4].ravel().tolist() + un_rows[..., 4].ravel().tolist())),
             max(eq_rows[..., 5].max(), un_rows[..., 5].max())))
    assert worst_eq <= TOL and worst_un <= TOL
    assert np.array_equal(eq_rows[6], [[0, 0, 0, 1, 16, 0]] * 6) and np.array_equal(un_rows[6], [[0, 0, 0, 1, 16, 0]] * 6)   # culled entirely


def test_device_calls_chain_without_leaving_the_device():
    """sites_dev -> quartet_exact_dev on the buffer where it lies, as pipeline.exact_quartet_tables does: the host twin's rows."""
    import torch
    from tapir_amd import pipeline
    engine = _engine()
    c = _real_case("gtr")
    plan = _real_plan(engine, c)
    try:
        un_sites = plan.unequal_quartet_sites(c["rates"], c["nres"], U6)
        host = plan.quartet_exact(un_sites[0], un_sites[1], un_sites[2])
        d_r, d_n = torch.from_numpy(c["rates"]).cuda(), torch.from_numpy(c["nres"]).cuda()
        d_sites = torch.zeros((3, 6, len(c["rates"])), dtype=torch.float64, device="cuda")
        d_rows = torch.zeros((len(SIZES), 6, 6), dtype=torch.float64, device="cuda")
        ws = torch.empty(plan.quartet_exact_workspace_bytes(6), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        plan.unequal_quartet_sites_dev(d_r, d_n, U6, d_sites, stream)
        plan.quartet_exact_dev(d_sites[0], d_sites[1], d_sites[2], 6, d_rows, ws, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_rows.cpu().numpy(), host)
        with pytest.raises(engine.TphipError, match="libtphip error 1: ws_bytes: workspace smaller"):
            plan.quartet_exact_dev(d_sites[0], d_sites[1], d_sites[2], 6, d_rows, ws[:64])
        for bad, message in ((dict(window_cap=48), "window_cap must be a power of two"), (dict(window_cap=1024), "window_cap must be"),
                             (dict(tail_tolerance=2.0), "tail_tolerance must be in"), (dict(tail_tolerance=-1e-3), "tail_tolerance must be in")):
            with pytest.raises(engine.TphipError, match=message):
                plan.quartet_exact(un_sites[0], un_sites[1], un_sites[2], **bad)
        with pytest.raises(engine.TphipError, match="n_q must be in 1..256"):
            plan.quartet_exact(np.zeros((257, len(c["rates"]))), np.zeros((257, len(c["rates"]))), np.zeros((257, len(c["rates"]))))
    finally:
        plan.close()
    # the pipeline on the same final rates (NaN = culled), in three tiles of two quartets
    fin = np.where(c["nres"] >= 3, c["rates"], np.nan)
    per_locus = [fin[c["off"][l]:c["off"][l + 1]] for l in range(len(SIZES))]
    old = pipeline.EXACT_QUARTET_BYTES
    pipeline.EXACT_QUARTET_BYTES = 4 * 8 * 440
    try:
        rows = pipeline.exact_unequal_quartet_tables(engine, per_locus, c["pi"], c["exch"],
                                                     pipeline.Run(["a", "b", "c", "d", "e"], PARENT, BLEN, LEAF, 8, [], [], device=0), U6)
    finally:
        pipeline.EXACT_QUARTET_BYTES = old
    assert np.array_equal(rows, host)


# ---- 2. synthetic planes fed straight to quartet_exact --------------------------------------------------------------
def _planes(rng, n, scale):
    y, x1, x2 = rng.gamma(1.0, scale, n), rng.gamma(1.0, 0.4 * scale, n), rng.gamma(1.0, 0.3 * scale, n)
    f = np.minimum(1.0, 0.95 / (y + x1 + x2))
    return y * f, x1 * f, x2 * f


def _synthetic():
    """Loci: all zero | y = 0.9 on 60 sites | 2000 columns | two point laws (window 16) | variances about 3 (64) | about 23
    (128) | about 100 (256: needs the cap raised) | one site.  Quartet 0 has x1 != x2, quartet 1 the same y with min(x1, x2)
    for both."""
    rng = np.random.default_rng(77)
    loci = [(np.zeros(37),) * 3,
            (np.full(60, 0.9), np.full(60, 0.03), np.full(60, 0.02)),
            _planes(rng, 2000, 0.004),
            (np.array([1.0, 0, 1, 0, 1, 0, 0]), np.zeros(7), np.array([0, 1.0, 0, 0, 0, 0, 0])),
            (np.zeros(5), np.array([0, 1.0, 1, 0, 1]), np.zeros(5)),
            _planes(rng, 50, 0.04),
            _planes(rng, 60, 0.35),
            _planes(rng, 700, 0.12),
            (np.array([0.3]), np.array([0.2]), np.array([0.1]))]
    off = np.concatenate([[0], np.cumsum([len(l[0]) for l in loci])]).astype(np.int64)
    y = np.concatenate([l[0] for l in loci])
    x1 = np.concatenate([l[1] for l in loci])
    x2 = np.concatenate([l[2] for l in loci])
    xm = np.minimum(x1, x2)
    planes = np.stack([np.stack([y, y]), np.stack([x1, xm]), np.stack([x2, xm])])     # [3][n_q = 2][ncols]
    ref = np.zeros((len(loci), 2, 5))                          # p_correct, p_ac, p_ad, p_polytomy, lost
    for l, (a, b) in enumerate(zip(off[:-1], off[1:])):
        for q in range(2):
            v = planes[:, q, a:b]
            ref[l, q] = (ur.exact_resolution(*v) + (0.0,)) if b - a <= 60 else er.windowed_dp(*v)
    want_window = [er.resolution(*planes[:, 0, a:b], cap=256)[4] for a, b in zip(off[:-1], off[1:])]
    assert want_window == [16, 128, 128, 16, 16, 64, 128, 256, 64]
    return dict(off=off, planes=planes, ref=ref)


@pytest.fixture(scope="module")
def synthetic():
    """Planes and CPU references, computed once and left unchanged."""
    return _synthetic()


def _synthetic_plan(engine, off):
    L = len(off) - 1
    return engine.Plan(5, PARENT, BLEN, LEAF, off, np.full((L, 4), 0.25), None, 8, [], [], correction=1.0, threshold=0, round_decimals=-1,
                       model="f81")


def test_synthetic_planes_against_the_dps(synthetic):
    engine = _engine()
    s = synthetic
    y, x1, x2 = s["planes"]
    plan = _synthetic_plan(engine, s["off"])
    try:
        rows = plan.quartet_exact(y, x1, x2, window_cap=256)
        at128 = plan.quartet_exact(y, x1, x2)
    finally:
        plan.close()
    _check_rows(rows)
    d = np.abs(rows[..., :4] - s["ref"][..., :4]).max(axis=-1)
    print("synthetic planes: difference per (locus, quartet) %s; DP lost %s; windows %s; tail bounds %s"
          % (d.tolist(), s["ref"][..., 4].tolist(), rows[..., 4].tolist(), rows[..., 5].tolist()))
    assert np.all(d <= TOL + s["ref"][..., 4])
    assert np.array_equal(rows[0], [[0, 0, 0, 1, 16, 0]] * 2)                       # all zero: exactly, tail bound 0
    assert np.array_equal(rows[3, 0], [1, 0, 0, 0, 16, 0]) and np.array_equal(rows[4, 0], [0, 1, 0, 0, 16, 0])   # point laws
    assert rows[1, 0, 4] == 128 and rows[2, 0, 4] == 128 and rows[5, 0, 4] == 64 and rows[6, 0, 4] == 128 and rows[7, 0, 4] == 256
    # the default cap: the 700-site locus (variance about 100) is not computed, every other row is the same bits
    keep = [0, 1, 2, 3, 4, 5, 6, 8]
    assert np.array_equal(at128[keep], rows[keep])
    assert np.all(np.isnan(at128[7, :, :4])) and np.all(at128[7, :, 4] == 0) and np.all(at128[7, :, 5] > 1e-12)


def test_a_cap_too_small_reports_nothing(synthetic):
    engine = _engine()
    s = synthetic
    a, b = int(s["off"][6]), int(s["off"][7])                                       # the 60-site locus, variances about 23
    (_, var) = er.moments(*s["planes"][:, 0, a:b])
    plan = _synthetic_plan(engine, [0, b - a])
    try:
        rows = plan.quartet_exact(*[np.ascontiguousarray(p[:, a:b]) for p in s["planes"]], window_cap=32)
    finally:
        plan.close()
    print("60 sites, variances %s, cap 32: rows %s" % (var, rows.tolist()))
    assert 15 < max(var) < 35
    assert np.all(np.isnan(rows[0, :, :4])) and np.all(rows[0, :, 4] == 0) and np.all(rows[0, :, 5] > 1e-12)
    assert abs(rows[0, 0, 5] / er.tail_bound(var, 32) - 1) <= 1e-9                  # the bound at the cap


def test_rows_are_bit_identical_whatever_surrounds_them(synthetic):
    engine = _engine()
    s = synthetic
    y, x1, x2 = s["planes"]
    off = s["off"]
    plan = _synthetic_plan(engine, off)
    try:
        first = plan.quartet_exact(y, x1, x2, window_cap=256)
        again = plan.quartet_exact(y, x1, x2, window_cap=256)
        swapped = plan.quartet_exact(*[np.ascontiguousarray(p[::-1]) for p in (y, x1, x2)], window_cap=256)
        wide = plan.quartet_exact(*[np.ascontiguousarray(np.concatenate([p[1:], p, p[:1]])) for p in (y, x1, x2)], window_cap=256)
    finally:
        plan.close()
    assert np.array_equal(first, again)
    assert np.array_equal(swapped[:, ::-1], first)                                   # a permuted quartet list
    assert np.array_equal(wide[:, 1:3], first) and np.array_equal(wide[:, 0], first[:, 1]) and np.array_equal(wide[:, 3], first[:, 0])
    for l in (2, 6, 7, 8):                                                          # a locus alone
        a, b = int(off[l]), int(off[l + 1])
        alone = _synthetic_plan(engine, [0, b - a])
        try:
            rows = alone.quartet_exact(*[np.ascontiguousarray(p[:, a:b]) for p in (y, x1, x2)], window_cap=256)
        finally:
            alone.close()
        assert np.array_equal(rows[0], first[l]), l
    print("rows bit-identical: twice, under a permuted or longer quartet list, alone")


# ---- 3. the command line --------------------------------------------------------------------------------------------
def test_cli_exact_quartets_on_the_bundled_locus(tmp_path, golden_dir):
    import shutil
    engine = _engine()
    from tapir_amd import cli, compute, newick, nexus
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    tree = os.path.join(golden_dir, "Euteleost.tree")
    out = tmp_path / "out"
    out.mkdir()
    run = cli.main([str(aln), tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                    "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1", "--quartets", "30:4", "--exact-quartets"])
    con = sqlite3.connect(os.path.join(run, "phylogenetic-informativeness-quartets.sqlite"))
    got = con.execute("select id, quartet, p_correct, p_incorrect, p_polytomy, window, tail_bound from quartet_exact").fetchall()
    approx = con.execute("select p_correct, p_incorrect, p_polytomy from quartet").fetchall()
    meta = dict(con.execute("select key, value from meta"))
    con.close()
    assert len(got) == 1 and got[0][:2] == (1, "30:4") and meta["exact_window_cap"] == "128"
    doc = json.load(open(os.path.join(run, "chr1_918.nex.rates")))["sites"]
    r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
    _, st = nexus.read_states(os.path.join(str(aln), "chr1_918.nex"))
    r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
    pi = [doc["freqs"][k] for k in "ACGT"]
    exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
    T = int(compute.correct_tree(newick.read_tree(tree))[0])
    plan = engine.Plan(3, [3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1], [0, r.size], [pi], [exch], T, [], [],
                       correction=1.0, threshold=0, round_decimals=-1)
    try:
        sites = plan.quartet_sites(r, None, [(30.0, 4.0)])
    finally:
        plan.close()
    pc, p1, p2, pp, lost = er.windowed_dp(sites[0, 0], sites[1, 0], sites[1, 0])
    d = max(abs(got[0][2] - pc), abs(got[0][3] - (p1 + p2)), abs(got[0][4] - pp))
    print("chr1_918 (%d sites), quartet 30:4: exact %s (window %d, tail bound %.1e) against the windowed DP %.2e (lost %.1e); the "
          "normal approximation %s" % (r.size, got[0][2:5], got[0][5], got[0][6], d, lost, approx[0]))
    assert got[0][5] in (64, 128) and 0 <= got[0][6] <= 1e-12
    assert d <= TOL + lost

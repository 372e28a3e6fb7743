"""Quartet signal and noise on the GPU (tphip_quartet_sites, tphip_quartet_tables, --quartets) against
tests/quartet_reference.py.  Run with -m gpu on the MI355X box.  Every test prints its figures before it asserts.

Bounds (stated by the definition, none tuned to the kernels):
  per-site y, x   relative, against the 40-digit twin: 16 x the largest relative error the fp64 numpy restatement shows
                  against the twin on the same (site, quartet) pairs, at least 64 * 2^-52.  The factor allows for the device's
                  Jacobi eigen-system against LAPACK's and for another expm1.  A reference of exactly 0 must come back as 0.
                  The twin enumerates 256 patterns at 40 digits (about 30 ms a pair), so it is taken on a sample of pairs:
                  the first and last columns of every locus, both sides of every 1024-column chunk boundary, the zero,
                  culled and saturated rates, the smallest and largest rates and a few others, under quartets that cover
                  T = 0, repeated T, repeated t_o and t_o from 1e-3 to 50.  Every other pair is held against the restatement
                  itself within bound + (the restatement's own error), which is what the two bounds above imply.
  sums            against math.fsum of the GPU's own per-site values: (n_l + 64) 2^-52 relative (non-negative terms)
  probabilities   against the restatement fed the GPU's sums: 1e-13 absolute (a 64-point rule on a smooth integrand; the
                  restatement is held against scipy on the same arguments in the same test -- against mpmath within 1e-9 of
                  |rho| = 1, where scipy answers for the singular case)
  bit identity    of a locus' row: alone against among its neighbours, n_q = 1 against the same quartet inside the list of
                  17, 130 and 256 quartets (three and four launches) against shorter calls cut at a launch boundary and
                  across it, the host-pointer call against the _dev call
"""
import json
import math
import os
import sqlite3

import numpy as np
import pytest

import hp_reference as hp
import quartet_reference as qr

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a three-taxon tree: this stage never looks at it
PARENT, BLEN, LEAF = [3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1]
LOCI = [0, 1, 3, 63, 64, 65, 1023, 1024, 1025, 2049]
F81_LOCI = [5, 64, 130, 1030]
CORRECTION = 1.25
# T = 0, repeated T (next to each other: the kernel reuses the matrix; and apart), repeated t_o, t_o from 1e-3 to 50
Q17 = [(0.0, 1e-3), (0.0, 3.0), (20.0, 3.0), (20.0, 5.0), (50.0, 5.0), (50.0, 10.0), (100.0, 2.0), (7.5, 2.0), (7.5, 50.0),
       (1e-2, 50.0), (1.0, 1.0), (300.0, 0.5), (20.0, 5.0), (3.0, 0.01), (3.0, 0.01), (64.0, 1e-3), (0.0, 50.0)]
QLISTS = {1: [Q17[5]], 3: Q17[3:6], 17: Q17}
TWIN_Q = [0, 3, 6, 11, 15]          # quartets of the twin's sample (indices into Q17)
# 256 distinct quartets (every t_o differs: 257 is prime); neighbours 2 k, 2 k + 1 share T, so matrices are reused inside a
# launch and never across the launch boundaries at 64, 128 and 192
Q256 = [(((k // 2) % 13) * 2.5 * (1.0 + (k // 26) / 16.0), 10.0 ** (-3.0 + 4.5 * ((k * 37) % 257) / 256.0)) for k in range(256)]
assert len(set(Q256)) == 256


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _inputs(sizes, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    rates = 10.0 ** rng.uniform(-9, 3, n) * CORRECTION            # final rates log-uniform in [1e-9, 1e3]
    nres = np.full(n, 5, np.int32)
    for a, b in zip(off[:-1], off[1:]):
        if b - a >= 3:
            rates[a] = 0.0                 # an exact zero
            nres[a + 1] = 2                # a culled column
            rates[a + 2] = 1e-9 * CORRECTION
        if b - a >= 63:
            rates[a + 40] = 0.0
            nres[a + 41] = 0
            rates[b - 1] = 1e3 * CORRECTION
    return rng, off, rates, nres


def _sample_columns(rng, off, extra):
    cols = set(extra)
    for a, b in zip(off[:-1], off[1:]):
        cols.update(c for c in (a, a + 1, a + 2, b - 1) if a <= c < b)
        cols.update(a + k for k in (1023, 1024, 2047, 2048) if a + k < b)   # both sides of the chunk boundaries
    cols.update(rng.integers(0, off[-1], 6).tolist())
    return np.array(sorted(cols), dtype=np.int64)


def _case(kind):
    if kind == "gtr":
        rng, off, rates, nres = _inputs(LOCI, 20261018)
        L = len(LOCI)
        pi = rng.dirichlet([6.0] * 4, L)
        exch = rng.uniform(0.3, 4.0, (L, 6))
        nres[off[5]:off[6]] = 0                                    # the 65-column locus culled entirely
        sat = int(off[7]) + 100
        rates[sat] = 1e4 * CORRECTION                              # one saturated rate, in the 1024-column locus
        extra = [sat]
    else:
        rng, off, rates, nres = _inputs(F81_LOCI, 20261019)
        L = len(F81_LOCI)
        pi = rng.dirichlet([6.0] * 4, L)
        pi[1] = [0.37, 0.0, 0.41, 0.22]                            # an absent base
        pi[3] = [0.25] * 4                                         # Jukes-Cantor
        exch = None
        extra = [int(off[1]) + 7]
    fin = hp.finalize_rates(rates, -1, CORRECTION, nres, 3)
    locus_of = np.searchsorted(off, np.arange(off[-1]), side="right") - 1
    cols = _sample_columns(rng, off, extra)
    ones = np.ones(6)
    # the restatement everywhere, the twin on the sample
    rest = np.zeros((2, len(Q17), int(off[-1])))
    for l in range(L):
        sl = slice(int(off[l]), int(off[l + 1]))
        for q, (tip, internode) in enumerate(Q17):
            rest[0, q, sl], rest[1, q, sl] = qr.site_values(kind, pi[l], ones if exch is None else exch[l], fin[sl], tip, internode)
    twin = {}
    for c in cols.tolist():
        l = int(locus_of[c])
        for q in TWIN_Q:
            ty, tx, _ = qr.twin_values(pi[l], ones if exch is None else exch[l], [fin[c]], *Q17[q])
            twin[(c, q)] = (ty[0], tx[0])
    return dict(kind=kind, sizes=LOCI if kind == "gtr" else F81_LOCI, off=off, rates=rates, nres=nres, fin=fin, pi=pi, exch=exch,
                cols=cols, rest=rest, twin=twin, locus_of=locus_of)


@pytest.fixture(scope="module")
def cases():
    """Inputs and CPU references of both plans, computed once and left unchanged."""
    return {k: _case(k) for k in ("gtr", "f81")}


def _plan(engine, c, loci=None):
    """The case's plan, or one over a subset of its loci (same models, same columns)."""
    ids = list(range(len(c["sizes"]))) if loci is None else list(loci)
    sizes = [c["sizes"][l] for l in ids]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pick = np.concatenate([np.arange(c["off"][l], c["off"][l + 1]) for l in ids]).astype(np.int64) if ids else np.zeros(0, np.int64)
    plan = engine.Plan(3, PARENT, BLEN, LEAF, off, c["pi"][ids], None if c["exch"] is None else c["exch"][ids], 8, [], [],
                       correction=CORRECTION, threshold=3, round_decimals=-1, model=c["kind"])
    return plan, c["rates"][pick], c["nres"][pick]


def _relative(got, ref):
    import mpmath as mp
    with mp.workdps(40):
        return float(abs(mp.mpf(float(got)) - ref) / ref)


# ---- 1. per-site values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_sites_against_the_40_digit_twin(cases, kind):
    engine = _engine()
    c = cases[kind]
    plan, rates, nres = _plan(engine, c)
    try:
        got = plan.quartet_sites(rates, nres, Q17)
    finally:
        plan.close()
    assert got.shape == (2, 17, len(rates))
    # the restatement's own error on the sample: it sets the bound, the GPU's output never does
    e_rest, e_gpu, zeros_ok = 0.0, 0.0, True
    for (col, q), ref in c["twin"].items():
        for which in (0, 1):
            if ref[which] == 0:
                zeros_ok = zeros_ok and got[which, q, col] == 0.0 and c["rest"][which, q, col] == 0.0
            else:
                e_rest = max(e_rest, _relative(c["rest"][which, q, col], ref[which]))
                e_gpu = max(e_gpu, _relative(got[which, q, col], ref[which]))
    bound = max(16 * e_rest, 64 * U)
    print("%s: %d (site, quartet) pairs; restatement against the twin %.3e, bound %.3e, GPU against the twin %.3e: "
          "error / bound = %.3f" % (kind, len(c["twin"]), e_rest, bound, e_gpu, e_gpu / bound))
    assert zeros_ok                                    # a reference of exactly 0 comes back as 0
    assert e_gpu <= bound
    # every other pair: against the restatement within bound + the restatement's own error
    ref = c["rest"]
    dead = ref == 0.0
    assert np.array_equal(got == 0.0, dead)
    rel = np.abs(got[~dead] - ref[~dead]) / ref[~dead]
    print("%s: all %d pairs against the restatement: largest relative difference %.3e (allowed %.3e)"
          % (kind, ref[0].size, rel.max(), bound + e_rest))
    assert rel.max() <= bound + e_rest
    assert np.all(got[:, :, ~np.isfinite(c["fin"])] == 0.0) and np.all(got[:, :, c["fin"] == 0.0] == 0.0)
    assert np.all(got[1][[0, 1, 16]] == 0.0)           # T = 0: M = I, no noise pattern


# ---- 2. sums and probabilities --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 3, 17])
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_sums_and_probabilities(cases, kind, n_q):
    engine = _engine()
    c = cases[kind]
    quartets = QLISTS[n_q]
    plan, rates, nres = _plan(engine, c)
    try:
        rows = plan.quartet_tables(rates, nres, quartets)
        sites = plan.quartet_sites(rates, nres, quartets)
    finally:
        plan.close()
    off = c["off"]
    assert rows.shape == (len(off) - 1, n_q, 8)
    worst_sum, worst_p, worst_sp = 0.0, 0.0, 0.0
    for l in range(len(off) - 1):
        sl = slice(int(off[l]), int(off[l + 1]))
        n_l = sl.stop - sl.start
        for q in range(n_q):
            want = qr.locus_sums(sites[0, q, sl], sites[1, q, sl])
            got = rows[l, q, :5]
            assert np.all(got[want == 0.0] == 0.0)
            live = want > 0
            if live.any():
                ratio = np.max(np.abs(got[live] - want[live]) / want[live]) / ((n_l + 64) * U)
                worst_sum = max(worst_sum, ratio)
            p = qr.probabilities(got)
            worst_p = max(worst_p, max(abs(a - b) for a, b in zip(rows[l, q, 5:], p)))
            for h, k, rho in qr.probability_arguments(got):      # the restatement's B against scipy on the same arguments
                worst_sp = max(worst_sp, abs(qr.bvn_upper(h, k, rho) - qr.bvn_reference(h, k, rho)))
            assert 0.0 <= rows[l, q, 5:].min() and rows[l, q, 5:].max() <= 1.0
    print("%s n_q=%d: sums against fsum of the GPU's per-site values, error / ((n_l + 64) 2^-52) = %.3f; probabilities against "
          "the restatement %.2e; the restatement's B against scipy %.2e (both allowed 1e-13)" % (kind, n_q, worst_sum, worst_p, worst_sp))
    assert worst_sum <= 1.0
    assert worst_sp <= 1e-13
    assert worst_p <= 1e-13
    empty = [l for l in range(len(off) - 1) if off[l + 1] == off[l]]
    if kind == "gtr":
        empty.append(5)                                            # culled entirely
    for l in empty:
        assert np.array_equal(rows[l], [[0, 0, 0, 0, 0, 0, 0, 1]] * n_q)


# ---- 3. bit identity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_rows_do_not_depend_on_neighbours_or_on_the_quartet_list(cases, kind):
    engine = _engine()
    c = cases[kind]
    plan, rates, nres = _plan(engine, c)
    try:
        full = plan.quartet_tables(rates, nres, Q17)
        full_sites = plan.quartet_sites(rates, nres, Q17)
        # one quartet alone against the same quartet inside the list of 17: first of a tile, matrices reused, last
        for q in (0, 3, 4, 5, 12, 14, 16):
            one = plan.quartet_tables(rates, nres, [Q17[q]])
            assert np.array_equal(one[:, 0], full[:, q]), q
            assert np.array_equal(plan.quartet_sites(rates, nres, [Q17[q]])[:, 0], full_sites[:, q]), q
        assert np.array_equal(full[:, 3], full[:, 12])             # the same quartet twice in the list
        # 130 distinct quartets are three launches of 64: every row and site against the two shorter calls that cut the list
        # at the first launch boundary, and 60..70 against a call of those eleven (other positions of a batch)
        big = plan.quartet_tables(rates, nres, Q256[:130])
        big_sites = plan.quartet_sites(rates, nres, Q256[:130])
        for a, b in ((0, 64), (64, 130), (60, 71)):
            assert np.array_equal(plan.quartet_tables(rates, nres, Q256[a:b]), big[:, a:b]), (a, b)
            assert np.array_equal(plan.quartet_sites(rates, nres, Q256[a:b]), big_sites[:, a:b]), (a, b)
        most = plan.quartet_tables(rates, nres, Q256)              # the longest list: four full launches
        assert most.shape == (len(c["sizes"]), 256, 8)
        assert np.array_equal(most[:, :130], big)
        assert np.array_equal(most[:, 192:], plan.quartet_tables(rates, nres, Q256[192:]))
    finally:
        plan.close()
    L = len(c["sizes"])
    for ids in ([L - 1], [L - 2], [3], [1, L - 1, 0] if kind == "f81" else [1, L - 1, 4]):
        part, r, n = _plan(engine, c, ids)
        try:
            rows = part.quartet_tables(r, n, Q17)
        finally:
            part.close()
        assert np.array_equal(rows, full[ids]), ids
    print("%s: rows bit-identical alone / among neighbours / in a list of 1, 17, 130 or 256" % kind)


def test_host_and_device_calls_agree(cases):
    import torch
    engine = _engine()
    c = cases["gtr"]
    plan, rates, nres = _plan(engine, c)
    try:
        host = plan.quartet_tables(rates, nres, Q17)
        host_sites = plan.quartet_sites(rates, nres, Q17)
        d_r, d_n = torch.from_numpy(rates).cuda(), torch.from_numpy(nres).cuda()
        d_rows = torch.zeros((len(LOCI), 17, 8), dtype=torch.float64, device="cuda")
        d_sites = torch.zeros((2, 17, len(rates)), dtype=torch.float64, device="cuda")
        ws = torch.empty(plan.quartet_workspace_bytes(Q17), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.quartet_tables_dev(d_r, d_n, Q17, d_rows, ws)
        plan.quartet_sites_dev(d_r, d_n, Q17, d_sites)
        torch.cuda.synchronize()
        assert np.array_equal(d_rows.cpu().numpy(), host) and np.array_equal(d_sites.cpu().numpy(), host_sites)
        with pytest.raises(engine.TphipError, match="libtphip error 4: workspace smaller"):
            plan.quartet_tables_dev(d_r, d_n, Q17, d_rows, ws[:64])
    finally:
        plan.close()


def test_bad_quartets_are_refused(cases):
    engine = _engine()
    c = cases["f81"]
    plan, rates, nres = _plan(engine, c)
    try:
        for bad, message in (([(1.0, 0.0)], "t_o must be finite and > 0"), ([(-1.0, 1.0)], "T must be finite and >= 0"),
                             ([(1.0, float("nan"))], "t_o must be finite"), ([(1.0, 1.0)] * 257, "n_q must be in 1..256")):
            with pytest.raises(engine.TphipError, match=message):
                plan.quartet_tables(rates, nres, bad)
        assert plan.quartet_tables(rates, nres, [(1.0, 1.0)] * 256).shape == (len(F81_LOCI), 256, 8)   # more than one batch
    finally:
        plan.close()


# ---- 4. the command line --------------------------------------------------------------------------------------------
def test_cli_quartets_on_the_bundled_locus(tmp_path, golden_dir):
    import shutil
    engine = _engine()
    from tapir_amd import cli, compute, newick, nexus
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    tree = os.path.join(golden_dir, "Euteleost.tree")
    name = "phylogenetic-informativeness-quartets.sqlite"
    dirs = []
    for d, extra in (("plain", []), ("quart", ["--quartets", "20:5,50:10,100:2"])):
        out = tmp_path / d
        out.mkdir()
        dirs.append(cli.main([str(aln), tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                              "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"] + extra))
    plain, quart = dirs
    assert sorted(set(os.listdir(quart)) - set(os.listdir(plain))) == [name]
    for f in os.listdir(plain):                                    # main outputs: byte for byte
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(quart, f), "rb").read(), f
    con = sqlite3.connect(os.path.join(quart, name))
    got = np.array(con.execute("select tip, internode, signal, noise, p_correct, p_incorrect, p_polytomy from quartet "
                               "where id = 1 order by rowid").fetchall())
    labels = [r[0] for r in con.execute("select quartet from quartet order by rowid")]
    con.close()
    assert labels == ["20:5", "50:10", "100:2"] and np.array_equal(got[:, :2], [[20, 5], [50, 10], [100, 2]])
    # the final rates of the run: the written corrected_rates, NaN where fewer than --threshold (3) cells are A/C/G/T; the
    # model is the one the .rates header carries
    doc = json.load(open(os.path.join(quart, "chr1_918.nex.rates")))["sites"]
    r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
    _, st = nexus.read_states(os.path.join(str(aln), "chr1_918.nex"))
    r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
    pi = [doc["freqs"][k] for k in "ACGT"]
    exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
    quartets = [(20.0, 5.0), (50.0, 10.0), (100.0, 2.0)]
    want = qr.rows("gtr", pi, exch, r, quartets)
    T = int(compute.correct_tree(newick.read_tree(tree))[0])
    plan = engine.Plan(3, PARENT, BLEN, LEAF, [0, r.size], [pi], [exch], T, [], [], correction=1.0, threshold=0, round_decimals=-1)
    try:
        rows = plan.quartet_tables(r, None, quartets)[0]
    finally:
        plan.close()
    assert np.array_equal(got[:, 2:], rows[:, [0, 1, 5, 6, 7]])     # the file holds what the engine computes on these rates
    # sums: per-site values within 64 * 2^-52 of the twin for the kernel and 128 * 2^-52 for the restatement (the floors of
    # their bounds), non-negative terms, n sites: (64 + 128 + n + 64) 2^-52 relative
    tol = (256 + r.size) * U
    rel = np.abs(rows[:, :5] - want[:, :5]) / want[:, :5]
    # probabilities: the restatement on the GPU's sums, 1e-13
    dp = max(max(abs(a - b) for a, b in zip(rows[q, 5:], qr.probabilities(rows[q, :5]))) for q in range(3))
    print("chr1_918 (%d sites, T = %d): signal %s noise %s; sums against the restatement %.2e relative (allowed %.2e), "
          "probabilities %.2e; p_correct %s p_incorrect %s" % (r.size, T, rows[:, 0], rows[:, 1], rel.max(), tol, dp, rows[:, 5], rows[:, 6]))
    assert rel.max() <= tol and dp <= 1e-13
    assert np.all(np.abs(rows[:, 5:].sum(axis=1) - 1.0) <= 4 * U)

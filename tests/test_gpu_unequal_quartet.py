"""Quartet signal and noise with unequal tips on the GPU (tphip_unequal_quartet_sites, tphip_unequal_quartet_tables,
--unequal-quartets / --tree-quartets) against tests/unequal_quartet_reference.py.  Run with -m gpu on the MI355X box.  Every
test prints its figures before it asserts.

Bounds (stated by the definition, none tuned to the kernels):
  per-site y, x1, x2   relative, against the 40-digit twin: 16 x the largest relative error the fp64 numpy restatement shows
                  against the twin on the same (site, quartet) pairs, at least 64 * 2^-52 (the factor: the device's Jacobi
                  eigen-system against LAPACK's, another expm1).  A reference of exactly 0 must come back as 0.  The twin is
                  taken on the sample of test_gpu_quartet.py: the first and last columns of every locus, both sides of every
                  1024-column chunk boundary, the zero, culled and saturated rates, the extremes and a few others.  Every
                  other pair is held against the restatement within bound + (the restatement's own error).
  equal tips      y against quartet_sites' y, x1 and x2 against its x: twice that bound (both are within it of the twin)
  sums            against math.fsum of the GPU's own per-site values: (n_l + 64) 2^-52 relative (non-negative terms)
  probabilities   against the restatement fed the GPU's sums: 1e-13 absolute
  bit identity    of a locus' row: alone against among its neighbours, one quartet alone against inside the list, the
                  repeated quartet twice, 130 quartets (three launches) against single calls, 130 and 256 distinct quartets
                  against shorter calls cut at a launch boundary and across it, host against _dev
"""
import json
import os
import sqlite3

import numpy as np
import pytest

import hp_reference as hp
import unequal_quartet_reference as ur

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
# a three-taxon tree: this stage never looks at it
PARENT, BLEN, LEAF = [3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1]
LOCI = [0, 1, 3, 63, 64, 65, 1023, 1024, 1025, 2049]
F81_LOCI = [5, 64, 130, 1030]
CORRECTION = 1.25
# all tips 0; equal tips; Ta != Tb only; the long-branch case and its mirror; one tip 0; t_o from 1e-3 to 50; tips of 300;
# a repeated quartet (1 and 11)
Q14 = [(0, 0, 0, 0, 1e-3), (20, 20, 20, 20, 5), (50, 50, 50, 50, 10), (20, 35, 27, 27, 5), (100, 5, 100, 5, 2), (100, 5, 5, 100, 2),
       (0, 12, 7.5, 30, 3), (30, 30, 45, 70, 10), (1, 2, 3, 4, 50), (300, 300, 300, 300, 0.5), (300, 1e-2, 64, 3, 1e-3),
       (20, 20, 20, 20, 5), (37, 37, 93, 107, 56), (7.5, 7.5, 7.5, 7.5, 2)]
Q14 = [tuple(float(v) for v in q) for q in Q14]
EQUAL = [1, 2, 9, 13]
QLISTS = {1: [Q14[4]], 3: Q14[3:6], 14: Q14}
TWIN_Q = [0, 1, 4, 6, 9, 10]        # quartets of the twin's sample (indices into Q14)


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


def _relative(got, ref):
    import mpmath as mp
    with mp.workdps(40):
        return float(abs(mp.mpf(float(got)) - ref) / ref)


def _case(kind):
    if kind == "gtr":
        rng, off, rates, nres = _inputs(LOCI, 20261019)
        L = len(LOCI)
        pi = rng.dirichlet([6.0] * 4, L)
        exch = rng.uniform(0.3, 4.0, (L, 6))
        nres[off[5]:off[6]] = 0                                    # the 65-column locus culled entirely
        sat = int(off[7]) + 100
        rates[sat] = 1e4 * CORRECTION                              # one saturated rate, in the 1024-column locus
        extra = [sat]
    else:
        rng, off, rates, nres = _inputs(F81_LOCI, 20261020)
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
    rest = np.zeros((3, len(Q14), int(off[-1])))
    for l in range(L):
        sl = slice(int(off[l]), int(off[l + 1]))
        for q, row in enumerate(Q14):
            rest[:, q, sl] = ur.site_values(kind, pi[l], ones if exch is None else exch[l], fin[sl], row[:4], row[4])
    twin = {}
    e_rest = 0.0
    for c in cols.tolist():
        l = int(locus_of[c])
        for q in TWIN_Q:
            t = ur.twin_values(pi[l], ones if exch is None else exch[l], [fin[c]], Q14[q][:4], Q14[q][4])
            twin[(c, q)] = tuple(v[0] for v in t)
            for which in range(3):
                if twin[(c, q)][which] != 0:
                    e_rest = max(e_rest, _relative(rest[which, q, c], twin[(c, q)][which]))
    # the restatement's own error on the sample sets the bound; the GPU's output never does
    return dict(kind=kind, sizes=LOCI if kind == "gtr" else F81_LOCI, off=off, rates=rates, nres=nres, fin=fin, pi=pi, exch=exch,
                cols=cols, rest=rest, twin=twin, locus_of=locus_of, e_rest=e_rest, bound=max(16 * e_rest, 64 * U))


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


# ---- 1. per-site values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_sites_against_the_40_digit_twin(cases, kind):
    engine = _engine()
    c = cases[kind]
    plan, rates, nres = _plan(engine, c)
    try:
        got = plan.unequal_quartet_sites(rates, nres, Q14)
    finally:
        plan.close()
    assert got.shape == (3, 14, len(rates))
    e_gpu, zeros_ok = 0.0, True
    for (col, q), ref in c["twin"].items():
        for which in range(3):
            if ref[which] == 0:
                zeros_ok = zeros_ok and got[which, q, col] == 0.0 and c["rest"][which, q, col] == 0.0
            else:
                e_gpu = max(e_gpu, _relative(got[which, q, col], ref[which]))
    e_rest, bound = c["e_rest"], c["bound"]
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
    assert np.all(got[1:, 0] == 0.0)                   # all tips 0: no noise pattern
    assert np.array_equal(got[1, [1, 2, 7, 9, 11, 12, 13]], got[2, [1, 2, 7, 9, 11, 12, 13]])   # Ta = Tb: x1 = x2, bit for bit


# ---- 2. equal tips against the equal-tip kernel ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_equal_tips_against_quartet_sites(cases, kind):
    engine = _engine()
    c = cases[kind]
    plan, rates, nres = _plan(engine, c)
    try:
        got = plan.unequal_quartet_sites(rates, nres, [Q14[q] for q in EQUAL])
        old = plan.quartet_sites(rates, nres, [(Q14[q][0], Q14[q][4]) for q in EQUAL])
    finally:
        plan.close()
    bound = c["bound"]
    live = old[0] > 0
    assert np.array_equal(got[0] > 0, live) and np.array_equal(got[1] > 0, old[1] > 0) and np.array_equal(got[2] > 0, old[1] > 0)
    dy = np.max(np.abs(got[0][live] / old[0][live] - 1))
    xl = old[1] > 0
    dx = max(np.max(np.abs(got[1][xl] / old[1][xl] - 1)), np.max(np.abs(got[2][xl] / old[1][xl] - 1)))
    # both kernels against the twin on the sample's equal-tip quartets (1 and 9 of Q14)
    e_old = 0.0
    for (col, q), ref in c["twin"].items():
        if q in EQUAL:
            k = EQUAL.index(q)
            for which, val in ((0, old[0, k, col]), (1, old[1, k, col])):
                if ref[which] != 0:
                    e_old = max(e_old, _relative(val, ref[which]))
    print("%s: equal tips, unequal kernel against quartet_sites: y %.3e, x %.3e (allowed %.3e); quartet_sites against the twin "
          "%.3e (allowed %.3e)" % (kind, dy, dx, 2 * bound, e_old, bound))
    assert e_old <= bound
    assert dy <= 2 * bound and dx <= 2 * bound


# ---- 3. sums and probabilities --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 3, 14])
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_sums_and_probabilities(cases, kind, n_q):
    engine = _engine()
    c = cases[kind]
    quartets = QLISTS[n_q]
    plan, rates, nres = _plan(engine, c)
    try:
        rows = plan.unequal_quartet_tables(rates, nres, quartets)
        sites = plan.unequal_quartet_sites(rates, nres, quartets)
    finally:
        plan.close()
    off = c["off"]
    assert rows.shape == (len(off) - 1, n_q, 13)
    worst_sum, worst_p = 0.0, 0.0
    for l in range(len(off) - 1):
        sl = slice(int(off[l]), int(off[l + 1]))
        n_l = sl.stop - sl.start
        for q in range(n_q):
            want = ur.locus_sums(sites[0, q, sl], sites[1, q, sl], sites[2, q, sl])
            got = rows[l, q, :9]
            assert np.all(got[want == 0.0] == 0.0)
            live = want > 0
            if live.any():
                worst_sum = max(worst_sum, np.max(np.abs(got[live] - want[live]) / want[live]) / ((n_l + 64) * U))
            p = ur.probabilities(got)
            worst_p = max(worst_p, max(abs(a - b) for a, b in zip(rows[l, q, 9:], p)))
            assert 0.0 <= rows[l, q, 9:].min() and rows[l, q, 9:].max() <= 1.0
    print("%s n_q=%d: sums against fsum of the GPU's per-site values, error / ((n_l + 64) 2^-52) = %.3f; probabilities against "
          "the restatement %.2e (allowed 1e-13)" % (kind, n_q, worst_sum, worst_p))
    assert worst_sum <= 1.0
    assert worst_p <= 1e-13
    empty = [l for l in range(len(off) - 1) if off[l + 1] == off[l]]
    if kind == "gtr":
        empty.append(5)                                            # culled entirely
    for l in empty:
        assert np.array_equal(rows[l], [[0] * 12 + [1]] * n_q)


# ---- 4. bit identity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_rows_do_not_depend_on_neighbours_or_on_the_quartet_list(cases, kind):
    engine = _engine()
    c = cases[kind]
    plan, rates, nres = _plan(engine, c)
    rng = np.random.default_rng(5)
    q130 = [Q14[k % 14] if k < 28 else tuple(rng.uniform(0.0, 120.0, 4)) + (float(rng.uniform(0.01, 30.0)),) for k in range(130)]
    try:
        full = plan.unequal_quartet_tables(rates, nres, Q14)
        full_sites = plan.unequal_quartet_sites(rates, nres, Q14)
        for q in (0, 1, 4, 5, 10, 13):                             # one quartet alone against the same quartet inside the list
            one = plan.unequal_quartet_tables(rates, nres, [Q14[q]])
            assert np.array_equal(one[:, 0], full[:, q]), q
            assert np.array_equal(plan.unequal_quartet_sites(rates, nres, [Q14[q]])[:, 0], full_sites[:, q]), q
        assert np.array_equal(full[:, 1], full[:, 11]) and np.array_equal(full_sites[:, 1], full_sites[:, 11])   # the repeated quartet
        big = plan.unequal_quartet_tables(rates, nres, q130)       # three launches
        big_sites = plan.unequal_quartet_sites(rates, nres, q130)
        assert np.array_equal(big[:, :14], full) and np.array_equal(big_sites[:, :14], full_sites)
        for q in (14, 63, 64, 65, 127, 128, 129):                  # both sides of the launches' boundaries, and the last
            assert np.array_equal(plan.unequal_quartet_tables(rates, nres, [q130[q]])[:, 0], big[:, q]), q
            assert np.array_equal(plan.unequal_quartet_sites(rates, nres, [q130[q]])[:, 0], big_sites[:, q]), q
        # 130 distinct quartets: every row and site against the two shorter calls that cut the list at the first launch
        # boundary, and 60..70 against a call of those eleven (other positions of a batch)
        d256 = [tuple(rng.uniform(0.0, 120.0, 4)) + (float(rng.uniform(0.01, 30.0)),) for k in range(256)]
        assert len(set(d256)) == 256
        big = plan.unequal_quartet_tables(rates, nres, d256[:130])
        big_sites = plan.unequal_quartet_sites(rates, nres, d256[:130])
        for a, b in ((0, 64), (64, 130), (60, 71)):
            assert np.array_equal(plan.unequal_quartet_tables(rates, nres, d256[a:b]), big[:, a:b]), (a, b)
            assert np.array_equal(plan.unequal_quartet_sites(rates, nres, d256[a:b]), big_sites[:, a:b]), (a, b)
        most = plan.unequal_quartet_tables(rates, nres, d256)      # the longest list: four full launches
        assert most.shape == (len(c["sizes"]), 256, 13)
        assert np.array_equal(most[:, :130], big)
        assert np.array_equal(most[:, 192:], plan.unequal_quartet_tables(rates, nres, d256[192:]))
    finally:
        plan.close()
    L = len(c["sizes"])
    for ids in ([L - 1], [L - 2], [3], [1, L - 1, 0] if kind == "f81" else [1, L - 1, 4]):
        part, r, n = _plan(engine, c, ids)
        try:
            rows = part.unequal_quartet_tables(r, n, Q14)
        finally:
            part.close()
        assert np.array_equal(rows, full[ids]), ids
    print("%s: rows bit-identical alone / among neighbours / in a list of 1, 14 or 130" % kind)


def test_host_and_device_calls_agree(cases):
    import torch
    engine = _engine()
    c = cases["gtr"]
    plan, rates, nres = _plan(engine, c)
    try:
        host = plan.unequal_quartet_tables(rates, nres, Q14)
        host_sites = plan.unequal_quartet_sites(rates, nres, Q14)
        d_r, d_n = torch.from_numpy(rates).cuda(), torch.from_numpy(nres).cuda()
        d_rows = torch.zeros((len(LOCI), 14, 13), dtype=torch.float64, device="cuda")
        d_sites = torch.zeros((3, 14, len(rates)), dtype=torch.float64, device="cuda")
        ws = torch.empty(plan.unequal_quartet_workspace_bytes(Q14), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.unequal_quartet_tables_dev(d_r, d_n, Q14, d_rows, ws)
        plan.unequal_quartet_sites_dev(d_r, d_n, Q14, d_sites)
        torch.cuda.synchronize()
        assert np.array_equal(d_rows.cpu().numpy(), host) and np.array_equal(d_sites.cpu().numpy(), host_sites)
        with pytest.raises(engine.TphipError, match="libtphip error 1: ws_bytes: workspace smaller"):
            plan.unequal_quartet_tables_dev(d_r, d_n, Q14, d_rows, ws[:64])
    finally:
        plan.close()


# ---- 5. bad options -------------------------------------------------------------------------------------------------
def test_bad_quartets_are_refused(cases):
    engine = _engine()
    c = cases["f81"]
    plan, rates, nres = _plan(engine, c)
    ok = (1.0, 2.0, 3.0, 4.0, 1.0)
    try:
        for bad, message in (([(1.0, 2.0, 3.0, 4.0, 0.0)], r"t_o \(internode\) must be finite and > 0"),
                             ([(1.0, 2.0, 3.0, 4.0, float("inf"))], r"t_o \(internode\) must be finite"),
                             ([(-1.0, 2.0, 3.0, 4.0, 1.0)], r"Ta \(tips\) must be finite and >= 0"),
                             ([ok, (1.0, 2.0, float("nan"), 4.0, 1.0)], r"quartet 1: the tip length Tc \(tips\) must be finite"),
                             ([(1.0, 2.0, 3.0, float("inf"), 1.0)], r"Td \(tips\) must be finite"),
                             ([ok] * 257, "n_q must be in 1..256")):
            with pytest.raises(engine.TphipError, match=message):
                plan.unequal_quartet_tables(rates, nres, bad)
            with pytest.raises(engine.TphipError, match=message):
                plan.unequal_quartet_sites(rates, nres, bad)
        assert plan.unequal_quartet_tables(rates, nres, [ok] * 256).shape == (len(F81_LOCI), 256, 13)   # four launches
    finally:
        plan.close()


# ---- 6. the command line --------------------------------------------------------------------------------------------
def test_cli_tree_quartets_on_the_bundled_locus(tmp_path, golden_dir):
    import shutil
    engine = _engine()
    from tapir_amd import cli, compute, newick, nexus
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    tree = os.path.join(golden_dir, "Euteleost.tree")
    name = "phylogenetic-informativeness-unequal-quartets.sqlite"
    dirs = []
    for d, extra in (("plain", []), ("quart", ["--tree-quartets", "--unequal-quartets", "100/5/100/5:2"])):
        out = tmp_path / d
        out.mkdir()
        dirs.append(cli.main([str(aln), tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                              "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"] + extra))
    plain, quart = dirs
    assert sorted(set(os.listdir(quart)) - set(os.listdir(plain))) == [name]
    for f in os.listdir(plain):                                    # every other output: byte for byte
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(quart, f), "rb").read(), f
    of_tree = compute.tree_quartets(newick.read_tree(tree))
    con = sqlite3.connect(os.path.join(quart, name))
    got = np.array(con.execute("select tip_a, tip_b, tip_c, tip_d, internode, signal, noise_ac, noise_ad, p_correct, p_ac, p_ad, "
                               "p_polytomy from quartet where id = 1 order by rowid").fetchall())
    labels = [r[0] for r in con.execute("select quartet from quartet order by rowid")]
    clades = con.execute("select quartet, ntaxa, taxa from clade order by rowid").fetchall()
    con.close()
    quartets = [(100.0, 5.0, 100.0, 5.0, 2.0)] + [q[2:] for q in of_tree]
    assert len(of_tree) == len(newick.leaves(newick.read_tree(tree))) - 3
    assert labels == ["100/5/100/5:2"] + [q[0] for q in of_tree] and np.array_equal(got[:, :5], quartets)   # typed rows first
    assert clades == [(q[0], len(q[1]), ",".join(q[1])) for q in of_tree]
    # a direct call on the run's final rates: the written corrected_rates, NaN where fewer than --threshold (3) cells are
    # A/C/G/T, under the model the .rates header carries
    doc = json.load(open(os.path.join(quart, "chr1_918.nex.rates")))["sites"]
    r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
    _, st = nexus.read_states(os.path.join(str(aln), "chr1_918.nex"))
    r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
    pi = [doc["freqs"][k] for k in "ACGT"]
    exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
    T = int(compute.correct_tree(newick.read_tree(tree))[0])
    plan = engine.Plan(3, PARENT, BLEN, LEAF, [0, r.size], [pi], [exch], T, [], [], correction=1.0, threshold=0, round_decimals=-1)
    try:
        rows = plan.unequal_quartet_tables(r, None, quartets)[0]
    finally:
        plan.close()
    assert np.array_equal(got[:, 5:], rows[:, [0, 1, 2, 9, 10, 11, 12]])    # the file holds what the engine computes on these rates
    want = ur.rows("gtr", pi, exch, r, quartets)
    # sums: per-site values within 64 * 2^-52 of the twin for the kernel and 128 * 2^-52 for the restatement (the floors of
    # their bounds), non-negative terms, n sites: (64 + 128 + n + 64) 2^-52 relative
    tol = (256 + r.size) * U
    rel = np.abs(rows[:, :9] - want[:, :9]) / want[:, :9]
    dp = max(max(abs(a - b) for a, b in zip(rows[q, 9:], ur.probabilities(rows[q, :9]))) for q in range(len(quartets)))
    print("chr1_918 (%d sites, T = %d): quartets %s; signal %s noise_ac %s noise_ad %s; sums against the restatement %.2e relative "
          "(allowed %.2e), probabilities %.2e; p_correct %s p_ac %s p_ad %s"
          % (r.size, T, labels, rows[:, 0], rows[:, 1], rows[:, 2], rel.max(), tol, dp, rows[:, 9], rows[:, 10], rows[:, 11]))
    assert rel.max() <= tol and dp <= 1e-13

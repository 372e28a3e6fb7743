"""Site bootstrap of the PI rows on the GPU (tphip_bootstrap_counts, tphip_pi_resample, tphip_pi_bootstrap, --bootstrap)
against tests/bootstrap_reference.py.  Run with -m gpu on the MI355X box.  Every test prints its figures before it asserts.

Bounds (stated by the definition, none tuned to the kernels):
  counts          exact
  net entries     |got - ref| <= ref (n_l + 64 + 4 r_max t) 2^-52 + 1e-290: the terms are non-negative, so any summation order
                  loses at most n_l units; 64 covers the 16-step recurrence and the exponential, 4 r t the rounding of the
                  exponent's argument, the absolute term subnormal products.  A reference of exactly 0 must come back as 0.
  integrals       1e-9 relative against the per-site scipy values (the project's table contract); the all-ones replicate
                  agrees with tphip_pi_tables' net and integral columns to (n_l + 64) 2^-52 relative (same per-site
                  functions, another summation order)
  summary         against numpy on the returned rows: mean (B + 2) 2^-52 relative, sd 8 B 2^-52 max_b |X_b| absolute
                  (two-pass, deviations cancel), quantiles 4 2^-52 relative
  bundled locus   |mean - point| <= 4 sd / sqrt(B) and lo <= point <= hi at every t >= 1 (the bootstrap mean is unbiased for
                  the point estimate; with the CPU reference alone the largest ratio at seed 1 is 0.96 of the allowance)
"""
import json
import os
import sqlite3

import numpy as np
import pytest

import bootstrap_reference as bsr
import hp_reference as hp

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a three-taxon tree: the PI stage never looks at it
PARENT, BLEN, LEAF = [3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1]
LOCI = [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025]
T_MAT = 37
IV_MAT = [[0, 10], [10, 20], [3, 37]]
NREPS = [1, 15, 16, 17, 65]


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _plan(engine, sizes, T, intervals, integ_mode=0, **kw):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    L = len(sizes)
    kw.setdefault("correction", 1.0)
    kw.setdefault("threshold", 3)
    kw.setdefault("round_decimals", -1)
    return engine.Plan(3, PARENT, BLEN, LEAF, off, np.full((L, 4), 0.25), np.ones((L, 6)), T, [], intervals,
                       integ_mode=integ_mode, **kw), off


# ---- 1. counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 226, 1025])
def test_counts_equal_the_reference(n):
    engine = _engine()
    for seed, locus_id, rep0, nrep in ((1, 0, 0, 4), (2 ** 40 + 7, 2 ** 33 + 1, 5, 3), (3, 17, 4095, 1)):
        got = engine.bootstrap_counts(n, rep0=rep0, nrep=nrep, seed=seed, locus_id=locus_id)
        ref = bsr.counts(seed, locus_id, n, rep0, nrep)
        print("n=%d seed=%d id=%d rep0=%d: sums %s, differing cells %d" % (n, seed, locus_id, rep0, got.sum(axis=1).tolist(),
                                                                         int((got != ref).sum())))
        assert got.dtype == np.uint16 and np.array_equal(got, ref)
        assert np.all(got.sum(axis=1) == n)


# ---- 2. the matrix core on caller-supplied counts ----------------------------------------------------------------
def _matrix_inputs():
    rng = np.random.default_rng(20261017)
    n = int(np.sum(LOCI))
    rates = rng.uniform(0.001, 0.5, n)
    nres = np.full(n, 5, np.int32)
    off = np.concatenate([[0], np.cumsum(LOCI)])
    for l, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if b - a >= 3:
            rates[a] = 0.0            # a constant column
            nres[a + 1] = 2           # a culled column
            rates[a + 2] = 1e-6
        if b - a >= 63:
            rates[a + 40] = 0.0
            nres[a + 41] = 0
    rates[off[9] + 100] = 1e4         # one saturated rate, in the 1024-column locus
    cnt = rng.integers(0, 4, (max(NREPS), n)).astype(np.uint16)
    cnt[0] = 1                        # the all-ones replicate: the point estimate
    cnt[1] = 0                        # one-hot rows: a single column per locus
    cnt[2] = 0
    for l, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if b > a:
            cnt[1, a + (7 * l) % (b - a)] = 1
            cnt[2, b - 1] = 1
    cnt[3, rng.integers(0, n, 40)] = 65535
    cnt[4] = 65535
    return rates, nres, cnt, off


@pytest.fixture(scope="module")
def matrix_case():
    """Inputs and the CPU reference of the matrix tests, computed once: per-site values (mpmath / scipy) and the exact rows."""
    rates, nres, cnt, off = _matrix_inputs()
    fin = hp.finalize_rates(rates, -1, 1.0, nres, 3)
    net = bsr.site_net(fin, T_MAT)
    integ = {0: bsr.site_integrals(fin, IV_MAT, exact=False), 1: bsr.site_integrals(fin, IV_MAT, exact=True)}
    return dict(rates=rates, nres=nres, cnt=cnt, off=off, fin=fin, net=net, integ=integ)


@pytest.mark.parametrize("integ_mode", [0, 1])
@pytest.mark.parametrize("nrep", NREPS)
def test_matrix_core_against_extended_precision(matrix_case, integ_mode, nrep):
    engine = _engine()
    c = matrix_case
    plan, off = _plan(engine, LOCI, T_MAT, IV_MAT, integ_mode)
    try:
        assert plan.bootstrap_width == T_MAT + len(IV_MAT)
        cnt = c["cnt"][:nrep]
        rows = plan.pi_resample(c["rates"], c["nres"], cnt)
        tables = plan.pi_tables(c["rates"], c["nres"])
    finally:
        plan.close()
    assert rows.shape == (len(LOCI), nrep, T_MAT + len(IV_MAT))
    t = np.arange(T_MAT)
    worst_net = worst_int = worst_tab = 0.0
    for l, n_l in enumerate(LOCI):
        a, b = off[l], off[l + 1]
        fin = c["fin"][a:b]
        ok = np.isfinite(fin)
        r_max = fin[ok].max() if ok.any() else 0.0
        ref = np.asarray(bsr.rows_from_counts(cnt[:, a:b], c["net"][a:b]), np.float64)
        got = rows[l, :, :T_MAT]
        bound = ref * (n_l + 64 + 4 * r_max * t)[None, :] * U + 1e-290
        err = np.abs(got - ref)
        worst_net = max(worst_net, float(np.max(err / bound, initial=0.0)))
        assert np.all(err <= bound), (l, n_l, float(np.max(err / bound)))
        assert np.all(got[ref == 0.0] == 0.0)
        refi = np.asarray(bsr.rows_from_counts(cnt[:, a:b], c["integ"][integ_mode][a:b]), np.float64)
        goti = rows[l, :, T_MAT:]
        erri = np.abs(goti - refi)
        worst_int = max(worst_int, float(np.max(erri / np.maximum(refi, 1e-300), initial=0.0)))
        assert np.all(erri <= 1e-9 * refi), (l, n_l)
        # replicate 0 has every count 1: the row of tphip_pi_tables, summed in another order
        point = np.concatenate([tables[l, :T_MAT], tables[l, T_MAT:T_MAT + len(IV_MAT)]])
        errp = np.abs(rows[l, 0] - point)
        worst_tab = max(worst_tab, float(np.max(errp / np.maximum(point * (n_l + 64) * U, 1e-300), initial=0.0)))
        assert np.all(errp <= point * (n_l + 64) * U), (l, n_l)
    print("integ_mode=%d nrep=%d: worst error / bound: net %.3f, integrals (relative) %.3g, all-ones vs pi_tables %.3f"
          % (integ_mode, nrep, worst_net, worst_int, worst_tab))


# ---- 3. bit identity ---------------------------------------------------------------------------------------------
def _rates_for(sizes, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0005, 0.3, int(np.sum(sizes)))
    r[rng.random(r.size) < 0.3] = 0.0
    return r


def test_rows_do_not_depend_on_neighbours_replicate_count_or_run():
    engine = _engine()
    T, iv = 21, [[0, 8], [4, 21]]
    x = _rates_for([300], 5)
    left, right = _rates_for([77], 6), _rates_for([1300], 7)
    plan, _ = _plan(engine, [300], T, iv)
    try:
        s_alone, r_alone = plan.pi_bootstrap(x, replicates=32, seed=11, locus_ids=[7], return_rows=True)
        s_again, r_again = plan.pi_bootstrap(x, replicates=32, seed=11, locus_ids=[7], return_rows=True)
        _, r_small = plan.pi_bootstrap(x, replicates=8, seed=11, locus_ids=[7], return_rows=True)
        _, r_other_id = plan.pi_bootstrap(x, replicates=8, seed=11, locus_ids=[8], return_rows=True)
        _, r_other_seed = plan.pi_bootstrap(x, replicates=8, seed=2 ** 40 + 11, locus_ids=[7], return_rows=True)
    finally:
        plan.close()
    plan, _ = _plan(engine, [77, 300, 1300], T, iv)
    try:
        s_mid, r_mid = plan.pi_bootstrap(np.concatenate([left, x, right]), replicates=32, seed=11, locus_ids=[3, 7, 2 ** 33],
                                         return_rows=True)
    finally:
        plan.close()
    print("rows differing: alone/again %d, alone/between neighbours %d, B=8/B=32 %d" % (
        int((r_alone != r_again).sum()), int((r_alone[0] != r_mid[1]).sum()), int((r_small[0] != r_alone[0, :8]).sum())))
    assert np.array_equal(r_alone, r_again) and np.array_equal(s_alone, s_again)
    assert np.array_equal(r_alone[0], r_mid[1]) and np.array_equal(s_alone[0], s_mid[1])
    assert np.array_equal(r_small[0], r_alone[0, :8])
    assert not np.array_equal(r_other_id, r_small) and not np.array_equal(r_other_seed, r_small)
    assert r_alone.min() >= 0.0 and r_alone.max() > 0.0


def test_minimal_and_preferred_workspace_give_the_same_bits():
    """The minimal workspace takes the loci one at a time and the long locus in replicate ranges of 128."""
    engine = _engine()
    import torch
    sizes, B, T, iv = [40, 5000, 0, 700, 129], 300, 21, [[0, 8], [4, 21]]
    rates = _rates_for(sizes, 9)
    plan, _ = _plan(engine, sizes, T, iv)
    try:
        mn, pf = plan.bootstrap_workspace_bytes(B)
        print("workspace: min %d bytes, preferred %d bytes" % (mn, pf))
        assert 0 < mn < pf
        dev = torch.device("cuda:0")
        d_rates = torch.from_numpy(rates).to(dev)
        Wb = plan.bootstrap_width
        out = []
        for nbytes in (mn, pf):
            ws = torch.empty(pf, dtype=torch.uint8, device=dev)
            d_sum = torch.zeros((len(sizes), 4, Wb), dtype=torch.float64, device=dev)
            d_rows = torch.zeros((len(sizes), B, Wb), dtype=torch.float64, device=dev)
            plan.pi_bootstrap_dev(d_rates, None, d_sum, d_rows, ws, B, seed=5, ws_bytes=nbytes)
            torch.cuda.synchronize()
            out.append((d_sum.cpu().numpy(), d_rows.cpu().numpy()))
        d_sum = torch.zeros((len(sizes), 4, Wb), dtype=torch.float64, device=dev)
        plan.pi_bootstrap_dev(d_rates, None, d_sum, None, ws, B, seed=5, ws_bytes=mn)   # rows kept in the workspace
        torch.cuda.synchronize()
        with pytest.raises(engine.TphipError):
            plan.pi_bootstrap_dev(d_rates, None, d_sum, None, ws, B, seed=5, ws_bytes=mn - 1)
        host_sum, host_rows = plan.pi_bootstrap(rates, replicates=B, seed=5, return_rows=True)
        # the resample core sizes its workspace without bootstrap options (integrals only): minimum = one locus at a time
        rmn, rpf = plan.resample_workspace_bytes()
        assert 0 < rmn <= rpf and rmn <= mn
        cnt = np.random.default_rng(2).integers(0, 3, (3, plan.ncols)).astype(np.uint16)
        d_cnt = torch.from_numpy(cnt.view(np.int16)).to(dev)
        res = []
        for nbytes in (rmn, rpf):
            d_rows3 = torch.zeros((len(sizes), 3, Wb), dtype=torch.float64, device=dev)
            plan.pi_resample_dev(d_rates, None, d_cnt, 3, d_rows3, torch.empty(nbytes, dtype=torch.uint8, device=dev))
            torch.cuda.synchronize()
            res.append(d_rows3.cpu().numpy())
        assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], plan.pi_resample(rates, None, cnt))
    finally:
        plan.close()
    print("differing: rows %d, summary %d" % (int((out[0][1] != out[1][1]).sum()), int((out[0][0] != out[1][0]).sum())))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(d_sum.cpu().numpy(), out[0][0])
    assert np.array_equal(host_rows, out[0][1]) and np.array_equal(host_sum, out[0][0])
    assert np.all(out[0][1][2] == 0.0) and np.all(out[0][0][2] == 0.0)      # the empty locus


# ---- 4. summary --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.95, 0.5])
@pytest.mark.parametrize("B", [2, 3, 100, 4096])
def test_summary_against_numpy(B, level):
    engine = _engine()
    sizes, T, iv = [50, 7], 10, [[0, 5]]
    rates = _rates_for(sizes, 3)
    plan, _ = _plan(engine, sizes, T, iv)
    try:
        summary, rows = plan.pi_bootstrap(rates, replicates=B, seed=4, level=level, return_rows=True)
    finally:
        plan.close()
    worst = [0.0, 0.0, 0.0]
    for l in range(len(sizes)):
        ref = bsr.summarize(rows[l], level)
        top = np.abs(rows[l]).max(axis=0)
        e_mean = np.abs(summary[l, 0] - ref[0])
        e_sd = np.abs(summary[l, 1] - ref[1])
        e_q = np.abs(summary[l, 2:] - ref[2:])
        worst[0] = max(worst[0], float(np.max(e_mean / np.maximum((B + 2) * U * np.abs(ref[0]), 1e-300))))
        worst[1] = max(worst[1], float(np.max(e_sd / np.maximum(8 * B * U * top, 1e-300))))
        worst[2] = max(worst[2], float(np.max(e_q / np.maximum(4 * U * np.abs(ref[2:]), 1e-300))))
        assert np.all(e_mean <= (B + 2) * U * np.abs(ref[0]))
        assert np.all(e_sd <= 8 * B * U * top)
        assert np.all(e_q <= 4 * U * np.abs(ref[2:]))
    print("B=%d level=%g: worst error / bound: mean %.3f, sd %.3f, quantiles %.3f" % (B, level, *worst))


def test_bad_arguments_are_refused():
    engine = _engine()
    plan, _ = _plan(engine, [10], 5, [])
    try:
        r = np.full(10, 0.1)
        for kw in (dict(replicates=1), dict(replicates=4097), dict(replicates=10, level=0.0), dict(replicates=10, level=1.0)):
            with pytest.raises(engine.TphipError):
                plan.pi_bootstrap(r, **kw)
    finally:
        plan.close()


# ---- 5. the bundled locus ----------------------------------------------------------------------------------------
def test_bundled_locus_bands_cover_the_point_estimate(chr1_918):
    engine = _engine()
    c = chr1_918
    T, B = int(c["depth"]), 2000
    rates = np.array(c["kat"]["rate"], dtype=np.float64)
    plan = engine.Plan(len(c["names"]), c["parent"], c["blen"], c["leaf"], [0, rates.size], [c["pi"]], [c["exch"]], T, [], [],
                       correction=c["factor"], threshold=3, round_decimals=4)
    try:
        assert T == 174 and rates.size == 226
        summary, rows = plan.pi_bootstrap(rates, replicates=B, seed=1, return_rows=True)
        point = plan.pi_tables(rates)[0, :T]
    finally:
        plan.close()
    mean, sd, lo, hi = summary[0]
    ratio = np.abs(mean[1:] - point[1:]) / (4 * sd[1:] / np.sqrt(B))
    print("bundled locus, B=%d seed=1: largest |mean - point| / (4 sd / sqrt B) = %.3f at t=%d; sd / point in [%.3f, %.3f]"
          % (B, ratio.max(), 1 + int(ratio.argmax()), (sd[1:] / point[1:]).min(), (sd[1:] / point[1:]).max()))
    assert rows.min() >= 0.0
    assert np.all(np.abs(mean[1:] - point[1:]) <= 4 * sd[1:] / np.sqrt(B))
    assert np.all(lo[1:] <= point[1:]) and np.all(point[1:] <= hi[1:])


# ---- 6. the command line ----------------------------------------------------------------------------------------
def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if "bootstrap" not in f}


def _check_cli(tmp_path, aln, tree):
    engine = _engine()
    from tapir_amd import cli, compute, newick, nexus
    dirs = []
    for name, extra in (("plain", []), ("boot", ["--bootstrap", "64", "--bootstrap-seed", "9"])):
        out = tmp_path / name
        out.mkdir()
        dirs.append(cli.main([aln, tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                              "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"] + extra))
    plain, boot = dirs
    a, b = _outputs(plain), _outputs(boot)
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == []          # main outputs: byte for byte
    assert sorted(set(os.listdir(boot)) - set(os.listdir(plain))) == ["phylogenetic-informativeness-bootstrap.sqlite"]
    con = sqlite3.connect(os.path.join(boot, "phylogenetic-informativeness-bootstrap.sqlite"))
    loci = con.execute("select id, locus from loci order by id").fetchall()
    assert dict(con.execute("select key, value from meta")) == {"replicates": "64", "seed": "9", "level": "0.95"}
    root = newick.read_tree(tree)
    T = int(compute.correct_tree(root)[0])
    iv = [[5, 15], [20, 40]]
    # the final rates of the run: the written corrected_rates, NaN where fewer than --threshold (3) cells are A/C/G/T
    per_locus = []
    for _, name in loci:
        doc = json.load(open(os.path.join(boot, name + ".nex.rates")))["sites"]
        r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
        _, st = nexus.read_states(os.path.join(aln, name + ".nex"))
        nres = np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0)
        per_locus.append(np.where(nres >= 3, r, np.nan))
    off = np.concatenate([[0], np.cumsum([r.size for r in per_locus])]).astype(np.int64)
    L = len(loci)
    plan = engine.Plan(3, PARENT, BLEN, LEAF, off, np.full((L, 4), 0.25), np.ones((L, 6)), T, [], iv,
                       correction=1.0, threshold=0, round_decimals=-1)
    try:
        summary = plan.pi_bootstrap(np.concatenate(per_locus), replicates=64, seed=9, locus_ids=np.arange(L))
    finally:
        plan.close()
    for l, (lid, _) in enumerate(loci):
        got = np.array(con.execute("select mean, sd, lo, hi from net_bootstrap where id = ? order by time", (lid,)).fetchall())
        assert np.array_equal(got.T, summary[l, :, :T])
        got = np.array(con.execute("select mean, sd, lo, hi from interval_bootstrap where id = ? order by rowid", (lid,)).fetchall())
        assert np.array_equal(got.T, summary[l, :, T:])
        got = np.array(con.execute("select mean, sd, lo, hi from discrete_bootstrap where id = ? order by time", (lid,)).fetchall())
        assert np.array_equal(got.T, summary[l][:, [10, 30]])
    count = lambda t: con.execute("select count(*) from %s" % t).fetchone()[0]  # noqa: E731
    assert (count("net_bootstrap"), count("discrete_bootstrap"), count("interval_bootstrap")) == (L * T, L * 2, L * 2)
    print("loci %d, T %d: bootstrap rows equal Plan.pi_bootstrap on the written rates; main outputs byte-equal" % (L, T))
    con.close()


def test_cli_bootstrap_on_the_bundled_locus(tmp_path, golden_dir):
    import shutil
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    _check_cli(tmp_path, str(aln), os.path.join(golden_dir, "Euteleost.tree"))


def test_cli_bootstrap_on_a_synthetic_directory(tmp_path):
    import shutil
    from tapir_amd import synth
    d = synth.simulate(5, 70, 6, 11)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    _check_cli(tmp_path, str(aln), str(tmp_path / "tree.newick"))

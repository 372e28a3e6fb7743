"""The empirical-Bayes rate posterior carried into the PI rows without a GPU: the numpy mirror of the
draw rule against the exact law, the analytic moments, the degenerate cases against pi_tables, and the command line on the
stand-in engine (tests/posterior_pi_engine.py)."""
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import posterior_pi_engine
import posterior_pi_reference as ppr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE3 = dict(parent=[3, 3, 4, 4, -1], blen=[0.1, 0.1, 0.2, 0.1, 0.0], leaf=[0, 1, 2, -1, -1])
CHI2_12_999 = 32.909      # the 0.999 quantile of chi-square with 12 degrees of freedom
LAW_SEED = 1


def _law_case():
    """K = 2, sixteen columns of which four are culled; the twelve live ones have unequal p_1 in 0.15 .. 0.85."""
    p1 = np.array([0.15, 0.22, 0.3, 0.35, 0.42, 0.5, 0.55, 0.61, 0.68, 0.74, 0.8, 0.85, 0.4, 0.6, 0.25, 0.7])
    live = np.ones(16, bool)
    live[[1, 6, 9, 14]] = False
    return np.stack([1.0 - p1, p1]), live


def _chi2(observed, law, B):
    e = B * np.asarray(law)[:13]
    return float(np.sum((observed - e) ** 2 / e))


def _law_statistics(seed):
    post, live = _law_case()
    B = 4096
    n1 = ppr.counts(post, live, seed, 7, B)[:, 1]
    obs = np.bincount(n1, minlength=13)[:13].astype(float)
    truth = ppr.poisson_binomial(post[1][live])
    shifted = ppr.poisson_binomial(post[1][live] + 0.05)
    with_culled = ppr.poisson_binomial(post[1])
    return _chi2(obs, truth, B), _chi2(obs, shifted, B), _chi2(obs, with_culled, B)


def test_mirrored_draws_follow_the_exact_law():
    """N_1 of 4096 mirrored replicates against the exact Poisson-binomial law of the twelve live columns: Pearson's X^2 over the
    13 values of N_1 against the 0.999 quantile of chi-square(12), 32.909.  The seed was chosen on the CPU so that the truth is
    accepted and two near-miss laws are rejected: every p_1 shifted by 0.05, and the four culled columns counted as well.
    Seed 1 (the first tried; seeds 1 to 7 all separate the three): X^2 = 8.60 (truth), 736.68 (shifted), 5133.61 (culled counted)."""
    truth, shifted, with_culled = _law_statistics(LAW_SEED)
    print("seed %d: X^2 truth %.2f, p shifted by 0.05 %.1f, culled columns counted %.1f" % (LAW_SEED, truth, shifted, with_culled))
    assert truth < CHI2_12_999 < min(shifted, with_culled)


def test_categories_follow_the_thresholds_at_the_edges():
    """The rule at the ends of the word range and at ties: category = #{k <= K - 2: (x + 0.5) 2^-32 >= c_k}."""
    p = np.array([[0.25], [0.5], [0.25]])
    x = np.array([[0], [2 ** 30 - 1], [2 ** 30], [3 * 2 ** 30 - 1], [3 * 2 ** 30], [2 ** 32 - 1]], np.uint32)
    assert ppr.categories(p, x)[:, 0].tolist() == [0, 0, 1, 1, 2, 2]
    assert ppr.categories(np.array([[0.0], [1.0]]), x)[:, 0].tolist() == [1] * 6       # p_0 = 0 is never drawn
    assert ppr.categories(np.array([[1.0], [0.0]]), x)[:, 0].tolist() == [0] * 6       # p_0 = 1 always
    # the stream does not move with the cull, nor with B; repeats draw independently
    w = ppr.words(3, 2 ** 33 + 5, 5, 9)
    assert np.array_equal(w[:3, :6], ppr.words(3, 2 ** 33 + 5, 3, 6)) and len(np.unique(w)) == 45


def _random_case(rng, K, n, Wb):
    post = rng.dirichlet(np.full(K, 0.7), n).T
    live = rng.random(n) > 0.25
    P = rng.uniform(0.0, 2.0, (K, Wb)) * rng.uniform(0.1, 3.0, K)[:, None]
    return np.ascontiguousarray(post), live, P


def test_sample_moments_of_mirrored_rows_match_the_analytic_ones():
    """Mean and sd of 4096 mirrored rows within 5 standard errors of the analytic moments: sd / sqrt(B) for the mean and
    sd / sqrt(2 (B - 1)) for the sd (the normal-theory value: a row is a sum over 45 independent sites)."""
    rng = np.random.default_rng(11)
    post, live, P = _random_case(rng, 4, 60, 7)
    B = 4096
    nk, mean, sd = ppr.analytic(post, live, P)
    rows = np.asarray(ppr.rows_from_counts(ppr.counts(post, live, 5, 3, B), P), np.float64)
    z_mean = np.abs(rows.mean(axis=0) - mean) / (sd / np.sqrt(B))
    z_sd = np.abs(rows.std(axis=0, ddof=1) - sd) / (sd / np.sqrt(2.0 * (B - 1)))
    print("largest deviation in standard errors: mean %.2f, sd %.2f" % (z_mean.max(), z_sd.max()))
    assert abs(float(nk.sum()) - live.sum()) < 1e-12 and z_mean.max() <= 5.0 and z_sd.max() <= 5.0
    # the uncentred form of the issue's definition is the same number
    q = post[:, live].astype(np.longdouble)
    var2 = ((q.T @ (np.asarray(P, np.longdouble) ** 2)) - (q.T @ np.asarray(P, np.longdouble)) ** 2).sum(axis=0)
    assert np.allclose(np.asarray(var2, float), np.asarray(sd, float) ** 2, rtol=1e-12, atol=0)


def _plan(sizes, **kw):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    L = len(sizes)
    kw.setdefault("correction", 100.0)
    kw.setdefault("threshold", 3)
    kw.setdefault("round_decimals", 4)
    return posterior_pi_engine.Plan(3, TREE3["parent"], TREE3["blen"], TREE3["leaf"], off, np.full((L, 4), 0.25), np.ones((L, 6)),
                                    12, [], [[0, 5], [3, 12]], **kw)


@pytest.mark.parametrize("integ_mode", [0, 1])
def test_degenerate_prior_gives_the_point_profile(integ_mode):
    """All rho_k = 1: every site has the one rate kappa mu, so the mean row is pi_tables' net and integral entries of that rate
    times the live columns (1e-13 relative) and the spread vanishes (sd <= 1e-7 mean)."""
    plan = _plan([9], integ_mode=integ_mode)
    K, mu = 4, 1.7321
    kappa = plan.models()[3][0]
    post = np.ascontiguousarray(np.random.default_rng(3).dirichlet(np.ones(K), 9).T)
    nres = np.array([3, 3, 2, 3, 0, 3, 3, 3, 3], np.int32)
    out = plan.posterior_pi(post, nres, [mu], np.ones((1, K)), replicates=8)
    tab = plan.pi_tables(np.full(9, kappa * mu), nres)[0]
    want = np.concatenate([tab[:12], tab[12:14]])
    assert np.all(want[1:] > 0)
    rel = np.abs(out["analytic"][0, 0][1:] - want[1:]) / want[1:]
    print("integ_mode %d: mean row against pi_tables %.3g relative, largest sd / mean %.3g" % (
        integ_mode, rel.max(), (out["analytic"][0, 1][1:] / out["analytic"][0, 0][1:]).max()))
    assert rel.max() <= 1e-13 and np.all(out["analytic"][0, 1] <= 1e-7 * out["analytic"][0, 0])
    assert np.allclose(out["expected_counts"][0].sum(), 7.0, rtol=1e-14) and np.all(out["summary"][0, 1] <= 1e-7 * out["summary"][0, 0])


def test_one_hot_posterior_reproduces_pi_of_the_category_rates():
    """Site i all in category k_i: the locus' row is pi_tables' at the rates kappa mu rho_(k_i), and every draw is that row."""
    plan = _plan([6])
    K, mu = 3, 2.0
    rho = np.array([[0.2, 1.0, 1.8]])
    kappa = plan.models()[3][0]
    pick = np.array([0, 2, 1, 1, 0, 2])
    post = np.zeros((K, 6))
    post[pick, np.arange(6)] = 1.0
    out = plan.posterior_pi(post, None, [mu], rho, replicates=5, return_rows=True, return_counts=True)
    tab = plan.pi_tables((kappa * mu) * rho[0][pick], None)[0]
    want = np.concatenate([tab[:12], tab[12:14]])
    assert np.allclose(out["analytic"][0, 0], want, rtol=1e-13, atol=0) and np.all(out["analytic"][0, 1] == 0.0)
    assert np.all(out["counts"][0] == np.bincount(pick, minlength=K)[None, :])
    assert np.allclose(out["rows"][0], want[None, :], rtol=1e-13, atol=0)
    assert np.array_equal(out["expected_counts"][0], [2.0, 2.0, 2.0])


def test_jensens_gap_has_the_expected_sign():
    """One site with a two-point posterior: PI(s, t) = 16 s^2 t e^(-4st) is convex in s where 4 s t is small and concave around
    its maximum 4 s t = 2, so the posterior mean of the profile lies above the profile at the mean rate at early times and
    below it near the peak."""
    plan = _plan([1], correction=1.0, round_decimals=-1)
    kappa = plan.models()[3][0]
    rho = np.array([[0.5, 1.5]])
    mu = 0.05 / kappa                                       # rates 0.025 and 0.075, mean 0.05: the peak of PI(0.05, t) is at t = 10
    out = plan.posterior_pi(np.array([[0.5], [0.5]]), None, [mu], rho, replicates=4)
    at_mean = plan.pi_tables(np.array([0.05]), None)[0]
    gap = out["analytic"][0, 0][:12] - at_mean[:12]
    print("E[PI] - PI(E[s]) at t = 1, 10: %.3g, %.3g" % (gap[1], gap[10]))
    assert gap[1] > 0 and gap[2] > 0 and gap[10] < 0 and gap[11] < 0 and np.all(out["analytic"][0, 1][1:] > 0)


# ---- pipeline and command line on the stand-in engine ------------------------------------------------------------
BASE = ["--times", "10,30", "--intervals", "5-15,20-40", "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1", "--rate-estimator", "eb",
        "--eb-categories", "4", "--eb-alpha", "0.8"]
PFLAG = ["--posterior-pi", "16", "--posterior-pi-seed", str(2 ** 40 + 7), "--posterior-pi-level", "0.8"]
PNAME = "phylogenetic-informativeness-posterior.sqlite"


def _synthetic_dir(tmp_path, nloci=3):
    from tapir_amd import synth
    d = synth.simulate(nloci, 30, 5, 3)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    return str(aln), str(tmp_path / "tree.newick")


def _dump(path):
    con = sqlite3.connect(path)
    try:
        return [list(con.execute("select * from %s order by rowid" % t))
                for t in ("loci", "net_posterior", "discrete_posterior", "interval_posterior", "category", "meta")]
    finally:
        con.close()


def test_cli_writes_the_posterior_database_and_nothing_else_changes(tmp_path):
    from tapir_amd import cli
    aln, tree = _synthetic_dir(tmp_path)
    outs = {}
    for name, extra in (("plain", []), ("post", PFLAG)):
        out = tmp_path / name
        out.mkdir()
        del posterior_pi_engine.CALLS[:]
        outs[name] = cli.main([aln, tree, "--output", str(out)] + BASE + extra, engine_mod=posterior_pi_engine)
    assert posterior_pi_engine.CALLS == [("table", 4), ("posterior_pi", 16, 2 ** 40 + 7, 0.8, [0, 1, 2])]
    plain, post = outs["plain"], outs["post"]
    assert sorted(os.listdir(post)) == sorted(os.listdir(plain) + [PNAME])
    for f in os.listdir(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(post, f), "rb").read(), f
    con = sqlite3.connect(os.path.join(post, PNAME))
    main = sqlite3.connect(os.path.join(post, "phylogenetic-informativeness.sqlite"))
    try:
        tables = {r[0] for r in con.execute("select name from sqlite_master where type = 'table'")} - {"sqlite_sequence"}
        assert tables == {"loci", "net_posterior", "discrete_posterior", "interval_posterior", "category", "meta"}
        cols = lambda t: [r[1] for r in con.execute("pragma table_info(%s)" % t)]  # noqa: E731
        assert cols("net_posterior") == cols("discrete_posterior") == ["id", "time", "mean", "sd", "lo", "hi"]
        assert cols("interval_posterior") == ["id", "interval", "mean", "sd", "lo", "hi"]
        assert cols("category") == ["id", "k", "rate", "expected_sites"] and cols("meta") == ["key", "value"]
        assert con.execute("select * from loci order by id").fetchall() == main.execute("select * from loci order by id").fetchall()
        T = main.execute("select count(*) from net where id = 1").fetchone()[0]
        count = lambda t: con.execute("select count(*) from %s" % t).fetchone()[0]  # noqa: E731
        assert (count("net_posterior"), count("discrete_posterior"), count("interval_posterior"), count("category")) == (3 * T, 6, 6, 12)
        meta = dict(con.execute("select key, value from meta"))
        assert {k: meta[k] for k in ("replicates", "seed", "level", "categories")} == {
            "replicates": "16", "seed": str(2 ** 40 + 7), "level": "0.8", "categories": "4"}
        import json
        for lid in (1, 2, 3):
            assert float(meta["alpha_%d" % lid]) == 0.8 and float(meta["scale_%d" % lid]) > 0
            net = dict((t, r) for t, *r in con.execute("select time, mean, sd, lo, hi from net_posterior where id = ?", (lid,)))
            for t, *r in con.execute("select time, mean, sd, lo, hi from discrete_posterior where id = ?", (lid,)):
                assert net[t] == r
            assert all(sd >= 0 and lo <= hi for mean, sd, lo, hi in net.values())
            cats = list(con.execute("select k, rate, expected_sites from category where id = ? order by k", (lid,)))
            assert [c[0] for c in cats] == [0, 1, 2, 3] and all(a[1] <= b[1] for a, b in zip(cats, cats[1:]))
            # the fit the bands are conditional on is the one the locus' document reports
            name = con.execute("select locus from loci where id = ?", (lid,)).fetchone()[0]
            doc = [f for f in os.listdir(post) if f.endswith(".rates") and name in f][0]
            sites = json.load(open(os.path.join(post, doc)))["sites"]
            assert float(meta["scale_%d" % lid]) == sites["gamma_scale"]
        # the posterior mean of the profile and the profile at the posterior mean rates are of one size, and differ
        point = dict(main.execute("select time, pi from net where id = 1"))
        mean10 = con.execute("select mean from net_posterior where id = 1 and time = 10").fetchone()[0]
        assert 0.2 * point[10] < mean10 < 5 * point[10] and mean10 != point[10]
    finally:
        con.close()
        main.close()


@pytest.mark.parametrize("extra, message", [
    (["--rate-estimator", "eb", "--posterior-pi", "1"], "--posterior-pi must be in 2..4096"),
    (["--rate-estimator", "eb", "--posterior-pi", "4097"], "--posterior-pi must be in 2..4096"),
    (["--posterior-pi", "10"], "--posterior-pi carries the empirical-Bayes rate posterior: it needs --rate-estimator eb"),
    (["--rate-estimator", "ml", "--posterior-pi", "10"], "it needs --rate-estimator eb"),
    (["--rate-estimator", "eb", "--posterior-pi", "10", "--posterior-pi-level", "0"], "--posterior-pi-level must be in (0, 1)"),
    (["--rate-estimator", "eb", "--posterior-pi", "10", "--posterior-pi-level", "1"], "--posterior-pi-level must be in (0, 1)"),
    (["--rate-estimator", "eb", "--posterior-pi-seed", "3"], "--posterior-pi-seed needs --posterior-pi"),
    (["--rate-estimator", "eb", "--posterior-pi-level", "0.9"], "--posterior-pi-level needs --posterior-pi"),
    (["--rate-estimator", "eb", "--posterior-pi", "10", "--posterior-pi-seed", "-1"], "--posterior-pi-seed must be in 0..2^64-1"),
    (["--rate-estimator", "eb", "--posterior-pi", "10", "--posterior-pi-seed", str(2 ** 64)], "--posterior-pi-seed must be in 0..2^64-1"),
])
def test_cli_refuses_bad_posterior_flags(tmp_path, golden_dir, extra, message, capsys):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args([str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10"] + extra)
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err and "unrecognized arguments" not in err


def test_cli_posterior_defaults(tmp_path, golden_dir):
    from tapir_amd import cli
    base = [str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10", "--rate-estimator", "eb"]
    a = cli.get_args(base)
    assert (a.posterior_pi, a.posterior_pi_seed, a.posterior_pi_level) == (0, None, None)
    a = cli.get_args(base + ["--posterior-pi", "200"])
    assert (a.posterior_pi, a.posterior_pi_seed, a.posterior_pi_level) == (200, 1, 0.95)


def test_posterior_tables_do_not_depend_on_the_shard_or_the_blocking(tmp_path, monkeypatch):
    """A rank's loci with their global ids and fits give the rows of the full run, whatever the byte budget of a block."""
    from tapir_amd import nexus, newick, pipeline
    aln, tree = _synthetic_dir(tmp_path, nloci=4)
    files = sorted(os.path.join(aln, f) for f in os.listdir(aln))
    root = newick.read_tree(tree, 'newick')
    names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, names)
    per_locus = [np.zeros(nexus.read_states(f)[1].shape[1]) for f in files]
    models = dict(pi=np.full((4, 4), 0.25), exch=np.tile([1, 1.2, 0.8, 0.9, 1.5, 1], (4, 1)), model="gtr")
    fit = dict(alpha=np.array([0.8, 1.5, 0.5, 3.0]), scale=np.array([0.4, 0.6, 0.5, 0.3]), categories=4)

    the_run = pipeline.Run(names, parent, blen, leaf, 12, [], [[0, 5], [3, 12]], correction=100.0, threshold=3, round_decimals=4,
                           device=0, integ_mode=0)

    def run(idx):
        sub = dict(alpha=fit["alpha"][idx], scale=fit["scale"][idx], categories=4)
        m = dict(pi=models["pi"][idx], exch=models["exch"][idx], model="gtr")
        return pipeline.posterior_pi_tables(posterior_pi_engine, [files[i] for i in idx], [per_locus[i] for i in idx], m, sub, the_run,
                                            idx, 16, seed=3, level=0.9)

    full = run([0, 1, 2, 3])
    assert full["bands"].shape == (4, 4, 14) and full["category_rate"].shape == (4, 4) and np.all(full["bands"][:, 1, 1:] > 0)
    monkeypatch.setattr(pipeline, "POSTERIOR_PI_BYTES", 8 * 4 * 31)     # one locus of 30 columns per block
    for idx in ([0, 1, 2, 3], [0, 2], [3]):
        part = run(idx)
        for k in full:
            assert np.array_equal(part[k], full[k][idx]), (idx, k)
    empty = pipeline.posterior_pi_tables(posterior_pi_engine, [], [], models, dict(alpha=[], scale=[], categories=4), the_run, [], 16)
    assert empty["bands"].shape == (0, 4, 14)


def test_estimate_can_return_the_table():
    """eb.estimate(table=True): the fit and the per-column outputs of the plain call, plus the category posterior at that fit."""
    from tapir_amd import eb, synth
    d = synth.simulate(2, 25, 5, 9)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    plan = posterior_pi_engine.Plan(5, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], d["pi"], d["exch"], 12, [], [[0, 5]])
    plain = eb.estimate(plan, st, ncat=4, alpha=1.0)
    full = eb.estimate(plan, st, ncat=4, alpha=1.0, table=True)
    assert "post" not in plain and full["post"].shape == (4, 50)
    for k in plain:
        assert np.array_equal(plain[k], full[k]), k
    rho, _ = eb.gamma_tables(full["alpha"], 4)
    kappa = plan.models()[3]
    assert np.allclose(full["post"].sum(axis=0), 1.0, rtol=0, atol=1e-12)
    for l in range(2):
        sl = slice(25 * l, 25 * (l + 1))
        assert np.allclose((full["post"][:, sl] * rho[l][:, None]).sum(axis=0) * kappa[l] * full["scale"][l], full["rate"][sl], rtol=1e-12)
    assert np.array_equal(eb.posterior_table(plan, st, full["alpha"], full["scale"], ncat=4)["post"], full["post"])


_CLI_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import posterior_pi_engine
from tapir_amd import cli
cli.main(%(argv)r, engine_mod=posterior_pi_engine)
'''


def test_cli_two_ranks_gloo_matches_single_process(tmp_path):
    """Three files on two ranks (ragged shards): the gathered posterior database equals the single-process run's, row for row."""
    import torch  # noqa: F401
    from tapir_amd import cli
    aln, tree = _synthetic_dir(tmp_path)
    outs = []
    for name in ("single", "multi"):
        out = tmp_path / name
        out.mkdir()
        outs.append(out)
    argv = [aln, tree] + BASE + PFLAG + ["--output"]
    single = cli.main(argv + [str(outs[0])], engine_mod=posterior_pi_engine)
    script = tmp_path / "w.py"
    script.write_text(_CLI_WORKER % {"root": ROOT, "argv": argv + [str(outs[1])]})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29563")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29563", str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = _dump(os.path.join(single, PNAME)), _dump(os.path.join(str(outs[1]), PNAME))
    assert a == b and len(a[0]) == 3


def test_engine_declares_the_posterior_entry_points():
    """The binding lists the new C entry points with the header's signatures (the struct's layout included)."""
    import ctypes
    from tapir_amd import engine
    names = {s[0] for s in engine.SYMBOLS}
    assert {"tphip_eb_posterior_table", "tphip_eb_posterior_table_dev", "tphip_posterior_pi_workspace_bytes", "tphip_posterior_pi_dev",
            "tphip_posterior_pi"} <= names
    assert ctypes.sizeof(engine.PosteriorPiOpts) == 40 and engine.PosteriorPiOpts.seed.offset == 16 and engine.PosteriorPiOpts.ncat.offset == 32
    for m in ("eb_posterior_table", "eb_posterior_table_dev", "posterior_pi", "posterior_pi_dev", "posterior_pi_workspace_bytes"):
        assert hasattr(engine.Plan, m)
    header = open(os.path.join(ROOT, "include", "tphip.h")).read()
    assert "tphip_posterior_pi_opts" in header and "#define TPHIP_VERSION 110" in header

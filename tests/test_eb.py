"""Empirical-Bayes site rates on the host side (no GPU): the reference (tests/eb_reference.py) against its 40-digit twin and
hand-written formulas, the ctypes options struct against the C header, the command line, and the pipeline end to end with
the CPU stand-in engine (tests/eb_engine.py: the two engine calls answered by the reference)."""
import dataclasses
import json
import math
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import eb_reference as ebr   # noqa: E402

GTR = ([0.1, 0.2, 0.3, 0.4], [0.6, 2.0, 0.5, 1.3, 3.0, 1.0])
TREES = {   # post-order (parent, leaf_taxon, branch_len), root last
    3: ([2, 2, 4, 4, -1], [0, 1, -1, 2, -1], [0.3, 0.7, 0.2, 0.9, 0.0]),
    5: ([5, 5, 6, 7, 7, 6, 8, 8, -1], [0, 1, 2, 3, 4, -1, -1, -1, -1], [0.2, 0.4, 0.6, 0.1, 0.9, 0.3, 0.5, 0.25, 0.0]),
}
COLUMNS = {3: [[1, 1, 1], [1, 2, 1], [4, 8, 1], [15, 2, 2], [5, 1, 4], [8, 8, 2]],
           5: [[1, 1, 1, 1, 1], [2, 2, 4, 2, 2], [1, 2, 4, 8, 1], [15, 8, 8, 15, 8], [3, 1, 1, 2, 1], [8, 4, 8, 4, 2], [2, 2, 2, 2, 8],
               [1, 1, 1, 1, 1]]}


def _locus(ntaxa, model="gtr", hp_model=None):
    parent, leaf, blen = TREES[ntaxa]
    cols = np.array(COLUMNS[ntaxa], np.uint8).T
    pi, exch = GTR
    return ebr.Locus(cols, parent, blen, leaf, pi, None if model == "f81" else exch, hp_model=hp_model)


@pytest.mark.parametrize("model", ["gtr", "f81"])
@pytest.mark.parametrize("ntaxa", [3, 5])
def test_reference_against_its_40_digit_twin(ntaxa, model):
    """<= 8 patterns of 3 and 5 taxa: the oracle-based reference and the mpmath one agree to the fp64 curves' accuracy."""
    fp, mp = _locus(ntaxa, model), _locus(ntaxa, model, hp_model=model)
    assert fp.pat.shape[1] <= 8 and fp.count.sum() == len(COLUMNS[ntaxa])
    for log_mu, alpha, K in ((0.0, 1.0, 4), (-1.0, 0.5, 8), (1.0, 3.0, 2)):
        a, b = fp.posterior(log_mu, alpha, K), mp.posterior(log_mu, alpha, K)
        for k in ("rate", "sd", "ll", "mean", "second"):
            assert np.allclose(a[k], b[k], rtol=1e-10, atol=1e-12), k
        assert np.allclose(a["weights"].sum(axis=0), 1.0, rtol=0, atol=1e-14)
        assert abs(fp.objective(log_mu, alpha, K) - mp.objective(log_mu, alpha, K)) <= 1e-10


def test_two_categories_by_hand():
    """K = 2 written out: m = (L1 + L2) / 2, p1 = L1 / (L1 + L2), mean = p1 rho1 + p2 rho2, var = p1 p2 (rho1 - rho2)^2."""
    from oracle import oracle as orc
    from tapir_amd import compute
    loc = _locus(5)
    alpha, log_mu = 0.8, -0.5
    rho, w = compute.discrete_gamma(alpha, 2)
    assert np.allclose(w, 0.5) and abs(rho.mean() - 1.0) < 1e-12
    post = loc.posterior(log_mu, alpha, 2)
    cols = np.array(COLUMNS[5], np.uint8).T
    parent, leaf, blen = TREES[5]
    pi = np.array(GTR[0])
    for c in range(cols.shape[1]):
        f = orc.column_curve(cols, np.array(parent, np.int32), np.array(blen), np.array(leaf, np.int32), pi, np.array(GTR[1]), c,
                             log_mu + np.log(rho))[0]
        l1, l2 = math.exp(f[0]), math.exp(f[1])
        p1 = l1 / (l1 + l2)
        mean = p1 * rho[0] + (1 - p1) * rho[1]
        km = loc.kappa * math.exp(log_mu)
        assert abs(post["ll"][c] - math.log(0.5 * (l1 + l2))) <= 1e-13
        assert abs(post["rate"][c] - km * mean) <= 1e-14 * km
        assert abs(post["sd"][c] - km * math.sqrt(p1 * (1 - p1)) * (rho[1] - rho[0])) <= 1e-9 * km
    assert abs(loc.kappa - 2 * sum(pi[i] * pi[j] * r for (i, j), r in zip(ebr.PAIRS, GTR[1]))) < 1e-15


def test_limits_when_one_category_carries_the_likelihood():
    """A column that differs at every tip on long branches, scale tiny: only the fastest category can explain it, so the
    posterior sits on rho_K: rate -> kappa mu rho_K, sd -> 0.  A constant column at a huge scale sits on rho_1."""
    from tapir_amd import compute
    parent, leaf, blen = TREES[5]
    loc = ebr.Locus(np.array([[1], [2], [4], [8], [1]], np.uint8), parent, blen, leaf, *GTR)   # at least three changes: L_k ~ rho_k^3
    rho, _ = compute.discrete_gamma(0.2, 4)
    log_mu = -14.0
    p = loc.posterior(log_mu, 0.2, 4)
    km = loc.kappa * math.exp(log_mu)
    assert p["weights"][-1, 0] > 1 - 2e-3 and abs(p["rate"][0] / (km * rho[-1]) - 1) < 2e-3 and p["sd"][0] < 0.1 * p["rate"][0]
    loc = ebr.Locus(np.array([[1], [1], [1], [1], [1]], np.uint8), parent, blen, leaf, *GTR)
    p = loc.posterior(5.0, 0.2, 4)
    assert p["weights"][0, 0] > 1 - 1e-3 and loc.kappa * math.exp(5.0) * rho[0] <= p["rate"][0] < loc.kappa * math.exp(5.0) * rho[1]


def test_gamma_tables_match_the_scalar_helper():
    from tapir_amd import compute, eb
    alphas = [0.2, 0.5, 1.0, 7.0, 50.0]
    for K in (2, 5, 16):
        r, w = eb.gamma_tables(alphas, K)
        for i, a in enumerate(alphas):
            rr, ww = compute.discrete_gamma(a, K)
            assert np.array_equal(r[i], rr) and np.array_equal(w[i], ww)
    for K in (1, 17):
        with pytest.raises(eb.EbError):
            eb.gamma_tables([1.0], K)


def test_parsimony_start():
    from tapir_amd import eb
    parent, leaf, blen = TREES[5]
    cols = np.array(COLUMNS[5], np.uint8).T
    assert list(eb.parsimony_changes(cols, parent, leaf)) == [0, 1, 3, 0, 1, 3, 1, 0]
    s = eb.start_scales(cols, [0, 4, 8, 8], parent, blen, leaf)
    length = sum(blen)
    assert np.allclose(s, [1.0 / length, 1.25 / length, 1.0 / length])   # (4 and 5 changes in 4 columns; an empty locus: 1 / length)
    assert np.allclose(eb.start_scales(cols, [0, 2, 8], parent, blen, leaf), [0.5 / length, 8 / 6 / length])


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "tphip.h"
#define F(name) printf("%s %zu\n", #name, offsetof(tphip_eb_opts, name));
int main(void) {
    printf("sizeof %zu\n", sizeof(tphip_eb_opts));
    F(struct_size) F(ncat) F(maxit_scale) F(use_patterns) F(tol_scale)
    printf("TPHIP_VERSION %d\n", TPHIP_VERSION);
    return 0;
}
"""


def test_eb_opts_ctypes_matches_header(tmp_path):
    import ctypes
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to read include/tphip.h with")
    src = tmp_path / "probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).split("\n") if ln.strip())}
    from tapir_amd import engine
    names = [f[0] for f in engine.EbOpts._fields_]
    assert names == ["struct_size", "ncat", "maxit_scale", "use_patterns", "tol_scale"]
    assert ctypes.sizeof(engine.EbOpts) == c["sizeof"]
    for n in names:
        assert getattr(engine.EbOpts, n).offset == c[n], n
    assert c["TPHIP_VERSION"] == 110
    bound = {s[0] for s in engine.SYMBOLS}
    assert {"tphip_eb_fit_scale", "tphip_eb_fit_scale_dev", "tphip_eb_posterior", "tphip_eb_posterior_dev"} <= bound


def _argv(tmp_path, golden_dir, *extra):
    aln = tmp_path / "aln"
    aln.mkdir(exist_ok=True)
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    return [str(aln), os.path.join(golden_dir, "Euteleost.tree"), "--output", str(out), "--times", "10,20,50",
            "--intervals", "0-10,10-15,20-100"] + list(extra)


def test_rate_estimator_flags_parse(tmp_path, golden_dir):
    from tapir_amd import cli
    a = cli.get_args(_argv(tmp_path, golden_dir))
    assert (a.rate_estimator, a.eb_categories, a.eb_alpha, a.eb_alpha_bounds) == ("ml", None, None, None)
    assert (a.gamma_categories, a.gamma_alpha) == (1, 0.5)
    a = cli.get_args(_argv(tmp_path, golden_dir, "--rate-estimator", "eb"))
    assert (a.rate_estimator, a.eb_categories, a.eb_alpha, a.eb_alpha_bounds) == ("eb", 8, None, (0.2, 50.0))
    a = cli.get_args(_argv(tmp_path, golden_dir, "--rate-estimator", "eb", "--eb-categories", "4", "--eb-alpha", "1.5",
                           "--eb-alpha-bounds", "0.5,10", "--site-model", "f81"))
    assert (a.eb_categories, a.eb_alpha, a.eb_alpha_bounds, a.site_model) == (4, 1.5, (0.5, 10.0), "f81")
    cli.get_args(_argv(tmp_path, golden_dir, "--rate-estimator", "eb", "--exchangeabilities", "1,2,1,1,2,1"))
    cli.get_args(_argv(tmp_path, golden_dir, "--rate-estimator", "ml", "--gamma-categories", "4", "--site-rates"))


@pytest.mark.parametrize("bad, names", [   # (arguments, what the error message must name)
    (["--rate-estimator", "map"], "--rate-estimator"),
    (["--eb-categories", "4"], "--eb-categories needs --rate-estimator eb"),
    (["--eb-alpha", "1"], "--eb-alpha needs --rate-estimator eb"),
    (["--eb-alpha-bounds", "1,2"], "--eb-alpha-bounds needs --rate-estimator eb"),
    (["--rate-estimator", "ml", "--eb-alpha", "1"], "--eb-alpha needs --rate-estimator eb"),
    (["--rate-estimator", "eb", "--site-rates"], "--site-rates"),
    (["--rate-estimator", "eb", "--gamma-categories", "4"], "--gamma-categories"),
    (["--rate-estimator", "eb", "--eb-categories", "1"], "--eb-categories must be in 2..16"),
    (["--rate-estimator", "eb", "--eb-categories", "17"], "--eb-categories must be in 2..16"),
    (["--rate-estimator", "eb", "--eb-alpha", "0"], "--eb-alpha must be positive"),
    (["--rate-estimator", "eb", "--eb-alpha-bounds", "2,1"], "--eb-alpha-bounds must be LO,HI"),
    (["--rate-estimator", "eb", "--eb-alpha-bounds", "1"], "--eb-alpha-bounds")])
def test_rate_estimator_conflicts_are_argparse_errors(tmp_path, golden_dir, capsys, bad, names):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args(_argv(tmp_path, golden_dir, *bad))
    assert e.value.code == 2
    assert names in capsys.readouterr().err


def test_pipeline_rejects_unknown_estimator(golden_dir):
    import eb_engine
    from tapir_amd import pipeline
    args = ([os.path.join(golden_dir, "chr1_918.nex")], pipeline.Run(["a"], [1, -1], [0.1, 0], [0, -1], 5, [1], [[0, 2]], 1.0, 3), np.ones(6))
    with pytest.raises(pipeline.PipelineError):
        pipeline.run_alignments(*args, engine_mod=eb_engine, rate_estimator="x")
    with pytest.raises(pipeline.PipelineError):
        pipeline.run_alignments(*args, engine_mod=eb_engine, rate_estimator="ml", eb_options=dict(categories=4))
    with pytest.raises(pipeline.PipelineError):
        pipeline.run_alignments(*args, engine_mod=eb_engine, rate_estimator="eb", eb_options=dict(categories=40))
    mixed = dataclasses.replace(args[1], cat_rates=[0.5, 1.5], cat_weights=[0.5, 0.5])
    with pytest.raises(pipeline.PipelineError):
        pipeline.run_alignments(args[0], mixed, args[2], engine_mod=eb_engine, rate_estimator="eb")


def _read_outputs(outdir):
    doc = json.load(open(os.path.join(outdir, "chr1_918.nex.rates")))["sites"]
    conn = sqlite3.connect(os.path.join(outdir, "phylogenetic-informativeness.sqlite"))
    net = [p for _, p in conn.execute("select time, pi from net order by time")]
    disc = dict(conn.execute("select time, pi from discrete"))
    iv = {k: (p, e) for k, p, e in conn.execute("select interval, pi, error from interval")}
    conn.close()
    return doc, net, disc, iv


def test_cli_eb_with_the_stand_in_engine(golden_dir, tmp_path, oracle):
    """chr1_918 + Euteleost through the command line with --rate-estimator eb (Jukes-Cantor, so no stage 1), the engine's two
    calls answered by the reference: JSON keys and values, corrected rates, sqlite rows against oracle.worker_tables on the
    reference's rates; and an ml run beside it, whose constant columns have rate 0 where every eb rate is positive."""
    import eb_engine
    from tapir_amd import cli, compute, newick, nexus
    eb_engine.CALLS.clear()
    K = 4
    outdir = cli.main(_argv(tmp_path, golden_dir, "--site-model", "jc", "--rate-estimator", "eb", "--eb-categories", str(K),
                            "--eb-alpha-bounds", "0.3,20"), engine_mod=eb_engine)
    assert ("posterior", K) in eb_engine.CALLS and eb_engine.CALLS.count(("fit", K)) > 10
    doc, net, disc, iv = _read_outputs(outdir)
    assert list(doc) == ["freqs", "subs_matrix", "estimator", "gamma_alpha", "gamma_scale", "gamma_categories", "locus_lnl", "rates",
                         "corrected_rates"]
    assert doc["estimator"] == "eb" and doc["gamma_categories"] == K and 0.3 <= doc["gamma_alpha"] <= 20
    names, st = nexus.read_states(os.path.join(golden_dir, "chr1_918.nex"))
    root = newick.read_tree(os.path.join(outdir, "Tree_100_174.0.newick"))
    leaf_names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, leaf_names)
    st = st[[names.index(n) for n in leaf_names]]
    ref = ebr.Locus(st, parent, blen, leaf, np.full(4, 0.25), None)
    # the search found the reference's optimum (same objective, the reference's own two-level scalar search)
    u_ref, a_ref, l_ref = ref.fit(K, alpha_bounds=(0.3, 20.0))
    assert doc["locus_lnl"] >= l_ref - 1e-7 and abs(doc["locus_lnl"] - ref.objective(math.log(doc["gamma_scale"]), doc["gamma_alpha"], K)) < 1e-9
    assert abs(math.log(doc["gamma_alpha"] / a_ref)) < 2e-2 and abs(math.log(doc["gamma_scale"]) - u_ref) < 1e-3
    want = ref.posterior(math.log(doc["gamma_scale"]), doc["gamma_alpha"], K)
    rows = doc["rates"]
    assert [r["site"] for r in rows] == list(range(1, 227)) and all(list(r) == ["site", "subst", "rate", "ll", "sd"] for r in rows)
    rate4 = compute.round_like_hyphy(want["rate"], 4)
    assert np.array_equal(np.array([r["rate"] for r in rows]), rate4)
    assert np.array_equal(np.array([r["sd"] for r in rows]), compute.round_like_hyphy(want["sd"], 4))
    assert np.array_equal(np.array([r["ll"] for r in rows]), compute.round_like_hyphy(want["ll"], 4))
    assert np.array_equal(np.array([r["subst"] for r in rows]), compute.round_like_hyphy(want["rate"] * blen[np.asarray(parent) >= 0].sum(), 4))
    corrected = rate4 / 100
    assert np.array_equal(np.array([r["rate"] for r in doc["corrected_rates"]]), corrected)
    rates = corrected.copy()
    rates[oracle.informative_counts(st) < 3] = np.nan
    pi_net, pi_times, pi_epochs = oracle.worker_tables(rates, 174, [10, 20, 50], [[0, 10], [10, 15], [20, 100]])
    assert np.allclose(net, pi_net, rtol=1e-12, atol=1e-300)
    assert set(disc) == {10, 20, 50} and all(abs(disc[t] - pi_times[t]) <= 1e-12 * abs(pi_times[t]) for t in disc)
    for k in ("0-10", "10-15", "20-100"):
        assert abs(iv[k][0] - pi_epochs[k]["sum(integral)"]) <= 1e-9 * pi_epochs[k]["sum(integral)"]
    # the ml run beside it: today's document (no new key), exact zeros on the constant columns
    ml_dir = tmp_path / "ml"
    ml_dir.mkdir()
    out_ml = cli.main(_argv(ml_dir, golden_dir, "--site-model", "jc"), engine_mod=eb_engine)
    ml = json.load(open(os.path.join(out_ml, "chr1_918.nex.rates")))["sites"]
    assert list(ml) == ["freqs", "subs_matrix", "rates", "corrected_rates"] and list(ml["rates"][0]) == ["site", "subst", "rate", "ll"]
    mlref = oracle.site_rates(st, parent, blen, leaf, np.full(4, 0.25), np.ones(6))
    assert np.array_equal(np.array([r["rate"] for r in ml["rates"]]), compute.round_like_hyphy(mlref["rate"], 4))
    norm = np.where(st == 0, 15, st & 15)
    const = (mlref["flag"] == 3)
    assert const.sum() == 133 and np.all(np.array([r["rate"] for r in ml["rates"]])[const] == 0.0)
    eb_rate = want["rate"]
    assert np.all(eb_rate[const] > 0) and np.all(np.isfinite(eb_rate)) and norm.shape[1] == 226


def test_dumps_rates_json_is_json_dumps_of_the_document():
    """The eb document's text is what json.dumps(indent=4) writes for the same content, and parses back."""
    from tapir_amd import pipeline
    n = 5
    rate, sd = np.linspace(0.01, 0.3, n), np.linspace(0.001, 0.2, n)
    meta = dict(alpha=1.25, scale=0.0123, categories=8, locus_lnl=-561.25)
    text = pipeline.dumps_rates_json([0.1, 0.2, 0.3, 0.4], [1, 2, 3, 4, 5, 6], np.arange(1, n + 1), rate * 3, rate, -rate, rate / 100, sd=sd, eb=meta)
    doc = json.loads(text)
    assert json.dumps(doc, indent=4) == text
    assert doc["sites"]["gamma_alpha"] == 1.25 and doc["sites"]["rates"][2]["sd"] == float("%.4f" % sd[2])
    plain = pipeline.dumps_rates_json([0.1, 0.2, 0.3, 0.4], [1, 2, 3, 4, 5, 6], np.arange(1, n + 1), rate * 3, rate, -rate, rate / 100)
    assert "sd" not in plain and "estimator" not in plain


def test_lockstep_search_against_the_scalar_search():
    """tapir_amd/eb.py's golden-section search for 24 synthetic loci at once (through the stand-in engine) against the
    reference's own two-level scalar search, locus by locus: same objective value to 1e-6, alpha to 2 % (the profile is flat
    near its top), also for loci whose best alpha is the upper end of the interval."""
    import eb_engine
    from tapir_amd import eb
    parent, leaf, blen = TREES[5]
    rng = np.random.default_rng(3)
    pool = np.array(COLUMNS[5], np.uint8).T
    L, n = 24, 30
    cols, off = [], [0]
    for l in range(L):
        pick = rng.choice(pool.shape[1], n, p=[0.35, 0.1, 0.03, 0.1, 0.05, 0.05, 0.07, 0.25] if l % 3 else
                          [0.45, 0.05, 0.02, 0.1, 0.03, 0.02, 0.03, 0.3])   # mostly constant columns, as short loci are
        cols.append(pool[:, pick])
        off.append(off[-1] + n)
    states = np.ascontiguousarray(np.concatenate(cols, axis=1))
    pi = np.tile(GTR[0], (L, 1))
    exch = np.tile(GTR[1], (L, 1))
    plan = eb_engine.Plan(5, parent, blen, leaf, off, pi, exch, 10, [5], [[0, 5]])
    est = eb.estimate(plan, states, ncat=4, alpha_bounds=(0.3, 20.0))
    at_end = 0
    for l in range(L):
        ref = ebr.Locus(states[:, off[l]:off[l + 1]], parent, blen, leaf, pi[l], exch[l])
        u, a, val = ref.fit(4, alpha_bounds=(0.3, 20.0))
        assert est["locus_lnl"][l] >= val - 1e-6, (l, est["locus_lnl"][l], val)
        assert abs(est["locus_lnl"][l] - ref.objective(math.log(est["scale"][l]), est["alpha"][l], 4)) < 1e-9
        if a > 19.9 or a < 0.301:
            at_end += 1
            assert abs(math.log(est["alpha"][l] / a)) < 1e-3
        else:
            assert abs(math.log(est["alpha"][l] / a)) < 2e-2, (l, est["alpha"][l], a)
    assert est["rounds"] < 40 and np.all(est["rate"] > 0)
    fixed = eb.estimate(plan, states, ncat=4, alpha=1.5)
    assert np.all(fixed["alpha"] == 1.5) and fixed["rounds"] == 1

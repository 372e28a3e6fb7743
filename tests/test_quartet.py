"""Quartet signal and noise without a GPU: the definition (tests/quartet_reference.py: the fp64
restatement against the 40-digit twin, the closed forms, the bivariate normal against scipy and mpmath, the normal
approximation against the exact distribution) and the host layers above the engine -- pipeline.quartet_tables, the
--quartets flag and the second sqlite file -- on the CPU stand-in engine (tests/quartet_engine.py).

Bounds:
  restatement against the twin   128 * 2^-52 relative.  y and x are sums of non-negative products of five matrix entries;
                                 an entry of M or N is a three-term sum of eigenvector products (each a few units from
                                 eigh's backward error on a well-separated 4 x 4 spectrum) times an expm1: about 20 units per
                                 entry at worst, five entries per product, the 16 + 10 term sums add at most their length.
                                 The models below have well-separated eigenvalues.  A reference of exactly 0 must be 0.
  JC closed form                 16 * 2^-52 relative per entry of M (one expm1, one fma against a three-term eigen-sum)
  B against scipy / mpmath       1e-13 absolute: the 64-point rule's error on a smooth integrand; both references are
                                 accurate to a few 1e-16 here
"""
import math
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import quartet_engine
import quartet_reference as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52

GTR = dict(model="gtr", pi=[0.31, 0.19, 0.27, 0.23], exch=[1.0, 2.7, 0.6, 1.2, 3.1, 0.9])
F81 = dict(model="f81", pi=[0.4, 0.0, 0.35, 0.25], exch=[1.0] * 6)          # one absent base
JC = dict(model="f81", pi=[0.25] * 4, exch=[1.0] * 6)
QUARTETS = [(0.0, 1e-3), (20.0, 5.0), (20.0, 0.5), (100.0, 50.0)]


def _rates():
    rng = np.random.default_rng(20261018)
    return np.concatenate([10.0 ** rng.uniform(-9, 3, 10), [0.0, np.nan, 1e4, 1e-9]])


# ---- the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, m", [("gtr", GTR), ("f81", F81), ("jc", JC)])
def test_restatement_against_the_40_digit_twin(name, m):
    rates = _rates()
    worst = 0.0
    for tip, internode in QUARTETS:
        ty, tx, tx2 = qr.twin_values(m["pi"], m["exch"], rates, tip, internode)
        y, x = qr.site_values(m["model"], m["pi"], m["exch"], rates, tip, internode)
        ey, zy = qr.relative_error(y, ty)
        ex, zx = qr.relative_error(x, tx)
        print("%s T=%g to=%g: relative error of y %.2e, of x %.2e (bound %.2e)" % (name, tip, internode, ey, ex, 128 * U))
        assert zy and zx                                   # culled and zero rates, and x at T = 0: exactly 0
        assert y[10] == 0.0 and y[11] == 0.0 and x[10] == 0.0 and x[11] == 0.0
        if tip == 0.0:
            assert np.all(x == 0.0) and all(v == 0 for v in tx)
        worst = max(worst, ey, ex)
        assert ey <= 128 * U and ex <= 128 * U
    if name == "jc":   # the eigen form of the same model (a triple eigenvalue) agrees with the closed form
        y2, x2 = qr.site_values("gtr", JC["pi"], JC["exch"], rates, 20.0, 5.0)
        y1, x1 = qr.site_values("f81", JC["pi"], JC["exch"], rates, 20.0, 5.0)
        live = y1 > 0
        assert np.max(np.abs(y2[live] / y1[live] - 1)) <= 128 * U and np.max(np.abs(x2[live] / x1[live] - 1)) <= 128 * U


def test_both_noise_patterns_have_the_same_probability():
    """x(ijij) = x(ijji): all four tip branches are equal, so one number serves both wrong topologies."""
    import mpmath as mp
    for m in (GTR, F81):
        _, x1, x2 = qr.twin_values(m["pi"], m["exch"], [1e-3, 0.04, 2.0], 20.0, 5.0)
        for a, b in zip(x1, x2):
            assert a > 0 and abs(a - b) <= mp.mpf(10) ** -35 * a


@pytest.mark.parametrize("model", ["f81", "gtr"])
def test_jukes_cantor_closed_form(model):
    """M_xx = 1/4 + 3/4 e, M_xy = 1/4 - 1/4 e, e = exp(-4 r tau / 3); the off-diagonal entry is compared in the form
    -expm1(-4 r tau / 3) / 4, the same number without the cancellation of 1/4 - e/4 at small r tau."""
    r = np.array([1e-9, 1e-4, 0.01, 0.3, 5.0, 1e3])
    for tau in (1e-3, 1.0, 40.0):
        P = qr.transition(model, [0.25] * 4, [1.0] * 6, r, tau)
        e = np.exp(-4.0 * r * tau / 3.0)
        off = -np.expm1(-4.0 * r * tau / 3.0) / 4.0
        for i in range(4):
            for j in range(4):
                want = 0.25 + 0.75 * e if i == j else off
                assert np.all(np.abs(P[:, i, j] - want) <= 16 * U * want), (model, tau, i, j)
        big = r * tau > 0.1
        assert np.allclose(P[big, 0, 1], 0.25 - 0.25 * e[big], rtol=1e-13, atol=0)
        assert np.all(np.abs(P.sum(axis=2) - 1.0) <= 8 * U)


@pytest.mark.parametrize("rho", [-0.3, 0.4, 0.95, 0.999, 1.0])
def test_bivariate_normal_against_scipy_and_mpmath(rho):
    for h, k in ((0.3, 0.3), (-1.2, -1.2), (2.5, 2.5), (0.0, 0.0), (1.1, 0.2), (-2.0, 0.4), (0.4, 3.0)):
        if rho > 0.99 and h != k:
            continue            # the definition evaluates unequal arguments at rho <= 0.99 only
        got, sp, mpv = qr.bvn_upper(h, k, rho), qr.bvn_scipy(h, k, rho), qr.bvn_mp(h, k, rho)
        print("B(%g, %g, %g) = %.16f: - scipy %.1e, - mpmath %.1e" % (h, k, rho, got, got - sp, got - mpv))
        assert abs(got - sp) <= 1e-13 and abs(got - mpv) <= 1e-13
    assert abs(qr.bvn_upper(0.7, 0.7, 0.0) - qr._phi_upper(0.7) ** 2) <= 4 * U


def test_unequal_arguments_at_the_cap():
    """p_incorrect's correlation is capped at 0.99: the general integrand there, against both references."""
    for h, k in ((1.1, 0.2), (-2.0, 0.4), (0.4, 3.0), (3.5, 0.05), (-6.0, 1.5)):
        got = qr.bvn_upper(h, k, 0.99)
        assert abs(got - qr.bvn_scipy(h, k, 0.99)) <= 1e-13 and abs(got - qr.bvn_mp(h, k, 0.99)) <= 1e-13


def _loci():
    rng = np.random.default_rng(7)
    out = []
    for n, lo, hi in ((400, -3.5, -1.0), (60, -3, -1), (30, -2, 0), (5, -4, -3), (200, -1, 1), (1, -2, -2)):
        out.append(10.0 ** rng.uniform(lo, hi, n))
    return out


def test_probabilities_lie_in_the_unit_interval_and_sum_to_one():
    for m in (GTR, F81):
        for r in _loci():
            for quartet in ((30.0, 4.0), (5.0, 20.0), (100.0, 0.5), (0.0, 2.0)):
                row = qr.rows(m["model"], m["pi"], m["exch"], r, [quartet])[0]
                pc, pw, pp = row[5:]
                assert 0.0 <= pc <= 1.0 and 0.0 <= pw <= 1.0 and 0.0 <= pp <= 1.0
                assert abs(pc + pw + pp - 1.0) <= 4 * U, (quartet, row)
                assert row[0] >= row[2] >= 0 and row[1] >= row[3] >= 0 and row[4] >= 0
    assert qr.probabilities([0, 0, 0, 0, 0]) == (0.0, 0.0, 1.0)                       # no variance: a polytomy
    empty = qr.rows("gtr", GTR["pi"], GTR["exch"], np.array([np.nan, 0.0]), [(10.0, 1.0)])[0]
    assert np.array_equal(empty, [0, 0, 0, 0, 0, 0, 0, 1])
    assert qr.probabilities([3.0, 0.0, 0.5, 0.0, 0.0])[1] == 0.0                      # X = 0: nothing can mislead


def test_normal_approximation_against_the_exact_distribution():
    """Printed, not asserted beyond sanity: the gap is a property of the approximation (recorded in DESIGN.md section 3.6)."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for n, lo, hi, quartet in ((60, -3.0, -1.0, (30.0, 4.0)), (60, -2.5, -1.5, (50.0, 10.0)), (40, -3.0, -1.0, (30.0, 4.0)),
                               (60, -2.0, -1.0, (100.0, 2.0)), (20, -2.0, -1.0, (20.0, 5.0)), (60, -4.0, -2.0, (20.0, 5.0))):
        r = 10.0 ** rng.uniform(lo, hi, n)
        y, x = qr.site_values("gtr", GTR["pi"], GTR["exch"], r, *quartet)
        s = qr.locus_sums(y, x)
        approx, exact = qr.probabilities(s), qr.exact_resolution(y, x)
        gap = max(abs(a - b) for a, b in zip(approx, exact))
        worst = max(worst, gap)
        print("n=%d T=%g to=%g: Y=%.3f X=%.3f normal %.4f / %.4f / %.4f, exact %.4f / %.4f / %.4f, largest gap %.4f"
              % ((n,) + quartet + (s[0], s[1]) + approx + exact + (gap,)))
        assert abs(sum(exact) - 1.0) < 1e-12 and min(exact) >= -1e-15
    print("largest gap between the normal approximation and the exact distribution: %.4f" % worst)


def test_exact_distribution_on_a_case_done_by_hand():
    # one site: correct iff it is a signal site, incorrect iff it is a noise site of either kind
    pc, pw, pp = qr.exact_resolution([0.3], [0.1])
    assert abs(pc - 0.3) < 1e-15 and abs(pw - 0.2) < 1e-15 and abs(pp - 0.5) < 1e-15
    # two sites with y = 0.5, x = 0.25 each: correct = at least one signal and no noise ahead ...
    pc, pw, pp = qr.exact_resolution([0.5, 0.5], [0.25, 0.25])
    # outcomes (site1, site2) in {S, N1, N2}: SS correct; S+N1 or S+N2: D = (0, 1) or (1, 0): tie; N1N1, N2N2 incorrect; N1N2 tie
    assert abs(pc - 0.25) < 1e-15 and abs(pw - 2 * 0.0625) < 1e-15 and abs(pp - 0.625) < 1e-15


# ---- pipeline and command line on the stand-in engine ------------------------------------------------------------
TREE3 = dict(leaf_names=["a", "b", "c"], parent=[3, 3, 4, 4, -1], blen=[0.1, 0.1, 0.2, 0.1, 0.0], leaf=[0, 1, 2, -1, -1])


def test_quartet_tables_do_not_depend_on_the_shard():
    from tapir_amd import pipeline
    rng = np.random.default_rng(5)
    per_locus = [rng.uniform(0.001, 0.2, n) for n in (30, 1, 17, 0, 64)]
    per_locus[0][3] = np.nan
    per_locus[2][:5] = 0.0
    pi = rng.dirichlet([5] * 4, 5)
    exch = rng.uniform(0.5, 3, (5, 6))
    t = TREE3
    quartets = [(20.0, 5.0), (1.5, 0.25)]
    args = (pipeline.Run(t["leaf_names"], t["parent"], t["blen"], t["leaf"], 12, [], [], device=0), quartets)
    full = pipeline.quartet_tables(quartet_engine, per_locus, pi, exch, *args)
    assert full.shape == (5, 2, 8)
    for ids in ([0, 2, 4], [1, 3], [4]):
        part = pipeline.quartet_tables(quartet_engine, [per_locus[i] for i in ids], pi[ids], exch[ids], *args)
        assert np.array_equal(part, full[ids])
    assert np.array_equal(full[3], [[0, 0, 0, 0, 0, 0, 0, 1]] * 2)                   # the empty locus
    for l in range(5):
        assert np.array_equal(full[l], qr.rows("gtr", pi[l], exch[l], per_locus[l], quartets))
    f81 = pipeline.quartet_tables(quartet_engine, per_locus, pi, None, *args, model="f81")
    assert np.array_equal(f81[0], qr.rows("f81", pi[0], None, per_locus[0], quartets))
    assert pipeline.quartet_tables(quartet_engine, [], pi[:0], exch[:0], *args).shape == (0, 2, 8)


def _synthetic_dir(tmp_path, nloci=4):
    from tapir_amd import synth
    d = synth.simulate(nloci, 40, 5, 3)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    return str(aln), str(tmp_path / "tree.newick")


BASE = ["--times", "10,30", "--intervals", "5-15,20-40", "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"]
QFLAG = ["--quartets", "20:5,10.5:0.25,0:3"]
QNAME = "phylogenetic-informativeness-quartets.sqlite"


def _run(tmp_path, name, aln, tree, extra, base=BASE):
    from tapir_amd import cli
    out = tmp_path / name
    out.mkdir()
    return cli.main([aln, tree, "--output", str(out)] + base + extra, engine_mod=quartet_engine)


def _quartet_rows(path):
    con = sqlite3.connect(path)
    rows = con.execute("select l.locus, q.quartet, q.tip, q.internode, q.signal, q.noise, q.p_correct, q.p_incorrect, q.p_polytomy "
                       "from loci l join quartet q on q.id = l.id order by l.id, q.rowid").fetchall()
    meta = dict(con.execute("select key, value from meta"))
    con.close()
    return rows, meta


def test_cli_writes_the_quartet_database_and_nothing_else_changes(tmp_path):
    import json
    from tapir_amd import nexus
    aln, tree = _synthetic_dir(tmp_path)
    plain = _run(tmp_path, "plain", aln, tree, [])
    del quartet_engine.CALLS[:]
    quart = _run(tmp_path, "quart", aln, tree, QFLAG)
    assert quartet_engine.CALLS == [("quartets", "gtr", [[20.0, 5.0], [10.5, 0.25], [0.0, 3.0]], 4)]
    assert sorted(os.listdir(quart)) == sorted(os.listdir(plain) + [QNAME])
    for f in os.listdir(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(quart, f), "rb").read(), f
    con = sqlite3.connect(os.path.join(quart, QNAME))
    main = sqlite3.connect(os.path.join(quart, "phylogenetic-informativeness.sqlite"))
    tables = {r[0] for r in con.execute("select name from sqlite_master where type = 'table'")} - {"sqlite_sequence"}
    assert tables == {"loci", "quartet", "meta"}
    cols = lambda t: [r[1] for r in con.execute("pragma table_info(%s)" % t)]  # noqa: E731
    assert cols("loci") == ["id", "locus"] and cols("meta") == ["key", "value"]
    assert cols("quartet") == ["id", "quartet", "tip", "internode", "signal", "noise", "p_correct", "p_incorrect", "p_polytomy"]
    loci = con.execute("select * from loci order by id").fetchall()
    assert loci == main.execute("select * from loci order by id").fetchall() and len(loci) == 4
    con.close()
    main.close()
    rows, meta = _quartet_rows(os.path.join(quart, QNAME))
    assert meta["quartets"] == "20:5,10.5:0.25,0:3" and meta["model"] == "gtr"
    assert len(rows) == 12 and [r[1] for r in rows[:3]] == ["20:5", "10.5:0.25", "0:3"]      # as typed
    assert [r[2:4] for r in rows[:3]] == [(20.0, 5.0), (10.5, 0.25), (0.0, 3.0)]
    # the rows are the restatement's on the run's final rates (written corrected_rates, culled below 3 informative cells)
    # under the model the .rates header carries
    for l, (_, name) in enumerate(loci):
        doc = json.load(open(os.path.join(quart, name + ".nex.rates")))["sites"]
        r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
        _, st = nexus.read_states(os.path.join(aln, name + ".nex"))
        r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
        pi = [doc["freqs"][k] for k in "ACGT"]
        exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
        want = qr.rows("gtr", pi, exch, r, [(20.0, 5.0), (10.5, 0.25), (0.0, 3.0)])
        got = np.array([row[4:] for row in rows[3 * l:3 * l + 3]])
        assert np.array_equal(got, want[:, [0, 1, 5, 6, 7]]), name
        assert np.all(got[:, 2:].sum(axis=1) <= 1 + 4 * U) and got[2, 1] == 0.0             # T = 0: no noise


def test_cli_quartets_under_a_fixed_site_model_and_from_rate_files(tmp_path):
    """--site-model f81 carries the F81 plan into the quartet stage; --site-rates reads rates only, so it takes the model
    from --site-model (with the frequencies of the .rates documents) and gives the rows of the run that wrote them."""
    aln, tree = _synthetic_dir(tmp_path)
    base = ["--times", "10,30", "--intervals", "5-15,20-40", "--threshold", "0"]
    del quartet_engine.CALLS[:]
    first = _run(tmp_path, "first", aln, tree, ["--site-model", "f81"] + QFLAG, base=base)
    assert [c[1] for c in quartet_engine.CALLS] == ["f81"]
    rows1, meta1 = _quartet_rows(os.path.join(first, QNAME))
    assert meta1["model"] == "f81"
    rates = tmp_path / "rates"
    rates.mkdir()
    for f in os.listdir(first):
        if f.endswith(".rates"):
            shutil.copy(os.path.join(first, f), rates)
    second = _run(tmp_path, "second", str(rates), tree, ["--site-rates", "--site-model", "f81"] + QFLAG, base=base)
    rows2, meta2 = _quartet_rows(os.path.join(second, QNAME))
    assert meta2["model"] == "f81" and len(rows2) == len(rows1) == 12
    by_name = {(r[0].replace(".nex", ""), r[1]): r for r in rows2}     # (the two runs list their files in their own orders)
    for a in rows1:
        b = by_name[(a[0], a[1])]
        # --threshold 0 culls nothing, and both runs divide the 4-decimal "rate" of the document by the same correction
        assert a[2:] == b[2:], (a, b)
    third = _run(tmp_path, "third", str(rates), tree, ["--site-rates", "--site-model", "jc"] + QFLAG, base=base)
    assert _quartet_rows(os.path.join(third, QNAME))[1]["model"] == "f81" and quartet_engine.CALLS[-1][1] == "f81"


def _argv(tmp_path, golden_dir, *extra):
    return [str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10"] + list(extra)


@pytest.mark.parametrize("value, message", [
    ("20", "Cannot convert quartet '20' to T:to"),
    ("20:5:1", "Cannot convert quartet '20:5:1' to T:to"),
    ("a:5", "Cannot convert quartet 'a:5' to T:to"),
    ("20:0", "the internode length to must be positive"),
    ("20:-1", "the internode length to must be positive"),
    ("-1:5", "the tip length T must not be negative"),
    ("20:5,,3:1", "Cannot convert quartet '' to T:to"),
    ("nan:5", "T and to must be finite"),
    ("3:inf", "T and to must be finite"),
    (",".join(["1:1"] * 257), "--quartets takes 1..256 quartets"),
])
def test_cli_refuses_bad_quartets(tmp_path, golden_dir, value, message, capsys):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args(_argv(tmp_path, golden_dir, "--quartets=" + value))
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err and "unrecognized arguments" not in err


def test_cli_quartet_flag_parses_and_needs_a_model_with_site_rates(tmp_path, golden_dir, capsys):
    from tapir_amd import cli
    assert cli.get_args(_argv(tmp_path, golden_dir)).quartets is None
    a = cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5,50.5:1e-1, 0:2.5"))
    assert a.quartets == [("20:5", 20.0, 5.0), ("50.5:1e-1", 50.5, 0.1), ("0:2.5", 0.0, 2.5)]
    with pytest.raises(SystemExit):
        cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5", "--site-rates"))
    assert "--site-model jc, --site-model f81 or --exchangeabilities" in capsys.readouterr().err
    for model in (["--site-model", "jc"], ["--site-model", "f81"], ["--exchangeabilities", "1,2,1,1,2,1"]):
        assert cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5", "--site-rates", *model)).site_rates
    with pytest.raises(SystemExit):          # without --quartets a fixed site model still cannot join --site-rates
        cli.get_args(_argv(tmp_path, golden_dir, "--site-rates", "--site-model", "jc"))


def test_cli_refuses_a_quartet_deeper_than_the_tree(tmp_path):
    aln, tree = _synthetic_dir(tmp_path)
    with pytest.raises(ValueError, match="exceeds the tree depth"):
        _run(tmp_path, "deep", aln, tree, ["--quartets", "20:5,1e5:1"])
    assert not any(f.endswith(".rates") for f in os.listdir(tmp_path / "deep"))       # refused before any work


_CLI_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import quartet_engine
from tapir_amd import cli
cli.main(%(argv)r, engine_mod=quartet_engine)
'''


def test_cli_two_ranks_gloo_matches_single_process(tmp_path):
    """Five files on two ranks (ragged shards): the gathered quartet rows equal the single-process run's, row for row."""
    import torch  # noqa: F401
    from tapir_amd import cli
    aln, tree = _synthetic_dir(tmp_path, nloci=5)
    outs = []
    for name in ("single", "multi"):
        out = tmp_path / name
        out.mkdir()
        outs.append(out)
    argv = [aln, tree] + BASE + QFLAG + ["--output"]
    single = cli.main(argv + [str(outs[0])], engine_mod=quartet_engine)
    script = tmp_path / "w.py"
    script.write_text(_CLI_WORKER % {"root": ROOT, "argv": argv + [str(outs[1])]})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = _quartet_rows(os.path.join(single, QNAME)), _quartet_rows(os.path.join(str(outs[1]), QNAME))
    assert a == b and len(a[0]) == 15


def test_engine_declares_the_quartet_entry_points():
    """The binding lists the new C entry points with the header's signatures (the struct's layout included)."""
    import ctypes
    from tapir_amd import engine
    names = {s[0] for s in engine.SYMBOLS}
    assert {"tphip_quartet_workspace_bytes", "tphip_quartet_tables", "tphip_quartet_tables_dev", "tphip_quartet_sites",
            "tphip_quartet_sites_dev"} <= names
    assert ctypes.sizeof(engine.QuartetOpts) == 24 and engine.QuartetOpts.tip.offset == 8
    for m in ("quartet_tables", "quartet_sites", "quartet_tables_dev", "quartet_sites_dev", "quartet_workspace_bytes"):
        assert hasattr(engine.Plan, m)
    header = open(os.path.join(ROOT, "include", "tphip.h")).read()
    assert "#define TPHIP_VERSION 110" in header and "tphip_quartet_opts" in header

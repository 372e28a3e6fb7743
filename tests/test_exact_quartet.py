"""The exact quartet resolution probabilities without a GPU: the numpy restatement of the formulas
(tests/exact_quartet_reference.py) against the dynamic programmes, the window rule (python and the host build of the header the
moment kernel compiles), the tiling of the pipeline and the command line through the CPU stand-in engine
(tests/exact_quartet_engine.py)."""
import os
import shutil
import sqlite3
import subprocess

import numpy as np
import pytest

import exact_quartet_engine
import exact_quartet_reference as er
import quartet_reference as qr
import unequal_quartet_reference as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planes(rng, n, scale):
    """y, x1, x2 of n sites with y + x1 + x2 <= 0.95"""
    y, x1, x2 = rng.gamma(1.0, scale, n), rng.gamma(1.0, 0.4 * scale, n), rng.gamma(1.0, 0.3 * scale, n)
    f = np.minimum(1.0, 0.95 / (y + x1 + x2))
    return y * f, x1 * f, x2 * f


# ---- the restatement against the dynamic programmes -----------------------------------------------------------------
@pytest.mark.parametrize("n, scale", [(20, 0.05), (20, 0.3), (40, 0.02), (40, 0.2), (60, 0.01), (60, 0.05), (60, 0.3)])
def test_restatement_against_both_exact_resolutions(n, scale):
    rng = np.random.default_rng(1000 * n + int(1000 * scale))
    y, x1, x2 = _planes(rng, n, scale)
    got = er.resolution(y, x1, x2)
    ref = ur.exact_resolution(y, x1, x2)
    d_unequal = max(abs(a - b) for a, b in zip(got[:4], ref))
    eq = er.resolution(y, x1, x1)
    ref_eq = qr.exact_resolution(y, x1)
    d_equal = max(abs(eq[0] - ref_eq[0]), abs(eq[1] + eq[2] - ref_eq[1]), abs(eq[3] - ref_eq[2]))
    print("n=%d scale=%g: windows %d / %d, tail bounds %.1e / %.1e, against the DPs %.2e (unequal) %.2e (equal)"
          % (n, scale, got[4], eq[4], got[5], eq[5], d_unequal, d_equal))
    assert got[4] in (64, 128) and eq[4] in (64, 128) and got[5] <= 1e-12 and eq[5] <= 1e-12
    assert d_unequal <= 1e-13 and d_equal <= 1e-13
    assert abs(eq[1] - eq[2]) <= 1e-14                   # equal tips: the two wrong topologies are one


@pytest.mark.parametrize("n, scale", [(700, 0.02), (2000, 0.004), (2000, 0.001)])
def test_restatement_against_the_windowed_dp(n, scale):
    rng = np.random.default_rng(n + int(1e4 * scale))
    y, x1, x2 = _planes(rng, n, scale)
    got = er.resolution(y, x1, x2)
    ref = er.windowed_dp(y, x1, x2)
    d = max(abs(a - b) for a, b in zip(got[:4], ref[:4]))
    print("n=%d scale=%g: window %d, tail bound %.1e, DP lost %.1e, difference %.2e" % (n, scale, got[4], got[5], ref[4], d))
    assert got[4] in (64, 128) and got[5] <= 1e-12
    assert d <= 1e-12 + ref[4]


def test_windowed_dp_is_the_plain_dp_on_short_loci():
    rng = np.random.default_rng(3)
    y, x1, x2 = _planes(rng, 60, 0.1)
    a, b = er.windowed_dp(y, x1, x2), ur.exact_resolution(y, x1, x2)
    assert a[4] <= 1e-15 and max(abs(u - v) for u, v in zip(a[:4], b)) <= 1e-14


def test_point_laws_and_the_window_wholly_inside_a_region():
    assert er.resolution(np.zeros(7), np.zeros(7), np.zeros(7)) == (0.0, 0.0, 0.0, 1.0, 16, 0.0)
    one = np.array([1.0, 0.0, 1.0, 0.0])
    assert er.resolution(one, 0 * one, 0 * one) == (1.0, 0.0, 0.0, 0.0, 16, 0.0)
    assert er.resolution(0 * one, one, 0 * one) == (0.0, 1.0, 0.0, 0.0, 16, 0.0)
    assert er.resolution(0 * one, 0 * one, one) == (0.0, 0.0, 1.0, 0.0, 16, 0.0)
    assert er.resolution(one, one[::-1], 0 * one) == (0.0, 0.0, 0.0, 1.0, 16, 0.0)      # S = N1 = 2: a tie
    # 60 sites with y = 0.9: the window of D1 and D2 lies wholly above 0
    y, x1, x2 = np.full(60, 0.9), np.full(60, 0.03), np.full(60, 0.02)
    got, ref = er.resolution(y, x1, x2), ur.exact_resolution(y, x1, x2)
    assert got[4] == 128 and max(abs(a - b) for a, b in zip(got[:4], ref)) <= 1e-12


# ---- the window rule ------------------------------------------------------------------------------------------------
def test_window_rule_is_monotone_and_meets_its_tolerance():
    last = 0
    for v in np.concatenate([[0.0], 10.0 ** np.linspace(-6, 3.2, 400)]):
        M, b = er.window_rule((v, 0.7 * v, 0.2 * v), cap=512)
        if M == 0:
            assert b > 1e-12 and b == er.tail_bound((v, 0.7 * v, 0.2 * v), 512)
            last = 1024
            continue
        assert M >= last and b <= 1e-12 and b == er.tail_bound((v, 0.7 * v, 0.2 * v), M)
        assert M == 16 or er.tail_bound((v, 0.7 * v, 0.2 * v), M // 2) > 1e-12        # the smallest that qualifies
        last = M
    assert last == 1024
    pick = lambda v, cap=512: er.window_rule((v, v, v), cap)[0]  # noqa: E731
    assert pick(0.0) == 16 and pick(1e-9) == 64          # any variance at all: t / 3 alone rules out 16 and 32
    assert [pick(v) for v in (5, 10, 40, 60, 200, 300, 900, 1500)] == [64, 128, 128, 256, 256, 512, 512, 0]
    assert pick(40, 128) == 128 and pick(60, 128) == 0 and pick(5, 32) == 0
    assert er.window_rule((23.0, 20.0, 5.0), cap=32)[1] > 1e-12
    assert er.window_rule((5.0, 5.0, 5.0), tol=1e-30)[0] == 128 and er.window_rule((5.0, 5.0, 5.0), tol=1e-6)[0] == 64


@pytest.fixture(scope="module")
def window_exe(tmp_path_factory):
    """tests/native/exact_window_dump.cpp: a host build of tapir_amd/csrc/exact_quartet_window.hpp"""
    exe = str(tmp_path_factory.mktemp("eqwin") / "exact_window_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tapir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "exact_window_dump.cpp"), "-o", exe])
    return exe


def test_the_header_the_kernel_compiles_states_the_same_rule(window_exe):
    rng = np.random.default_rng(9)
    cases = [(0.0, 0.0, 0.0, 128, 1e-12), (0.0, 3.0, 0.0, 128, 1e-12), (23.0, 20.0, 5.0, 32, 1e-12), (2000.0, 1.0, 1.0, 512, 1e-12)]
    for _ in range(200):
        v = 10.0 ** rng.uniform(-3, 3.2, 3)
        cases.append((v[0], v[1], v[2], int(2 ** rng.integers(4, 10)), float(10.0 ** rng.uniform(-15, -6))))
    text = "".join("%.17g %.17g %.17g %d %.17g\n" % c for c in cases)
    out = subprocess.run([window_exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    for c, line in zip(cases, out):
        M, bound = line.split()
        want_M, want_b = er.window_rule(c[:3], c[3], c[4])
        margin = min(abs(er.tail_bound(c[:3], m) / c[4] - 1) for m in (16, 32, 64, 128, 256, 512))
        if margin > 1e-9:                                 # (not a tie between the two exp)
            assert int(M) == want_M, c
            assert abs(float(bound) - want_b) <= 1e-12 * want_b, c
    assert subprocess.run([window_exe], input="1 1 1 48 1e-12\n1 1 1 1024 1e-12\n", capture_output=True, text=True,
                          check=True).stdout.split() == ["invalid", "invalid"]


# ---- the pipeline's tiles -------------------------------------------------------------------------------------------
def test_tiles_keep_planes_and_workspace_within_the_bound():
    from tapir_amd import pipeline
    B = pipeline.EXACT_QUARTET_BYTES
    assert B == 256 << 20
    assert pipeline.exact_quartet_tile(1000, 500000, 100, 2, 128) == 33            # planes: 2 x 33 x 500000 x 8 <= 256 MiB
    assert 8 * 2 * 33 * 500000 <= B < 8 * 2 * 34 * 500000
    assert pipeline.exact_quartet_tile(1000, 500000, 100, 3, 128) == 22
    assert pipeline.exact_quartet_tile(10, 600, 300, 3, 128) == 256                # the engine's limit
    assert pipeline.exact_quartet_tile(10, 600, 7, 3, 128) == 7
    assert pipeline.exact_quartet_tile(100000, 100, 100, 2, 512) == 1              # workspace: 6200 bytes a pair at cap 512
    assert pipeline.exact_quartet_tile(100000, 100, 100, 2, 128) == 6              # 440 bytes a pair at cap 128
    assert 100000 * 6 * 440 <= B < 100000 * 7 * 440
    assert pipeline.exact_quartet_tile(1, 10 ** 9, 5, 2, 128) == 1                 # at least one


def test_tiled_rows_equal_untiled_rows(monkeypatch):
    from tapir_amd import pipeline
    rng = np.random.default_rng(4)
    per_locus = [10.0 ** rng.uniform(-3, -1, n) for n in (7, 30, 1, 19)]
    per_locus[1][3] = np.nan
    pi = rng.dirichlet([5.0] * 4, 4)
    exch = rng.uniform(0.5, 2.0, (4, 6))
    tree = ([3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1])
    q2 = np.array([[20.0, 5.0], [0.0, 3.0], [35.0, 1.0], [7.0, 7.0], [50.0, 0.5]])
    q5 = np.array([[20.0, 22.0, 25.0, 30.0, 5.0], [1.0, 0.0, 3.0, 40.0, 2.0], [9.0, 9.0, 9.0, 9.0, 4.0]])
    args = (exact_quartet_engine, per_locus, pi, exch, pipeline.Run(["a", "b", "c"], *tree, 8, [], [], device=0))
    whole = pipeline.exact_quartet_tables(*args, q2), pipeline.exact_unequal_quartet_tables(*args, q5)
    assert whole[0].shape == (4, 5, 6) and whole[1].shape == (4, 3, 6)
    del exact_quartet_engine.CALLS[:]
    monkeypatch.setattr(pipeline, "EXACT_QUARTET_BYTES", 2 * 4 * 440)              # the workspace of two quartets of four loci
    tiled = pipeline.exact_quartet_tables(*args, q2), pipeline.exact_unequal_quartet_tables(*args, q5)
    assert [c[1] for c in exact_quartet_engine.CALLS] == [2, 2, 1, 2, 1]
    assert np.array_equal(whole[0], tiled[0]) and np.array_equal(whole[1], tiled[1])
    assert np.all(whole[0][:, :, 4] > 0) and np.all(np.abs(whole[0][:, :, :4].sum(axis=2) - 1) <= 1e-12)
    assert pipeline.exact_quartet_tables(exact_quartet_engine, [], pi[:0], exch[:0], args[4], q2).shape == (0, 5, 6)


# ---- the command line -----------------------------------------------------------------------------------------------
def _synthetic_dir(tmp_path, nloci=3):
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
    return cli.main([aln, tree, "--output", str(out)] + BASE + extra, engine_mod=exact_quartet_engine)


def _table(con, name):
    return con.execute("select * from %s order by rowid" % name).fetchall()


def test_cli_adds_the_tables_and_changes_nothing_without_the_flag(tmp_path):
    import json
    from tapir_amd import compute, newick, nexus
    aln, tree = _synthetic_dir(tmp_path)
    plain = _run(tmp_path, "plain", aln, tree, QFLAGS)
    exact = _run(tmp_path, "exact", aln, tree, QFLAGS + ["--exact-quartets"])
    small = _run(tmp_path, "small", aln, tree, QFLAGS + ["--exact-quartets", "--exact-quartets-window", "32"])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(exact))
    for f in os.listdir(plain):
        same = open(os.path.join(plain, f), "rb").read() == open(os.path.join(exact, f), "rb").read()
        assert same == (f not in (QNAME, UNAME)), f           # every other output: byte for byte
    of_tree = compute.tree_quartets(newick.read_tree(tree))
    for name, unequal in ((QNAME, False), (UNAME, True)):
        old, new, cut = (sqlite3.connect(os.path.join(d, name)) for d in (plain, exact, small))
        tables = lambda con: {r[0] for r in con.execute("select name from sqlite_master where type = 'table'")} - {"sqlite_sequence"}  # noqa: E731
        assert tables(new) == tables(old) | {"quartet_exact"} and "quartet_exact" not in tables(old)
        for t in tables(old) - {"meta"}:                      # what the file holds without the flag is still there, unchanged
            assert _table(old, t) == _table(new, t), t
        meta_old, meta_new = dict(_table(old, "meta")), dict(_table(new, "meta"))
        assert {k: meta_new[k] for k in meta_old} == meta_old
        assert set(meta_new) - set(meta_old) == {"exact", "exact_window_cap", "exact_tail_tolerance"}
        assert meta_new["exact_window_cap"] == "128" and meta_new["exact_tail_tolerance"] == "1e-12"
        assert dict(_table(cut, "meta"))["exact_window_cap"] == "32"
        cols = [r[1] for r in new.execute("pragma table_info(quartet_exact)")]
        wrong = ["p_ac", "p_ad"] if unequal else ["p_incorrect"]
        assert cols == ["id", "quartet", "p_correct"] + wrong + ["p_polytomy", "window", "tail_bound"]
        rows = _table(new, "quartet_exact")
        labels = ["100/5/100/5:2"] + [q[0] for q in of_tree] if unequal else ["20:5", "0:3"]
        lengths = [[100.0, 5.0, 100.0, 5.0, 2.0]] + [list(q[2:]) for q in of_tree] if unequal else [[20.0, 5.0], [0.0, 3.0]]
        loci = _table(new, "loci")
        assert [(r[0], r[1]) for r in rows] == [(i, lab) for i, _ in loci for lab in labels]
        worst = 0.0
        for l, (key, locus) in enumerate(loci):
            doc = json.load(open(os.path.join(exact, locus + ".nex.rates")))["sites"]
            r = np.array([x["rate"] for x in doc["corrected_rates"]], dtype=np.float64)
            _, st = nexus.read_states(os.path.join(aln, locus + ".nex"))
            r = np.where(np.isin(st & 15, [1, 2, 4, 8]).sum(axis=0) >= 3, r, np.nan)
            pi = [doc["freqs"][k] for k in "ACGT"]
            exch = [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]
            for q, row in enumerate(lengths):
                got = rows[l * len(labels) + q]
                if unequal:
                    y, x1, x2 = ur.site_values("gtr", pi, exch, r, row[:4], row[4])
                    want = ur.exact_resolution(y, x1, x2)
                else:
                    y, x = qr.site_values("gtr", pi, exch, r, row[0], row[1])
                    want = qr.exact_resolution(y, x)
                assert got[-2] in (16, 64, 128) and got[-1] <= 1e-12
                worst = max(worst, max(abs(a - b) for a, b in zip(got[2:-2], want)))
        assert worst <= 1e-12, worst
        # a cap of 32 holds point laws only: everything else is reported as not computed, never truncated
        for got in _table(cut, "quartet_exact"):
            assert (got[-2] == 0 and all(v is None for v in got[2:-2]) and got[-1] > 1e-12) or (got[-2] == 16 and got[-1] == 0.0)
        assert any(got[-2] == 0 for got in _table(cut, "quartet_exact"))
        for con in (old, new, cut):
            con.close()
    # one kind of quartet alone: only its file gains the table
    only = _run(tmp_path, "only", aln, tree, ["--tree-quartets", "--exact-quartets"])
    assert QNAME not in os.listdir(only)
    con = sqlite3.connect(os.path.join(only, UNAME))
    assert len(_table(con, "quartet_exact")) == 3 * len(of_tree)
    con.close()


def _argv(tmp_path, golden_dir, *extra):
    return [str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10"] + list(extra)


def test_cli_flags_parse_and_argument_errors_fire_before_any_work(tmp_path, golden_dir, capsys):
    from tapir_amd import cli
    a = cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5"))
    assert a.exact_quartets is False and a.exact_quartets_window is None
    a = cli.get_args(_argv(tmp_path, golden_dir, "--quartets", "20:5", "--exact-quartets"))
    assert a.exact_quartets is True and a.exact_quartets_window == 128
    for flags in (["--unequal-quartets", "1/2/3/4:5"], ["--tree-quartets"]):
        assert cli.get_args(_argv(tmp_path, golden_dir, "--exact-quartets", "--exact-quartets-window", "512", *flags)).exact_quartets_window == 512
    for extra, message in ((["--exact-quartets"], "--exact-quartets needs --quartets, --unequal-quartets or --tree-quartets"),
                           (["--bootstrap", "10", "--exact-quartets"], "--exact-quartets needs --quartets"),
                           (["--quartets", "20:5", "--exact-quartets-window", "64"], "--exact-quartets-window needs --exact-quartets"),
                           (["--quartets", "20:5", "--exact-quartets", "--exact-quartets-window", "48"], "a power of two in 16..512"),
                           (["--quartets", "20:5", "--exact-quartets", "--exact-quartets-window", "8"], "a power of two in 16..512"),
                           (["--quartets", "20:5", "--exact-quartets", "--exact-quartets-window", "1024"], "a power of two in 16..512"),
                           (["--quartets", "20:5", "--exact-quartets", "--exact-quartets-window", "x"], "invalid int value")):
        with pytest.raises(SystemExit) as e:
            cli.get_args(_argv(tmp_path, golden_dir, *extra))
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err, (extra, err)


def test_engine_and_header_declare_the_entry_points():
    import ctypes
    from tapir_amd import engine
    names = {s[0] for s in engine.SYMBOLS}
    entry = {"tphip_quartet_exact_workspace_bytes", "tphip_quartet_exact_dev", "tphip_quartet_exact"}
    assert entry <= names
    assert ctypes.sizeof(engine.QuartetExactOpts) == 24 and engine.QuartetExactOpts.window_cap.offset == 8
    assert engine.QuartetExactOpts.tail_tolerance.offset == 16
    for m in ("quartet_exact", "quartet_exact_dev", "quartet_exact_workspace_bytes"):
        assert hasattr(engine.Plan, m)
    header = open(os.path.join(ROOT, "include", "tphip.h")).read()
    assert "#define TPHIP_VERSION 110" in header and "tphip_quartet_exact_opts" in header
    for name in entry:
        assert "int %s(" % name in header
    assert os.path.exists(os.path.join(ROOT, "tapir_amd", "csrc", "exact_quartet_driver.hip"))
    import __graft_entry__ as ge
    unit = [u for u in ge.HIP_UNITS if u["src"] == "exact_quartet_driver.hip"]
    assert len(unit) == 1 and unit[0]["flags"] == []      # the compiler's defaults, as the quartet units

"""Site bootstrap of the PI rows without a GPU: the generator's definition (tests/bootstrap_reference.py against the known
answers of Philox4x32-10), and the host layers above the engine -- pipeline.bootstrap_tables, the --bootstrap flags and the
second sqlite file -- on the CPU stand-in engine (tests/bootstrap_engine.py)."""
import os
import shutil
import sqlite3
import subprocess

import numpy as np
import pytest

import bootstrap_engine
import bootstrap_reference as bsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    out = bsr.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert " ".join("%08x" % int(v) for v in out) == want


@pytest.fixture(scope="module")
def philox_exe(tmp_path_factory):
    """tests/native/philox_kat.cpp: a host build of tapir_amd/csrc/philox4x32.hpp, the generator the draw kernel runs."""
    exe = str(tmp_path_factory.mktemp("philox") / "philox_kat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tapir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "philox_kat.cpp"), "-o", exe])
    return exe


def test_library_generator_meets_the_known_answers_and_the_reference_draws(philox_exe):
    """The C++ the kernel compiles: the three known answers, and the draws of the numpy restatement for odd and even n,
    a 64-bit seed and a 64-bit locus id."""
    cases = [(1, 0, 0, 1), (1, 0, 3, 2), (7, 5, 2, 227), (2 ** 40 + 7, 2 ** 33 + 1, 4095, 64), (2 ** 64 - 1, 2 ** 63 + 5, 9, 1025)]
    text = ("kat 0 0 0 0 0 0\nkat ffffffff ffffffff ffffffff ffffffff ffffffff ffffffff\n"
            "kat 243f6a88 85a308d3 13198a2e 03707344 a4093822 299f31d0\n" +
            "".join("draws %d %d %d %d\n" % c for c in cases))
    out = subprocess.run([philox_exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert out[:3] == ["6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd",
                       "d16cfe09 94fdcceb 5001e420 24126ea1"]
    for line, (seed, lid, b, n) in zip(out[3:], cases):
        assert [int(v) for v in line.split()] == bsr.draws(seed, lid, b, n), (seed, lid, b, n)


def test_philox_is_vectorised_over_counters():
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], np.uint64)
    key = np.array([[0, 0], [0xFFFFFFFF] * 2], np.uint64)
    out = bsr.philox4x32_10(ctr, key)
    assert "%08x" % int(out[0, 0]) == "6627e8d5" and "%08x" % int(out[1, 3]) == "6d5451fd"


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 226])
def test_counts_sum_to_the_locus_length(n):
    c = bsr.counts(1, 0, n, 0, 7)
    assert c.shape == (7, n) and c.dtype == np.uint16 and np.all(c.sum(axis=1) == n)
    if n == 1:
        assert np.all(c == 1)
    assert np.array_equal(bsr.counts(1, 0, n, 5, 2), c[5:7])      # every draw is addressable: a slice is the same rows


def test_draws_are_uniform_indices_and_odd_lengths_discard_one():
    d = bsr.draws(3, 9, 2, 227)
    assert len(d) == 227 and min(d) >= 0 and max(d) < 227
    assert bsr.draws(3, 9, 2, 228)[:226] != d[:226]               # n enters every draw
    assert bsr.draws(3, 9, 2, 0) == []


def test_seed_and_locus_id_use_all_64_bits():
    base = bsr.counts(7, 1, 226, 0, 2)
    assert not np.array_equal(bsr.counts(2 ** 32 + 7, 1, 226, 0, 2), base)
    assert not np.array_equal(bsr.counts(7, 2 ** 32 + 1, 226, 0, 2), base)
    assert not np.array_equal(bsr.counts(7, 1, 226, 1, 2)[0], base[0]) and np.array_equal(bsr.counts(7, 1, 226, 1, 1)[0], base[1])


def test_summary_is_numpys():
    rng = np.random.default_rng(1)
    rows = rng.random((50, 3))
    s = bsr.summarize(rows, 0.9)
    assert np.allclose(s[0], rows.mean(axis=0)) and np.allclose(s[1], rows.std(axis=0, ddof=1))
    assert np.array_equal(s[2], np.quantile(rows, (1 - 0.9) / 2, axis=0)) and np.all(s[2] <= s[3])


# ---- pipeline and command line on the stand-in engine ------------------------------------------------------------
TREE3 = dict(leaf_names=["a", "b", "c"], parent=[3, 3, 4, 4, -1], blen=[0.1, 0.1, 0.2, 0.1, 0.0], leaf=[0, 1, 2, -1, -1])


def _final_rates():
    rng = np.random.default_rng(5)
    per_locus = [rng.uniform(0.001, 0.2, n) for n in (30, 1, 17, 0, 64)]
    per_locus[0][3] = np.nan
    per_locus[2][:5] = 0.0
    return per_locus


def test_bootstrap_tables_do_not_depend_on_the_shard():
    """A rank's loci with their global ids give the rows of the full run: what makes the bands independent of the world size."""
    from tapir_amd import pipeline
    per_locus = _final_rates()
    t = TREE3
    args = (pipeline.Run(t["leaf_names"], t["parent"], t["blen"], t["leaf"], 12, [], [[0, 5], [3, 12]], device=0, integ_mode=1),)
    full = pipeline.bootstrap_tables(bootstrap_engine, per_locus, *args, locus_ids=np.arange(5), replicates=16, seed=3, level=0.9)
    assert full.shape == (5, 4, 14)
    for ids in ([0, 2, 4], [1, 3], [4]):
        part = pipeline.bootstrap_tables(bootstrap_engine, [per_locus[i] for i in ids], *args, locus_ids=ids, replicates=16,
                                         seed=3, level=0.9)
        assert np.array_equal(part, full[ids])
    other = pipeline.bootstrap_tables(bootstrap_engine, per_locus[:1], *args, locus_ids=[1], replicates=16, seed=3, level=0.9)
    assert not np.array_equal(other[0], full[0])
    assert np.all(full[3] == 0.0)                                 # the empty locus
    assert np.all(full[:, 2] <= full[:, 0] * (1 + 1e-15)) and np.all(full[:, 0] <= full[:, 3] * (1 + 1e-15))   # lo <= mean <= hi
    assert pipeline.bootstrap_tables(bootstrap_engine, [], *args, locus_ids=[], replicates=16).shape == (0, 4, 14)


def _synthetic_dir(tmp_path):
    from tapir_amd import synth
    d = synth.simulate(4, 40, 5, 3)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    return str(aln), str(tmp_path / "tree.newick")


def _run(tmp_path, name, aln, tree, extra):
    from tapir_amd import cli
    out = tmp_path / name
    out.mkdir()
    return cli.main([aln, tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                     "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"] + extra, engine_mod=bootstrap_engine)


def test_cli_writes_the_bootstrap_database_and_nothing_else_changes(tmp_path):
    aln, tree = _synthetic_dir(tmp_path)
    plain = _run(tmp_path, "plain", aln, tree, [])
    del bootstrap_engine.CALLS[:]
    boot = _run(tmp_path, "boot", aln, tree, ["--bootstrap", "8", "--bootstrap-seed", str(2 ** 40 + 7), "--bootstrap-level", "0.8"])
    assert bootstrap_engine.CALLS == [("bootstrap", 8, 2 ** 40 + 7, 0.8, [0, 1, 2, 3])]
    name = "phylogenetic-informativeness-bootstrap.sqlite"
    assert sorted(os.listdir(boot)) == sorted(os.listdir(plain) + [name])
    for f in os.listdir(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(boot, f), "rb").read(), f
    con = sqlite3.connect(os.path.join(boot, name))
    main = sqlite3.connect(os.path.join(boot, "phylogenetic-informativeness.sqlite"))
    tables = {r[0] for r in con.execute("select name from sqlite_master where type = 'table'")} - {"sqlite_sequence"}
    assert tables == {"loci", "net_bootstrap", "discrete_bootstrap", "interval_bootstrap", "meta"}
    cols = lambda t: [r[1] for r in con.execute("pragma table_info(%s)" % t)]  # noqa: E731
    assert cols("loci") == ["id", "locus"] and cols("meta") == ["key", "value"]
    assert cols("net_bootstrap") == cols("discrete_bootstrap") == ["id", "time", "mean", "sd", "lo", "hi"]
    assert cols("interval_bootstrap") == ["id", "interval", "mean", "sd", "lo", "hi"]
    assert con.execute("select * from loci order by id").fetchall() == main.execute("select * from loci order by id").fetchall()
    T = main.execute("select count(*) from net where id = 1").fetchone()[0]
    count = lambda t: con.execute("select count(*) from %s" % t).fetchone()[0]  # noqa: E731
    assert (count("loci"), count("net_bootstrap"), count("discrete_bootstrap"), count("interval_bootstrap")) == (4, 4 * T, 8, 8)
    assert dict(con.execute("select key, value from meta")) == {"replicates": "8", "seed": str(2 ** 40 + 7), "level": "0.8"}
    assert [r[0] for r in con.execute("select interval from interval_bootstrap where id = 2 order by rowid")] == ["5-15", "20-40"]
    # --times rows are the net rows at those times; the band brackets the mean; the point estimate is of the mean's size
    for lid in (1, 4):
        net = dict((t, r) for t, *r in con.execute("select time, mean, sd, lo, hi from net_bootstrap where id = ?", (lid,)))
        for t, *r in con.execute("select time, mean, sd, lo, hi from discrete_bootstrap where id = ?", (lid,)):
            assert net[t] == r
        for t, (mean, sd, lo, hi) in net.items():
            assert lo <= mean <= hi and sd >= 0
        point = dict(main.execute("select time, pi from net where id = ?", (lid,)))
        assert abs(net[10][0] - point[10]) < 6 * net[10][1] + 1e-300
    con.close()
    main.close()


@pytest.mark.parametrize("extra, message", [
    (["--bootstrap", "1"], "--bootstrap must be in 2..4096"),
    (["--bootstrap", "4097"], "--bootstrap must be in 2..4096"),
    (["--bootstrap", "-3"], "--bootstrap must be in 2..4096"),
    (["--bootstrap", "10", "--bootstrap-level", "0"], "--bootstrap-level must be in (0, 1)"),
    (["--bootstrap", "10", "--bootstrap-level", "1"], "--bootstrap-level must be in (0, 1)"),
    (["--bootstrap", "10", "--bootstrap-level", "1.5"], "--bootstrap-level must be in (0, 1)"),
    (["--bootstrap-seed", "3"], "--bootstrap-seed needs --bootstrap"),
    (["--bootstrap-level", "0.9"], "--bootstrap-level needs --bootstrap"),
    (["--bootstrap", "10", "--bootstrap-seed", "-1"], "--bootstrap-seed must be in 0..2^64-1"),
    (["--bootstrap", "10", "--bootstrap-seed", str(2 ** 64)], "--bootstrap-seed must be in 0..2^64-1"),
])
def test_cli_refuses_bad_bootstrap_flags(tmp_path, golden_dir, extra, message, capsys):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args([str(tmp_path), os.path.join(golden_dir, "Euteleost.tree"), "--times", "10", "--intervals", "0-10"] + extra)
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err and "unrecognized arguments" not in err


def test_cli_bootstrap_defaults():
    from tapir_amd import cli
    a = cli.get_args([ROOT, os.path.join(ROOT, "tests", "golden", "Euteleost.tree"), "--times", "10", "--intervals", "0-10"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level) == (0, None, None)
    a = cli.get_args([ROOT, os.path.join(ROOT, "tests", "golden", "Euteleost.tree"), "--times", "10", "--intervals", "0-10",
                      "--bootstrap", "200"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level) == (200, 1, 0.95)


def test_engine_declares_the_bootstrap_entry_points():
    """The binding lists the new C entry points with the header's signatures (the struct's layout included)."""
    import ctypes
    from tapir_amd import engine
    names = {s[0] for s in engine.SYMBOLS}
    assert {"tphip_bootstrap_width", "tphip_bootstrap_workspace_bytes", "tphip_pi_resample_dev", "tphip_pi_bootstrap_dev",
            "tphip_pi_resample", "tphip_pi_bootstrap", "tphip_bootstrap_counts"} <= names
    assert ctypes.sizeof(engine.BootstrapOpts) == 32 and engine.BootstrapOpts.seed.offset == 16
    for m in ("pi_bootstrap", "pi_resample", "pi_bootstrap_dev", "pi_resample_dev", "bootstrap_workspace_bytes"):
        assert hasattr(engine.Plan, m)
    assert callable(engine.bootstrap_counts)

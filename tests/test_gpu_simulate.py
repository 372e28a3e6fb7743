"""Parametric bootstrap on the GPU (tphip_simulate_columns, tphip_pi_parametric_bootstrap, tphip_summarize_rows,
--parametric-bootstrap) against tests/simulate_reference.py.  Run with -m gpu on the MI355X box.  Every test prints its figures
before it asserts.

Bounds (stated by the definition, none tuned to the kernels):
  bytes           a draw is decided when the mirror has |v - c_k| > 1e-12 c3 for every k; a cell whose path from the root has
                  only decided draws must match exactly; at most 1e-6 of all draws may be undecided (the mirror alone, on the
                  CPU, has none on these inputs)
  distribution    max |z| <= 5 over the 16 joint frequencies of 65 536 two-taxon columns (tests/test_simulate.py)
  composition     rows of the driver = tables of run_fused on simulate_columns, bit for bit; moments against numpy over the same
                  replicates: mean (B + 2) 2^-52 relative, sd 8 B 2^-52 max |rate| absolute, NaN exactly on the culled columns
  summary         the bounds of test_gpu_bootstrap.py::test_summary_against_numpy
"""
import functools
import json
import os
import sqlite3

import numpy as np
import pytest

import bootstrap_reference as bsr
import simulate_reference as sim

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SIZES = [1, 63, 64, 65, 1025]            # a lone column, the wave boundaries, a PI-chunk boundary
IDS = [0, 5, 2 ** 33 + 11, 7, 2 ** 40 + 1]
BIG_SIZES = [1, 63, 64, 65, 129, 257, 1025]      # and the boundaries of blocks of 128 and 256 threads
BIG_IDS = IDS + [2 ** 63 - 1, 12]
MASK_CODES = np.array([1, 2, 4, 8, 15, 0, 5, 10, 14], np.uint8)
# (replicate, seed, with mask)
RUNS = [(0, 1, True), (1, 2 ** 40 + 7, False), (4095, 1, True), (1, 1, False)]


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


# Yule trees at the edges of the launch shape (simulate_launch_shape.hpp, tests/test_sim_launch.py), by internal nodes = taxa - 1:
# 769 the first launch above 48 KiB of LDS, 2561 the first block of 128, 5121 the first block of 64, 10240 the last tree taken
BIG_TREES = {"yule770": 770, "yule2562": 2562, "yule5122": 5122, "yule10241": 10241}
BIG_RUNS = [0, 1]            # of RUNS: one with the mask, one without


@functools.lru_cache(maxsize=None)
def tree_arrays(name):
    """(ntaxa, parent, blen, leaf)"""
    if name == "two":
        return 2, [2, 2, -1], [0.7, 0.4, 0.0], [0, 1, -1]
    if name == "trifurcation":
        return 3, [3, 3, 3, -1], [0.5, 0.05, 1.5, 0.0], [2, 0, 1, -1]
    if name == "caterpillar17":       # 33 nodes: an odd count, 16 internal nodes below the root: the packed states cross a word
        return (17,) + sim.caterpillar(17)
    from tapir_amd import synth
    ntaxa = BIG_TREES.get(name, 70)
    root, names = synth.yule_tree(ntaxa, 4)
    pin = synth.plan_inputs(root, names)
    return ntaxa, pin["parent"], pin["blen"], pin["leaf"]


def locus_models(kind, L):
    rng = np.random.default_rng(11)
    pi = rng.dirichlet([2.0] * 4, size=L)
    pi[0] = [0.05, 0.45, 0.2, 0.3]
    exch = np.concatenate([rng.lognormal(0.0, 0.5, size=(L, 1)), np.ones((L, 1)), rng.lognormal(0.0, 0.5, size=(L, 4))], axis=1)
    if kind == "f81":
        return pi, None, [sim.f81_system(p) for p in pi]
    return pi, exch, [sim.eigen_system(p, e) for p, e in zip(pi, exch)]


def byte_case(tree, kind):
    """The inputs of the byte comparison: every rate of the list in every locus that has room for them."""
    ntaxa, parent, blen, leaf = tree_arrays(tree)
    sizes, ids = (BIG_SIZES, BIG_IDS) if tree in BIG_TREES else (SIZES, IDS)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pi, exch, models = locus_models(kind, len(sizes))
    rates = np.empty(off[-1])
    for l, m in enumerate(models):
        pattern = np.array([0.0, 1e-9, 0.01, 1.0, 1e4 * m["kappa"], np.nan, -1.0])
        rates[off[l]:off[l + 1]] = pattern[(np.arange(sizes[l]) + l) % len(pattern)]
    mask = np.random.default_rng(5).choice(MASK_CODES, size=(ntaxa, int(off[-1])))
    return dict(ntaxa=ntaxa, parent=parent, blen=blen, leaf=leaf, off=off, pi=pi, exch=exch, models=models, rates=rates, mask=mask,
                ids=ids, big=tree in BIG_TREES)


def mirror(c, b, seed, with_mask):
    """(the big trees: every locus advanced together, simulate_reference.simulate_all_loci -- seconds where simulate takes minutes)"""
    run = sim.simulate_all_loci if c["big"] else sim.simulate
    return run(c["parent"], c["blen"], c["leaf"], c["ntaxa"], c["off"], c["models"], c["rates"], locus_ids=c["ids"], b=b, seed=seed,
               mask=c["mask"] if with_mask else None)


def _sim_plan(engine, c, kind, **kw):
    return engine.Plan(c["ntaxa"], c["parent"], c["blen"], c["leaf"], c["off"], c["pi"], c["exch"], 5, [], [], model=kind, **kw)


# ---- 1. bytes against the mirror ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
@pytest.mark.parametrize("tree", ["two", "trifurcation", "caterpillar17", "yule70"] + sorted(BIG_TREES, key=BIG_TREES.get))
def test_bytes_equal_the_mirror(tree, kind):
    """The four small trees: loci of SIZES columns, all four RUNS.  The Yule trees of BIG_TREES: loci of BIG_SIZES columns and the
    two runs of BIG_RUNS; with them every launch shape of the simulation has produced bytes -- more than 48 KiB of LDS (769
    internal nodes), blocks of 128 (2561) and of 64 threads (5121), and the largest tree taken (10240: 160 KiB).  The mirror alone
    has no undecided draw on any of these inputs (tests/test_simulate.py runs it on the first of them)."""
    engine = _engine()
    c = byte_case(tree, kind)
    runs = [RUNS[k] for k in BIG_RUNS] if c["big"] else RUNS
    plan = _sim_plan(engine, c, kind)
    try:
        got = [plan.simulate_columns(c["rates"], mask=c["mask"] if m else None, replicate=b, seed=seed, locus_ids=c["ids"])
               for b, seed, m in runs]
    finally:
        plan.close()
    draws = undecided = 0
    for (b, seed, m), g in zip(runs, got):
        ref = mirror(c, b, seed, m)
        draws += ref["draws"]
        undecided += ref["undecided"]
        wrong = int((g != ref["states"])[ref["sure"]].sum())
        loose = int((g != ref["states"])[~ref["sure"]].sum())
        print("%s %s b=%d seed=%d mask=%s: %d cells, %d sure, %d sure cells differ, %d unsure cells differ"
              % (tree, kind, b, seed, m, g.size, int(ref["sure"].sum()), wrong, loose))
        assert wrong == 0
    print("%s %s: %d draws, %d undecided" % (tree, kind, draws, undecided))
    assert undecided <= 1e-6 * draws
    if not c["big"]:
        assert not np.array_equal(got[1], got[3])      # another seed, same replicate: other bytes


def test_a_tree_of_10241_internal_nodes_is_refused():
    """One internal node more than 64 columns' packed states fit into 160 KiB: the plan is made, the simulation refuses it."""
    engine = _engine()
    parent, blen, leaf = sim.caterpillar(10242)         # (made in no time; a Yule tree of this size takes seconds to draw)
    plan = engine.Plan(10242, parent, blen, leaf, [0, 64], [[0.25] * 4], [[1.0] * 6], 5, [], [])
    try:
        with pytest.raises(engine.TphipError) as e:
            plan.simulate_columns(np.full(64, 0.1))
    finally:
        plan.close()
    print(str(e.value))
    assert "10241 internal nodes" in str(e.value) and "10240" in str(e.value)


# ---- 2. neighbours and launches ----------------------------------------------------------------------------------
def test_a_locus_does_not_depend_on_its_neighbours():
    engine = _engine()
    ntaxa, parent, blen, leaf = tree_arrays("caterpillar17")
    pi, exch, _ = locus_models("gtr", 3)
    rng = np.random.default_rng(2)
    r = rng.gamma(0.5, 1.0, size=65)
    alone = engine.Plan(ntaxa, parent, blen, leaf, [0, 65], pi[1:2], exch[1:2], 5, [], [])
    among = engine.Plan(ntaxa, parent, blen, leaf, [0, 30, 95, 1200], pi, exch, 5, [], [])
    try:
        a = alone.simulate_columns(r, replicate=3, seed=8, locus_ids=[77])
        a2 = alone.simulate_columns(r, replicate=3, seed=8, locus_ids=[77])
        other_id = alone.simulate_columns(r, replicate=3, seed=8, locus_ids=[78])
        other_seed = alone.simulate_columns(r, replicate=3, seed=9, locus_ids=[77])
        rates = np.concatenate([rng.gamma(0.5, 1.0, size=30), r, rng.gamma(0.5, 1.0, size=1105)])
        m = among.simulate_columns(rates, replicate=3, seed=8, locus_ids=[1, 77, 2])[:, 30:95]
    finally:
        alone.close()
        among.close()
    print("alone vs among: %d cells differ; second run: %d; other id: %d; other seed: %d"
          % ((a != m).sum(), (a != a2).sum(), (a != other_id).sum(), (a != other_seed).sum()))
    assert np.array_equal(a, m) and np.array_equal(a, a2)
    assert (a != other_id).sum() > a.size // 10 and (a != other_seed).sum() > a.size // 10


# ---- 3. distribution on the GPU ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_two_taxon_joint_frequencies_on_the_gpu(kind):
    engine = _engine()
    pi, exch = np.array([0.10, 0.35, 0.15, 0.40]), np.array([1.3, 1.0, 0.6, 0.9, 2.1, 0.7])
    model = sim.eigen_system(pi, exch) if kind == "gtr" else sim.f81_system(pi)
    t, n = 0.7, 65536
    r = 0.8 * model["kappa"]
    plan = engine.Plan(2, [2, 2, -1], [t, t, 0.0], [0, 1, -1], [0, n], [pi], None if kind == "f81" else [exch], 5, [], [], model=kind)
    try:
        got = plan.simulate_columns(np.full(n, r), replicate=0, seed=1, locus_ids=[3])
    finally:
        plan.close()
    z, counts, expect = sim.joint_z(got, model, 2 * t * r)
    print("%s on the GPU: max |z| = %.3f over 16 cells, N = %d" % (kind, z, n))
    assert z <= 5.0


# ---- 4. the driver equals the composition of its parts -----------------------------------------------------------
B4, SEED4, LEVEL4 = 5, 12, 0.9


@pytest.fixture(scope="module")
def driver_case():
    """16 taxa, loci of 300 and 65 columns with gaps, B = 5: the driver's outputs and the same replicates one by one."""
    engine = _engine()
    from tapir_amd import synth
    root, names = synth.yule_tree(16, 6)
    pin = synth.plan_inputs(root, names)
    off = np.array([0, 300, 365], np.int64)
    pi, exch, _ = locus_models("gtr", 2)
    T, times, iv = pin["T"], [10, 30], [[5, 15], [20, 60]]
    plan = engine.Plan(16, pin["parent"], pin["blen"], pin["leaf"], off, pi, exch, T, times, iv, correction=pin["correction"],
                       threshold=3, round_decimals=4)
    try:
        rng = np.random.default_rng(9)
        truth = rng.gamma(0.5, 0.008, size=365) * pin["correction"] * np.repeat(plan.models()[3], [300, 65])
        observed = plan.simulate_columns(truth, replicate=0, seed=99)
        observed[rng.random(observed.shape) < 0.05] = 15
        observed[:, 40:46] = 15            # culled columns: fewer than three informative cells
        observed[:2, 44] = [1, 2]
        observed[:, 120] = 4               # a constant column: rate exactly 0
        first = plan.run_fused(observed)
        rates = first["rate"].copy()
        ids = [2 ** 35 + 3, 4]
        summary, rows, mean, sd = plan.pi_parametric_bootstrap(rates, observed, replicates=B4, seed=SEED4, level=LEVEL4,
                                                               locus_ids=ids, return_rows=True, return_rate_moments=True)
        reps = []
        for b in range(B4):
            st = plan.simulate_columns(rates, mask=observed, replicate=b, seed=SEED4, locus_ids=ids)
            out = plan.run_fused(st)
            reps.append(dict(tables=out["tables"], final=plan.corrected_rates(out["rate"], out["nres"])))
    finally:
        plan.close()
    return dict(T=T, n_t=len(times), n_i=len(iv), observed=observed, first=first, rates=rates, summary=summary, rows=rows, mean=mean,
                sd=sd, reps=reps)


def test_driver_rows_equal_run_fused_on_simulated_columns(driver_case):
    c = driver_case
    T, n_t, n_i = c["T"], c["n_t"], c["n_i"]
    for b, rep in enumerate(c["reps"]):
        want = np.concatenate([rep["tables"][:, :T], rep["tables"][:, T + n_t:T + n_t + n_i]], axis=1)
        diff = int((c["rows"][:, b] != want).sum())
        print("replicate %d: %d of %d row entries differ from run_fused(simulate_columns)" % (b, diff, want.size))
        assert np.array_equal(c["rows"][:, b], want)


def test_driver_rate_moments(driver_case):
    c = driver_case
    final = np.stack([rep["final"] for rep in c["reps"]])          # [B, ncols]
    culled = c["first"]["nres"] < 3
    print("columns %d, culled %d, NaN means %d, zero-rate columns %d" % (final.shape[1], culled.sum(), np.isnan(c["mean"]).sum(),
                                                                      (c["rates"] == 0).sum()))
    assert culled.sum() >= 5 and np.array_equal(np.isnan(c["mean"]), culled) and np.array_equal(np.isnan(c["sd"]), culled)
    ok = ~culled
    ref_mean, ref_sd = final[:, ok].mean(axis=0), final[:, ok].std(axis=0, ddof=1)
    top = np.abs(final[:, ok]).max(axis=0)
    e_mean = np.abs(c["mean"][ok] - ref_mean)
    e_sd = np.abs(c["sd"][ok] - ref_sd)
    print("worst error / bound: mean %.3f, sd %.3f" % (float(np.max(e_mean / np.maximum((B4 + 2) * U * np.abs(ref_mean), 1e-300))),
                                                       float(np.max(e_sd / np.maximum(8 * B4 * U * top, 1e-300)))))
    assert np.all(e_mean <= (B4 + 2) * U * np.abs(ref_mean))
    assert np.all(e_sd <= 8 * B4 * U * top)
    zero = ok & (c["rates"] == 0)
    assert zero.sum() >= 1 and np.all(c["mean"][zero] == 0) and np.all(c["sd"][zero] == 0)


# ---- 5. the summary kernel on its own ------------------------------------------------------------------------------
def _documented_quantiles(rows, level):
    """The two quantiles by the rule the summary kernel documents (bootstrap_driver.hip: bs_quantile_index, numpy_lerp): virtual
    index n q + (1 + q (1 - 1 - 1)) - 1 in fp64, lower neighbour = its floor, numpy's _lerp with the fractional part."""
    v = np.sort(np.asarray(rows, np.float64), axis=0)
    n = v.shape[0]
    out = []
    for q in ((1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0):
        q = np.float64(q)
        vi = (np.float64(n) * q + (np.float64(1.0) + q * np.float64(-1.0))) - np.float64(1.0)
        i = int(np.floor(vi))
        if i < 0:
            i, t = 0, np.float64(0.0)
        elif vi >= n - 1:
            i, t = n - 1, np.float64(0.0)
        else:
            t = vi - np.floor(vi)
        a, b = v[i], v[min(i + 1, n - 1)]
        d = b - a
        out.append(b - d * (1.0 - t) if t >= 0.5 else a + d * t)
    return np.stack(out)


@pytest.mark.parametrize("B", [2, 3, 100])
def test_summarize_rows_against_numpy(B):
    """Two sets of rows.  `narrow`: what the kernel is for, replicate rows of a bootstrap -- every entry scatters by a few per
    cent around its value; mean, sd and quantiles against numpy with the bounds of
    test_gpu_bootstrap.py::test_summary_against_numpy.  `wide`: gamma(2, 3) values, whose neighbouring order statistics lie as
    far apart as the values are large; mean and sd against numpy with the same bounds, the quantiles with the same bound against
    the rule the kernel documents, evaluated in numpy.  Why the quantiles of `wide` are not compared with np.quantile: the
    documented virtual index n q + (1 - q) - 1 and the (n - 1) q that numpy 2 evaluates for its default rule round differently,
    by up to an ulp of n in the interpolation weight; that moves a quantile by (ulp of n) x (gap between the two neighbours),
    within 4 x 2^-52 of the quantile only while the gap is below about 4 / n of it -- true of bootstrap replicates, not of
    arbitrary values (measured on `wide`: up to 3.7 x the bound at B = 100)."""
    engine = _engine()
    level = 0.95
    rng = np.random.default_rng(B)
    narrow = rng.gamma(2.0, 3.0, size=(3, 1, 11)) * (1.0 + 0.02 * rng.standard_normal((3, B, 11)))
    narrow[1, :, 4] = 0.0
    wide = rng.gamma(2.0, 3.0, size=(3, B, 11))
    for name, rows in (("narrow", narrow), ("wide", wide)):
        summary = engine.summarize_rows(rows, level=level)
        errs = []
        for l in range(rows.shape[0]):
            ref = bsr.summarize(rows[l], level)
            qref = ref[2:] if name == "narrow" else _documented_quantiles(rows[l], level)
            top = np.abs(rows[l]).max(axis=0)
            errs.append((np.abs(summary[l, 0] - ref[0]), (B + 2) * U * np.abs(ref[0]), np.abs(summary[l, 1] - ref[1]), 8 * B * U * top,
                         np.abs(summary[l, 2:] - qref), 4 * U * np.abs(qref), np.abs(summary[l, 2:] - ref[2:]), 4 * U * np.abs(ref[2:])))
        worst = [max(float(np.max(e[2 * k] / np.maximum(e[2 * k + 1], 1e-300))) for e in errs) for k in range(4)]
        print("B=%d %s: worst error / bound: mean %.3f, sd %.3f, quantiles %.3f (against np.quantile: %.3f)" % (B, name, *worst))
        for e in errs:
            assert np.all(e[0] <= e[1]) and np.all(e[2] <= e[3]) and np.all(e[4] <= e[5])


def test_driver_summary_is_summarize_rows_of_its_rows(driver_case):
    engine = _engine()
    c = driver_case
    again = engine.summarize_rows(c["rows"], level=LEVEL4)
    print("summary entries that differ from summarize_rows(rows): %d of %d" % ((again != c["summary"]).sum(), again.size))
    assert np.array_equal(again, c["summary"])


# ---- 6. bad arguments ----------------------------------------------------------------------------------------------
def _refused(engine, fn):
    with pytest.raises(engine.TphipError) as e:
        fn()
    text = str(e.value)
    print(text)
    assert text.startswith("libtphip error 1: ") and len(text) > len("libtphip error 1: ")   # TPHIP_ERR_INVALID with a message


def test_bad_arguments_are_refused():
    engine = _engine()
    import torch
    ntaxa, parent, blen, leaf = tree_arrays("trifurcation")
    pi, exch = np.full((1, 4), 0.25), np.ones((1, 6))
    mix = engine.Plan(ntaxa, parent, blen, leaf, [0, 10], pi, exch, 5, [], [], cat_rates=[0.5, 1.5])
    plan = engine.Plan(ntaxa, parent, blen, leaf, [0, 10], pi, exch, 5, [], [[0, 3]])
    try:
        r = np.full(10, 0.1)
        st = np.full((ntaxa, 10), 1, np.uint8)
        _refused(engine, lambda: mix.simulate_columns(r))
        _refused(engine, lambda: mix.pi_parametric_bootstrap(r, st, replicates=4))
        for kw in (dict(replicates=1), dict(replicates=4097), dict(replicates=10, level=0.0), dict(replicates=10, level=1.0)):
            _refused(engine, lambda: plan.pi_parametric_bootstrap(r, st, **kw))
        _refused(engine, lambda: plan.pi_parametric_bootstrap(r, None, replicates=4))
        _refused(engine, lambda: plan.simulate_columns(r, replicate=65536))
        need = plan.parboot_workspace_bytes(4)
        d_r, d_st = torch.from_numpy(r).cuda(), torch.from_numpy(st).cuda()
        d_sum = torch.zeros((1, 4, plan.bootstrap_width), dtype=torch.float64, device="cuda")
        d_ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        _refused(engine, lambda: plan.pi_parametric_bootstrap_dev(d_r, d_st, d_sum, None, None, None, d_ws, 4, ws_bytes=need // 2))
        _refused(engine, lambda: plan.pi_parametric_bootstrap_dev(d_r, None, d_sum, None, None, None, d_ws, 4))
        plan.pi_parametric_bootstrap_dev(d_r, d_st, d_sum, None, None, None, d_ws, 4)     # the full workspace is enough
        torch.cuda.synchronize()
        assert np.all(np.isfinite(d_sum.cpu().numpy()))
    finally:
        mix.close()
        plan.close()


# ---- 7. the command line on the bundled locus ----------------------------------------------------------------------
def test_cli_parametric_bootstrap_on_the_bundled_locus(tmp_path, golden_dir):
    import shutil
    _engine()
    from tapir_amd import cli, compute, newick
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    tree = os.path.join(golden_dir, "Euteleost.tree")
    dirs = []
    for name, extra in (("plain", []), ("parboot", ["--parametric-bootstrap", "8", "--parametric-bootstrap-seed", "5"])):
        out = tmp_path / name
        out.mkdir()
        dirs.append(cli.main([str(aln), tree, "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40",
                              "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"] + extra))
    plain, boot = dirs
    new = sorted(set(os.listdir(boot)) - set(os.listdir(plain)))
    print("new files:", new)
    assert new == ["chr1_918.nex.rates-bootstrap.json", "phylogenetic-informativeness-parametric-bootstrap.sqlite"]
    for f in sorted(os.listdir(plain)):
        same = open(os.path.join(plain, f), "rb").read() == open(os.path.join(boot, f), "rb").read()
        print("%s: %s" % (f, "byte-identical" if same else "DIFFERS"))
        assert same
    T = int(compute.correct_tree(newick.read_tree(tree))[0])
    con = sqlite3.connect(os.path.join(boot, "phylogenetic-informativeness-parametric-bootstrap.sqlite"))
    meta = dict(con.execute("select key, value from meta"))
    print("meta:", meta)
    assert meta == {"replicates": "8", "seed": "5", "level": "0.95", "method": "parametric"}
    net = np.array(con.execute("select time, mean, sd, lo, hi from net_bootstrap order by time").fetchall())
    iv = np.array(con.execute("select mean, sd, lo, hi from interval_bootstrap order by rowid").fetchall())
    disc = np.array(con.execute("select mean, sd, lo, hi from discrete_bootstrap order by time").fetchall())
    con.close()
    assert net.shape == (T, 5) and np.array_equal(net[:, 0], np.arange(T)) and iv.shape == (2, 4) and disc.shape == (2, 4)
    for name, block in (("net", net[:, 1:]), ("interval", iv), ("discrete", disc)):
        print("%s: mean in [%g, %g], largest sd %g" % (name, block[:, 0].min(), block[:, 0].max(), block[:, 1].max()))
        assert np.all(block[:, 2] <= block[:, 0]) and np.all(block[:, 0] <= block[:, 3]) and np.all(block[:, 1] >= 0)
    moments = json.load(open(os.path.join(boot, "chr1_918.nex.rates-bootstrap.json")))
    sites = json.load(open(os.path.join(boot, "chr1_918.nex.rates")))["sites"]["rates"]
    print("sites %d, moments %d, culled %d" % (len(sites), len(moments["mean"]), sum(v is None for v in moments["mean"])))
    assert len(moments["mean"]) == len(moments["sd"]) == len(sites)

"""The F81 / Jukes-Cantor site-rate kernel (tphip_plan_desc.model = TPHIP_MODEL_F81) on the MI355X: against the CPU oracle
with exchangeabilities of 1, against the GTR kernel on the same model, its derivative algebra against finite differences,
the invariants the GTR path holds, plan validation, and the command line with --site-model jc."""
import json
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL_RATE = 1e-6
ONES = np.ones(6)
MODES = [dict(), dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_MIXED="0"), dict(TPHIP_SITE_PERSISTENT="0", TPHIP_SITE_MIXED="0"),
         dict(TPHIP_SITE_PERSISTENT="0", TPHIP_SITE_MIXED="1")]
ENV_KEYS = ("TPHIP_SITE_PERSISTENT", "TPHIP_SITE_MIXED", "TPHIP_SITE_WAVES", "TPHIP_DEDUP")


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _rel(a, b, floor=1e-12):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def _env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _batch(ntaxa, seed, ncols):
    """Five loci: synthetic pi, JC's pi, a locus without T (pi_T = 0), an empty locus, a ragged short one."""
    from tapir_amd import nexus, synth
    from tapir_amd import engine
    d = synth.simulate(4, ncols, ntaxa, seed)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy().copy()
    a = st[:, 2 * ncols:3 * ncols]
    a[(a & 8) != 0] = 1          # no cell of locus 2 may be T (gaps and IUPAC codes with T included): pi_T = 0
    off = np.array([0, ncols, 2 * ncols, 3 * ncols, 3 * ncols, 3 * ncols + ncols // 3], dtype=np.int64)
    st = np.ascontiguousarray(st[:, :off[-1]])
    pi = np.array(d["pi"][:4]).copy()
    with np.errstate(invalid="ignore"):   # (the empty locus has no frequencies)
        emp = nexus.base_frequencies_from_histogram(engine.state_histogram(st, off))[2]
    pi = np.vstack([pi[0], [.25] * 4, emp, pi[2], pi[3]])
    assert pi[2, 3] == 0.0
    return st, off, pi, pin


def _floored(p, eps=1e-12):
    q = np.maximum(p, eps * p.sum())
    return q / q.sum()


def _f81_plan(engine, st, off, pi, pin, **kw):
    return engine.Plan(st.shape[0], pin["parent"], pin["blen"], pin["leaf"], off, pi, None, pin["T"], [10], [[5, 15]],
                       correction=pin["correction"], model="f81", **kw)


def _check_vs_oracle(oracle, got, st, off, pi, pin, kappa, cat=None):
    for l in range(len(off) - 1):
        sl = slice(int(off[l]), int(off[l + 1]))
        if sl.stop == sl.start:
            continue
        ref = oracle.site_rates(st[:, sl], pin["parent"], pin["blen"], pin["leaf"], _floored(pi[l]), ONES,
                                *(cat or ()))
        assert np.array_equal(got["nres"][sl], ref["nres"])
        assert np.array_equal(got["flag"][sl], ref["flag"]), (l, np.flatnonzero(got["flag"][sl] != ref["flag"]))
        ok = (ref["flag"] == 0) | (ref["flag"] == 3)
        rr = _rel(got["rate"][sl][ok], ref["rate"][ok])
        lnl_err = np.abs(got["lnl"][sl] - ref["lnl"]) / np.maximum(1.0, np.abs(ref["lnl"]))
        assert lnl_err.max() <= 1e-10, (l, lnl_err.max())
        # an almost flat maximum: a stationary point of the oracle's curve (whose pi carries the floor on an absent base)
        gtol = 5e-14 if (pi[l] > 0).all() else 5e-12
        for c in np.flatnonzero(ok)[rr >= RTOL_RATE]:
            u = np.log(got["rate"][sl][c] / kappa[l])
            f, g, h = oracle.column_curve(st[:, sl], pin["parent"], pin["blen"], pin["leaf"], _floored(pi[l]), ONES, int(c),
                                          np.array([u]))
            assert abs(g[0]) <= gtol and abs(h[0]) < 1e-7, (l, int(c), rr[list(np.flatnonzero(ok)).index(c)], g[0], h[0])


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("ntaxa,ncols", [(20, 400), (64, 300), (130, 150), (300, 60), (500, 40)])
def test_f81_kernel_vs_oracle(oracle, monkeypatch, ntaxa, ncols, mode):
    """Packed words in registers (20, 64 taxa), streamed words (130, 300, 500), rescaling (300, 500); every scheduling mode;
    JC's and synthetic pi, an absent base, empty and ragged loci.  (Not the spilled stack: TPHIP_SITE_SPILL=1 only asks for
    it, and tphip_plan_create grants it when a wave's share would reach 1000 columns, which a few hundred columns never do;
    every case here keeps all parked partials in LDS.)"""
    engine = _engine()
    _env(monkeypatch, MODES[mode])
    if ntaxa >= 300 and mode == 1:
        monkeypatch.setenv("TPHIP_SITE_SPILL", "1")
    st, off, pi, pin = _batch(ntaxa, 100 + ntaxa, ncols)
    plan = _f81_plan(engine, st, off, pi, pin)
    got = plan.site_rates(st)
    kappa = plan.models()[3]
    _check_vs_oracle(oracle, got, st, off, pi, pin, kappa)
    assert (got["flag"] == 0).sum() > off[-1] // 4
    plan.close()


def test_f81_plan_vs_gtr_plan_and_derivatives(oracle):
    """The same (pi, 1s) model through both kernels on the same bytes; the diagnostic f, g, h at fixed u agree to 1e-10
    and match central finite differences of f -- the independent check of the closed-form derivative algebra."""
    engine = _engine()
    for ntaxa, ncols, seed in ((16, 500, 3), (64, 300, 4), (200, 80, 5)):
        st, off, pi, pin = _batch(ntaxa, seed, ncols)
        f81 = _f81_plan(engine, st, off, pi, pin)
        gtr = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], off, pi, np.ones((len(pi), 6)), pin["T"], [10],
                          [[5, 15]], correction=pin["correction"])
        a, b = f81.run_fused(st), gtr.run_fused(st)
        assert np.array_equal(a["nres"], b["nres"])
        assert np.array_equal(a["flag"], b["flag"]), np.flatnonzero(a["flag"] != b["flag"])
        ok = (b["flag"] == 0) | (b["flag"] == 3)
        lnl_err = np.abs(a["lnl"] - b["lnl"]) / np.maximum(1.0, np.abs(b["lnl"]))
        assert lnl_err.max() <= 1e-10, lnl_err.max()
        assert _rel(a["rate"][ok], b["rate"][ok]).max() < RTOL_RATE, _rel(a["rate"][ok], b["rate"][ok]).max()
        rng = np.random.default_rng(seed)
        u = rng.uniform(-4.0, 3.0, st.shape[1])
        fa, ga, ha = f81.eval_columns(st, u)
        fb, gb, hb = gtr.eval_columns(st, u)
        # (h = L''/L - g^2 is a difference: its rounding scales with g^2 where that is the larger term)
        for x, y, scale, what in ((fa, fb, 1.0, "f"), (ga, gb, 1.0, "g"), (ha, hb, np.maximum(1.0, gb * gb), "h")):
            err = np.abs(x - y) / np.maximum(scale, np.abs(y))
            assert err.max() <= 1e-10, (what, err.max(), int(err.argmax()))
        e = 1e-5
        fp, gp, _ = f81.eval_columns(st, u + e)
        fm, gm, _ = f81.eval_columns(st, u - e)
        for fd, an, what in (((fp - fm) / (2 * e), ga, "g"), ((gp - gm) / (2 * e), ha, "h")):
            err = np.abs(fd - an) / np.maximum(1.0, np.abs(an))
            assert err.max() < 1e-6, (what, err.max(), int(err.argmax()))
        # and the oracle's curve at the same points
        for l in (0, 2):
            sl = slice(int(off[l]), int(off[l + 1]))
            for c in range(0, sl.stop - sl.start, 37):
                fo, go, ho = oracle.column_curve(st[:, sl], pin["parent"], pin["blen"], pin["leaf"], _floored(pi[l]), ONES, c,
                                                 np.array([u[sl.start + c]]))
                assert abs(fa[sl.start + c] - fo[0]) <= 1e-10 * max(1.0, abs(fo[0])), (l, c, fa[sl.start + c], fo[0])
                assert abs(ga[sl.start + c] - go[0]) <= 1e-9 * max(1.0, abs(go[0])), (l, c, ga[sl.start + c], go[0])
        f81.close()
        gtr.close()


@pytest.mark.parametrize("ntaxa", [12, 40])
def test_f81_scheduling_modes_dedup_and_waves_are_bit_identical(monkeypatch, ntaxa):
    """Mixed-loci, slice and persistent modes, pattern de-duplication on and off and the number of waves give the same
    bits, as they do on the GTR path."""
    engine = _engine()
    from tapir_amd import synth
    rng = np.random.default_rng(5 + ntaxa)
    nloci = 200
    d = synth.simulate(nloci, 150, ntaxa, 700 + ntaxa)
    pin = synth.plan_inputs(d["root"], d["names"])
    lens = rng.integers(0, 151, size=nloci)
    lens[rng.random(nloci) < 0.3] = 2
    off = np.zeros(nloci + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    st = np.ascontiguousarray(d["states"].numpy()[:, :int(off[-1])])
    st[:, 1::3] = st[:, 0::3][:, :st[:, 1::3].shape[1]]     # repeated columns for the de-duplication to find
    runs = {}
    for name, env in [("default", {}), ("mixed", dict(TPHIP_SITE_MIXED="1")), ("mixed_few", dict(TPHIP_SITE_MIXED="1", TPHIP_SITE_WAVES="5")),
                      ("slices", dict(TPHIP_SITE_MIXED="0", TPHIP_SITE_PERSISTENT="0")),
                      ("persistent", dict(TPHIP_SITE_MIXED="0", TPHIP_SITE_PERSISTENT="1")),
                      ("persistent_37", dict(TPHIP_SITE_MIXED="0", TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES="37")),
                      ("dedup_on", dict(TPHIP_DEDUP="1")), ("dedup_off", dict(TPHIP_DEDUP="0"))]:
        _env(monkeypatch, env)
        plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], None, pin["T"], [10], [[5, 15]],
                           correction=pin["correction"], model="f81")
        runs[name] = plan.run_fused(st)
        plan.close()
    base = runs["slices"]
    assert (base["flag"] == 0).sum() > off[-1] // 4
    for name, got in runs.items():
        for key in ("rate", "subst", "lnl", "flag", "nres", "tables"):
            assert np.array_equal(got[key], base[key]), (name, key)


def test_f81_gamma_mixture_vs_oracle(oracle):
    engine = _engine()
    from tapir_amd import compute
    r, w = compute.discrete_gamma(0.5, 4)
    for ntaxa, ncols, seed in ((8, 500, 5), (40, 300, 6)):
        st, off, pi, pin = _batch(ntaxa, seed, ncols)
        plan = _f81_plan(engine, st, off, pi, pin, cat_rates=r, cat_weights=w)
        got = plan.site_rates(st)
        _check_vs_oracle(oracle, got, st, off, pi, pin, plan.models()[3], cat=(r, w))
        plan.close()


def test_f81_plan_validation_and_model():
    engine = _engine()
    st, off, pi, pin = _batch(16, 9, 100)
    args = (16, pin["parent"], pin["blen"], pin["leaf"], off, pi)
    with pytest.raises(engine.TphipError, match="exch must be NULL"):
        engine.Plan(*args, np.ones((len(pi), 6)), pin["T"], [10], [[5, 15]], model="f81")
    plan = engine.Plan(*args, None, pin["T"], [10], [[5, 15]], model="f81")
    with pytest.raises(engine.TphipError, match="stage1_fit"):
        plan.stage1_fit(st, details=False)
    with pytest.raises(engine.TphipError, match="exch must be NULL"):
        plan.set_models(exch=np.ones((len(pi), 6)))
    lam, U, Ui, kappa = plan.models()
    for l in range(len(pi)):
        p = pi[l] / pi[l].sum()
        assert abs(kappa[l] - (1.0 - np.sum(p * p))) <= 1e-15
        assert np.array_equal(lam[l], [0.0, -1.0, -1.0, -1.0])
        Q = U[l] @ np.diag(lam[l]) @ Ui[l]
        assert np.abs(Q - (np.tile(p, (4, 1)) - np.eye(4))).max() < 1e-15
    # set_models(pi) takes new frequencies: same answers as a plan made with them
    a = plan.site_rates(st)
    plan.set_models(pi=np.tile([.25] * 4, (len(pi), 1)))
    b = plan.site_rates(st)
    jc = engine.Plan(*args[:5], np.tile([.25] * 4, (len(pi), 1)), None, pin["T"], [10], [[5, 15]], model="f81")
    c = jc.site_rates(st)
    assert not np.array_equal(a["rate"], b["rate"])
    for k in ("rate", "lnl", "flag"):
        assert np.array_equal(b[k], c[k])
    assert abs(plan.models()[3][0] - 0.75) <= 1e-15
    plan.close()
    jc.close()
    with pytest.raises(engine.TphipError):
        engine.Plan(*args, None, pin["T"], [10], [[5, 15]])   # GTR needs exch


def _cli(golden_dir, tmp_path, tag, extra=(), env=None):
    aln = tmp_path / ("aln_" + tag)
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln / "chr1_918_copy.nex")
    out = tmp_path / ("out_" + tag)
    out.mkdir()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = [str(aln), os.path.join(golden_dir, "Euteleost.tree"), "--output", str(out), "--times", "10,20,50",
            "--intervals", "0-10,10-15,20-100", "--site-model", "jc"] + list(extra)
    code = ("import sys; sys.path.insert(0, %r); from tapir_amd import cli; o = cli.main(%r); "
            "print('STAGES=' + ','.join(sorted(cli.LAST_TIMINGS))); print('OUT=' + o)" % (root, argv))
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    stages = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("STAGES=")][-1].split(",")
    assert "stage1_model_averaging" not in stages
    return [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("OUT=")][-1], stages


def _sqlite_dump(path):
    conn = sqlite3.connect(path)
    rows = [list(conn.execute("select * from %s order by rowid" % t)) for t in ("loci", "net", "discrete", "interval")]
    conn.close()
    return rows


def test_cli_site_model_jc_vs_oracle_and_streamed(golden_dir, tmp_path, oracle):
    """--site-model jc on chr1_918 against the oracle (pi = 1/4, exchangeabilities 1); the streamed block pipeline
    (TPHIP_STREAM_BLOCK=1, two loci, --multiprocessing) writes the same .rates and sqlite bytes as the unstreamed run."""
    _engine()
    from tapir_amd import compute, newick, nexus
    plain, s1 = _cli(golden_dir, tmp_path, "plain", ["--multiprocessing"], dict(TPHIP_NO_STREAM="1"))
    streamed, s2 = _cli(golden_dir, tmp_path, "streamed", ["--multiprocessing"], dict(TPHIP_STREAM_BLOCK="1"))
    assert "sqlite_tail" in s2 and "sqlite_tail" not in s1     # the block pipeline ran, and only in the second run
    for f in ("chr1_918.nex.rates", "chr1_918_copy.nex.rates"):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(streamed, f), "rb").read()
    assert _sqlite_dump(os.path.join(plain, "phylogenetic-informativeness.sqlite")) == \
        _sqlite_dump(os.path.join(streamed, "phylogenetic-informativeness.sqlite"))
    doc = json.load(open(os.path.join(plain, "chr1_918.nex.rates")))["sites"]
    assert [doc["freqs"][b] for b in "ACGT"] == [0.25] * 4
    assert [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")] == [1.0] * 6
    names, st = nexus.read_states(os.path.join(golden_dir, "chr1_918.nex"))
    root = newick.read_tree(os.path.join(plain, "Tree_100_174.0.newick"))
    leaf_names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, leaf_names)
    st = st[[names.index(n) for n in leaf_names]]
    ref = oracle.site_rates(st, parent, blen, leaf, np.full(4, 0.25), ONES)
    ok = (ref["flag"] == 0) | (ref["flag"] == 3)
    got = np.array([r["rate"] for r in doc["rates"]])
    assert np.abs(got - compute.round_like_hyphy(ref["rate"], 4))[ok].max() <= 1e-4 + 1e-12
    assert np.abs(np.array([r["ll"] for r in doc["rates"]]) - ref["lnl"]).max() < 5.1e-5
    rows = _sqlite_dump(os.path.join(plain, "phylogenetic-informativeness.sqlite"))
    rates = got / 100
    rates[ref["nres"] < 3] = np.nan
    pi_net, pi_times, pi_epochs = oracle.worker_tables(rates, 174, [10, 20, 50], [[0, 10], [10, 15], [20, 100]])
    net = [p for i, t, p in rows[1] if i == 1]
    assert np.allclose(net, pi_net, rtol=1e-9, atol=1e-300)

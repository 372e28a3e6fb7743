"""HyPhy stage 1 (model-averaged exchangeabilities, models_and_rates.bf:405-897) on the GPU against the
independent CPU restatement in oracle/stage1_oracle.py.

Parity unpinned against HyPhy itself: the reference holds no stage-1 output and its HyPhy binary is neither
present nor run; what is checked is that the GPU likelihood + batched optimiser reach the same optimum, weights
and averaged rates as scipy's L-BFGS-B over the oracle's C likelihood (tolerance 1e-3 relative, set by the
optimisers' stopping rules on a flat likelihood surface, not by the arithmetic: the likelihood, its gradient and its
curvature are pinned to a 40-digit reference on every kernel path by tests/test_gpu_stage1_numerics.py; the oracle
shares the kernels' formulas and is a parity check only)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("GPU tests need a GPU and tapir_amd/libtphip.so")
    return engine


def test_stage1_matches_independent_restatement():
    engine = _engine()
    from oracle import stage1_oracle
    from tapir_amd import stage1, synth
    L, n, nt = 3, 200, 7
    d = synth.simulate(L, n, nt, 23)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    st[2, 5:40] = 15  # gaps and an ambiguity code take the same path as in stage 2
    st[4, 100:120] = 5
    pi = np.asarray(d["pi"])
    blen = np.asarray(pin["blen"]) / pin["correction"]
    plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"],
                       [1], [[0, 1]], correction=pin["correction"])
    got = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], blen)
    plan.close()
    assert np.allclose(got["weights"].sum(1), 1.0) and np.all(got["exch"][:, 1] == 1.0)
    for l in range(L):
        ref = stage1_oracle.model_averaged(st[:, l * n:(l + 1) * n], pin["parent"], blen, pin["leaf"], pi[l])
        assert np.max(np.abs(got["exch"][l] - ref["exch"]) / ref["exch"]) < 1e-3
        lnl = np.array([ref["lnl"][m] for m in got["models"]])
        w = np.array([ref["weights"][m] for m in got["models"]])
        keep = w > 1e-9   # models abandoned early (weight < e^-21) are not polished to their optimum
        assert np.max(np.abs(lnl - got["lnl"][l])[keep]) < 1e-3
        assert np.all(got["lnl"][l] <= lnl + 1e-3)
        assert np.max(np.abs(w - got["weights"][l])) < 1e-4


def test_stage1_recovers_generating_rates_on_long_loci():
    """Statistical sanity at a size the CPU restatement cannot reach: with 20 000 columns per locus the
    model-averaged estimates are close to the exchangeabilities the alignment was simulated under (simulated
    without rate variation among columns, which stage 1 does not model and which would bias them towards 1)."""
    engine = _engine()
    from tapir_amd import stage1, synth
    L, n, nt = 4, 20000, 16
    d = synth.simulate(L, n, nt, 5, rate_shape=1e6, rate_mean=0.002)  # one rate for all columns: the model stage 1 fits
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    hist = engine.state_histogram(st, d["locus_offsets"])
    from tapir_amd import nexus
    pi = nexus.base_frequencies_from_histogram(hist)
    plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"],
                       [1], [[0, 1]], correction=pin["correction"])
    got = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], np.asarray(pin["blen"]) / pin["correction"])
    plan.close()
    true = np.asarray(d["exch"])
    true = true / true[:, 1:2]
    assert np.max(np.abs(got["exch"] - true) / true) < 0.15, (got["exch"], true)


def test_cli_default_model_averaging_on_gpu(tmp_path):
    """tapir_compute.py without --exchangeabilities: stage 1 + stage 2 + PI in one run on the GPU."""
    _engine()
    import json
    import shutil
    from tapir_amd import cli, synth
    d = synth.simulate(3, 150, 6, 9)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    out = tmp_path / "out"
    out.mkdir()
    cli.main([str(aln), str(tmp_path / "tree.newick"), "--output", str(out), "--times", "10", "--intervals", "5-15"])
    files = sorted(f for f in os.listdir(out) if f.endswith(".rates"))
    assert len(files) == 3
    for f in files:
        m = json.load(open(out / f))["sites"]["subs_matrix"]
        assert m["AG"] == 1.0 and all(0 < m[k] < 1e4 for k in m)


def test_cli_streamed_run_writes_the_same_bytes(tmp_path):
    """The command line with --multiprocessing streams a big batch block by block (pipeline._run_streamed: stage 1, the
    per-site loop and PI of block k on the GPU while the pool writes block k - 1's `.rates` files and a second thread fills
    sqlite).  Forced here on 40 small loci in blocks of 16 (TPHIP_STREAM_BLOCK), in fresh processes (the pool forks before the
    GPU is touched): every `.rates` file and every sqlite row must equal those of the unstreamed run (TPHIP_NO_STREAM)."""
    _engine()
    import shutil
    import sqlite3
    import subprocess
    from tapir_amd import synth
    d = synth.simulate(40, 90, 6, 21)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    shutil.move(tree, tmp_path / "tree.newick")
    outs = []
    for name, env in (("streamed", {"TPHIP_STREAM_BLOCK": "16"}), ("plain", {"TPHIP_STREAM_BLOCK": "16", "TPHIP_NO_STREAM": "1"})):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "tapir_compute.py"), str(aln), str(tmp_path / "tree.newick"),
                            "--output", str(out), "--times", "10,30", "--intervals", "5-15,20-40", "--multiprocessing"],
                           capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        outs.append(out)
    a, b = outs
    files = sorted(f for f in os.listdir(a) if f.endswith(".rates"))
    assert len(files) == 40 and files == sorted(f for f in os.listdir(b) if f.endswith(".rates"))
    for f in files:
        assert open(a / f, "rb").read() == open(b / f, "rb").read(), f
    rows = []
    for o in outs:
        con = sqlite3.connect(str(o / "phylogenetic-informativeness.sqlite"))
        rows.append({t: con.execute("SELECT * FROM %s" % t).fetchall() for t in ("loci", "net", "discrete", "interval")})
        rows[-1]["schema"] = con.execute("SELECT sql FROM sqlite_master ORDER BY name").fetchall()
        con.close()
    assert rows[0] == rows[1] and len(rows[0]["loci"]) == 40 and len(rows[0]["interval"]) == 80


def test_stage1_analytic_and_finite_difference_gradients_agree():
    """Second opinions on the engine's stage 1 (tphip_stage1_fit): the host optimiser of tapir_amd/stage1.py driven by the
    reverse-mode gradient kernel and the same optimiser driven by central differences of the value kernel reach the same
    model-averaged rates (1e-3, lnL 1e-3, weights 1e-4), the engine reaches them too, and abandoning hopeless models early
    changes nothing in what the engine reports (1e-6) while saving likelihood evaluations."""
    engine = _engine()
    from tapir_amd import stage1, synth
    L, n, nt = 4, 400, 12
    d = synth.simulate(L, n, nt, 31)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    pi = np.asarray(d["pi"])
    blen = np.asarray(pin["blen"]) / pin["correction"]
    plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"],
                       [1], [[0, 1]], correction=pin["correction"])
    a = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], blen, analytic=True, prune_models=False)
    b = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], blen, analytic=False, prune_models=False)
    c = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], blen)   # the product path: one engine call
    e = plan.stage1_fit(st, prune_models=False)
    plan.close()
    assert a["ngrads"] > 0 and b["ngrads"] == 0 and c["ngrads"] > 0
    assert np.max(np.abs(c["exch"] - e["exch"]) / e["exch"]) < 1e-6 and c["nevals"] < e["stats"]["nevals"] < b["nevals"]
    assert np.max(np.abs(a["exch"] - b["exch"]) / b["exch"]) < 1e-3
    assert np.max(np.abs(a["lnl"] - b["lnl"])) < 1e-3
    assert np.max(np.abs(a["weights"] - b["weights"])) < 1e-4
    assert np.max(np.abs(e["exch"] - a["exch"]) / a["exch"]) < 1e-3
    assert np.max(np.abs(e["weights"] - a["weights"])) < 1e-4
    assert np.all(e["lnl"] >= a["lnl"] - 1e-3)      # the engine never ends below the host optimiser


def test_stage1_on_the_bundled_locus_vs_restatement_and_phydesign():
    """BASELINE config C1's data (chr1_918.nex, Euteleost.tree) through the GPU stage 1, site patterns and all: equal
    to the independent restatement (1e-3) and within 6 % of the exchangeabilities PhyDesign published for this
    locus (see tests/test_oracle_golden.py::test_stage1_restatement_against_phydesign_header)."""
    engine = _engine()
    import json
    from oracle import stage1_oracle
    from tapir_amd import compute, newick, nexus, pipeline
    g = os.path.join(ROOT, "tests", "golden")
    names, states = nexus.read_states(os.path.join(g, "chr1_918.nex"))
    root = newick.read_tree(os.path.join(g, "Euteleost.tree"))
    depth, factor = compute.correct_tree(root)
    parent, blen, leaf = newick.to_arrays(root, names)
    off = np.array([0, states.shape[1]])
    pi = nexus.base_frequencies_from_histogram(engine.state_histogram(states, off))
    got = pipeline.model_averaged_exchangeabilities(engine, states, off, pi, len(names), parent, blen, leaf, int(depth), [10],
                                                    [[0, 10]], factor)
    ref = stage1_oracle.model_averaged(states, parent, np.asarray(blen) / factor, leaf, pi[0])
    assert np.max(np.abs(got[0] - ref["exch"]) / ref["exch"]) < 1e-3, (got, ref["exch"])
    kat = json.load(open(os.path.join(g, "chr1_918_phydesign_rates.json")))
    want = np.array([kat[k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")])
    assert np.max(np.abs(got[0] - want) / want) < 0.06


def test_stage1_engine_matches_host_optimiser():
    """The engine's optimisers (csrc/stage1_opt_kernels.hpp: L-BFGS and dense BFGS as device kernels, sequenced by
    csrc/stage1_driver.hip) against the numpy optimiser of stage1.py over the same likelihood kernels -- on short loci
    (many models matter) and on long ones (a handful).  Both must reach the same optima: averaged rates 1e-3 (the stage's
    tolerance; observed 3e-5), weights 1e-4, and the engine's log-likelihoods are never below the host's by more than its own
    stopping tolerance (it may be above: its metric for short branches finds optima the host optimiser stops short of)."""
    engine = _engine()
    from tapir_amd import stage1, synth
    for L, n, nt, seed in ((12, 300, 10, 41), (3, 6000, 16, 42)):
        d = synth.simulate(L, n, nt, seed)
        pin = synth.plan_inputs(d["root"], d["names"])
        st = d["states"].numpy()
        pi = np.asarray(d["pi"])
        blen = np.asarray(pin["blen"]) / pin["correction"]
        plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"],
                           [1], [[0, 1]], correction=pin["correction"])
        a = plan.stage1_fit(st)
        a2 = plan.stage1_fit(st, free_root_pair=True)   # HyPhy's parameter list: both branches below the root free
        s_host = stage1.Stage1(plan, st, pi, pin["parent"], blen)
        b = s_host.run()
        s_host.close()
        plan.close()
        assert np.max(np.abs(a["exch"] - b["exch"]) / b["exch"]) < 1e-3
        assert np.max(np.abs(a["weights"] - b["weights"])) < 1e-4
        heavy = b["weights"] > 1e-8
        # the two general-model fits stop within their tolerance of each other (lnL 2e-6 apart here) at slightly different branch
        # lengths; every rate-class model inherits those (bf:613-619), which moves their lnL together by up to 5e-5
        short = (b["lnl"] - a["lnl"])[heavy]
        assert short.max() < 1e-4, short.max()
        assert np.max(np.abs(a["lnl"] - b["lnl"])[heavy]) < 1e-3
        # the likelihood of a reversible model sees only the SUM of the two branches below the root
        assert np.max(np.abs(a2["lnl"][:, 0] - a["lnl"][:, 0])) < 1e-4 and np.max(np.abs(a2["exch"] - a["exch"]) / a["exch"]) < 1e-4
        par = np.asarray(pin["parent"])
        rk = np.flatnonzero(par == len(par) - 1)
        if len(rk) == 2:
            assert np.allclose(a["grm_blen"][:, rk].sum(1), a2["grm_blen"][:, rk].sum(1), rtol=5e-3, atol=1e-9)


def test_stage1_patterns_and_frequencies_on_the_device():
    """tphip_stage1_fit with compress_patterns / empirical_pi / a column range of a bigger array (row_pitch) against the
    same steps done by the caller: tphip_compress_columns + column weights, HarvestFrequencies from tphip_state_histogram,
    a contiguous copy.  Site patterns with counts are the same likelihood as the raw columns (1e-8 of lnL: the order of the
    column sum differs), so the estimates agree within the optimiser's reproducibility; tphip_plan_set_models then makes the
    same plan run the per-site loop on them."""
    engine = _engine()
    from tapir_amd import nexus, synth
    L, n, nt = 6, 400, 9
    d = synth.simulate(L + 2, n, nt, 17)
    pin = synth.plan_inputs(d["root"], d["names"])
    big = d["states"].numpy()                       # [nt, (L + 2) * n]: the middle L loci are the batch
    rng = np.random.default_rng(3)
    big[:, n:n + 150] = big[:, n + 150:n + 300]     # repeated columns: patterns with counts > 1
    big[rng.integers(0, nt, 40), rng.integers(n, (L + 1) * n, 40)] = 15
    view = big[:, n:(L + 1) * n]
    sub = np.ascontiguousarray(view)
    off = np.arange(L + 1, dtype=np.int64) * n
    pi = nexus.base_frequencies_from_histogram(engine.state_histogram(sub, off))

    def plan_for(offsets, p):
        return engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], offsets, p, np.ones((L, 6)), pin["T"], [10], [[5, 15]],
                           correction=pin["correction"])
    # the caller does the steps
    pst, poff, w, _ = engine.compress_columns(sub, off, want_map=False)
    assert pst.shape[1] < sub.shape[1]
    ref_plan = plan_for(poff, pi)
    ref_plan.set_column_weights(w)
    ref = ref_plan.stage1_fit(pst)
    ref_plan.close()
    # the engine does them, from the strided view, starting from placeholder frequencies
    plan = plan_for(off, np.full((L, 4), 0.25))
    got = plan.stage1_fit(view, compress_patterns=True, empirical_pi=True)
    assert np.max(np.abs(got["pi"] - pi)) < 1e-14
    assert np.max(np.abs(got["lnl"][:, 0] - ref["lnl"][:, 0]) / np.abs(ref["lnl"][:, 0])) < 1e-8
    assert np.max(np.abs(got["exch"] - ref["exch"]) / ref["exch"]) < 1e-4
    assert np.max(np.abs(got["weights"] - ref["weights"])) < 1e-4
    raw = plan.stage1_fit(sub)                      # raw columns, no patterns: the same likelihood column by column
    assert np.max(np.abs(raw["lnl"][:, 0] - ref["lnl"][:, 0]) / np.abs(ref["lnl"][:, 0])) < 1e-8
    assert np.max(np.abs(raw["exch"] - ref["exch"]) / ref["exch"]) < 1e-4
    # the same plan goes on to the per-site loop with the estimates
    plan.set_models(exch=got["exch"])
    out = plan.run_fused(sub)
    plan.close()
    fresh = plan_for(off, pi)
    fresh.set_models(pi=pi, exch=got["exch"])
    want = fresh.run_fused(sub)
    fresh.close()
    direct = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, pi, got["exch"], pin["T"], [10], [[5, 15]],
                         correction=pin["correction"])
    base = direct.run_fused(sub)
    direct.close()
    for k in ("rate", "lnl", "flag", "nres", "tables"):
        assert np.array_equal(out[k], want[k], equal_nan=True) and np.array_equal(out[k], base[k], equal_nan=True), k


def test_stage1_randomised_sweep_against_the_restatement():
    """tools/fuzz_stage1.py on a fixed window of a fixed seed: random 3..7-taxon trees with polytomies (the eigenbasis gradient
    kernel), 40..160 columns, gaps and ambiguity codes, against oracle/stage1_oracle.py (1e-3 on the averaged rates).  The
    window holds the case that exposed the creeping class-model fits of round 3 (a rate the general model puts at its lower
    bound and 21 class models want at 0.2-0.5: 6e-3 off before the escape test ran on every iteration)."""
    _engine()
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_stage1.py"), "22", "7", "17"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "5 cases, 0 beyond 1e-3" in r.stdout, r.stdout[-1500:]


def test_stage1_degenerate_loci_stay_finite():
    """Edge cases of the domain: an empty locus, a locus of gaps only, an invariant locus (nothing to estimate: every
    model fits equally, lengths collapse to the lower bound), one informative locus among them, and a 2-taxon tree.
    Nothing may turn NaN/inf; AG stays 1; weights sum to 1; the flat loci average to the e^-k prior over models."""
    engine = _engine()
    from tapir_amd import pipeline, stage1, synth, newick
    d = synth.simulate(1, 300, 6, 3)
    pin = synth.plan_inputs(d["root"], d["names"])
    good = d["states"].numpy()
    gaps = np.full((6, 50), 15, np.uint8)
    same = np.tile(np.array([[1], [1], [1], [1], [1], [1]], np.uint8), (1, 80))
    st = np.concatenate([gaps, same, good], axis=1)
    off = np.array([0, 0, 50, 130, 430])     # empty, gaps, invariant, informative
    pi = np.tile(np.array([0.25, 0.25, 0.25, 0.25]), (4, 1))
    pi[3] = np.asarray(d["pi"][0])
    exch = pipeline.model_averaged_exchangeabilities(engine, st, off, pi, 6, pin["parent"], pin["blen"], pin["leaf"], pin["T"],
                                                     [1], [[0, 1]], pin["correction"])
    assert exch.shape == (4, 6) and np.all(np.isfinite(exch)) and np.all(exch[:, 1] == 1.0)
    assert np.all(exch > 5e-4) and np.all(exch < 2e4)
    assert np.allclose(exch[0], 1.0) and np.allclose(exch[1], 1.0)      # no data: every rate stays at its start
    # the informative locus is unaffected by its degenerate neighbours
    alone = pipeline.model_averaged_exchangeabilities(engine, good, np.array([0, 300]), pi[3:], 6, pin["parent"], pin["blen"],
                                                      pin["leaf"], pin["T"], [1], [[0, 1]], pin["correction"])
    assert np.max(np.abs(alone[0] - exch[3]) / exch[3]) < 1e-6
    # two taxa
    root = newick.parse("(a:10,b:20);")
    parent, blen, leaf = newick.to_arrays(root, ["a", "b"])
    rng = np.random.default_rng(1)
    two = (1 << rng.integers(0, 4, size=(2, 400))).astype(np.uint8)
    two[1, :300] = two[0, :300]
    e2 = pipeline.model_averaged_exchangeabilities(engine, two, np.array([0, 400]), np.full((1, 4), 0.25), 2, parent, blen, leaf,
                                                   30, [1], [[0, 1]], 1.0)
    assert np.all(np.isfinite(e2)) and e2[0, 1] == 1.0


def test_stage1_engine_call_on_degenerate_and_large_inputs():
    """tphip_stage1_fit with empirical frequencies and device-side patterns where the data give little to go on: an empty
    locus, a locus of gaps only (no cell: frequencies fall back to 1/4), an invariant locus (one base only: its frequency
    goes to ~1 and the others to the floor) next to an informative one -- everything stays finite, AG = 1, weights sum to 1,
    and the informative locus gets the estimates it gets alone.  And a 256-taxon tree (the C5 shape's tree size: deeper
    register / adjoint stacks, 32 packed words per column): the engine agrees with the host second opinion."""
    engine = _engine()
    from tapir_amd import nexus, stage1, synth
    d = synth.simulate(1, 300, 6, 3)
    pin = synth.plan_inputs(d["root"], d["names"])
    good = d["states"].numpy()
    gaps = np.full((6, 50), 15, np.uint8)
    same = np.full((6, 80), 2, np.uint8)
    st = np.ascontiguousarray(np.concatenate([gaps, same, good], axis=1))
    off = np.array([0, 0, 50, 130, 430])
    mk = lambda o, L: engine.Plan(6, pin["parent"], pin["blen"], pin["leaf"], o, np.full((L, 4), 0.25), np.ones((L, 6)), pin["T"],  # noqa: E731
                                  [1], [[0, 1]], correction=pin["correction"])
    plan = mk(off, 4)
    out = plan.stage1_fit(st, compress_patterns=True, empirical_pi=True)
    plan.close()
    assert np.all(np.isfinite(out["exch"])) and np.all(out["exch"][:, 1] == 1.0) and np.all(np.isfinite(out["lnl"]))
    assert np.allclose(out["weights"].sum(1), 1.0) and np.all(out["exch"] > 5e-4) and np.all(out["exch"] < 2e4)
    assert np.allclose(out["pi"][0], 0.25) and np.allclose(out["pi"][1], 0.25)
    assert out["pi"][2, 1] > 0.999 and np.allclose(out["pi"].sum(1), 1.0, atol=1e-9)
    assert np.allclose(out["exch"][0], 1.0) and np.allclose(out["exch"][1], 1.0)
    alone = mk(np.array([0, 300]), 1)
    ref = alone.stage1_fit(good, compress_patterns=True, empirical_pi=True)
    alone.close()
    assert np.max(np.abs(ref["pi"][0] - out["pi"][3])) < 1e-15
    assert np.max(np.abs(ref["exch"][0] - out["exch"][3]) / out["exch"][3]) < 1e-6
    # conserved loci (a fifth of the columns vary, most branches end at their lower bound): the search must END there, not run
    # to its iteration limit (it did, 300 iterations of 23 likelihood calls, before bound coordinates were projected out)
    d = synth.simulate(4, 150, 32, 41, rate_mean=0.0002)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    pi = nexus.base_frequencies_from_histogram(engine.state_histogram(st, d["locus_offsets"]))
    plan = engine.Plan(32, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((4, 6)), pin["T"], [1], [[0, 1]],
                       correction=pin["correction"])
    a = plan.stage1_fit(st)
    host = stage1.Stage1(plan, st, pi, pin["parent"], np.asarray(pin["blen"]))
    b = host.run()
    host.close()
    plan.close()
    assert a["grm_iters"].max() < 150 and a["stats"]["grm_evals"] < 2000, (a["grm_iters"], a["stats"])
    assert np.all(a["lnl"][:, 0] >= b["lnl"][:, 0] - 1e-5) and np.max(np.abs(a["exch"] - b["exch"]) / b["exch"]) < 1e-3
    # 256 taxa
    L, n, nt = 3, 600, 256
    d = synth.simulate(L, n, nt, 77)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    pi = nexus.base_frequencies_from_histogram(engine.state_histogram(st, d["locus_offsets"]))
    plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"], [1], [[0, 1]],
                       correction=pin["correction"])
    a = plan.stage1_fit(st)
    host = stage1.Stage1(plan, st, pi, pin["parent"], np.asarray(pin["blen"]))
    b = host.run()
    host.close()
    plan.close()
    assert np.max(np.abs(a["exch"] - b["exch"]) / b["exch"]) < 1e-3
    assert np.all(a["lnl"][:, 0] >= b["lnl"][:, 0] - 1e-3)
    assert np.max(np.abs(a["weights"] - b["weights"])) < 2e-3   # (two optimisers on 510 branch lengths: the stash differs within tolerance)


def test_stage1_start_from_branch_parsimony_counts(monkeypatch):
    """The general model starts from the better of two points: the input tree's shape at the best of 17 scales, and per-branch
    Fitch parsimony counts shrunk towards that.  On loci that follow the input tree the two starts end at the
    same optimum.  With input branch lengths that are off by a factor exp(N(0, 2)) each -- same topology, same data -- the shape
    start parks branches at saturating lengths where the gradient vanishes and ends hundreds of log-units lower; the counts
    do not care what the input lengths were: same optimum as with the right tree, in fewer iterations than the shape start."""
    engine = _engine()
    from tapir_amd import nexus, synth
    L, n, nt = 24, 400, 24
    d = synth.simulate(L, n, nt, 8)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    pi = nexus.base_frequencies_from_histogram(engine.state_histogram(st, d["locus_offsets"]))
    rng = np.random.default_rng(3)
    right = np.asarray(pin["blen"], dtype=np.float64)
    wrong = right * np.exp(2.0 * rng.standard_normal(len(right)))
    res = {}
    for tree, blen in (("right", right), ("wrong", wrong)):
        plan = engine.Plan(nt, pin["parent"], blen, pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"], [1], [[0, 1]],
                           correction=pin["correction"])
        for start in ("grid", "shrunk"):
            monkeypatch.setenv("TPHIP_S1_START", start)
            res[tree, start] = plan.stage1_fit(st)
        plan.close()
    monkeypatch.delenv("TPHIP_S1_START")
    ref = res["right", "grid"]
    a = res["right", "shrunk"]
    assert np.abs(a["lnl"][:, 0] - ref["lnl"][:, 0]).max() < 1e-3
    assert (np.abs(a["exch"] - ref["exch"]) / ref["exch"]).max() < 1e-3
    b, g = res["wrong", "shrunk"], res["wrong", "grid"]
    assert np.abs(b["lnl"][:, 0] - ref["lnl"][:, 0]).max() < 1e-3            # the optimum does not depend on the input lengths
    assert (np.abs(b["exch"] - ref["exch"]) / ref["exch"]).max() < 2e-3
    assert ((b["lnl"][:, 0] - g["lnl"][:, 0]) > 1.0).sum() >= L // 2          # ... which the shape start misses by a lot
    assert (b["lnl"][:, 0] - g["lnl"][:, 0]).min() > -1e-3
    assert b["grm_iters"].mean() < g["grm_iters"].mean()


def test_stage1_fullsize_properties():
    """Stage 1 at the C3 shape (50 000 columns x 64 taxa per locus; 4 loci), through size-independent properties:
    the general model's point is stationary (gradient kernel at the returned point), nesting holds (no constrained
    model beats the general one), weights are a distribution, the averaged rates lie within the range of the models'
    rates, and the optimum does not depend on how many loci are fitted together."""
    engine = _engine()
    from tapir_amd import nexus, stage1, synth
    L, n, nt = 4, 50000, 64
    d = synth.simulate(L, n, nt, synth.WORKLOAD_SEED["C3"], device="cuda")
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].cpu().numpy()
    pi = nexus.base_frequencies_from_histogram(engine.state_histogram(st, d["locus_offsets"]))
    blen = np.asarray(pin["blen"]) / pin["correction"]
    plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"], [1], [[0, 1]],
                       correction=pin["correction"])
    res = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], blen)
    lnl, w, exch = res["lnl"], res["weights"], res["exch"]
    assert np.allclose(w.sum(1), 1.0) and np.all(w >= 0) and np.all(exch[:, 1] == 1.0)
    assert np.all(lnl[:, 1:] <= lnl[:, :1] + 1e-3 * (1 + np.abs(lnl[:, :1]) * 1e-6))       # nested models
    lo, hi = res["model_exch"].min(axis=1), res["model_exch"].max(axis=1)
    assert np.all(exch >= lo - 1e-12) and np.all(exch <= hi + 1e-12)
    # stationarity of the general model in (log rates, log lengths)
    ge, gt = res["model_exch"][:, 0], res["grm_blen"]
    val, dex, dlt, _ = plan.locus_gradient(st, gt, np.arange(L), ge)
    assert np.max(np.abs(val - lnl[:, 0]) / np.abs(val)) < 1e-9
    br = np.asarray(pin["parent"]) >= 0
    glog = np.concatenate([dex[:, [0, 2, 3, 4, 5]] * ge[:, [0, 2, 3, 4, 5]], dlt[:, br]], axis=1)
    # branches at the lower bound may keep a (small, inward-pointing) gradient; everything else must vanish
    free = np.concatenate([np.ones((L, 5), bool), gt[:, br] > 2e-10], axis=1)
    assert np.max(np.abs(glog[free])) < 2e-6 * np.abs(val).max(), np.max(np.abs(glog[free]))
    # one locus alone
    one = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], [0, n], pi[:1], np.ones((1, 6)), pin["T"], [1], [[0, 1]],
                      correction=pin["correction"])
    alone = stage1.model_averaged_exchangeabilities(one, st[:, :n], pi[:1], pin["parent"], blen)["exch"]
    assert np.max(np.abs(alone[0] - exch[0]) / exch[0]) < 1e-4
    plan.close()
    one.close()

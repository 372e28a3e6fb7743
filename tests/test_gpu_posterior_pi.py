"""The empirical-Bayes rate posterior carried into the PI rows on the GPU (tphip_eb_posterior_table, tphip_posterior_pi,
--posterior-pi) against tests/posterior_pi_reference.py and tests/eb_reference.py.  Run with -m gpu on
the MI355X box.  Every test prints its figures before it asserts.

Bounds (stated by the definitions, none tuned to the kernels):
  category posterior  |p - p_ref| <= 2 B_f max(1, fmax) p_ref: p_k = exp(f_k + log w_k - f) is a ratio of the quantities whose
                      error tests/test_gpu_eb.py bounds by B_f max(1, fmax) each (its module docstring; B_f from
                      test_gpu_numerics.BOUNDS, B_f81 + B_gtr where the oracle's GTR forms are the F81 reference); column sums
                      1 within 1e-14; sum_k p rho_k = rate / (kappa mu) within 1e-13
  counts              exact (byte-equal to the mirror fed the same table)
  analytic moments    1e-12 relative against longdouble arithmetic on the same table and the same category rows (the rows
                      themselves: 1e-13 relative against tphip_pi_tables at the category rates, one site per category)
  rows                1e-13 relative against counts . P
  summary             the bounds of tests/test_gpu_bootstrap.py::test_summary_against_numpy
"""
import functools
import math
import os
import sqlite3

import numpy as np
import pytest

import bootstrap_reference as bsr
import eb_reference as ebr
import hp_reference as hp
import posterior_pi_reference as ppr
import test_gpu_eb as geb
import test_gpu_numerics as num

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
B_F = dict(num.BOUNDS)
SIZES = [1, 3, 4, 5, 255, 256, 257, 1030]   # the Philox block of four; the draw kernel's staging tile of 256 columns
T_PI, IV_PI = 12, [[0, 5], [3, 12]]
LOCUS_IDS = np.array([5, 2 ** 33 + 1, 0, 7, 11, 3, 2 ** 40, 1], np.int64)


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _ragged(ntaxa, sizes, seed):
    """Synthetic loci of the given lengths (the first columns of equally long simulated loci)."""
    from tapir_amd import synth
    d = synth.simulate(len(sizes), max(sizes), ntaxa, seed)
    st, off0 = d["states"].numpy(), np.asarray(d["locus_offsets"])
    states = np.ascontiguousarray(np.concatenate([st[:, off0[l]:off0[l] + n] for l, n in enumerate(sizes)], axis=1))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pin = synth.plan_inputs(d["root"], d["names"])
    return states, off, pin, np.asarray(d["pi"], float), np.asarray(d["exch"], float)


@functools.lru_cache(maxsize=None)
def _batch():
    return _ragged(8, SIZES, 77)


def _pi_plan(engine, states, off, pin, pi, exch, model="gtr", **kw):
    kw.setdefault("correction", pin["correction"])
    kw.setdefault("threshold", 3)
    kw.setdefault("round_decimals", 4)
    return engine.Plan(states.shape[0], pin["parent"], pin["blen"], pin["leaf"], off, pi, None if model == "f81" else exch,
                       T_PI, [], IV_PI, model=model, **kw)


def _scales(states, off, pin):
    from tapir_amd import eb
    return eb.start_scales(states, off, pin["parent"], pin["blen"], pin["leaf"])


@functools.lru_cache(maxsize=None)
def _table(K):
    """The GPU's own table of the ragged batch at K categories, a cull of a third of the columns, and the inputs behind it."""
    engine = _engine()
    states, off, pin, pi, exch = _batch()
    L = len(SIZES)
    rho, w = geb._tables(np.linspace(0.4, 3.0, L), K)
    scales = _scales(states, off, pin)
    plan = _pi_plan(engine, states, off, pin, pi, exch)
    try:
        t = plan.eb_posterior_table(states, rho, w, scales)
    finally:
        plan.close()
    nres = np.where(np.random.default_rng(5).random(states.shape[1]) < 1 / 3, 2, 5).astype(np.int32)
    return t, nres, rho, w, scales


def _check_table(tag, post, want, bound):
    scale = np.maximum(1.0, want["fmax"])[None, :]
    e = np.abs(post - want["weights"]) / want["weights"] / (2 * bound * scale)
    print("%s: posterior error / bound %.3g  (smallest p_ref %.3g, max |f| %.1f)" % (tag, e.max(), want["weights"].min(), want["fmax"].max()))
    assert np.all(np.isfinite(post)) and np.all(post >= 0)
    assert e.max() <= 1.0, tag
    return e.max()


def _check_consistency(tag, t, plain, rho_l, km):
    s = np.abs(t["post"].sum(axis=0) - 1.0).max()
    m = np.abs((t["post"] * rho_l[:, None]).sum(axis=0) / (t["rate"] / km) - 1.0).max()
    print("%s: column sums off by %.3g, sum_k p rho_k against rate / (kappa mu) %.3g" % (tag, s, m))
    assert s <= 1e-14 and m <= 1e-13
    for k in ("rate", "sd", "lnl", "nres"):
        assert np.array_equal(t[k], plain[k]), (tag, k)


# ---- 1. the table against the 40-digit twin -----------------------------------------------------------------------
@pytest.mark.parametrize("setting", [(1.0, 4, 0.0), (0.5, 8, 2.0), (1.0, 2, 0.0), (2.0, 16, 0.0)])
@pytest.mark.parametrize("mname", ["gtr", "gtr_absent_base", "f81"])
@pytest.mark.parametrize("tname", ["balanced8", "caterpillar17"])
def test_table_against_the_40_digit_twin(mname, tname, setting):
    """The trees, models, columns and (alpha, K, log mu) of test_gpu_eb.py::test_posterior_against_the_40_digit_twin, plus K = 2
    and K = 16 with every category inside the domain [-3, kUMax] for which test_gpu_numerics.py pins B_f."""
    engine = _engine()
    alpha, K, log_mu = setting
    _, model, pi, exch = [m for m in num.MODELS if m[0] == mname][0]
    spec = dict(num.TREES)[tname]()
    rng = np.random.default_rng(len(tname) * 11 + len(mname))
    parent, blen, leaf = num._tree(spec, rng)
    ntaxa = int((leaf >= 0).sum())
    cols = num._columns(ntaxa, rng)
    cols = np.ascontiguousarray(np.concatenate([cols[:, :12], cols[:, :3]], axis=1))   # <= 12 patterns, three of them repeated
    pi_eff = hp.floored_pi(pi) if model == "gtr" else np.asarray(pi, float) / np.sum(pi)
    ref = ebr.Locus(cols, parent, blen, leaf, pi_eff, exch, hp_model=model)
    kap = hp.kappa(pi_eff, exch, model)
    rho, w = geb._tables([alpha], K)
    assert log_mu + math.log(rho.min()) >= -3.0 and log_mu + math.log(rho.max()) <= num.U_MAX
    want = ref.posterior(log_mu, alpha, K)
    plan = geb._plan(engine, ntaxa, parent, blen, leaf, [0, cols.shape[1]], [pi], None if model == "f81" else [exch], model=model)
    try:
        got = [plan.eb_posterior_table(cols, rho, w, [math.exp(log_mu)], use_patterns=pat) for pat in (False, True)]
        plain = plan.eb_posterior(cols, rho, w, [math.exp(log_mu)])
    finally:
        plan.close()
    tag = "%s %s alpha=%g K=%d" % (mname, tname, alpha, K)
    _check_table(tag, got[0]["post"], want, B_F[mname][0])
    _check_consistency(tag, got[0], plain, rho[0], float(kap) * math.exp(log_mu))
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), (tag, k)          # site patterns change no bit


# ---- 2. the three tip-word paths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["gtr", "f81"])
@pytest.mark.parametrize("ntaxa", [8, 40, 70])
def test_table_on_every_tip_word_path(ntaxa, family):
    """8, 40 and 70 taxa (2 words, 8 words, streamed words), loci of 1, 63, 64, 65 and 130 columns in one ragged plan, against
    the oracle-curve reference at the rule of test_gpu_eb.py::test_posterior_against_the_reference.  That rule holds for every
    ENTRY of the table only where each f_k meets B_f, the domain u = log(mu rho_k) in [-3, kUMax] for which test_gpu_numerics.py
    pins it (asserted below); a moment damps the loss of a category at t s << 1 by its small weight, a table entry does not.
    Seen on one MI355X with alpha = 0.2 at half the parsimony scale (u down to -19): 1.6e3 x the bound in entries of p ~ 1e-16,
    the curves' own loss that DESIGN section 9 records.  Those categories stay covered through the moments (test_gpu_eb.py) and
    through rate / sd / lnl, which are bit-identical to eb_posterior's here."""
    engine = _engine()
    sizes = [1, 63, 64, 65, 130]
    states, off, pin, pi, exch = _ragged(ntaxa, sizes, 400 + ntaxa)
    model = family
    ex = None if model == "f81" else exch
    bound = B_F[family][0] + (B_F["gtr"][0] if model == "f81" else 0.0)
    K = 8
    rho, w = geb._tables(np.array([2.0, 3.0, 5.0, 2.0, 8.0]), K)
    scales = np.array([0.5, 1.0, 0.6, 0.8, 2.0])          # per unit of the tree's depth
    assert np.all(np.log(scales[:, None] * rho) >= -3.0) and np.all(np.log(scales[:, None] * rho) <= num.U_MAX)
    plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], off, pi, ex, 10, [5], [[0, 5]], model=model)
    try:
        raw = plan.eb_posterior_table(states, rho, w, scales, use_patterns=False)
        pat = plan.eb_posterior_table(states, rho, w, scales, use_patterns=True)
        plain = plan.eb_posterior(states, rho, w, scales)
    finally:
        plan.close()
    for k in raw:
        assert np.array_equal(raw[k], pat[k]), k
    worst = 0.0
    for l in range(len(sizes)):
        sl = slice(off[l], off[l + 1])
        loc = ebr.Locus(states[:, sl], pin["parent"], pin["blen"], pin["leaf"], pi[l], None if ex is None else ex[l])
        want = loc.posterior_of(math.log(scales[l]), rho[l], w[l])
        tag = "%s %d taxa locus %d" % (family, ntaxa, l)
        worst = max(worst, _check_table(tag, raw["post"][:, sl], want, bound))
        _check_consistency(tag, {k: (v[:, sl] if k == "post" else v[sl]) for k, v in raw.items()},
                           {k: v[sl] for k, v in plain.items()}, rho[l], loc.kappa * scales[l])
    print("SEEN %s %d taxa: largest posterior error / bound %.3g" % (family, ntaxa, worst))


# ---- 3. counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 8, 16])
def test_counts_equal_the_mirror(K):
    """The GPU's own table back into tphip_posterior_pi: the counts of every replicate byte-equal to the numpy mirror of the draw
    rule, a third of the columns culled, stream ids that are not the locus indices."""
    engine = _engine()
    states, off, pin, pi, exch = _batch()
    t, nres, rho, w, scales = _table(K)
    live = nres >= 3
    plan = _pi_plan(engine, states, off, pin, pi, exch)
    try:
        for B in (2, 64, 65, 300):
            out = plan.posterior_pi(t["post"], nres, scales, rho, replicates=B, seed=2 ** 40 + 9, locus_ids=LOCUS_IDS,
                                    return_counts=True)
            differing = 0
            for l in range(len(SIZES)):
                sl = slice(off[l], off[l + 1])
                want = ppr.counts(t["post"][:, sl], live[sl], 2 ** 40 + 9, int(LOCUS_IDS[l]), B)
                differing += int((out["counts"][l] != want).sum())
                assert np.all(out["counts"][l].sum(axis=1) == live[sl].sum())
            print("K=%d B=%d: counts differing from the mirror %d of %d" % (K, B, differing, out["counts"].size))
            assert differing == 0
    finally:
        plan.close()


@pytest.mark.parametrize("nshort", [299, 520])
def test_counts_of_a_long_locus_among_many(nshort):
    """How a locus is cut into column segments depends on the workgroups the other loci supply: a locus of 600 columns among 299
    loci of two (two segments: two staging tiles, then one) and among 520 (one segment of three tiles), any table."""
    engine = _engine()
    sizes = [2] * nshort + [600]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    L, K, B = len(sizes), 8, 300
    rng = np.random.default_rng(nshort)
    post = np.ascontiguousarray(rng.dirichlet(np.full(K, 0.5), int(off[-1])).T)
    nres = np.where(rng.random(int(off[-1])) < 1 / 3, 2, 5).astype(np.int32)
    plan = engine.Plan(3, [3, 3, 4, 4, -1], [0.1, 0.1, 0.2, 0.1, 0.0], [0, 1, 2, -1, -1], off, np.full((L, 4), 0.25), np.ones((L, 6)),
                       T_PI, [], IV_PI, correction=1.0, threshold=3, round_decimals=-1)
    try:
        out = plan.posterior_pi(post, nres, np.full(L, 0.05), np.tile(np.linspace(0.2, 2.0, K), (L, 1)), replicates=B, seed=4,
                                return_counts=True)
    finally:
        plan.close()
    differing = 0
    for l in (0, 1, nshort - 1, nshort):
        sl = slice(off[l], off[l + 1])
        differing += int((out["counts"][l] != ppr.counts(post[:, sl], nres[sl] >= 3, 4, l, B)).sum())
    live = np.add.reduceat((nres >= 3).astype(np.int64), off[:-1])
    print("%d loci: counts of four loci differing from the mirror %d" % (L, differing))
    assert differing == 0 and np.array_equal(out["counts"].sum(axis=2), np.repeat(live[:, None], B, axis=1))


# ---- 4. analytic moments, rows, summary ---------------------------------------------------------------------------
def _category_rows(engine, pin, pi, exch, scales, rho, **kw):
    """The GPU's P_l[k][.] through the public call: one locus of one site per (locus, category) with a one-hot posterior, whose
    mean row is P_l[k] itself; and tphip_pi_tables' rows at the same raw rates."""
    L, K = rho.shape
    rep = np.repeat(np.arange(L), K)
    ntaxa = int((np.asarray(pin["leaf"]) >= 0).sum())
    plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], np.arange(L * K + 1), pi[rep], exch[rep], T_PI, [], IV_PI,
                       correction=pin["correction"], threshold=3, round_decimals=4, integ_mode=kw.get("integ_mode", 0))
    try:
        post = np.tile(np.eye(K), (1, L))                 # column l K + k: all of the posterior on category k
        out = plan.posterior_pi(post, None, scales[rep], rho[rep], replicates=2)
        kappa = np.asarray(plan.models()[3])
        raw = (kappa * scales[rep]) * rho.reshape(-1)
        tables = plan.pi_tables(raw, None)
    finally:
        plan.close()
    assert np.all(out["analytic"][:, 1] == 0.0)          # a one-hot posterior has no spread
    return out["analytic"][:, 0].reshape(L, K, -1), tables.reshape(L, K, -1), raw.reshape(L, K)


@pytest.mark.parametrize("integ_mode", [0, 1])
def test_moments_rows_and_summary(integ_mode):
    engine = _engine()
    states, off, pin, pi, exch = _batch()
    K, B, level = 8, 300, 0.9
    t, nres, rho, w, scales = _table(K)
    live = nres >= 3
    P, tables, raw = _category_rows(engine, pin, pi, exch, scales, rho, integ_mode=integ_mode)
    n_i = len(IV_PI)
    same_net = np.abs(P[:, :, :T_PI] - tables[:, :, :T_PI]) <= 1e-13 * np.abs(tables[:, :, :T_PI])
    same_int = np.abs(P[:, :, T_PI:] - tables[:, :, T_PI:T_PI + n_i]) <= 1e-13 * np.abs(tables[:, :, T_PI:T_PI + n_i])
    print("category rows against pi_tables at the category rates: %d net and %d integral entries beyond 1e-13 (rates %.3g .. %.3g)" % (
        int((~same_net).sum()), int((~same_int).sum()), raw.min(), raw.max()))
    assert same_net.all() and same_int.all() and np.any(P > 0)
    plan = _pi_plan(engine, states, off, pin, pi, exch, integ_mode=integ_mode)
    try:
        out = plan.posterior_pi(t["post"], nres, scales, rho, replicates=B, seed=3, level=level, locus_ids=LOCUS_IDS,
                                return_rows=True, return_counts=True)
    finally:
        plan.close()
    worst = dict(nk=0.0, mean=0.0, sd=0.0, rows=0.0, s_mean=0.0, s_sd=0.0, s_q=0.0)
    for l in range(len(SIZES)):
        sl = slice(off[l], off[l + 1])
        nk, mean, sd = ppr.analytic(t["post"][:, sl], live[sl], P[l])
        rel = lambda got, ref: float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0))   # noqa: E731
        if live[sl].any():
            worst["nk"] = max(worst["nk"], rel(out["expected_counts"][l], nk))
            worst["mean"] = max(worst["mean"], rel(out["analytic"][l, 0, 1:], mean[1:]))
            worst["sd"] = max(worst["sd"], rel(out["analytic"][l, 1, 1:], sd[1:]))
        else:
            assert np.all(out["analytic"][l] == 0.0) and np.all(out["expected_counts"][l] == 0.0)
        assert np.all(out["analytic"][l, :, 0] == 0.0)                 # PI(0) = 0
        want_rows = ppr.rows_from_counts(out["counts"][l], P[l])
        worst["rows"] = max(worst["rows"], rel(out["rows"][l], want_rows))
        ref = bsr.summarize(out["rows"][l], level)
        top = np.abs(out["rows"][l]).max(axis=0)
        e_mean, e_sd, e_q = np.abs(out["summary"][l, 0] - ref[0]), np.abs(out["summary"][l, 1] - ref[1]), np.abs(out["summary"][l, 2:] - ref[2:])
        worst["s_mean"] = max(worst["s_mean"], float(np.max(e_mean / np.maximum((B + 2) * U * np.abs(ref[0]), 1e-300))))
        worst["s_sd"] = max(worst["s_sd"], float(np.max(e_sd / np.maximum(8 * B * U * top, 1e-300))))
        worst["s_q"] = max(worst["s_q"], float(np.max(e_q / np.maximum(4 * U * np.abs(ref[2:]), 1e-300))))
        assert np.all(e_mean <= (B + 2) * U * np.abs(ref[0])) and np.all(e_sd <= 8 * B * U * top) and np.all(e_q <= 4 * U * np.abs(ref[2:]))
        # the draws scatter about the analytic moments as B draws do: 5 standard errors of the mean
        spread = out["analytic"][l, 1] > 0
        if spread.any():
            z = np.abs(out["summary"][l, 0] - out["analytic"][l, 0])[spread] / (out["analytic"][l, 1][spread] / math.sqrt(B))
            assert z.max() <= 5.0, (l, z.max())
    print("integ_mode %d: relative errors  n_lk %.3g  mean %.3g  sd %.3g  rows %.3g | summary error / bound  mean %.3f sd %.3f quantiles %.3f" % (
        integ_mode, worst["nk"], worst["mean"], worst["sd"], worst["rows"], worst["s_mean"], worst["s_sd"], worst["s_q"]))
    assert worst["nk"] <= 1e-12 and worst["mean"] <= 1e-12 and worst["sd"] <= 1e-12 and worst["rows"] <= 1e-13


# ---- 5. bit identity ----------------------------------------------------------------------------------------------
def test_bit_identity():
    """Twice; a locus alone against the same locus in the batch; minimal against preferred workspace; B = 64 against the first 64
    rows of B = 300; the device-pointer call against the host call."""
    engine = _engine()
    import torch
    states, off, pin, pi, exch = _batch()
    K, B = 8, 300
    t, nres, rho, w, scales = _table(K)
    keys = ("analytic", "expected_counts", "summary", "rows", "counts")
    plan = _pi_plan(engine, states, off, pin, pi, exch)
    try:
        kw = dict(seed=11, locus_ids=LOCUS_IDS, return_rows=True, return_counts=True)
        a = plan.posterior_pi(t["post"], nres, scales, rho, replicates=B, **kw)
        b = plan.posterior_pi(t["post"], nres, scales, rho, replicates=B, **kw)
        for k in keys:
            assert np.array_equal(a[k], b[k]), k
        small = plan.posterior_pi(t["post"], nres, scales, rho, replicates=64, **kw)
        assert np.array_equal(small["rows"], a["rows"][:, :64]) and np.array_equal(small["counts"], a["counts"][:, :64])
        assert np.array_equal(small["analytic"], a["analytic"]) and np.array_equal(small["expected_counts"], a["expected_counts"])
        # device pointers, minimal and preferred workspace
        mn, pf = plan.posterior_pi_workspace_bytes(K, B)
        print("workspace: min %d bytes, preferred %d bytes" % (mn, pf))
        assert 0 < mn < pf
        dev = torch.device("cuda:0")
        L, Wb = len(SIZES), plan.bootstrap_width
        d_post, d_nres = torch.from_numpy(t["post"]).to(dev), torch.from_numpy(nres).to(dev)
        d_scale, d_cat = torch.from_numpy(scales).to(dev), torch.from_numpy(rho).to(dev)
        ws = torch.empty(pf, dtype=torch.uint8, device=dev)
        for nbytes in (mn, pf):
            d = dict(analytic=torch.zeros((L, 2, Wb), dtype=torch.float64, device=dev),
                     expected_counts=torch.zeros((L, K), dtype=torch.float64, device=dev),
                     summary=torch.zeros((L, 4, Wb), dtype=torch.float64, device=dev),
                     rows=torch.zeros((L, B, Wb), dtype=torch.float64, device=dev),
                     counts=torch.zeros((L, B, K), dtype=torch.int32, device=dev))
            plan.posterior_pi_dev(d_post, d_nres, d_scale, d_cat, K, d["analytic"], d["expected_counts"], d["summary"], d["rows"],
                                  d["counts"], ws, B, seed=11, locus_ids=LOCUS_IDS, ws_bytes=nbytes)
            torch.cuda.synchronize()
            for k in keys:
                assert np.array_equal(d[k].cpu().numpy(), a[k]), (nbytes, k)
        d_sum = torch.zeros((L, 4, Wb), dtype=torch.float64, device=dev)
        plan.posterior_pi_dev(d_post, d_nres, d_scale, d_cat, K, d["analytic"], d["expected_counts"], d_sum, None, None, ws, B, seed=11,
                              locus_ids=LOCUS_IDS, ws_bytes=mn)          # rows and counts kept in the workspace
        torch.cuda.synchronize()
        assert np.array_equal(d_sum.cpu().numpy(), a["summary"])
        with pytest.raises(engine.TphipError):
            plan.posterior_pi_dev(d_post, d_nres, d_scale, d_cat, K, d["analytic"], d["expected_counts"], d_sum, None, None, ws, B,
                                  seed=11, ws_bytes=mn - 1)
    finally:
        plan.close()
    # locus 6 (257 columns) alone, with the stream id it has in the batch: the table and everything after it
    l = 6
    sl = slice(off[l], off[l + 1])
    alone = _pi_plan(engine, np.ascontiguousarray(states[:, sl]), [0, SIZES[l]], pin, pi[l:l + 1], exch[l:l + 1])
    try:
        t1 = alone.eb_posterior_table(np.ascontiguousarray(states[:, sl]), rho[l:l + 1], w[l:l + 1], scales[l:l + 1])
        o1 = alone.posterior_pi(t1["post"], nres[sl], scales[l:l + 1], rho[l:l + 1], replicates=B, seed=11, locus_ids=LOCUS_IDS[l:l + 1],
                                return_rows=True, return_counts=True)
    finally:
        alone.close()
    assert np.array_equal(t1["post"], t["post"][:, sl])
    for k in keys:
        assert np.array_equal(o1[k][0], a[k][l]), k


# ---- 6. arguments, empty and fully culled loci --------------------------------------------------------------------
def test_bad_arguments_and_degenerate_loci():
    engine = _engine()
    states, off, pin, pi, exch = _ragged(8, [6, 0, 9], 5)
    sizes = [6, 0, 9]
    K = 4
    rho, w = geb._tables([1.0, 1.0, 2.0], K)
    scales = np.array([0.5, 0.5, 0.5])
    plan = _pi_plan(engine, states, off, pin, pi, exch)
    try:
        t = dict(post=np.ascontiguousarray(np.random.default_rng(1).dirichlet(np.ones(K), 15).T))   # any table: [K, 15]
        nres = np.array([5] * 6 + [0] * 9, np.int32)                 # the last locus fully culled
        for kw in (dict(replicates=1), dict(replicates=4097), dict(replicates=10, level=0.0), dict(replicates=10, level=1.0)):
            with pytest.raises(engine.TphipError):
                plan.posterior_pi(t["post"], nres, scales, rho, **kw)
        for K_bad in (1, 17):
            with pytest.raises(engine.TphipError):
                plan.posterior_pi(np.full((K_bad, 15), 1.0 / K_bad), nres, scales, np.ones((3, K_bad)), replicates=10)
            with pytest.raises(engine.TphipError):
                plan.posterior_pi_workspace_bytes(K_bad, 10)
        lib = engine.load()
        opts = engine.PosteriorPiOpts(struct_size=8, replicates=10, level=0.9, seed=1, locus_ids=None, ncat=K)   # struct_size too small
        mn = engine.ctypes.c_size_t()
        assert lib.tphip_posterior_pi_workspace_bytes(plan._h, engine.ctypes.byref(opts), engine.ctypes.byref(mn), None) == 1
        out = plan.posterior_pi(t["post"], nres, scales, rho, replicates=10, return_rows=True, return_counts=True)
    finally:
        plan.close()
    for l in (1, 2):
        for k in ("analytic", "expected_counts", "summary", "rows", "counts"):
            assert np.all(out[k][l] == 0), (l, k)
    assert np.all(out["counts"][0].sum(axis=1) == sizes[0]) and np.all(out["analytic"][0, 0, 1:] > 0)


# ---- 7. the command line ------------------------------------------------------------------------------------------
def test_cli_posterior_pi_on_the_bundled_locus(golden_dir, tmp_path):
    """--rate-estimator eb --posterior-pi 200 on chr1_918: the new file with lo <= mean <= hi, every other output byte-equal to the
    run without the flag."""
    _engine()
    import shutil
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    tree = os.path.join(golden_dir, "Euteleost.tree")
    outs = {}
    for tag, extra in (("plain", []), ("posterior", ["--posterior-pi", "200"])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        outs[tag] = geb._cli(aln, tree, out, ["--site-model", "jc", "--rate-estimator", "eb"] + extra)
    geb._same_outputs(outs["plain"], outs["posterior"])
    name = "phylogenetic-informativeness-posterior.sqlite"
    assert not os.path.exists(os.path.join(outs["plain"], name))
    conn = sqlite3.connect(os.path.join(outs["posterior"], name))
    try:
        net = list(conn.execute("select time, mean, sd, lo, hi from net_posterior where id = 1 order by time"))
        epochs = list(conn.execute("select mean, sd, lo, hi from interval_posterior where id = 1"))
        cats = list(conn.execute("select k, rate, expected_sites from category where id = 1 order by k"))
        meta = dict(conn.execute("select key, value from meta"))
    finally:
        conn.close()
    assert len(net) == 174 and len(epochs) == 3 and len(cats) == 8 and meta["replicates"] == "200"
    rows = np.array([r[1:] for r in net[1:]] + epochs)
    print("posterior bands of chr1_918: largest sd / mean %.3g, categories' expected sites %s" % (
        (rows[:, 1] / rows[:, 0]).max(), ["%.1f" % c[2] for c in cats]))
    assert np.all(rows[:, 2] <= rows[:, 0]) and np.all(rows[:, 0] <= rows[:, 3]) and np.all(rows[:, 1] > 0)

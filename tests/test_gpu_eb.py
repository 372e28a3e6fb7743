"""Empirical-Bayes site rates on the GPU (tphip_eb_posterior, tphip_eb_fit_scale, tapir_amd/eb.py, --rate-estimator eb)
against tests/eb_reference.py.  Run with -m gpu on the MI355X box.  Every test prints its figures before it asserts.

Tolerances of the per-column outputs are derived, not tuned.  tests/test_gpu_numerics.py pins |df| <= B max(1, |f|) for
the column log-likelihood (B = 3e-13 GTR, 8e-13 GTR with a floored base, 1e-14 / 2e-14 F81).  ll = log sum_k w_k exp(f_k)
inherits B max(1, max_k |f_k|); the posterior mean and second moment of rho are ratios of positively weighted sums of
exp(f_k), so their relative error is at most 2 B max(1, max_k |f_k|).  Exactly that is asserted.

Those B were pinned for u in [-3, 25] on that file's trees, so the comparison with the 40-digit twin uses trees built by
that file's helpers and (mu, alpha, K) whose categories all lie in [-3, kUMax]: alpha = 1, K = 4 at log mu = 0 (lowest
category 1.99 under mu, highest 0.87 over) and alpha = 0.5, K = 8 at log mu = 2 (4.80 under: -2.80; 1.39 over: 3.39).
Everything outside that domain (5 to 256 taxa, small alpha, K = 16, categories clamped at kUMin) is compared by the same
rule with the oracle-based reference, which shares the GTR kernels' fp64 forms.  It has no closed-form F81 twin: an F81
plan is compared with the oracle's GTR forms at exchangeabilities of 1, a reference whose own error is the GTR bound, so
the bound of that comparison is B_f81 + B_gtr (the F81 kernels meet B_f81 itself against the 40-digit twin above).
Scales: every locus is evaluated near its parsimony rate (x 1, x 2.5, x 0.5).  Categories clamped at kUMin are reached the way
data reaches them, through the units of the tree: the same batch on the tree stretched by 1e4 (scales divided by 1e4), every locus at
alpha = 0.2, K = 16, puts the lowest categories below kUMin while t s of the categories that carry weight stays where it was.
(A scale 1e-3 x the parsimony rate on the unstretched tree puts ALL categories of a variable column at t s << 1, where
DESIGN section 9 records that the fp64 forms lose digits and test_gpu_numerics.py keeps a strict xfail: seen there on one
MI355X, GTR 16 / 64 taxa, error / bound up to 11 in ll and 2.6 in the moments.  That this is the curves' own loss and not the
mixture's: the plain eval_columns diagnostic against the oracle at the very same u (those loci, alpha = 0.2) misses the same B by
factors of 615 / 297 (16 / 64 taxa) at K = 2 and beyond 1e6 at K = 16, whose lowest categories reach kUMin; the mixture only
damps it, because the categories with t s << 1 carry little weight.  The expm1 forms are not part of this work.)

Fitted quantities.  The reference's own optimum comes from a derivative-free search on fp64 values, which resolves log mu
only to about sqrt(eps |l| / |l''|) ~ 1e-7; gaps seen on one MI355X are printed by every test and recorded in DESIGN section 8.
  log mu-hat at fixed alpha    |d log mu| <= BOUND_LOG_MU = 5e-7: at most 10x the largest gap seen (6.1e-8, the bundled locus)
  l at the GPU's mu-hat        l_ref(gpu) >= l_ref(ref) - (8 eps |l| + |l''| BOUND_LOG_MU^2 / 2): the rounding of the reference's
                               own sum plus what the bound on log mu allows at the optimum's curvature (seen: 2.3e-13 at |l| = 561)
  full fit vs the dense grid   l_ref(gpu mu, alpha) >= grid max - BOUND_LNL_FULL max(1, |l|), BOUND_LNL_FULL = 1e-9.  Seen: the
                               GPU's point lies ABOVE the grid's best by 2.5e-5 (the grid's nodes straddle the top), so the 10x
                               rule gives no number; the bound is the search's own resolution instead: a final bracket of
                               LOG_ALPHA_TOL = 1e-4 in log alpha at a profile curvature of order 1 to 100 costs at most 5e-7 of l
  tree scaled by 1e-2, 1, 1e2  at FIXED alpha (2, K = 8; one eb_start_scale + eb_fit_scale + eb_posterior per scale; the bundled locus and
                               three 16-taxon loci), each bound at most 10x the largest gap seen: log(mu-hat x scale) 3.3e-15 (seen
                               3.33e-16), l relative 2e-15 (1.97e-16), rate x length relative 3.1e-14 (3.11e-15).  With alpha free on the
                               same loci rounding flipped no comparison of the golden section: log alpha-hat agreed to the bit (seen 0)
                               and log(mu-hat x scale) to 4.44e-16, so the alpha-free bounds follow the same rule: 4.4e-15 for both
                               logarithms, 3.1e-14 for rate x length (seen 3.11e-15)
  sums of eb_fit_scale         l' and l'' against fourth-order differences of the reference objective: BOUND_FD, see that test
"""
import json
import math
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import eb_reference as ebr
import hp_reference as hp
import test_gpu_numerics as num

pytestmark = pytest.mark.gpu

B = dict(num.BOUNDS)            # family -> (f bound, g/h bound)
BOUND_LOG_MU = 5e-7
BOUND_LNL_FULL = 1e-9
BOUND_UNITS_MU = 3.3e-15         # tree units at fixed alpha: log(mu-hat x scale) ...
BOUND_UNITS_L = 2e-15            # ... l, relative ...
BOUND_UNITS_RATE = 3.1e-14       # ... rate x tree length, relative
BOUND_UNITS_FREE = 4.4e-15       # alpha free: log(mu-hat x scale) and log alpha-hat (rate x length: BOUND_UNITS_RATE)
EPS = 2.220446049250313e-16
BOUND_FD = 1e-8                 # sums of eb_fit_scale against fourth-order differences of the reference objective
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _plan(engine, ntaxa, parent, blen, leaf, offsets, pi, exch, model="gtr", **kw):
    return engine.Plan(ntaxa, parent, blen, leaf, offsets, pi, exch, 10, [5], [[0, 5]], model=model, **kw)


def _tables(alphas, K):
    from tapir_amd import eb
    return eb.gamma_tables(alphas, K)


def _check_posterior(tag, got, ref, km, bound_f):
    """The derived rule of the module docstring; returns the largest ratios error / bound seen."""
    scale = np.maximum(1.0, ref["fmax"])
    e_ll = np.abs(got["lnl"] - ref["ll"]) / (bound_f * scale)
    mean = got["rate"] / km
    second = (got["sd"] / km) ** 2 + mean ** 2
    e_m = np.abs(mean - ref["mean"]) / ref["mean"] / (2 * bound_f * scale)
    e_s = np.abs(second - ref["second"]) / ref["second"] / (2 * bound_f * scale)
    print("%s: error / bound  ll %.3g  mean %.3g  second %.3g   (max |f| %.1f)" % (tag, e_ll.max(), e_m.max(), e_s.max(), ref["fmax"].max()))
    assert np.all(np.isfinite(got["rate"])) and np.all(got["rate"] > 0) and np.all(got["sd"] >= 0)
    assert e_ll.max() <= 1.0 and e_m.max() <= 1.0 and e_s.max() <= 1.0, tag
    return e_ll.max(), e_m.max(), e_s.max()


@pytest.mark.parametrize("mname", ["gtr", "gtr_absent_base", "f81"])
@pytest.mark.parametrize("tname", ["balanced8", "caterpillar17"])
def test_posterior_against_the_40_digit_twin(mname, tname):
    """eb_posterior at fixed (mu, alpha, K) against the mpmath twin of the reference, inside the domain for which
    test_gpu_numerics.py pins B (module docstring): (alpha, K, log mu) = (1, 4, 0) and (0.5, 8, 2); raw columns and patterns."""
    engine = _engine()
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
    plan = _plan(engine, ntaxa, parent, blen, leaf, [0, cols.shape[1]], [pi], None if model == "f81" else [exch], model=model)
    try:
        for alpha, K, log_mu in ((1.0, 4, 0.0), (0.5, 8, 2.0)):
            rho, w = _tables([alpha], K)
            assert log_mu + math.log(rho.min()) >= -3.0 and log_mu + math.log(rho.max()) <= num.U_MAX
            want = ref.posterior(log_mu, alpha, K)
            assert np.allclose(want["weights"].sum(axis=0), 1.0, rtol=0, atol=1e-12)
            for pat in (False, True):
                got = plan.eb_posterior(cols, rho, w, [math.exp(log_mu)], use_patterns=pat)
                _check_posterior("%s %s alpha=%g K=%d patterns=%d" % (mname, tname, alpha, K, pat), got, want,
                                 kap * math.exp(log_mu), B[mname][0])
    finally:
        plan.close()


def _synthetic(ntaxa, nloci, ncols, seed):
    from tapir_amd import synth
    d = synth.simulate(nloci, ncols, ntaxa, seed)
    pin = synth.plan_inputs(d["root"], d["names"])
    return d["states"].numpy(), np.asarray(d["locus_offsets"]), pin, np.asarray(d["pi"], float), np.asarray(d["exch"], float)


def _bundled(chr1_918):
    c = chr1_918
    return (c["states"], np.array([0, c["states"].shape[1]]), dict(parent=c["parent"], blen=c["blen"], leaf=c["leaf"]),
            c["pi"][None, :], c["exch"][None, :])


@pytest.mark.parametrize("ntaxa", [5, 16, 64])
def test_f81_posterior_against_the_40_digit_twin_on_larger_trees(chr1_918, ntaxa):
    """F81 plans at 5 (the bundled locus), 16 and 64 taxa against the 40-digit twin at the issue's own B (1e-14: ll B, moments
    2 B), not the B_f81 + B_gtr of the oracle comparison below: ten site patterns of the first locus (its first columns, the
    constant ones included), categories inside [-3, kUMax]: (alpha, K, log mu) = (1, 4, -1), lowest category at -2.99 and close
    to where these loci's fits end, and (0.5, 8, 2).  256 taxa stay with the oracle comparison: the twin's plain pruning in
    mpmath is too slow there."""
    engine = _engine()
    if ntaxa == 5:
        states, off, pin, pi, _ = _bundled(chr1_918)
    else:
        states, off, pin, pi, _ = _synthetic(ntaxa, 1, 200, 300 + ntaxa)
    pat, _, _ = ebr.patterns(states[:, off[0]:off[1]])
    const = (pat == pat[0]).all(axis=0)
    keep = np.concatenate([np.flatnonzero(const)[:3], np.flatnonzero(~const)[:7]])
    cols = np.ascontiguousarray(np.concatenate([pat[:, keep], pat[:, keep[:2]]], axis=1))   # two patterns repeated
    ref = ebr.Locus(cols, pin["parent"], pin["blen"], pin["leaf"], pi[0], None, hp_model="f81")
    kap = hp.kappa(pi[0], None, "f81")
    plan = _plan(engine, states.shape[0], pin["parent"], pin["blen"], pin["leaf"], [0, cols.shape[1]], pi[:1], None, model="f81")
    try:
        for alpha, K, log_mu in ((1.0, 4, -1.0), (0.5, 8, 2.0)):
            rho, w = _tables([alpha], K)
            assert log_mu + math.log(rho.min()) >= -3.0 and log_mu + math.log(rho.max()) <= num.U_MAX
            want = ref.posterior(log_mu, alpha, K)
            for pat_mode in (False, True):
                got = plan.eb_posterior(cols, rho, w, [math.exp(log_mu)], use_patterns=pat_mode)
                _check_posterior("f81 twin %d taxa alpha=%g K=%d patterns=%d" % (ntaxa, alpha, K, pat_mode), got, want,
                                 kap * math.exp(log_mu), B["f81"][0])
    finally:
        plan.close()


@pytest.mark.parametrize("family", ["gtr", "gtr_absent_base", "f81"])
@pytest.mark.parametrize("ntaxa", [5, 16, 64, 256])
def test_posterior_against_the_reference(chr1_918, ntaxa, family):
    """eb_posterior against the oracle-based reference by the derived rule: 5 taxa (the bundled locus), 16, 64 and 256 taxa
    (synthetic, three loci in one batch with different mu and alpha, one of them with alpha = 0.2); K = 2, 4, 8, 16; then the
    batch on the tree stretched by 1e4, where categories sit at kUMin; raw columns and site patterns, which must agree bit for bit."""
    engine = _engine()
    from tapir_amd import eb
    if ntaxa == 5:
        states, off, pin, pi, exch = _bundled(chr1_918)
    else:
        states, off, pin, pi, exch = _synthetic(ntaxa, 3, 40, 100 + ntaxa)
    L = len(off) - 1
    pi = pi.copy()
    if family == "gtr_absent_base":
        pi[:, 3] = 0.0
        pi /= pi.sum(axis=1, keepdims=True)
    model = "f81" if family == "f81" else "gtr"
    pi_eff = np.array([hp.floored_pi(p) for p in pi]) if model == "gtr" else pi
    ex = None if model == "f81" else exch
    start = eb.start_scales(states, off, pin["parent"], pin["blen"], pin["leaf"])
    alphas = np.array([0.7, 3.0, 0.2])[:L]
    scales = (start * np.array([1.0, 2.5, 0.5])[:L])
    bound = B[family][0] + (B["gtr"][0] if model == "f81" else 0.0)   # module docstring: the oracle's GTR forms are the F81 reference
    refs = [ebr.Locus(states[:, off[l]:off[l + 1]], pin["parent"], pin["blen"], pin["leaf"], pi_eff[l], None if ex is None else ex[l])
            for l in range(L)]
    plan = _plan(engine, states.shape[0], pin["parent"], pin["blen"], pin["leaf"], off, pi, ex, model=model)
    try:
        for K in (2, 4, 8, 16):
            rho, w = _tables(alphas, K)
            raw = plan.eb_posterior(states, rho, w, scales, use_patterns=False)
            pat = plan.eb_posterior(states, rho, w, scales, use_patterns=True)
            for k in ("rate", "sd", "lnl", "nres"):
                assert np.array_equal(raw[k], pat[k]), (k, K)
            for l in range(L):
                sl = slice(off[l], off[l + 1])
                want = refs[l].posterior_of(math.log(scales[l]), rho[l], w[l])
                _check_posterior("%s %d taxa K=%d locus %d" % (family, ntaxa, K, l), {k: raw[k][sl] for k in raw}, want,
                                 refs[l].kappa * scales[l], bound)
                assert np.array_equal(raw["nres"][sl], ebr.orc.informative_counts(states[:, sl]))
    finally:
        plan.close()
    # the clamp at kUMin, reached through the units of the tree
    stretch, K = 1e4, 16
    blen = np.asarray(pin["blen"], float) * stretch
    rho, w = _tables(np.full(L, 0.2), K)   # every locus at the smallest shape: lowest category 14.5 log-units under mu
    plan = _plan(engine, states.shape[0], pin["parent"], blen, pin["leaf"], off, pi, ex, model=model)
    try:
        got = plan.eb_posterior(states, rho, w, scales / stretch)
    finally:
        plan.close()
    clamped = 0
    for l in range(L):
        sl = slice(off[l], off[l + 1])
        ref = ebr.Locus(states[:, sl], pin["parent"], blen, pin["leaf"], pi_eff[l], None if ex is None else ex[l])
        clamped += int(np.sum(math.log(scales[l] / stretch) + np.log(rho[l]) < ebr.U_MIN))
        want = ref.posterior_of(math.log(scales[l] / stretch), rho[l], w[l])
        _check_posterior("%s %d taxa K=%d locus %d, tree x 1e4" % (family, ntaxa, K, l), {k: got[k][sl] for k in got}, want,
                         ref.kappa * scales[l] / stretch, bound)
    assert clamped > 0


def test_fit_scale_against_the_reference(chr1_918):
    """tphip_eb_fit_scale at fixed categories: the sums at the start point (maxit_scale = 1 evaluates once and moves
    nowhere) against the reference objective and its central second difference, then the converged scale against the
    reference's derivative-free optimum (bounds: module docstring).
    The sums: l at the start against the reference objective; l'' against its fourth-order central second difference; l'
    through the Newton step the kernel takes from them (maxit_scale = 2 evaluates at the start, steps by -l' / l'' and stops:
    l' = -log(scale / start) l''), against the fourth-order central first difference.  Step d = 1e-2: truncation d^4 / 90
    |l^(6)| and d^4 / 30 |l^(5)| ~ 1e-10 of the derivative's size, rounding 6 eps |l| / d^2 ~ 4e-8 and 2 eps |l| / d ~ 1e-10 at
    |l| = 3000 if the reference's values were exact; they carry the oracle curves' own error (up to the l bound above, ~1e-9),
    which the differences amplify by 1.5 / d and 5.3 / d^2.  BOUND_FD = 1e-8 max(1, |l'|, |l''|) is at most 10x the largest gap
    seen on one MI355X (l': 2.2e-7 at max(|l'|, |l''|) = 233, i.e. 9.3e-10; l'': 5.1e-8, i.e. 2.2e-10).
    Gaps seen on one MI355X: module docstring and DESIGN section 8."""
    engine = _engine()
    from tapir_amd import eb
    cases = [("bundled",) + _bundled(chr1_918), ("synthetic16",) + _synthetic(16, 4, 300, 7)]
    worst_u = worst_l = 0.0
    for name, states, off, pin, pi, exch in cases:
        L = len(off) - 1
        start = eb.start_scales(states, off, pin["parent"], pin["blen"], pin["leaf"])
        alphas = np.array([1.0, 0.4, 5.0, 2.0])[:L]
        K = 8
        rho, w = _tables(alphas, K)
        plan = _plan(engine, states.shape[0], pin["parent"], pin["blen"], pin["leaf"], off, pi, exch)
        try:
            one = plan.eb_fit_scale(states, rho, w, start, maxit_scale=1)
            two = plan.eb_fit_scale(states, rho, w, start, maxit_scale=2)
            fit = plan.eb_fit_scale(states, rho, w, start)
            fit_raw = plan.eb_fit_scale(states, rho, w, start, use_patterns=False)
        finally:
            plan.close()
        for k in ("scale", "locus_lnl", "curvature"):
            assert np.array_equal(fit[k], fit_raw[k]), k          # site patterns change no bit of the fit
        assert np.all(one["iters"] == -1) and np.allclose(one["scale"], start, rtol=1e-14, atol=0)   # exp(log(start))
        assert np.all(fit["iters"] > 0), fit["iters"]             # converged
        for l in range(L):
            ref = ebr.Locus(states[:, off[l]:off[l + 1]], pin["parent"], pin["blen"], pin["leaf"], pi[l], exch[l])
            u0, d = math.log(start[l]), 1e-2
            fm2, fm, f0, fp, fp2 = (ref.objective_of(u0 + j * d, rho[l], w[l]) for j in (-2, -1, 0, 1, 2))
            h_fd = (-fp2 + 16 * fp - 30 * f0 + 16 * fm - fm2) / (12 * d ** 2)
            g_fd = (-fp2 + 8 * fp - 8 * fm + fm2) / (12 * d)
            step = math.log(two["scale"][l] / start[l])
            assert 0 < abs(step) < 2.0 and one["curvature"][l] < 0      # a plain Newton step, not the bracket's or the limit's
            g_gpu = -step * one["curvature"][l]
            post = ref.posterior_of(u0, rho[l], w[l])
            lnl_bound = B["gtr"][0] * float(np.sum(np.maximum(1.0, post["fmax"])))
            fd_bound = BOUND_FD * max(1.0, abs(g_fd), abs(h_fd))
            print("%s locus %d start: l gap %.3g (bound %.3g)  l'' %.9g vs difference %.9g (gap %.3g)  l' %.9g vs difference %.9g (gap %.3g; "
                  "bound %.3g)" % (name, l, abs(one["locus_lnl"][l] - f0), lnl_bound, one["curvature"][l], h_fd,
                                   abs(one["curvature"][l] - h_fd), g_gpu, g_fd, abs(g_gpu - g_fd), fd_bound))
            assert abs(one["locus_lnl"][l] - f0) <= lnl_bound
            assert abs(one["curvature"][l] - h_fd) <= fd_bound
            assert abs(g_gpu - g_fd) <= fd_bound
            u_ref, l_ref = ref.fit_scale_of(rho[l], w[l])
            u_gpu = math.log(fit["scale"][l])
            l_at_gpu = ref.objective_of(u_gpu, rho[l], w[l])
            slope = (ref.objective_of(u_gpu + 1e-4, rho[l], w[l]) - ref.objective_of(u_gpu - 1e-4, rho[l], w[l])) / 2e-4
            print("%s locus %d fit: log mu gpu %.10f ref %.10f gap %.3g | l_ref(gpu) - l_ref(ref) %.3g (|l| %.1f) | slope at gpu %.3g | "
                  "curvature %.5g | iters %d" % (name, l, u_gpu, u_ref, abs(u_gpu - u_ref), l_at_gpu - l_ref, abs(l_ref), slope,
                                                 fit["curvature"][l], fit["iters"][l]))
            worst_u = max(worst_u, abs(u_gpu - u_ref))
            worst_l = max(worst_l, (l_ref - l_at_gpu) / max(1.0, abs(l_ref)))
            assert abs(u_gpu - u_ref) <= BOUND_LOG_MU
            assert l_at_gpu >= l_ref - (8 * EPS * abs(l_ref) + 0.5 * abs(fit["curvature"][l]) * BOUND_LOG_MU ** 2)
            assert abs(slope) <= 1e-3 * max(1.0, abs(fit["curvature"][l]))   # the slope vanishes at the GPU's optimum
            assert abs(fit["locus_lnl"][l] - l_at_gpu) <= lnl_bound
    print("SEEN fit_scale: largest |d log mu| %.3g, largest relative objective deficit %.3g" % (worst_u, worst_l))


def test_full_estimate_against_a_dense_grid(chr1_918):
    """alpha free (tapir_amd/eb.py on the real engine): the reference objective at the GPU's (mu-hat, alpha-hat) against the
    maximum of the reference objective over a dense grid of 200 log alpha values in the search interval, each with its own
    optimal mu.  A search stuck in the wrong place shows here even if two searches agree."""
    engine = _engine()
    from tapir_amd import eb
    states, off, pin, pi, exch = _bundled(chr1_918)
    K = 8
    plan = _plan(engine, states.shape[0], pin["parent"], pin["blen"], pin["leaf"], off, pi, exch)
    try:
        est = eb.estimate(plan, states, ncat=K)
    finally:
        plan.close()
    ref = ebr.Locus(states, pin["parent"], pin["blen"], pin["leaf"], pi[0], exch[0])
    la = np.linspace(math.log(eb.ALPHA_BOUNDS[0]), math.log(eb.ALPHA_BOUNDS[1]), 200)
    prof = ref.profile(K, la)
    at_gpu = ref.objective(math.log(est["scale"][0]), est["alpha"][0], K)
    print("full fit: alpha-hat %.6f mu-hat %.6g l_gpu(own) %.9f | l_ref(gpu point) %.9f | grid max %.9f at alpha %.4f | deficit %.3g | "
          "rounds %d evaluations per column %d" % (est["alpha"][0], est["scale"][0], est["locus_lnl"][0], at_gpu, prof.max(),
                                                   math.exp(la[int(np.argmax(prof))]), prof.max() - at_gpu, est["rounds"], est["evaluations"]))
    assert at_gpu >= prof.max() - BOUND_LNL_FULL * max(1.0, abs(prof.max()))
    assert abs(math.log(est["alpha"][0]) - la[int(np.argmax(prof))]) <= (la[1] - la[0])   # within one grid cell of the grid's best
    const = (np.where(states == 0, 15, states & 15) == np.where(states[0] == 0, 15, states[0] & 15)).all(axis=0)
    assert const.sum() > 100 and np.all(est["rate"][const] > 0) and np.all(np.isfinite(est["rate"]))


def test_outputs_do_not_depend_on_the_batch():
    """Bit for bit at fixed hyperparameters: a locus' per-column outputs and its fit do not depend on the other loci of the
    batch (alone, first of four, last of four with the others in another order)."""
    engine = _engine()
    from tapir_amd import eb
    states, off, pin, pi, exch = _synthetic(16, 4, 700, 21)
    K = 4
    alphas = np.array([0.5, 1.0, 2.0, 8.0])
    start = eb.start_scales(states, off, pin["parent"], pin["blen"], pin["leaf"])
    rho, w = _tables(alphas, K)

    def run(order):
        st = np.ascontiguousarray(np.concatenate([states[:, off[l]:off[l + 1]] for l in order], axis=1))
        o = np.concatenate([[0], np.cumsum([off[l + 1] - off[l] for l in order])])
        plan = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], o, pi[order], exch[order])
        try:
            fit = plan.eb_fit_scale(st, rho[order], w[order], start[order])
            post = plan.eb_posterior(st, rho[order], w[order], fit["scale"])
        finally:
            plan.close()
        return fit, post, o

    full_fit, full_post, o_full = run([0, 1, 2, 3])
    for order in ([2], [3, 1, 0, 2], [2, 0]):
        fit, post, o = run(order)
        i = order.index(2)
        for k in ("scale", "locus_lnl", "curvature", "iters"):
            assert fit[k][i] == full_fit[k][2], (order, k)
        for k in ("rate", "sd", "lnl", "nres"):
            assert np.array_equal(post[k][o[i]:o[i + 1]], full_post[k][o_full[2]:o_full[3]]), (order, k)


def _scaled_cases(chr1_918):
    return [("bundled",) + _bundled(chr1_918), ("synthetic16",) + _synthetic(16, 3, 300, 11)]


def test_fit_at_fixed_alpha_does_not_depend_on_the_units_of_the_tree(chr1_918):
    """The same loci on the tree scaled by 1e-2, 1 and 1e2 at FIXED alpha (2, K = 8): one eb_start_scale + eb_fit_scale +
    eb_posterior per scale.  mu-hat x scale, l and rate x tree length must agree within BOUND_UNITS_* (module docstring: at
    most 10x the largest gap seen).  At 1e2 x the tree a start at siteRate = 1 would sit on the plateau of l; the library's
    start and the bracket must not care, nor may the absolute constants kUMin and kStepMax show."""
    engine = _engine()
    worst = [0.0, 0.0, 0.0]
    for name, states, off, pin, pi, exch in _scaled_cases(chr1_918):
        L = len(off) - 1
        rho, w = _tables(np.full(L, 2.0), 8)
        res = {}
        for s in (1e-2, 1.0, 1e2):
            blen = np.asarray(pin["blen"], float) * s
            plan = _plan(engine, states.shape[0], pin["parent"], blen, pin["leaf"], off, pi, exch)
            try:
                start = plan.eb_start_scale(states)
                fit = plan.eb_fit_scale(states, rho, w, start)
                post = plan.eb_posterior(states, rho, w, fit["scale"])
            finally:
                plan.close()
            assert np.all(fit["iters"] > 0)
            res[s] = (start, fit, post, blen[np.asarray(pin["parent"]) >= 0].sum())
        b_start, b_fit, b_post, b_len = res[1.0]
        for s in (1e-2, 1e2):
            start, fit, post, length = res[s]
            d_start = np.max(np.abs(np.log(start * s / b_start)))
            d_mu = np.max(np.abs(np.log(fit["scale"] * s / b_fit["scale"])))
            d_l = np.max(np.abs(fit["locus_lnl"] - b_fit["locus_lnl"]) / np.abs(b_fit["locus_lnl"]))
            d_rate = np.max(np.abs(post["rate"] * length / (b_post["rate"] * b_len) - 1.0))
            print("fixed alpha, %s, tree x %g: |d log(start x scale)| %.3g  |d log(mu x scale)| %.3g  l relative %.3g  rate x length "
                  "relative %.3g  iters %s vs %s" % (name, s, d_start, d_mu, d_l, d_rate, fit["iters"], b_fit["iters"]))
            worst = [max(a, b) for a, b in zip(worst, (d_mu, d_l, d_rate))]
            assert d_mu <= BOUND_UNITS_MU and d_l <= BOUND_UNITS_L and d_rate <= BOUND_UNITS_RATE
    print("SEEN units at fixed alpha: log(mu x scale) %.3g, l relative %.3g, rate x length relative %.3g" % tuple(worst))


def test_full_fit_does_not_depend_on_the_units_of_the_tree(chr1_918):
    """The same with alpha free (tapir_amd/eb.py): mu-hat x scale, alpha-hat and rate x tree length within BOUND_UNITS_FREE / BOUND_UNITS_RATE
    (module docstring)."""
    engine = _engine()
    from tapir_amd import eb
    worst = [0.0, 0.0, 0.0]
    for name, states, off, pin, pi, exch in _scaled_cases(chr1_918):
        res = {}
        for s in (1e-2, 1.0, 1e2):
            blen = np.asarray(pin["blen"], float) * s
            plan = _plan(engine, states.shape[0], pin["parent"], blen, pin["leaf"], off, pi, exch)
            try:
                res[s] = eb.estimate(plan, states, ncat=8)
            finally:
                plan.close()
            res[s]["length"] = blen[np.asarray(pin["parent"]) >= 0].sum()
        base = res[1.0]
        for s in (1e-2, 1e2):
            r = res[s]
            d_mu = np.max(np.abs(np.log(r["scale"] * s / base["scale"])))
            d_al = np.max(np.abs(np.log(r["alpha"] / base["alpha"])))
            d_rate = np.max(np.abs(r["rate"] * r["length"] / (base["rate"] * base["length"]) - 1.0))
            print("alpha free, %s, tree x %g: |d log(mu x scale)| %.3g  |d log alpha| %.3g  rate x length relative %.3g" % (
                name, s, d_mu, d_al, d_rate))
            worst = [max(a, b) for a, b in zip(worst, (d_mu, d_al, d_rate))]
            assert d_mu <= BOUND_UNITS_FREE and d_al <= BOUND_UNITS_FREE and d_rate <= BOUND_UNITS_RATE
    print("SEEN units, alpha free: log(mu x scale) %.3g, log alpha %.3g, rate x length relative %.3g" % tuple(worst))


def test_start_scale():
    """tphip_eb_start_scale: positive and finite, 1 / tree length for a locus without a change, the same bits whatever the batch;
    the fit converges from it within kStepMax of where it started."""
    engine = _engine()
    states, off, pin, pi, exch = _synthetic(16, 3, 300, 13)
    states = states.copy()
    states[:, off[1]:off[2]] = 1          # locus 1: nothing but A
    plan = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], off, pi, exch)
    alone = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], [0, off[3] - off[2]], pi[2:], exch[2:])
    try:
        s = plan.eb_start_scale(states)
        s2 = alone.eb_start_scale(np.ascontiguousarray(states[:, off[2]:off[3]]))
        rho, w = _tables(np.full(3, 1.0), 4)
        fit = plan.eb_fit_scale(states, rho, w, s)
    finally:
        plan.close()
        alone.close()
    length = np.asarray(pin["blen"], float)[np.asarray(pin["parent"]) >= 0].sum()
    print("start scales %s, fitted %s, iters %s" % (s, fit["scale"], fit["iters"]))
    assert np.all(np.isfinite(s)) and np.all(s > 0) and abs(s[1] * length - 1.0) < 1e-14 and s2[0] == s[2]
    assert np.all(fit["iters"] > 0) and np.all(np.abs(np.log(fit["scale"][[0, 2]] / s[[0, 2]])) < 2.0)


def test_validation_f81_and_the_plans_own_mixture():
    """Errors, not crashes, for bad options and tables; an F81 plan is accepted; the plan's own rate mixture is ignored."""
    engine = _engine()
    states, off, pin, pi, exch = _synthetic(16, 2, 200, 5)
    rho, w = _tables([1.0, 2.0], 4)
    plan = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], off, pi, exch)
    mixed = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], off, pi, exch, cat_rates=[0.5, 1.5], cat_weights=[0.5, 0.5])
    f81 = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], off, pi, None, model="f81")
    try:
        good = plan.eb_posterior(states, rho, w, [0.01, 0.02])
        for bad in (dict(cat_rate=rho[:, :1], cat_weight=w[:, :1]), dict(cat_rate=np.tile(rho, (1, 5))[:, :17], cat_weight=np.full((2, 17), 1 / 17)),
                    dict(cat_rate=-rho), dict(cat_weight=w * 0), dict(scale=[0.01, 0.0]), dict(scale=[0.01, -1.0]),
                    dict(cat_rate=np.where(rho > 1, np.nan, rho))):
            args = dict(cat_rate=rho, cat_weight=w, scale=[0.01, 0.02])
            args.update(bad)
            with pytest.raises(engine.TphipError):
                plan.eb_posterior(states, args["cat_rate"], args["cat_weight"], args["scale"])
            with pytest.raises(engine.TphipError):
                plan.eb_fit_scale(states, args["cat_rate"], args["cat_weight"], args["scale"])
        lib = engine.load()
        opts = engine.EbOpts(4, 4, 0, 1, 0.0)   # struct_size too small
        sc = np.array([0.01, 0.02])
        assert lib.tphip_eb_fit_scale(plan._h, states.ctypes.data, opts, rho.ctypes.data, w.ctypes.data, sc.ctypes.data, None, None, None) == 1
        opts = engine.EbOpts(24, 4, 0, 1, 0.0)
        assert lib.tphip_eb_fit_scale(plan._h, states.ctypes.data, opts, None, w.ctypes.data, sc.ctypes.data, None, None, None) == 1
        again = mixed.eb_posterior(states, rho, w, [0.01, 0.02])
        for k in good:
            assert np.array_equal(good[k], again[k]), k
        jc = f81.eb_posterior(states, rho, w, [0.01, 0.02])
        ones = _plan(engine, 16, pin["parent"], pin["blen"], pin["leaf"], off, pi, np.ones((2, 6)))
        try:
            gtr1 = ones.eb_posterior(states, rho, w, [0.01, 0.02])
        finally:
            ones.close()
        assert np.allclose(jc["rate"], gtr1["rate"], rtol=1e-9) and np.allclose(jc["lnl"], gtr1["lnl"], rtol=1e-10)
        assert np.array_equal(jc["nres"], good["nres"])
    finally:
        plan.close()
        mixed.close()
        f81.close()


def _cli(aln, tree, out, extra, env=None):
    argv = [str(aln), str(tree), "--output", str(out), "--times", "10,20,50", "--intervals", "0-10,10-15,20-100"] + list(extra)
    code = ("import sys; sys.path.insert(0, %r); from tapir_amd import cli; o = cli.main(%r); print('OUT=' + o)" % (ROOT, argv))
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("OUT=")][-1]


def _sqlite_dump(path):
    conn = sqlite3.connect(path)
    rows = [list(conn.execute("select * from %s order by rowid" % t)) for t in ("loci", "net", "discrete", "interval")]
    conn.close()
    return rows


def _same_outputs(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".rates"))
    assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".rates"))
    for f in names:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert _sqlite_dump(os.path.join(a, "phylogenetic-informativeness.sqlite")) == _sqlite_dump(os.path.join(b, "phylogenetic-informativeness.sqlite"))


def _check_rates_document(path, states, parent, blen, leaf, pi, exch, K):
    """A .rates document of an eb run against the reference posterior at the document's own (alpha, scale), and that point
    against the reference's own fit."""
    from tapir_amd import compute
    doc = json.load(open(path))["sites"]
    assert doc["estimator"] == "eb" and doc["gamma_categories"] == K
    ref = ebr.Locus(states, parent, blen, leaf, pi, exch)
    want = ref.posterior(math.log(doc["gamma_scale"]), doc["gamma_alpha"], K)
    got = {k: np.array([r[k] for r in doc["rates"]]) for k in ("rate", "sd", "ll", "subst")}
    assert np.abs(got["rate"] - compute.round_like_hyphy(want["rate"], 4)).max() <= 1e-4 + 1e-12
    assert np.abs(got["sd"] - compute.round_like_hyphy(want["sd"], 4)).max() <= 1e-4 + 1e-12
    assert np.abs(got["ll"] - want["ll"]).max() < 5.1e-5
    assert abs(doc["locus_lnl"] - ref.objective(math.log(doc["gamma_scale"]), doc["gamma_alpha"], K)) <= 1e-9 * abs(doc["locus_lnl"])
    return doc, ref


def test_cli_eb_on_the_bundled_locus(golden_dir, tmp_path, oracle):
    """--rate-estimator eb on chr1_918 (two copies, --site-model jc so that no stage 1 runs): documents against the CPU
    reference, the fitted point against the reference's own search, PI tables against oracle.worker_tables on the
    document's rates; the streamed block pipeline writes the same bytes as the unstreamed run."""
    _engine()
    from tapir_amd import newick, nexus
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln / "chr1_918_copy.nex")
    tree = os.path.join(golden_dir, "Euteleost.tree")
    outs = {}
    for tag, env in (("plain", dict(TPHIP_NO_STREAM="1")), ("streamed", dict(TPHIP_STREAM_BLOCK="1"))):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        outs[tag] = _cli(aln, tree, out, ["--site-model", "jc", "--rate-estimator", "eb", "--multiprocessing"], env)
    _same_outputs(outs["plain"], outs["streamed"])
    names, st = nexus.read_states(os.path.join(golden_dir, "chr1_918.nex"))
    root = newick.read_tree(os.path.join(outs["plain"], "Tree_100_174.0.newick"))
    leaf_names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, leaf_names)
    st = st[[names.index(n) for n in leaf_names]]
    doc, ref = _check_rates_document(os.path.join(outs["plain"], "chr1_918.nex.rates"), st, parent, blen, leaf, np.full(4, 0.25), None, 8)
    u_ref, a_ref, l_ref = ref.fit(8)
    print("cli bundled: alpha %.6f (ref %.6f)  scale %.6g (ref %.6g)  l %.9f (ref %.9f)" % (
        doc["gamma_alpha"], a_ref, doc["gamma_scale"], math.exp(u_ref), doc["locus_lnl"], l_ref))
    assert doc["locus_lnl"] >= l_ref - BOUND_LNL_FULL * abs(l_ref)
    rates = np.array([r["rate"] for r in doc["rates"]]) / 100
    assert np.array_equal(rates, np.array([r["rate"] for r in doc["corrected_rates"]]))
    rates[oracle.informative_counts(st) < 3] = np.nan
    pi_net, pi_times, pi_epochs = oracle.worker_tables(rates, 174, [10, 20, 50], [[0, 10], [10, 15], [20, 100]])
    rows = _sqlite_dump(os.path.join(outs["plain"], "phylogenetic-informativeness.sqlite"))
    assert np.allclose([p for i, t, p in rows[1] if i == 1], pi_net, rtol=1e-9, atol=1e-300)


def test_cli_eb_on_a_synthetic_directory(tmp_path):
    """--rate-estimator eb on six 64-taxon synthetic loci with given exchangeabilities and a fixed shape: every document
    against the CPU reference at its own fit, streamed and unstreamed runs writing the same bytes."""
    _engine()
    from tapir_amd import newick, nexus, synth
    d = synth.simulate(6, 120, 64, 33)
    aln = tmp_path / "aln"
    aln.mkdir()
    tree = synth.write_nexus_dir(str(aln), d["states"].numpy(), d["locus_offsets"], d["names"], d["root"])
    exch = [1.0, 2.5, 0.7, 1.3, 3.1, 1.0]
    extra = ["--exchangeabilities", ",".join(map(str, exch)), "--rate-estimator", "eb", "--eb-categories", "4", "--eb-alpha", "0.8", "--multiprocessing"]
    outs = {}
    for tag, env in (("plain", dict(TPHIP_NO_STREAM="1")), ("streamed", dict(TPHIP_STREAM_BLOCK="2"))):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        outs[tag] = _cli(aln, tree, out, extra, env)
    _same_outputs(outs["plain"], outs["streamed"])
    tname = [f for f in os.listdir(outs["plain"]) if f.startswith("Tree_")][0]
    root = newick.read_tree(os.path.join(outs["plain"], tname))
    leaf_names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, leaf_names)
    files = sorted(f for f in os.listdir(str(aln)) if f.endswith(".nex") or f.endswith(".nexus"))
    for f in files[:3]:
        names, st = nexus.read_states(os.path.join(str(aln), f))
        st = st[[names.index(n) for n in leaf_names]]
        doc = json.load(open(os.path.join(outs["plain"], f + ".rates")))["sites"]
        pi = np.array([doc["freqs"][b] for b in "ACGT"])
        _check_rates_document(os.path.join(outs["plain"], f + ".rates"), st, parent, blen, leaf, pi, exch, 4)

"""The high-precision references of tests/hp_reference.py against the CPU oracle and scipy, the closed-form interval
integral against the exact value, and the clamp of the kernels' table exponential (on its bit-level emulation).  CPU
only."""
import math

import mpmath
import numpy as np
import pytest

import fast_exp_emulation as fexp
import hp_reference as hp
import test_gpu_numerics as num


def test_column_curves_agree_with_the_oracle(oracle):
    """Ordinary inputs: a 12-taxon synthetic locus, GTR and F81 (exchangeabilities of 1)."""
    from tapir_amd import synth
    d = synth.simulate(2, 24, 12, 21)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()[:, :24]
    u = np.array([-4.0, -1.0, 0.0, 0.8, 3.0])
    for model, exch in (("gtr", d["exch"][0]), ("f81", None)):
        ex = np.ones(6) if exch is None else exch
        F, G, H = hp.column_curves(st, pin["parent"], pin["blen"], pin["leaf"], d["pi"][0], exch, u, model=model)
        for c in range(st.shape[1]):
            f, g, h = oracle.column_curve(st, pin["parent"], pin["blen"], pin["leaf"], d["pi"][0], ex, c, u)
            assert np.all(np.abs(f - F[:, c]) <= 1e-12 * np.maximum(1.0, np.abs(F[:, c]))), (model, c)
            assert np.all(np.abs(g - G[:, c]) <= 1e-10 * (1.0 + np.abs(H[:, c]))), (model, c)
            assert np.all(np.abs(h - H[:, c]) <= 1e-10 * (1.0 + np.abs(H[:, c]))), (model, c)
        assert abs(hp.kappa(d["pi"][0], ex) - oracle.gtr_eigen(d["pi"][0], ex)[3]) < 1e-15


DEEP_MODELS = [  # (name, pi, exchangeabilities for the oracle, the reference's exch, the reference's model)
    ("gtr", num.MODELS[0][2], num.MODELS[0][3], num.MODELS[0][3], "gtr"),
    ("gtr_skewed", hp.SKEW_PI, hp.SKEW_EXCH, hp.SKEW_EXCH, "gtr"),
    ("f81_skewed", hp.SKEW_PI, [1.0] * 6, None, "f81"),    # the oracle's stand-in for F81: exchangeabilities of 1
]
DEEP_U = [-3.0, 0.0, 3.0, num.U_MAX, 17.0, 25.0]
# of test_gpu_numerics._columns: all A, all T, all different, one resolved cell, IUPAC masks 2, 6, 13 and 15 (gaps) on every other
# taxon, two random columns
DEEP_COLUMNS = [0, 3, 4, 5, 8, 12, 19, 21, 22, 24]


@pytest.mark.parametrize("ntaxa", [16, 64, 130, 300])
@pytest.mark.parametrize("mname,pi,exch,ref_exch,ref_model", DEEP_MODELS, ids=[m[0] for m in DEEP_MODELS])
def test_oracle_curve_on_deep_trees_at_far_rates(oracle, mname, pi, exch, ref_exch, ref_model, ntaxa):
    """The rule of test_column_curves_agree_with_the_oracle where the parity tests trust the oracle and nothing checked it:
    balanced trees of 16 to 300 taxa (the oracle rescales from 64 on) with a 1e-9 branch and a branch of 3000, u from -3
    through kUMax to 25 (300 taxa: kUMax and 25 only, the reference takes 2.8 s per u there).  With the stationary eigenvalue
    left at Jacobi's ~1e-14 instead of 0, exp(lam_0 t s) on the branch of 3000 cost the oracle 1.4e-8 of f at kUMax and
    1.0e-1 at u = 25 (gtr, 16 taxa); with it exact the largest misses seen are 3.0e-13 in f (f81_skewed, 16 taxa, u = -3) and
    2.1e-11 in g, h (f81_skewed, 130 taxa, u = -3)."""
    rng = np.random.default_rng(1000 + ntaxa)
    parent, blen, leaf = num._tree(num._balanced(list(range(ntaxa))), rng, tiny=0, long=1)
    st = np.ascontiguousarray(num._columns(ntaxa, rng)[:, DEEP_COLUMNS])
    u = np.array(DEEP_U[3::2] if ntaxa == 300 else DEEP_U)
    F, G, H = hp.column_curves(st, parent, blen, leaf, pi, ref_exch, u, model=ref_model)
    ef, egh = np.zeros_like(F), np.zeros_like(F)
    for c in range(st.shape[1]):
        f, g, h = oracle.column_curve(st, parent, blen, leaf, pi, exch, c, u)
        ef[:, c] = np.abs(f - F[:, c]) / np.maximum(1.0, np.abs(F[:, c]))
        egh[:, c] = np.maximum(np.abs(g - G[:, c]), np.abs(h - H[:, c])) / (1.0 + np.abs(H[:, c]))
    print("oracle vs reference, %s, %d taxa, per u: |df| %s ; |dg|,|dh| %s" % (
        mname, ntaxa, " ".join("%.1e" % v for v in ef.max(axis=1)), " ".join("%.1e" % v for v in egh.max(axis=1))))
    assert np.isfinite(ef).all() and np.isfinite(egh).all()
    assert ef.max() <= 1e-12, (np.unravel_index(ef.argmax(), ef.shape), ef.max())
    assert egh.max() <= 1e-10, (np.unravel_index(egh.argmax(), egh.shape), egh.max())


def test_oracle_site_rates_are_maxima_of_the_reference_curve(oracle):
    """At the oracle's rate the reference curve is stationary (to the 1e-6 to which rates are located), its value is the
    oracle's lnL, and it is a maximum."""
    from tapir_amd import synth
    d = synth.simulate(1, 60, 10, 22)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()[:, :60]
    pi, exch = d["pi"][0], d["exch"][0]
    ref = oracle.site_rates(st, pin["parent"], pin["blen"], pin["leaf"], pi, exch)
    kap = hp.kappa(pi, exch)
    interior = np.flatnonzero(ref["flag"] == 0)
    assert interior.size >= 20
    for c in interior:
        u = math.log(ref["rate"][c] / kap)
        F, G, H = hp.column_curves(st[:, c:c + 1], pin["parent"], pin["blen"], pin["leaf"], pi, exch, [u])
        assert abs(F[0, 0] - ref["lnl"][c]) <= 1e-11 * max(1.0, abs(F[0, 0])), c
        assert abs(G[0, 0]) <= 1e-6 * (1.0 + abs(H[0, 0])) and H[0, 0] < 0, (c, G[0, 0], H[0, 0])


def test_quad_and_exact_integral_agree_with_the_oracle_quadpack(oracle):
    rng = np.random.default_rng(3)
    for a, b in ([0, 10], [3, 7], [85, 95], [0, 500]):
        for r in np.exp(rng.uniform(np.log(1e-6), np.log(50.0), 40)):
            q, e = hp.quad(a, b, r)
            res, err, _, _ = oracle.quad_townsend(a, b, r)
            assert abs(q - res) <= 1e-14 * abs(q) and abs(e - err) <= 0.1 * e
            # (quad itself is the reference's behaviour, not the truth: with the integrand's peak at 1/(4r) far narrower
            #  than the interval, its first panels never sample it -- [0,500] at r = 20 gives 1.6e-15 for 1.0)
            if 4.0 * r * (b - a) <= 200.0:
                ex = float(hp.integral_exact(a, b, r))
                assert abs(q - ex) <= max(1.49e-8 * ex, e), (a, b, r)


# the cancelling cases: g(4rb) - g(4ra) with both terms close to 1
CANCELLING = [(85, 95, 0.05), (85, 95, 0.1), (85, 95, 0.2), (85, 95, 1.0), (45, 55, 0.2), (499, 500, 0.3)]


def test_closed_form_integral_is_exact_to_1e12(oracle):
    """orc_integral_closed against the 40-digit value, relative, with no absolute floor (a result of 0 for 2e-28 used to
    pass a 1e-15 floor)."""
    rng = np.random.default_rng(4)
    cases = list(CANCELLING)
    for a, b in ([0, 1], [0, 500], [3, 7], [10, 11], [100, 101], [499, 500], [45, 55], [20, 100]):
        cases += [(a, b, r) for r in np.exp(rng.uniform(np.log(1e-8), np.log(1e3), 60))]
    worst = 0.0
    for a, b, r in cases:
        ex = float(hp.integral_exact(a, b, r))
        if ex < 1e-290:      # below that, fp64 results are subnormal or 0
            continue
        got = oracle.lib().orc_integral_closed(float(a), float(b), float(r))
        worst = max(worst, abs(got - ex) / ex)
    assert worst <= 1e-12, worst


def test_table_exponential_clamp_changes_nothing_above_the_wrap():
    """exp_nonpos_tab with the clamp at -1e4: bit-identical to the unclamped version for x > -2.33e7, within 1.5 ulp of
    exp(x) on [-745, 0], 0 below; the unclamped version returned +inf in bands below -2.33e7."""
    rng = np.random.default_rng(8)
    xs = np.concatenate([-np.exp(rng.uniform(np.log(1e-12), np.log(745.0), 400)), rng.uniform(-745.2, -700.0, 100),
                         -np.exp(rng.uniform(np.log(745.2), np.log(-fexp.WRAP), 200)), [0.0, -0.0, -1e4, -1e4 - 1e-9]])
    for x in xs:
        new, old = fexp.exp_nonpos_tab(float(x)), fexp.exp_nonpos_tab(float(x), clamp=False)
        assert new == old, x
        with mpmath.workdps(40):
            ex = mpmath.exp(mpmath.mpf(float(x)))
        if x >= -708.0:
            assert abs(new - float(ex)) <= 1.5 * math.ulp(float(ex)), x
        elif x < -745.2:
            assert new == 0.0
    for x in (-2.33e7, -3e7, -4.6e7, -1e9, -1e15, -1e300, -math.inf):
        assert fexp.exp_nonpos_tab(x) == 0.0
    assert fexp.exp_nonpos_tab(-2.33e7, clamp=False) == math.inf and fexp.exp_nonpos_tab(-3e7, clamp=False) == math.inf


@pytest.mark.parametrize("a,b,r", CANCELLING)
def test_closed_form_cancelling_cases(oracle, a, b, r):
    ex = float(hp.integral_exact(a, b, r))
    got = oracle.lib().orc_integral_closed(float(a), float(b), float(r))
    assert abs(got - ex) <= 1e-12 * ex, (got, ex)


# ---- whole-locus reference (stage 1) ----------------------------------------------------------------------------------

def _locus_case():
    from tapir_amd import synth
    d = synth.simulate(1, 48, 9, 33, rate_mean=0.02)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()[:, :48].copy()
    st[2, 3:9] = 5
    st[4, 20] = 0       # a zero byte is a gap
    return st, np.asarray(pin["parent"]), np.asarray(pin["blen"], np.float64) * 3.0, np.asarray(pin["leaf"]), d["pi"][0], d["exch"][0]


def test_locus_reference_agrees_with_the_oracle(oracle):
    """lnL against oracle.locus_loglik at the 1e-9 of test_gpu_parity.test_locus_loglik_vs_oracle, the analytic branch
    derivatives and the six rate derivatives against central differences of the oracle at the 2e-6 max(1, |g|) of
    test_locus_gradient_vs_oracle_finite_differences, the second derivatives at 1e-4 (the differences' own noise)."""
    st, parent, blen, leaf, pi, exch = _locus_case()
    lnl, g, h = hp.locus_reference(st, None, parent, blen, leaf, pi, exch)
    dex = hp.locus_dexch_reference(st, None, parent, blen, leaf, pi, exch)
    stz = np.where(st == 0, 15, st).astype(np.uint8)
    f = lambda e, b: oracle.locus_loglik(stz, parent, b, leaf, pi, e)   # noqa: E731
    ref = f(exch, blen)
    assert abs(lnl - ref) < 1e-9 * abs(ref)
    assert abs(lnl - ref) < 1e-13 * abs(ref)     # (what it really is on ordinary inputs)
    step = 1e-5
    rdex = np.zeros(6)
    for q in range(6):
        ep, em = exch.copy(), exch.copy()
        ep[q] *= 1 + step
        em[q] *= 1 - step
        rdex[q] = (f(ep, blen) - f(em, blen)) / (2 * step * exch[q])
    br = np.flatnonzero(parent >= 0)
    rg, rh = np.zeros(len(parent)), np.zeros(len(parent))
    s2 = 1e-3
    for b in br:
        bp, bm = blen.copy(), blen.copy()
        bp[b] *= np.exp(step)
        bm[b] *= np.exp(-step)
        rg[b] = (f(exch, bp) - f(exch, bm)) / (2 * step)
        bp[b], bm[b] = blen[b] * np.exp(s2), blen[b] * np.exp(-s2)
        rh[b] = (f(exch, bp) - 2 * ref + f(exch, bm)) / (s2 * s2)
    tol = 2e-6 * max(1.0, np.abs(rdex).max(), np.abs(rg).max())
    assert np.abs(dex - rdex).max() < tol and np.abs(g[br] - rg[br]).max() < tol
    assert np.abs(h[br] - rh[br]).max() < 1e-4 * max(1.0, np.abs(rh).max())
    assert np.isnan(g[parent < 0]).all()
    # column weights are multiplicities: weight 2 on a column = the column twice
    w = np.ones(st.shape[1])
    w[5], w[11] = 2.0, 3.0
    rep = np.concatenate([st, st[:, [5, 11, 11]]], axis=1)
    a = hp.locus_reference(st, w, parent, blen, leaf, pi, exch, branches=br[:3])
    b = hp.locus_reference(rep, None, parent, blen, leaf, pi, exch, branches=br[:3])
    assert abs(a[0] - b[0]) < 1e-13 * abs(b[0]) and np.allclose(a[1][br[:3]], b[1][br[:3]], rtol=1e-13, atol=0)
    assert np.isnan(a[1][br[3]]) and np.allclose(a[2][br[:3]], b[2][br[:3]], rtol=1e-13, atol=0)


def test_locus_reference_two_taxon_closed_form():
    """Two taxa: L = pi_i P_ij(t_a + t_b).  Under Jukes-Cantor in HyPhy's parametrisation (Q_ij = 1/4) P is elementary:
    P_ii = 1/4 + 3/4 e^-t, P_ij = 1/4 - 1/4 e^-t, and so are the derivatives in log t_a; under GTR P comes from mpmath's expm of
    Q (t_a + t_b), not from the eigen-decomposition the reference uses."""
    parent, leaf = np.array([2, 2, -1]), np.array([0, 1, -1])
    ta, tb = 0.3, 0.045
    st = np.array([[1, 2, 4, 8, 1, 8], [1, 2, 8, 8, 4, 2]], np.uint8)
    same = st[0] == st[1]
    w = np.array([3.0, 1.0, 2.0, 1.0, 1.0, 4.0])
    lnl, g, h = hp.locus_reference(st, w, parent, [ta, tb, 0.0], leaf, [0.25] * 4, np.ones(6), as_float=False)
    with mpmath.workdps(hp.DPS):
        t, a = mpmath.mpf(ta) + mpmath.mpf(tb), mpmath.mpf(ta)
        e = mpmath.exp(-t)
        want = want_g = want_h = 0
        for c in range(st.shape[1]):
            L = (1 + 3 * e) / 16 if same[c] else (1 - e) / 16
            dL = (-3 * e if same[c] else e) / 16          # dL/dt
            d2L = -dL
            u1, u2 = a * dL / L, (a * a * d2L + a * dL) / L   # d/dlog t_a = t_a d/dt
            want += w[c] * mpmath.log(L)
            want_g += w[c] * u1
            want_h += w[c] * (u2 - u1 * u1)
        assert abs(lnl - want) < mpmath.mpf(10) ** -35 * abs(want)
        assert abs(g[0] - want_g) < mpmath.mpf(10) ** -35 * abs(want_g)
        assert abs(h[0] - want_h) < mpmath.mpf(10) ** -35 * abs(want_h)
        # GTR: pi_i expm(Q t)_ij
        pi, exch = [0.1, 0.2, 0.3, 0.4], [0.7, 1.0, 1.9, 0.4, 2.5, 1.1]
        Q, pim, _ = hp.rate_matrix(pi, exch)
        P = mpmath.expm(Q * t, method="taylor")
        idx = {1: 0, 2: 1, 4: 2, 8: 3}
        want = mpmath.fsum(w[c] * mpmath.log(pim[idx[st[0, c]]] * P[idx[st[0, c]], idx[st[1, c]]]) for c in range(st.shape[1]))
        lnl = hp.locus_reference(st, w, parent, [ta, tb, 0.0], leaf, pi, exch, as_float=False)[0]
        assert abs(lnl - want) < mpmath.mpf(10) ** -30 * abs(want)


def test_locus_reference_does_not_depend_on_its_precision():
    """Doubling the working precision moves nothing at 1e-30: lnL, every branch derivative, the six rate derivatives (60 and
    120 digits at the same 1e-18 step bound rounding; 1e-18 and 1e-20 steps bound truncation, through fp64 1e-15)."""
    st, parent, blen, leaf, pi, exch = _locus_case()
    st = st[:, :12]
    a = hp.locus_reference(st, None, parent, blen, leaf, pi, exch, as_float=False)
    b = hp.locus_reference(st, None, parent, blen, leaf, pi, exch, dps=2 * hp.DPS, as_float=False)
    with mpmath.workdps(2 * hp.DPS):
        tiny = mpmath.mpf(10) ** -30
        assert abs(a[0] - b[0]) <= tiny * abs(b[0])
        for k in (1, 2):
            for n in b[k]:
                assert abs(a[k][n] - b[k][n]) <= tiny * max(1, abs(b[k][n])), (k, n)
    d60 = hp.locus_dexch_reference(st, None, parent, blen, leaf, pi, exch, as_float=False)
    d120 = hp.locus_dexch_reference(st, None, parent, blen, leaf, pi, exch, dps=120, as_float=False)
    d20 = hp.locus_dexch_reference(st, None, parent, blen, leaf, pi, exch, dps=120, step=1e-20, as_float=False)
    with mpmath.workdps(120):
        for q in range(6):
            assert abs(d60[q] - d120[q]) <= tiny * max(1, abs(d120[q])) and abs(d60[q] - d20[q]) <= tiny * max(1, abs(d20[q])), q
    # an mpf step survives rate_matrix (a float cast would round 1 + 1e-18 to 1)
    with mpmath.workdps(60):
        r = mpmath.mpf(1) + mpmath.mpf("1e-18")
        Q = hp.rate_matrix([0.25] * 4, [r] + [1.0] * 5, dps=60)[0]
        assert Q[0, 1] != Q[0, 2] and abs(Q[0, 1] / Q[0, 2] - r) < mpmath.mpf("1e-50")


# ---- the rate-class models of stage 1 --------------------------------------------------------------------------------

_CLASS = {}


def _class_case():
    """Locus 0 of synth.simulate(2, 80, 5, 23, rate_mean=0.01) as site patterns with counts (47 patterns), its tree, its
    empirical base frequencies, and the restatement's fit of all 203 models (about 8 s, once)."""
    if not _CLASS:
        from oracle import stage1_oracle
        from tapir_amd import synth
        d = synth.simulate(2, 80, 5, 23, rate_mean=0.01)
        pin = synth.plan_inputs(d["root"], d["names"])
        st = d["states"].numpy()[:, :80]
        pat, cnt = np.unique(st, axis=1, return_counts=True)
        hist = np.bincount(st.ravel(), minlength=16).astype(np.float64)
        pi = np.array([sum(hist[m] / bin(m).count("1") for m in range(1, 16) if (m >> k) & 1) for k in range(4)])
        pi /= pi.sum()
        parent, leaf = np.asarray(pin["parent"]), np.asarray(pin["leaf"])
        fit = stage1_oracle.model_averaged(st, parent, np.asarray(pin["blen"]) / pin["correction"], leaf, pi)
        _CLASS.update(pat=np.ascontiguousarray(pat), cnt=cnt.astype(np.float64), parent=parent, leaf=leaf, pi=pi, fit=fit)
    return _CLASS


def test_partitions_and_akaike_weights_against_the_restatement():
    """hp.rate_partitions (a filter over all digit strings) against the restatement's recursion and the engine's documented
    order; hp.akaike_weights (mpmath, no shift by the maximum) against the restatement's weights at 1e-12."""
    from oracle import stage1_oracle
    ms = hp.rate_partitions()
    assert len(ms) == 203 and len(set(ms)) == 203 and ms[:4] == ["012345", "000000", "000001", "000010"]
    assert ms[1:] == sorted(ms[1:]) and set(ms) == set(stage1_oracle.partitions6())
    assert hp.partition_classes("012345") == ([0, -1, 1, 2, 3, 4], 5) and hp.partition_classes("000000") == ([-1] * 6, 0)
    assert hp.partition_classes("010010") == ([0, -1, 0, 0, -1, 0], 1) and hp.partition_classes("011201") == ([0, -1, -1, 1, 0, -1], 2)
    assert sorted(k for _, k in map(hp.partition_classes, ms[1:])) == [0] + [1] * 31 + [2] * 90 + [3] * 65 + [4] * 15   # Stirling
    pi = [0.1, 0.2, 0.3, 0.4]
    assert abs(float(hp.total_factor(pi, np.ones(6))) - (1 - sum(x * x for x in pi))) < 1e-15
    fit = _class_case()["fit"]
    nfree = [5] + [hp.partition_classes(s)[1] for s in ms[1:]]
    w = hp.akaike_weights([fit["lnl"][s] for s in ms], nfree)
    assert max(abs(float(w[i]) - fit["weights"][s]) for i, s in enumerate(ms)) <= 1e-12
    with mpmath.workdps(hp.DPS):      # hundreds of nats behind: tiny, positive, and the sum is still 1
        far = hp.akaike_weights([-300.0, -1500.0, -301.0], [5, 0, 2])
        assert 0 < far[1] < mpmath.mpf(10) ** -500 and abs(mpmath.fsum(far) - 1) < mpmath.mpf(10) ** -35


def test_class_model_gradient_is_the_chain_rule():
    """d phi / d theta_j = sum_{q in class j} r_q (d lnL / d r_q - (sum_b d lnL / d log t_b) 2 pi_i pi_j / totalFactor), the two
    pieces from locus_dexch_reference and locus_reference at t = b / totalFactor: to 1e-25 for one to four free classes."""
    c = _class_case()
    rng = np.random.default_rng(6)
    b = np.where(c["parent"] >= 0, np.exp(rng.uniform(np.log(0.02), np.log(0.5), len(c["parent"]))), 0.0)
    pif = hp.floored_pi(c["pi"])
    for part in ("010010", "011021", "010213", "012340"):
        cls, k = hp.partition_classes(part)
        exch = np.array([1.0 if x < 0 else math.exp(rng.normal(0, 0.7)) for x in range(k)])[cls]
        exch[np.array(cls) < 0] = 1.0
        with mpmath.workdps(60):
            theta = [mpmath.log(mpmath.mpf(float(exch[cls.index(a)]))) for a in range(k)]
            tf = hp.total_factor(pif, exch, 60)
            t = [mpmath.mpf(float(x)) / tf for x in b]
            phi, g, _ = hp.class_model_reference(c["pat"], c["cnt"], c["parent"], b, c["leaf"], c["pi"], part, theta, order=1)
            lnl, d1, _ = hp.locus_reference(c["pat"], c["cnt"], c["parent"], t, c["leaf"], c["pi"], exch, dps=60, as_float=False)
            dex = hp.locus_dexch_reference(c["pat"], c["cnt"], c["parent"], t, c["leaf"], c["pi"], exch, as_float=False)
            slope = mpmath.fsum(d1.values())
            tiny = mpmath.mpf(10) ** -25
            assert abs(phi - lnl) <= tiny
            for a in range(k):
                want = mpmath.fsum(mpmath.mpf(float(exch[q])) * (dex[q] - slope * 2 * mpmath.mpf(float(pif[i])) * mpmath.mpf(float(pif[j])) / tf)
                                   for q, (i, j) in enumerate(hp.PAIRS) if cls[q] == a)
                assert abs(g[a] - want) <= tiny * max(1, abs(want)), (part, a, g[a], want)


def test_class_model_reference_does_not_depend_on_its_precision():
    """60 digits with h = 1e-15 against 120 digits with h = 1e-17 (truncation 10^4 times smaller, rounding 10^56 times): the
    value, the gradient and the Hessian of a three-class model move by less than 1e-25."""
    c = _class_case()
    b = np.where(c["parent"] >= 0, 0.07, 0.0)
    a = hp.class_model_reference(c["pat"], c["cnt"], c["parent"], b, c["leaf"], c["pi"], "010213", [0.2, -0.4, 0.1])
    z = hp.class_model_reference(c["pat"], c["cnt"], c["parent"], b, c["leaf"], c["pi"], "010213", [0.2, -0.4, 0.1], dps=120, step=1e-17)
    with mpmath.workdps(120):
        tiny = mpmath.mpf(10) ** -25
        assert abs(a[0] - z[0]) <= tiny and max(abs(a[1][i] - z[1][i]) for i in range(3)) <= tiny
        assert max(abs(a[2][i][j] - z[2][i][j]) for i in range(3) for j in range(3)) <= tiny
        assert all(a[2][i][j] == a[2][j][i] for i in range(3) for j in range(3)) and max(abs(x) for x in z[1]) > 0.1
    assert hp.class_model_reference(c["pat"], c["cnt"], c["parent"], b, c["leaf"], c["pi"], "000000", [])[1:] == (None, None)


def test_restatement_optima_against_the_class_model_reference():
    """At the optima oracle.stage1_oracle.model_averaged finds on the same locus, for every class model whose rates are all
    interior (all 202 here): the reference's phi is the restatement's lnL within 1e-10 (1 + |lnL|), -H is positive definite,
    and the Newton gain 1/2 g'(-H)^-1 g still to be had is below what the restatement's stopping rule implies:
    scipy's L-BFGS-B stops on max_i |g_i| <= gtol for ITS gradient, forward differences of step eps of an objective with
    absolute noise d, so the true slope is within gtol + eps |H_ii| / 2 + 2 d / eps =: s, and the gain is at most
    k s^2 / (2 lambda_min(-H)).  Of the restatement's two runs (gtol 1e-7 with eps 1e-6, then 1e-8 with 1e-7) either may be
    the one returned, so each term takes its larger value: s = 1e-7 + 5e-7 max|H_ii| + 2 d / 1e-7, with d = 1e-13 |lnL| (what the
    oracle's likelihood keeps on ordinary inputs: test_locus_reference_agrees_with_the_oracle).  The largest gain must also be
    below 1e-4, a tenth of the 1e-3 in lnL at which the GPU tests use the restatement as a cross-check."""
    c = _class_case()
    fit = c["fit"]
    with mpmath.workdps(60):
        tf0 = hp.total_factor(hp.floored_pi(c["pi"]), fit["grm_exch"], 60)
        b = [mpmath.mpf(float(x)) * tf0 for x in fit["grm_blen"]]
    rows = []
    for s in hp.rate_partitions()[1:]:
        cls, k = hp.partition_classes(s)
        theta = np.log([fit["rates"][s][cls.index(a)] for a in range(k)])
        if k == 0 or np.any(theta < -7.0 + 1e-6) or np.any(theta > 9.2 - 1e-6):
            continue
        with mpmath.workdps(60):
            th = [mpmath.log(mpmath.mpf(float(fit["rates"][s][cls.index(a)]))) for a in range(k)]
        phi, g, H = hp.class_model_reference(c["pat"], c["cnt"], c["parent"], b, c["leaf"], c["pi"], s, th)
        gain, lam = hp.newton_gain(g, H)
        lnl = float(phi)
        slope = 1e-7 + 5e-7 * max(abs(float(H[a][a])) for a in range(k)) + 2 * 1e-13 * abs(lnl) / 1e-7
        rows.append((s, abs(lnl - fit["lnl"][s]) / (1e-10 * (1 + abs(lnl))), gain, k * slope ** 2 / (2 * lam) if lam > 0 else 0.0, lam))
    worst = max(rows, key=lambda r: r[2] / r[3] if r[3] > 0 else math.inf)
    print("restatement optima: %d models; largest |d lnL| / bound %.3g; largest Newton gain %.3g; largest gain / implied bound %.3g "
          "(model %s: gain %.3g, bound %.3g, smallest eigenvalue of -H %.3g)"
          % (len(rows), max(r[1] for r in rows), max(r[2] for r in rows), worst[2] / worst[3] if worst[3] > 0 else math.inf, worst[0],
             worst[2], worst[3], worst[4]))
    assert len(rows) == 201      # every class model but "000000", which has no free rate
    assert max(r[1] for r in rows) <= 1.0
    bad = [r for r in rows if not (r[4] > 0 and r[2] <= r[3])]
    assert not bad, bad
    assert max(r[2] for r in rows) <= 1e-4

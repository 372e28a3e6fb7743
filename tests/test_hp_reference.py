"""The high-precision references of tests/hp_reference.py against the CPU oracle and scipy, the closed-form interval
integral against the exact value, and the clamp of the kernels' table exponential (on its bit-level emulation).  CPU
only."""
import math

import mpmath
import numpy as np
import pytest

import fast_exp_emulation as fexp
import hp_reference as hp


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

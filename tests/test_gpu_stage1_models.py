"""Stage 1's 203 model fits and the Akaike averaging (tphip_stage1_fit: csrc/stage1_opt_kernels.hpp, csrc/stage1_driver.hip)
against the 40-digit reference of tests/hp_reference.py (locus_reference, class_model_reference).  Run with -m gpu on the
MI355X box.

Everything else that checks the fits shares the engine's likelihood, its formulas or its optimiser (the oracle restatement at
1e-3, the host optimiser over the same kernels, the pruned run against the unpruned one).  Here the class tables, the
theta -> exch map, the branch lengths stash / totalFactor(exch), the screen with its prune rules and average_kernel are held to
a reference that shares nothing with them: the partitions, totalFactor and the Akaike weights are written out in
hp_reference from the mathematics, and nothing comes from tapir_amd.stage1 or oracle.stage1_oracle.

One plan holds four loci of 5 taxa on the tree of synth.yule_tree(5, 23), with 80, 75, 60 and 100 000 columns (offsets 0, 80, 155,
215, 100 215), simulated by synth.simulate(..., tree=that tree):
  A  simulate(2, 80, 5, 23, rate_mean=0.01) locus 0: every model matters (203 Akaike scores within 21 of the best, no rate at a bound);
  C  A's first 75 columns;
  B  simulate(6, 60, 5, 2, rate_mean=0.01) locus 5: no CG change is observed, so the 51 models that give CG a class of its own (or
     share it with another unobserved type) end with that class rate at e^-7;
  D  simulate(1, 100000, 5, 29, rate_mean=0.0003, rate_shape=1e6, gap_frac=0): 151 models trail by more than 21 and 150 are abandoned.
     One low rate and no gaps keep it at 194 site patterns, so the reference, which works on patterns, costs 0.06 s a value.
The conditions are asserted on the engine's own output (test_inputs_meet_their_conditions), so an input that stops meeting them
fails instead of testing nothing; every fitted general-model branch lies in [1e-3, e^4] (branches of 1e-6 and below are the known
defect of DESIGN.md section 9).  Why D is long: at 60 to 100 columns no 5-taxon locus of synth.simulate has a model that trails by 21
(tools/stage1_locus_survey.py: 330 loci, none with a trailing model), and none has at 3000 columns (780 patterns with the default 5 % gaps); at
20 000 columns 136 trail, on 1831 patterns (1 s a value).  On the two 80-column loci where oracle/stage1_oracle.py reports 195
trailing models, scipy had parked four branches at e^4, 150 log-units below the engine's optimum.
Hessians: every class model of A, C and B; on D the models with weight > 1e-9 (the 157 left out are asserted to weigh less).
Calls: "product" = stage1_fit(st, compress_patterns=True, empirical_pi=True), "plain" = stage1_fit(st) on the same plan with
the simulated frequencies, "full" = the product call with prune_models=False, and each locus alone in a plan of its own.  The
reference works on np.unique patterns with counts.

Bounds (all derived, none fitted to what the engine gives):
  value      |lnl[l, m] - ref| <= B max(1, |ref|) + 4 eps sum_b |d lnL / d log t_b|, B = the ordinary lnL bound of
             test_gpu_stage1_numerics.BOUNDS (2e-14).  The reference is evaluated at exch = model_exch[l, m] and
             t = grm_blen tf_0 / tf_m with tf = totalFactor(model_exch[l, .]) exact; the engine's t is stash * fl(1 / fl(tf_m)) with
             stash = b and grm_blen = fl(b / fl(tf_0)).  To first order lnL moves by sum_b (d lnL / d log t_b) delta_b, and
             delta_b collects the roundings that separate the two t: one each for b / tf_0, 1 / tf_m and the product (3 u,
             u = eps / 2), the sums tf_0 (a product and three additions of positive terms: 4 u) and tf_m (six fused multiply-adds:
             at most 6 u, 3 u on average over the terms), and what is left of the roundings of 2 pi_i pi_j, which both sums
             share (at most 4 u, 0 when the two models have the same rates).  That is 17 u = 8.5 eps if every rounding had the
             same sign and 8 u = 4 eps if the two sums are taken at their mean; the bound keeps 4 eps, and the term is
             a hundredth of B |lnL| on these loci.
  optimum    for every fitted class model, on the class rates not at a bound: the reference's Newton gain 1/2 g'(-H)^-1 g
             <= 10 * 1e-10 (1 + |lnL|) (a fit stops when g'H^-1 g <= 1e-10 (1 + |lnL|); the 10 is for
             the engine measuring g by central differences of step 1e-4 and H by its screen / BFGS metric), -H positive definite;
             on a rate at the lower (upper) bound the slope is <= (>=) +(-) 2e-6 |lnL| of the locus, the rule of
             test_fitted_point_is_an_optimum_of_the_reference.  A model counts as fitted when its weight exceeds 1e-9: the
             engine abandons only models whose score trails the best by more than 21, which have weight < e^-21 = 7.6e-10.  The
             general model has branch-length coordinates and is held by test_fitted_point_is_an_optimum_of_the_reference.
  abandoning G_m = 1e-9 (1 + |lnL_m|), the gain bound above.  With D the models whose lnL in the pruned run is below the full
             run's by more than G_m and W their summed full-run weight: inside D each run moves a rate by at most its weight there
             times the distance of the model's rate from the average, and the pruned run's weight in D is at most e^G W / (1 - W):
             2 W max_{m in D} |r_mq - exch_q| to first order in W.  Outside D a lnL may differ by up to G, which moves a weight by at
             most e^2G - 1 <= 4 G relative: 4 G max_m |r_mq - exch_q|.  The two averages round separately: 8 * 203 eps exch_q.
             |exch_pruned - exch_full| is held to the sum of the three.
  weights    relative error 4 eps (2 max|lnL| + 203): the exponent fl(fl(lnL - k) - smax) is off by at most
             u (|lnL| + k + |lnL - k - smax|) <= u 3 max|lnL| (smax itself is common to all terms and cancels), which is the
             relative error of exp of it, plus 2 u for exp; the sum of 203 positive terms adds 202 u and the same weighted mean
             of the terms' errors, the division u: u (6 max|lnL| + 209) < 4 eps (2 max|lnL| + 203).  A weight below 2^-1022
             may come out as any denormal or 0.  Sum of the weights: 203 eps.  exch against sum_m w_m model_exch in mpmath:
             4 * 203 eps relative (203 fused multiply-adds of positive terms and the weights' own roundings).
  batch      a locus fitted alone gives the same lnl, weights, exch, model_exch, pi and grm_blen rows bit for bit (D included).

Largest error / bound seen on one MI355X (A / C / B / D, product call; plain call in parentheses):
  value      0.157 / 0.129 / 0.118 / 0.277 (0.120 / 0.138 / 0.118 / 0.656), D's 150 abandoned models included; the rounding of t is
             at most 3e-4 of the bound
  optimum    gain / threshold 0.52 / 0.68 / 0.52 / 0.004 of the 10 allowed (201, 201, 201 and 45 models); smallest eigenvalue of -H
             0.148 / 0.035 / 0.546 / 314; the slopes at B's bounds all point out of the box (largest -2.2e-3, limit +5.3e-4).
             Before sub_direction_kernel held the step of a rate at its bound at 0, four models of B (001211, 010200, 010230,
             010233) stood at 13.5, 29.4, 34.9 and 30.8, two of them after 100 iterations
  abandoning D: 150 models up to 0.97 below their full-run lnL, summed weight 1.95e-12 (largest 6.5e-13, e^-21 = 7.6e-10),
             |exch_pruned - exch_full| 4.1e-14 (bound 4.6e-4); A, C, B: nothing abandoned, rows identical
  weights    1.2e-3 of the bound, their sum 1.6e-2, averaged rates 3.9e-3; smallest weight 1.9e-72; empirical pi 0.47 ulp of 2

The references are the slow side, 1.5 to 3 minutes of one CPU core in all (82 s beside the MI355X): 0.025 s per value on 40 to 47 patterns and 0.06 s on D's
194, 203 values per (call, locus), and a stencil of 1 + k + k^2 values per model for the Hessians (40 s a locus).  They are computed
once per module and shared.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import hp_reference as hp
from test_gpu_stage1_numerics import ALL_PATHS, BOUNDS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LOG_RATE_MIN, LOG_RATE_MAX = -7.0, 9.2      # the box of the class rates
BLEN_MIN, BLEN_MAX = 1e-3, math.exp(4.0)    # the "ordinary" class of BOUNDS
PRUNE_NATS = 21.0
STOP, GAIN_MARGIN = 1e-10, 10.0             # the documented stopping threshold and the margin on it
MODELS = hp.rate_partitions()
CLASSES = [hp.partition_classes(s) for s in MODELS]
NFREE = np.array([5] + [k for _, k in CLASSES[1:]])
# name, arguments of synth.simulate (loci, columns, taxa, seed), rate_mean, locus of that batch, columns kept; all on TREE_SEED's tree
TREE_SEED = 23
LOCI = (("A", (2, 80, 5, 23), dict(rate_mean=0.01), 0, 80), ("C", (2, 80, 5, 23), dict(rate_mean=0.01), 0, 75),
        ("B", (6, 60, 5, 2), dict(rate_mean=0.01), 5, 60),
        ("D", (1, 100000, 5, 29), dict(rate_mean=0.0003, rate_shape=1e6, gap_frac=0.0), 0, 100000))
NAMES = [x[0] for x in LOCI]
REF_NAMES = NAMES
HESSIAN_WEIGHT = 1e-9
CALLS = ("product", "plain")
_CACHE = {}


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _inputs():
    """states [5, 100215], offsets, simulated pi [4, 4], tree arrays of TREE_SEED."""
    if "inputs" not in _CACHE:
        from tapir_amd import synth
        tree = synth.yule_tree(5, TREE_SEED)
        pin = synth.plan_inputs(*tree)
        cols, pis = [], []
        for name, args, kw, l, n in LOCI:
            d = synth.simulate(*args, tree=tree, **kw)
            cols.append(d["states"].numpy()[:, l * args[1]:l * args[1] + n])
            pis.append(d["pi"][l])
        off = np.concatenate([[0], np.cumsum([c.shape[1] for c in cols])]).astype(np.int64)
        _CACHE["inputs"] = (np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=np.uint8), off, np.array(pis), pin)
    return _CACHE["inputs"]


def _plan(engine, off, pi, pin):
    L = len(off) - 1
    return engine.Plan(5, pin["parent"], pin["blen"], pin["leaf"], off, pi, np.ones((L, 6)), pin["T"], [1], [[0, 1]],
                       correction=pin["correction"])


def _fits():
    """Every engine call of the module, once: plain, product, full on the three-locus plan, and each locus alone."""
    if "fits" not in _CACHE:
        engine = _engine()
        st, off, pi, pin = _inputs()
        product = dict(compress_patterns=True, empirical_pi=True)
        plan = _plan(engine, off, pi, pin)
        fits = {"plain": plan.stage1_fit(st)}     # first: empirical_pi puts its frequencies into the plan
        fits["product"] = plan.stage1_fit(st, **product)
        fits["full"] = plan.stage1_fit(st, prune_models=False, **product)
        plan.close()
        fits["alone"] = []
        for l in range(len(LOCI)):
            sub = np.ascontiguousarray(st[:, off[l]:off[l + 1]])
            plan = _plan(engine, np.array([0, sub.shape[1]]), pi[l:l + 1], pin)
            fits["alone"].append(plan.stage1_fit(sub, **product))
            plan.close()
        _CACHE["fits"] = fits
    return _CACHE["fits"]


def _patterns(l):
    if ("patterns", l) not in _CACHE:
        st, off, _, _ = _inputs()
        pat, cnt = np.unique(st[:, off[l]:off[l + 1]], axis=1, return_counts=True)
        _CACHE["patterns", l] = (np.ascontiguousarray(pat), cnt.astype(np.float64))
    return _CACHE["patterns", l]


def _tree():
    pin = _inputs()[3]
    return np.asarray(pin["parent"]), np.asarray(pin["leaf"])


def _point(call, l, m):
    """Exchangeabilities and branch lengths (mpf) of the point the engine reports for model m: exch = model_exch[l, m],
    t = grm_blen tf_0 / tf_m."""
    fit = _fits()[call]
    pi = hp.floored_pi(fit["pi"][l])
    with mpmath.workdps(hp.DPS):
        scale = hp.total_factor(pi, fit["model_exch"][l, 0]) / hp.total_factor(pi, fit["model_exch"][l, m])
        return fit["model_exch"][l, m], [mpmath.mpf(float(x)) * scale for x in fit["grm_blen"][l]]


def _point_reference(call, l):
    """The reference lnL of every model at its reported point, floats [203]."""
    if ("point", call, l) not in _CACHE:
        pat, cnt = _patterns(l)
        parent, leaf = _tree()
        lnl = np.empty(203)
        for m in range(203):
            exch, t = _point(call, l, m)
            lnl[m] = hp.locus_reference(pat, cnt, parent, t, leaf, _fits()[call]["pi"][l], exch, branches=[])[0]
        _CACHE["point", call, l] = lnl
    return _CACHE["point", call, l]


def _point_slope(call, l, m):
    """sum_b |d lnL / d log t_b| of the reference at the reported point of model m."""
    pat, cnt = _patterns(l)
    parent, leaf = _tree()
    exch, t = _point(call, l, m)
    d1 = hp.locus_reference(pat, cnt, parent, t, leaf, _fits()[call]["pi"][l], exch, as_float=False)[1]
    return float(mpmath.fsum(abs(x) for x in d1.values()))


def _theta(fit, l, m):
    """The class rates of model m as the engine reports them: float log rates [k] and the rate itself per class."""
    cls, k = CLASSES[m]
    r = [fit["model_exch"][l, m, cls.index(c)] for c in range(k)]
    return np.log(np.array(r, np.float64)), r


def _model_derivatives(l, m):
    """(phi, g, H) of class model m of the product call at its reported point (hp.class_model_reference)."""
    if ("derivs", l, m) not in _CACHE:
        fit = _fits()["product"]
        pat, cnt = _patterns(l)
        parent, leaf = _tree()
        pi = fit["pi"][l]
        with mpmath.workdps(60):
            tf0 = hp.total_factor(hp.floored_pi(pi), fit["model_exch"][l, 0], 60)
            b = [mpmath.mpf(float(x)) * tf0 for x in fit["grm_blen"][l]]
            theta = [mpmath.log(mpmath.mpf(float(r))) for r in _theta(fit, l, m)[1]]
            _CACHE["derivs", l, m] = hp.class_model_reference(pat, cnt, parent, b, leaf, pi, MODELS[m], theta)
    return _CACHE["derivs", l, m]


def _scores(fit, l):
    return fit["lnl"][l] - NFREE


def _at_bound(theta):
    return (theta <= LOG_RATE_MIN + 1e-6) | (theta >= LOG_RATE_MAX - 1e-6)


# ---- the inputs ------------------------------------------------------------------------------------------------------

def test_enumeration_is_the_documented_one():
    assert len(MODELS) == 203 and len(set(MODELS)) == 203 and MODELS[:3] == ["012345", "000000", "000001"]
    assert MODELS[1:] == sorted(MODELS[1:]) and NFREE[1] == 0 and NFREE[1:].max() == 4


@pytest.mark.parametrize("name", NAMES)
def test_inputs_meet_their_conditions(name):
    l = NAMES.index(name)
    fit = _fits()["product"]
    parent, _ = _tree()
    br = fit["grm_blen"][l][parent >= 0]
    sc = _scores(fit, l)
    trailing = int((sc < sc.max() - PRUNE_NATS).sum())
    bound = sum(bool(_at_bound(_theta(fit, l, m)[0]).any()) for m in range(1, 203))
    print("stage1-models inputs %s: branches %.3g .. %.3g, %d models trail by more than 21, %d with a class rate at a bound, "
          "%d with weight > 1e-9" % (name, br.min(), br.max(), trailing, bound, int((fit["weights"][l] > 1e-9).sum())))
    if True:
        assert BLEN_MIN <= br.min() and br.max() <= BLEN_MAX, (br.min(), br.max())
    if name == "A":
        assert trailing == 0 and bound == 0
        free = np.log(fit["model_exch"][l, 0, [0, 2, 3, 4, 5]])
        assert not _at_bound(free).any()
    if name == "B":
        assert bound >= 50
    if name == "D":
        assert trailing >= 150 and fit["stats"]["pruned"] >= 150


# ---- 1. structure ----------------------------------------------------------------------------------------------------

def _empirical_pi(st):
    """HarvestFrequencies in exact arithmetic: every cell adds 1 / popcount(mask) to each base it may be (0 is a gap)."""
    c = [Fraction(0)] * 4
    for mask, n in zip(*np.unique(st, return_counts=True)):
        mask = int(mask) & 15 or 15
        for k in range(4):
            if (mask >> k) & 1:
                c[k] += Fraction(int(n), bin(mask).count("1"))
    tot = sum(c)
    return [x / tot for x in c]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("call", CALLS)
def test_structure(call, name):
    l = NAMES.index(name)
    fit = _fits()[call]
    st, off, pi, _ = _inputs()
    for m, s in enumerate(MODELS):
        r = fit["model_exch"][l, m]
        for a in range(6):
            if s[a] == s[1]:
                assert r[a] == 1.0, (m, s, r)
            for b in range(a + 1, 6):
                if s[a] == s[b]:
                    assert r[a] == r[b], (m, s, r)
                elif name == "A":
                    assert r[a] != r[b], (m, s, r)
    assert fit["exch"][l, 1] == 1.0 and np.all(fit["exch"][l] > 0)
    if call == "product":
        want = _empirical_pi(st[:, off[l]:off[l + 1]])
        ulps = max(abs(Fraction(float(fit["pi"][l, k])) - want[k]) / Fraction(math.ulp(float(want[k]))) for k in range(4))
        print("stage1-models structure %s: empirical pi off by %.2f ulp (bound 2)" % (name, float(ulps)))
        assert ulps <= 2
    else:
        assert np.array_equal(fit["pi"][l], pi[l])


# ---- 2. the reported value is the true likelihood at the reported point ---------------------------------------------

@pytest.mark.parametrize("name", REF_NAMES)
@pytest.mark.parametrize("call", CALLS)
def test_reported_value_is_the_true_likelihood(call, name):
    """All 203 models, fitted or abandoned; the bound and the propagated rounding of t are derived in the module docstring."""
    l = NAMES.index(name)
    fit = _fits()[call]
    ref = _point_reference(call, l)
    rel = max(BOUNDS["ordinary"][p]["lnl"] for p in ALL_PATHS)
    err = np.abs(fit["lnl"][l] - ref)
    bound = rel * np.maximum(1.0, np.abs(ref))
    # the rounding of t can only add to the bound: it is worked out (seven more reference sweeps) for the worst model, for the
    # figure, and for every model that needs it
    for m in set(np.flatnonzero(err > bound)) | {int(np.argmax(err / bound))}:
        bound[m] += 4 * EPS * _point_slope(call, l, m)
    ratio = err / bound
    m = int(np.argmax(ratio))
    print("stage1-models value %s %s: largest error / bound %.3g (model %s, |d lnL| %.2e, bound %.2e, of it rounding of t %.1e)"
          % (name, call, ratio[m], MODELS[m], err[m], bound[m], bound[m] - rel * max(1.0, abs(ref[m]))))
    assert np.isfinite(fit["lnl"][l]).all()
    assert ratio.max() <= 1.0, [(MODELS[i], float("%.3g" % ratio[i])) for i in np.flatnonzero(ratio > 1.0)]


# ---- 3. optimality against the reference ----------------------------------------------------------------------------

def _hessian_set(l):
    """Every class model of A, C and B; on D the models with weight > 1e-9 (none of which can have been abandoned)."""
    w = _fits()["product"]["weights"][l]
    return [m for m in range(1, 203) if NAMES[l] != "D" or w[m] > HESSIAN_WEIGHT]


def _optimality(l):
    """Per model of the Hessian set: gain / threshold on the interior rates, the smallest eigenvalue of -H there, and the worst
    slope into the box of a rate at a bound (positive: the likelihood rises into the box)."""
    return [r for r in (_optimality_row(l, m) for m in _hessian_set(l)) if r is not None]


def _optimality_row(l, m):
    fit = _fits()["product"]
    theta, _ = _theta(fit, l, m)
    if len(theta) == 0:
        return None
    f, g, H = _model_derivatives(l, m)
    inner = [a for a in range(len(theta)) if not _at_bound(theta[a:a + 1])[0]]
    gain, lam = hp.newton_gain(g, H, inner)
    into = [float(g[a]) * (1.0 if theta[a] < 0 else -1.0) for a in range(len(theta)) if a not in inner]
    return (m, gain / (STOP * (1.0 + abs(float(f)))), lam, max(into) if into else -math.inf, len(inner))


def _is_optimum(row, scale):
    return row[1] <= GAIN_MARGIN and row[2] > 0 and row[3] <= 2e-6 * scale


@pytest.mark.parametrize("name", REF_NAMES)
def test_fitted_models_are_optima_of_the_reference(name):
    l = NAMES.index(name)
    fit = _fits()["product"]
    rows = _optimality(l)
    left_out = [m for m in range(1, 203) if m not in _hessian_set(l)]
    scale = float(abs(fit["lnl"][l, 0]))
    worst = max(rows, key=lambda r: r[1])
    slopes = [r[3] for r in rows if r[3] > -math.inf]
    print("stage1-models optimum %s: %d models, largest gain / threshold %.3g of %g allowed (model %s, %d interior rates); smallest "
          "eigenvalue of -H %.3g; largest slope into the box at a bound %s (limit %.2e); %d models left out, heaviest %.2e"
          % (name, len(rows), worst[1], GAIN_MARGIN, MODELS[worst[0]], worst[4], min(r[2] for r in rows),
             "%.2e" % max(slopes) if slopes else "none at a bound", 2e-6 * scale, len(left_out),
             fit["weights"][l][left_out].max() if left_out else 0.0))
    assert all(fit["weights"][l, m] <= HESSIAN_WEIGHT for m in left_out)
    assert len(rows) >= (3 if name == "D" else 201)
    bad = [(MODELS[r[0]], float("%.3g" % r[1]), float("%.3g" % r[2]), float("%.3g" % r[3])) for r in rows
           if not _is_optimum(r, scale)]
    assert not bad, bad


# ---- 4. abandoning is invisible -------------------------------------------------------------------------------------

def test_abandoning_is_invisible():
    fits = _fits()
    pruned, full = fits["product"], fits["full"]
    dropped = 0
    for l, name in enumerate(NAMES):
        G = GAIN_MARGIN * STOP * (1.0 + np.abs(full["lnl"][l]))
        over = pruned["lnl"][l] - full["lnl"][l]
        D = np.flatnonzero(over < -G)
        dropped += len(D)
        W = math.fsum(full["weights"][l, D])
        lim = np.zeros(6)
        for m in D:
            for f in (pruned, full):
                lim = np.maximum(lim, np.abs(f["model_exch"][l, m] - full["exch"][l]))
        # outside D a lnL may differ by up to G, which moves a weight by at most e^2G - 1 <= 4 G relative, and the two averages
        # round separately (4 * 203 eps relative, as in test_averaging)
        spread = np.abs(np.concatenate([pruned["model_exch"][l], full["model_exch"][l]]) - full["exch"][l]).max(axis=0)
        lim = 2.0 * W * lim + 4.0 * G.max() * spread + 8 * 203 * EPS * full["exch"][l]
        diff = np.abs(pruned["exch"][l] - full["exch"][l])
        print("stage1-models abandoning %s: %d models below the full run by more than G, deficits up to %.3g, their weight %.3g (largest %.3g, "
              "e^-21 = %.3g); largest lnl_pruned - lnl_full %.3g (G %.3g); |exch_pruned - exch_full| %.3g, bound %.3g"
              % (name, len(D), -over.min(), W, full["weights"][l, D].max() if len(D) else 0.0, math.exp(-PRUNE_NATS), over.max(), G.min(),
                 diff.max(), lim.max()))
        assert np.all(over <= G), name
        assert np.all(full["weights"][l, D] < math.exp(-PRUNE_NATS)), name
        if name == "A":
            assert len(D) == 0
        assert np.all(diff <= lim), (name, diff, lim)
    print("stage1-models abandoning: %d models in all, stats['pruned'] %d" % (dropped, pruned["stats"]["pruned"]))
    assert dropped <= pruned["stats"]["pruned"] and full["stats"]["pruned"] == 0


# ---- 5. averaging ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("call", CALLS)
def test_averaging(call, name):
    l = NAMES.index(name)
    fit = _fits()[call]
    w, lnl = fit["weights"][l], fit["lnl"][l]
    assert np.isfinite(w).all() and np.all(w >= 0.0)
    bound = 4 * EPS * (2 * np.abs(lnl).max() + 203)
    tiny = 2.0 ** -1022
    with mpmath.workdps(hp.DPS):
        ref = hp.akaike_weights(lnl, NFREE)
        worst = 0.0
        for m in range(203):
            if ref[m] < tiny:
                assert w[m] <= tiny * (1 + bound), (m, w[m])
            else:
                worst = max(worst, float(abs(mpmath.mpf(float(w[m])) - ref[m]) / ref[m]))
        total = float(abs(mpmath.fsum(mpmath.mpf(float(x)) for x in w) - 1))
        avg = [mpmath.fsum(mpmath.mpf(float(w[m])) * mpmath.mpf(float(fit["model_exch"][l, m, q])) for m in range(203)) for q in range(6)]
        eavg = max(float(abs(mpmath.mpf(float(fit["exch"][l, q])) - avg[q]) / avg[q]) for q in range(6) if q != 1)
    print("stage1-models averaging %s %s: weights error / bound %.3g (bound %.2e), |sum - 1| / bound %.3g, exch error / bound %.3g, "
          "smallest weight %.3g" % (name, call, worst / bound, bound, total / (203 * EPS), eavg / (4 * 203 * EPS), w.min()))
    assert worst <= bound and total <= 203 * EPS and eavg <= 4 * 203 * EPS and fit["exch"][l, 1] == 1.0
    if name == "D":       # the trailing models
        assert w.min() < math.exp(-PRUNE_NATS)


# ---- 6. batch independence ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_a_locus_fitted_alone_gives_the_same_rows(name):
    l = NAMES.index(name)
    batch, alone = _fits()["product"], _fits()["alone"][l]
    for key in ("lnl", "weights", "exch", "model_exch", "pi", "grm_blen"):
        assert np.array_equal(batch[key][l], alone[key][0]), (key, np.abs(batch[key][l] - alone[key][0]).max())

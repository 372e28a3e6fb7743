"""The site-likelihood and PI kernels against plain high-precision references (tests/hp_reference.py: mpmath at 40
digits, scipy.integrate.quad), over the whole domain the kernels accept and at the edges of their tiling.  Run with
-m gpu on the MI355X box.

The CPU oracle restates the kernels' formulas on purpose, so an approximation both share is invisible to the parity
tests; these references share nothing with either.  Bounds, with the largest error observed on one MI355X in
parentheses (each bound is at most 10x its record):
  eval_columns, u in [-3, 25]     |df| / max(1, |f|)              |dg|, |dh| / (1 + |h_ref|)
    GTR                           3e-13   (3.7e-14)               2e-12   (2.2e-13)
    GTR, absent base floored      8e-13   (8.0e-14)               1.5e-11 (1.9e-12)
    F81                           1e-14   (1.5e-15)               1e-12   (1.0e-13)
    F81, absent base              2e-14   (2.9e-15)               1e-12   (1.2e-13)
  eval_columns at u = kUMin, -15, -8: the same bounds, xfail (t s << 1 costs the fp64 forms their digits: up to 8e-2 in f
    at kUMin on the 3-taxon tree, and one NaN with a floored base)
  site_rates        flags, rates and lnL vs the oracle by the rules of test_gpu_parity._assert_rates_match
  net PI, disc      1e-12 relative, absolute below 1e-290                                  (2.9e-14)
  sum(integral)     QUADPACK: 1e-12 relative to math.fsum of the scipy values              (2.4e-16)
                    closed form: 1e-12 relative to math.fsum of the exact values           (2.8e-14)
  sum(error)        1e-6 relative over loci of >= 1000 sites (the golden rule), else 1e-3: a few sites' abserr keep their
                    rounding noise                                                         (1.9e-7; 4.6e-4 on 5 sites)
  per site          the rule of test_gpu_parity.test_per_site_quad_vs_reference
"""
import math

import numpy as np
import pytest

import fast_exp_emulation as fexp
import hp_reference as hp

pytestmark = pytest.mark.gpu

U_MIN = -23.025850929940457   # kUMin = log(1e-10)
U_MAX = 9.210340371976184     # kUMax = log(1e4)
S_MAX = 1e4
ONES = np.ones(6)


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _arrays(spec):
    """Nested lists of taxon indices -> post-order (parent, leaf_taxon), root last."""
    parent, leaf = [], []

    def walk(node):
        if isinstance(node, int):
            parent.append(-1)
            leaf.append(node)
            return len(parent) - 1
        kids = [walk(c) for c in node]
        parent.append(-1)
        leaf.append(-1)
        me = len(parent) - 1
        for k in kids:
            parent[k] = me
        return me

    walk(spec)
    return np.array(parent, np.int32), np.array(leaf, np.int32)


def _caterpillar(n):
    spec = [0, 1]
    for i in range(2, n):
        spec = [spec, i]
    return spec


def _balanced(taxa):
    if len(taxa) == 1:
        return taxa[0]
    h = len(taxa) // 2
    return [_balanced(taxa[:h]), _balanced(taxa[h:])]


def _tree(spec, rng, tiny=None, long=None, long_len=3000.0):
    parent, leaf = _arrays(spec)
    blen = np.exp(rng.uniform(np.log(0.01), np.log(2.0), len(parent)))
    blen[parent < 0] = 0.0
    if tiny is not None:
        blen[tiny] = 1e-9
    if long is not None:
        blen[long] = long_len
    return parent, blen, leaf


def _columns(ntaxa, rng):
    """Constant columns, an all-different one, single-resolved ones, every IUPAC mask among resolved bases, random."""
    cols = [[b] * ntaxa for b in (1, 2, 4, 8)]
    cols.append([1 << (i % 4) for i in range(ntaxa)])
    cols.append([1] + [15] * (ntaxa - 1))
    cols.append([15] * (ntaxa - 1) + [4])
    for m in range(1, 16):
        cols.append([m if i % 2 == 0 else 1 << ((i + m) % 4) for i in range(ntaxa)])
    for _ in range(4):
        cols.append(list(rng.choice([1, 2, 4, 8, 1, 2, 4, 8, 5, 10, 15, 3], ntaxa)))
    return np.ascontiguousarray(np.array(cols, np.uint8).T)


TREES = [("caterpillar3", lambda: _caterpillar(3)), ("balanced8", lambda: _balanced(list(range(8)))),
         ("caterpillar17", lambda: _caterpillar(17))]
MODELS = [  # (name, model, pi, exch)
    ("gtr", "gtr", [0.1, 0.2, 0.3, 0.4], [1e-3, 1e3, 0.5, 20.0, 100.0, 3e-2]),
    ("gtr_absent_base", "gtr", [0.3, 0.4, 0.3, 0.0], [1.0, 2.0, 0.5, 1.5, 3.0, 1.0]),
    ("f81", "f81", [0.1, 0.2, 0.3, 0.4], None),
    ("f81_absent_base", "f81", [0.5, 0.0, 0.25, 0.25], None),
]
U_GRID = [-3.0, -1.0, 0.0, 1.0, 3.0, U_MAX, 12.0, 17.0, 21.0, 25.0]
U_TINY = [U_MIN, -15.0, -8.0]   # t s << 1: see test_likelihood_curve_at_tiny_rates
# (f bound, g/h bound) per model family; see the module docstring for the record behind them
BOUNDS = {"gtr": (3e-13, 2e-12), "gtr_absent_base": (8e-13, 1.5e-11), "f81": (1e-14, 1e-12), "f81_absent_base": (2e-14, 1e-12)}


def _curve_errors(engine, mname, model, pi, exch, tname, spec, grid):
    rng = np.random.default_rng(len(tname) * 7 + len(mname))
    parent, blen, leaf = _tree(spec(), rng, tiny=0, long=1)
    ntaxa = int((leaf >= 0).sum())
    st = _columns(ntaxa, rng)
    for b in np.flatnonzero(np.asarray(pi) == 0.0):     # an absent base is nobody's only state (its frequency is 0)
        st[st == 1 << b] = 1 if b else 2
    ncols = st.shape[1]
    plan = engine.Plan(ntaxa, parent, blen, leaf, [0, ncols], [pi], None if exch is None else [exch], 10, [1], [[0, 1]],
                       model=model)
    pi_ref = hp.floored_pi(pi) if model == "gtr" else np.asarray(pi) / np.sum(pi)
    F, G, H = hp.column_curves(st, parent, blen, leaf, pi_ref, exch, grid, model=model)
    ef, egh = np.zeros((len(grid), ncols)), np.zeros((len(grid), ncols))
    finite = True
    for iu, u in enumerate(grid):
        f, g, h = plan.eval_columns(st, np.full(ncols, u))
        finite = finite and bool(np.isfinite(f).all() and np.isfinite(g).all() and np.isfinite(h).all())
        ef[iu] = np.abs(f - F[iu]) / np.maximum(1.0, np.abs(F[iu]))
        egh[iu] = np.maximum(np.abs(g - G[iu]), np.abs(h - H[iu])) / (1.0 + np.abs(H[iu]))
    plan.close()
    print("curve %s %s per u: |df| %s ; |dg|,|dh| %s" % (tname, mname, " ".join("%.1e" % v for v in ef.max(axis=1)),
                                                        " ".join("%.1e" % v for v in egh.max(axis=1))))
    return finite, ef, egh


@pytest.mark.parametrize("mname,model,pi,exch", MODELS, ids=[m[0] for m in MODELS])
@pytest.mark.parametrize("tname,spec", TREES, ids=[t[0] for t in TREES])
def test_likelihood_curve_over_its_whole_domain(mname, model, pi, exch, tname, spec):
    """f, g, h of eval_columns from u = -3 to 25 (kUMax included exactly) on trees with a 1e-9 branch and a branch of
    3000: every value finite and within the bounds of the module docstring of the 40-digit reference."""
    finite, ef, egh = _curve_errors(_engine(), mname, model, pi, exch, tname, spec, U_GRID)
    fb, gb = BOUNDS[mname]
    assert finite
    assert ef.max() <= fb, (np.unravel_index(ef.argmax(), ef.shape), ef.max())
    assert egh.max() <= gb, (np.unravel_index(egh.argmax(), egh.shape), egh.max())


@pytest.mark.xfail(strict=True, reason="known: P(t s) - I and 1 - exp(-t s) cancel in fp64 when t s << 1 (DESIGN.md section 9)")
@pytest.mark.parametrize("mname,model,pi,exch", MODELS, ids=[m[0] for m in MODELS])
@pytest.mark.parametrize("tname,spec", TREES, ids=[t[0] for t in TREES])
def test_likelihood_curve_at_tiny_rates(mname, model, pi, exch, tname, spec):
    """The same bounds at u = kUMin, -15 and -8.  The kernels form a change probability as U e^{Lambda t s} U^-1 (GTR) or
    1 - e^{-t s} (F81): at t s = 1e-11 it keeps about five digits, and with a floored base frequency the GTR form can go
    negative (a NaN log-likelihood).  Fixing it needs the expm1 form of the transition matrix; until then this records it."""
    finite, ef, egh = _curve_errors(_engine(), mname, model, pi, exch, tname, spec, U_TINY)
    fb, gb = BOUNDS[mname]
    assert finite and ef.max() <= fb and egh.max() <= gb


def _long_branch_case(rng, model):
    """An 8-taxon tree with one branch whose exponent lambda_k t s at s = 1e4 fell in a band where the unclamped
    exp_nonpos_tab returned +inf, checked on the emulation.  F81: lambda = -1, a branch of 3000.  GTR: the branch that puts
    the largest |lambda_k| t s at 3.5e7.  (Only the F81 case reached the band in the parent's optimiser: there the
    confirmation of far optima evaluated at s = 1e4; the GTR columns stopped by the flatness rule before.)"""
    parent, blen, leaf = _tree(_balanced(list(range(8))), rng)
    if model == "f81":
        pi, exch, t = np.array([0.2, 0.3, 0.15, 0.35]), None, 3000.0
        lam = np.array([-1.0])
    else:
        pi, exch = np.array([0.2, 0.3, 0.15, 0.35]), np.array([1.0, 3.0, 0.7, 1.2, 2.5, 0.9])
        Q, pim, _ = hp.rate_matrix(pi, exch)
        lam = np.sort(np.linalg.eigvals(np.array(Q.tolist(), dtype=float)).real)[:3]
        t = 1.5 * fexp.WRAP / (lam[0] * S_MAX)     # the largest |lambda_k| t s in the middle of the first band
    blen[2] = t
    x = lam * t * S_MAX
    assert any(fexp.exp_nonpos_tab(float(v), clamp=False) == math.inf for v in x), x
    assert all(fexp.exp_nonpos_tab(float(v)) == 0.0 for v in x)
    # comfortably inside a band: the device eigenvalues differ from these in the last bits only
    assert any(1.05 * fexp.WRAP > v > 1.95 * fexp.WRAP for v in x), x
    return parent, blen, leaf, pi, exch


@pytest.mark.parametrize("model", ["f81", "gtr"])
def test_optimiser_on_a_long_branch(oracle, model):
    """site_rates where the saturation check at s = 1e4 meets an exponent beyond -2.33e7 on one branch (before the
    clamp: +inf from exp, NaN lnL, wrong flags).  Flags, rates and lnL against the oracle (libm exp)."""
    engine = _engine()
    from test_gpu_parity import _assert_rates_match
    rng = np.random.default_rng(5 if model == "f81" else 6)
    parent, blen, leaf, pi, exch = _long_branch_case(rng, model)
    st = np.concatenate([_columns(8, rng), rng.choice(np.array([1, 2, 4, 8, 1, 2, 4, 8, 15, 5], np.uint8), (8, 200))],
                        axis=1)
    st = np.ascontiguousarray(st)
    ncols = st.shape[1]
    plan = engine.Plan(8, parent, blen, leaf, [0, ncols], [pi], None if exch is None else [exch], 10, [1], [[0, 1]],
                       model=model)
    got = plan.site_rates(st)
    kappa = plan.models()[3][0]
    ex = ONES if exch is None else exch
    ref = oracle.site_rates(st, parent, blen, leaf, pi, ex)
    assert np.isfinite(got["lnl"]).all() and np.isfinite(got["rate"]).all()
    assert np.array_equal(got["nres"], ref["nres"])
    assert np.array_equal(got["flag"], ref["flag"]), np.flatnonzero(got["flag"] != ref["flag"])
    assert (ref["flag"] == 2).sum() >= 3 and (ref["flag"] == 0).sum() >= 20, np.bincount(ref["flag"])
    pin = dict(parent=parent, blen=blen, leaf=leaf)
    _assert_rates_match(oracle, got, ref, slice(0, ncols), st, pin, pi, ex, kappa)
    assert np.abs(got["lnl"] - ref["lnl"]).max() < 1e-10 * max(1.0, np.abs(ref["lnl"]).max())
    plan.close()


# ---- PI tables ------------------------------------------------------------------------------------------------------

_DUMMY_TREE = ([2, 2, 4, 4, -1], [1.0, 1.0, 1.0, 1.0, 0.0], [0, 1, -1, 2, -1])   # the PI stage never looks at it


def _pi_rates(rng, n, correction):
    """Log-uniform rates in 1e-8..1e3 (final, i.e. after / correction), with exact zeros, NaNs, values that round to 0 at
    four decimals, and pairs on both sides of 4 r hl = 30 (the factored / generic panel switch) in every 64-column group."""
    r = np.exp(rng.uniform(np.log(1e-8), np.log(1e3), n)) * correction
    k = np.arange(n)
    r[k % 17 == 3] = 0.0
    r[k % 23 == 5] = np.nan
    r[k % 19 == 7] = 3e-5
    for hl in (0.5, 2.0, 5.0, 250.0):
        edge = 30.0 / (4.0 * hl) * correction
        r[k % 64 == int(hl * 7) % 61] = edge * (1 - 1e-9)
        r[k % 64 == (int(hl * 7) + 1) % 61] = edge * (1 + 1e-9)
    return r


def _check_table(tab, off, rates, nres, T, times, iv, mode, round_decimals, correction, threshold=3):
    n_t, n_i = len(times), len(iv)
    fin = hp.finalize_rates(rates, round_decimals, correction, nres, threshold)
    worst = {}
    for l in range(len(off) - 1):
        r = fin[off[l]:off[l + 1]]
        row = tab[l]
        net = hp.net_pi(r, T)
        assert np.isfinite(row).all(), l
        rel = np.abs(row[:T] - net) / np.maximum(np.abs(net), 1e-290)
        assert rel.max(initial=0) <= 1e-12, (l, int(rel.argmax()), row[rel.argmax()], net[rel.argmax()])
        assert np.array_equal(row[T:T + n_t], row[np.asarray(times, int)])
        worst["net"] = max(worst.get("net", 0.0), rel.max(initial=0))
        if n_i == 0:
            continue
        si, se = row[T + n_t:T + n_t + n_i], row[T + n_t + n_i:]
        if mode == 0:
            ri, re = hp.net_integrals_quad(r, iv)
            rel_e = np.abs(se - re) / np.maximum(np.abs(re), 1e-300)
            # the golden rule holds for sums over many sites; a few sites' abserr keep their rounding noise (the per-site
            # rule of test_per_site_quad_vs_reference)
            assert rel_e.max() <= (1e-6 if r.size >= 1000 else 1e-3), (l, r.size, rel_e.max())
            worst["error"] = max(worst.get("error", 0.0), rel_e.max())
        else:
            ri = hp.net_integrals_exact(r, iv)
            assert np.all(se == 0.0)
        rel_i = np.abs(si - ri) / np.maximum(np.abs(ri), 1e-290)
        assert rel_i.max() <= 1e-12, (l, int(rel_i.argmax()), si[rel_i.argmax()], ri[rel_i.argmax()])
        worst["integral"] = max(worst.get("integral", 0.0), rel_i.max())
    return worst


@pytest.mark.parametrize("mode,round_decimals,correction", [(0, 4, 10.0), (1, -1, 1.0), (1, 4, 100.0)],
                         ids=["quadpack-round4-corr10", "closed-noround", "closed-round4-corr100"])
def test_pi_tables_at_column_tiling_edges(mode, round_decimals, correction):
    """Loci of 0, 1, 5, 1023, 1024, 1025, 2049 and 4097 columns (1024 per workgroup) in one plan, nine intervals (the second
    interval tile), culled columns."""
    engine = _engine()
    rng = np.random.default_rng(40 + mode + round_decimals)
    sizes = [0, 1, 5, 1023, 1024, 1025, 2049, 4097]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    rates = _pi_rates(rng, n, correction)
    nres = rng.integers(0, 12, n).astype(np.int32)
    nres[off[1]] = 5          # the 1-column locus keeps its site
    T, times = 17, [0, 16]
    iv = [[0, 1], [0, 500], [3, 7], [10, 20], [20, 30], [85, 95], [45, 55], [0, 10], [499, 500]]
    parent, blen, leaf = _DUMMY_TREE
    L = len(sizes)
    plan = engine.Plan(3, parent, blen, leaf, off, [[.25] * 4] * L, [[1.0] * 6] * L, T, times, iv, correction=correction,
                       threshold=3, round_decimals=round_decimals, integ_mode=mode)
    tab = plan.pi_tables(rates, nres)
    worst = _check_table(tab, off, rates, nres, T, times, iv, mode, round_decimals, correction)
    print("pi tiling mode %d: %s" % (mode, {k: "%.2e" % v for k, v in worst.items()}))
    plan.close()


@pytest.mark.parametrize("T,n_i", [(1, 0), (15, 1), (16, 8), (17, 9), (200, 33)])
@pytest.mark.parametrize("mode", [0, 1], ids=["quadpack", "closed"])
def test_pi_tables_at_time_and_interval_tiling_edges(T, n_i, mode):
    """T around the 16-point time tile, n_i around the 8-interval tile; equal- and mixed-length intervals, [0,1] and
    [0,500]; times at 0 and T - 1."""
    engine = _engine()
    rng = np.random.default_rng(T * 100 + n_i * 3 + mode)
    off = np.array([0, 1, 65, 365], np.int64)
    n = int(off[-1])
    rates = _pi_rates(rng, n, 1.0)
    base = [[0, 1], [0, 500], [85, 95], [45, 55], [10, 11], [100, 101], [3, 7], [0, 100], [499, 500]]
    iv = [base[k] if k < len(base) else [5 * (k - 9), 5 * (k - 9) + 5] for k in range(n_i)]   # mixed, then equal lengths
    times = [0, T - 1]
    parent, blen, leaf = _DUMMY_TREE
    plan = engine.Plan(3, parent, blen, leaf, off, [[.25] * 4] * 3, [[1.0] * 6] * 3, T, times, iv, correction=1.0,
                       threshold=0, round_decimals=-1, integ_mode=mode)
    tab = plan.pi_tables(rates)
    worst = _check_table(tab, off, rates, None, T, times, iv, mode, -1, 1.0)
    print("pi T=%d n_i=%d mode %d: %s" % (T, n_i, mode, {k: "%.2e" % v for k, v in worst.items()}))
    plan.close()


def _per_site_rule(integral, abserr, rates, a, b):
    ref = np.array([hp.quad(float(a), float(b), float(r)) for r in rates])
    ref_int, ref_err = ref[:, 0], ref[:, 1]
    assert np.all(np.abs(integral - ref_int) <= 1e-13 * np.abs(ref_int) + 1e-28), (a, b)
    rel = np.abs(abserr - ref_err) / np.maximum(np.abs(ref_err), 1e-300)
    big = ref_err > 1e-12
    assert np.all(rel[big] < 1e-3) and np.median(rel) < 1e-9 and rel.max() < 0.5, (a, b, rel.max())


def test_per_site_factored_panel_vs_scipy():
    """One-column loci: every table row is one site's integral and abserr from pi_partial_kernel, which takes the factored
    first panel below 4 r hl = 30 and the generic one above it inside one wave.  Also engine.quad_townsend (the generic
    panel only) at extreme rates."""
    engine = _engine()
    rng = np.random.default_rng(9)
    rates = np.concatenate([np.exp(rng.uniform(np.log(1e-8), np.log(1e3), 96)),
                            [30.0 / 4.0 * (1 - 1e-9), 30.0 / 4.0 * (1 + 1e-9), 15.0 * (1 - 1e-9), 15.0 * (1 + 1e-9),
                             0.03 * (1 - 1e-9), 0.03 * (1 + 1e-9), 1.5, 3.75]])
    n = rates.size
    iv = [[0, 1], [3, 7], [0, 500], [85, 95], [0, 4], [4, 8], [8, 12]]
    parent, blen, leaf = _DUMMY_TREE
    off = np.arange(n + 1, dtype=np.int64)
    plan = engine.Plan(3, parent, blen, leaf, off, [[.25] * 4] * n, [[1.0] * 6] * n, 1, [0], iv, correction=1.0,
                       threshold=0, round_decimals=-1, integ_mode=0)
    tab = plan.pi_tables(rates)
    n_i = len(iv)
    for k, (a, b) in enumerate(iv):
        _per_site_rule(tab[:, 2 + k], tab[:, 2 + n_i + k], rates, a, b)
    plan.close()
    extreme = np.array([1e-300, 1e-30, 1e-12, 1e-8, 7.5 * (1 - 1e-12), 7.5, 7.5 * (1 + 1e-12), 1e3, 1e4, 1e6])
    for a, b in ([0, 1], [0, 500], [85, 95], [499, 500]):
        integral, abserr = engine.quad_townsend(a, b, extreme)
        _per_site_rule(integral, abserr, extreme, a, b)

"""Stage 2 on the spectra of tests/test_model_spectra.py: what gtr_setup_kernel writes into a LocusModel, and what
eval_columns, site_rates and the two quartet families make of it, against the 40-digit references, on exactly degenerate,
nearly degenerate and nearly reducible GTR models.  Run with -m gpu on the MI355X box.  Every test prints its figures before it
asserts.  The CPU side (tests/test_model_spectra.py, tests/gtr_setup_emulation.py) explains why the kept eigenvectors are
projected against sqrt(pi), and shows on the emulation that nothing else separates the two columns below.

Structure of plan.models() (test_model_structure), k = 1..3, a condition and not a measurement:
  |sum_j Ui[k][j]| <= 16 eps sum_j |Ui[k][j]|   and   |sum_i pi_i U[i][k]| <= 16 eps sum_i pi_i |U[i][k]|
with lam[0] == 0, U[:, 0] == 1, Ui[0] == pi and lam[1..3] < 0.

Curves (test_model_curves): f, g, h of eval_columns against hp.column_curves on test_gpu_numerics' balanced8 and caterpillar17
with its 1e-9 branch, its branch of 3000 and its columns, u in (-3, -1, 0, 3, kUMax), in that file's normalisations.  No
bound is fixed in advance: per (spectrum, tree) it is max(BOUNDS["gtr"] of test_gpu_numerics, 10 x the largest error the CPU
oracle shows against the reference on the very same (column, u) pairs), the rule of test_gpu_deep_tree_numerics.  The oracle
keeps all four Jacobi vectors (a consistent set), so its error is what the product form 1 pi + U e^(Lambda t s) U^-1 costs by
itself on entries of P of size |lam_1| t s; the GPU's output never enters the bound.

Seen on one MI355X, with the kept vectors as Jacobi left them -> projected against sqrt(pi) (the kernel): the larger structure sum
in eps, and error / bound as "f ; larger of g and h" at the worst u, which is always -3:
                      structure        balanced8                           caterpillar17
  blocks_1e-2         6.0 -> 6.0       .17 ; .17 -> the same               .26 ; .21 -> the same     (below the kernel's 8 eps: left alone)
  blocks_e-7          45.9 -> 1.3      4.5 ; 3.1 -> .069 ; .070            1.2 ; .93 -> .077 ; .072
  blocks_1e-4         1.19e3 -> 0.34   38 ; 38 -> .076 ; .076              18 ; 26 -> .049 ; .068
  blocks_1e-6         1.52e4 -> 0.57   117 ; 117 -> .11 ; .11              128 ; 117 -> .13 ; .15
  blocks_ac_gt        279 -> 0.41      38 ; 18 -> .25 ; .062               16 ; 18 -> .059 ; .78
  cut_off_t           783 -> 1.4       27 ; 23 -> .12 ; .098               14 ; 14 -> .11 ; 1.4
  the other nine      <= 1.8 (left alone: their bits do not move)  <= .27 ; .71      <= .15 ; 3.4
(bounds from 3.0e-13 ; 3.3e-12 on the degenerate spectra to 1.3e-6 ; 4.2e-5 under blocks_1e-6: even a perfect eigen-system cannot
give entries of P of size |lam_1| t s to 3e-13 in the product form, DESIGN section 9 "accuracy at t s << 1").  Run against the
kernel before the projection this file fails in test_model_structure on the five spectra from e^-7 on, in test_model_curves on
both trees of each and on caterpillar17 under f81_ct_1e-9, and in test_site_rates_on_block_models under blocks_1e-4.
The two figures above 1 that are left are h alone, on one random column of caterpillar17 at u = -3: 3.4 under f81_ct_1e-9 (1.1e-11
against 3.3e-12; the model's bits are those from before the projection, so this is none of its doing) and 1.4 under cut_off_t
(7.6e-8 against 5.5e-8, the oracle being at 5.5e-9).  h on a ladder at u = -3 is DESIGN section 9's "curvature on long ladders":
on caterpillar17 it sits between 0.1 and 3.4 of this bound on every spectrum and moves with the last bits of the model (a variant
of the kernel that re-orthonormalised every model, well separated ones too, put jc at 1.5 and these two at .14 and .63).  f and g
are inside there, and so is h at every other u: test_model_curves_residue holds h on those two (spectrum, tree, u) as a strict xfail.

site_rates (test_site_rates_on_block_models): caterpillar17 with a cherry of two branches of 2e-5, the e^-7 and 1e-4 block models,
by the rules of test_gpu_deep_tree_numerics for every flag.  Largest error / bound, before -> after: lnl at an interior optimum
.058 -> .0039 (e^-7) and 70 -> .11 (1e-4: 6.96e-10 against 1e-11 before); slope 1.5e-5 -> 1.9e-5 and 1.8e-5 after; lnl of the
saturated columns .31 -> .0052 and .14 after.

Quartets (test_quartet_sites_on_a_double_eigenvalue_and_on_blocks): error / bound .034 (equal) and .022 (unequal) under
blocks_e-7 before, .027 / .015 (equal: hky / blocks_e-7) and .037 / .014 (unequal) after.  Both families build their matrices as
I + U expm1(Lambda t) U^-1 (csrc/transition_row.hpp), which multiplies the stray component by expm1(lam_1 t): inside either way.

The product reaching the domain (test_stage1_hands_stage2_a_nearly_reducible_model): stage1_fit on 60 hand-made columns whose only
differences are transitions gives AC AG AT CG CT GT = 9.12e-4 1 9.12e-4 9.12e-4 0.885 9.12e-4 (the transversions parked at
e^-7, largest transversion / smallest transition 1.03e-3; lam_1 = -9.1e-4); eval_columns under that model: .028 ; .023 of the
bound after (not taken before).
"""
import math

import numpy as np
import pytest

import hp_reference as hp
import quartet_reference as qr
import test_gpu_deep_tree_numerics as deep
import test_gpu_numerics as num
import test_gpu_quartet as gq
import test_gpu_unequal_quartet as guq
import test_model_spectra as ms
import unequal_quartet_reference as ur

pytestmark = pytest.mark.gpu

EPS = ms.EPS
NAMES = list(ms.SPECTRA)
U_GRID = (-3.0, -1.0, 0.0, 3.0, num.U_MAX)       # -3 matters most: the loss grows as t s falls
CURVE_TREES = ("balanced8", "caterpillar17")
_CACHE = {}


def _spectrum_arrays(names):
    return (np.array([hp.floored_pi(ms.SPECTRA[n][0]) for n in names]), np.array([ms.SPECTRA[n][1] for n in names], float))


# ---- the eigen-system itself ------------------------------------------------------------------------------------------

def _models():
    if "models" not in _CACHE:
        engine = num._engine()
        pi, exch = _spectrum_arrays(NAMES)
        parent, blen, leaf = num._DUMMY_TREE
        plan = engine.Plan(3, parent, blen, leaf, np.arange(len(NAMES) + 1), pi, exch, 10, [1], [[0, 1]])
        try:
            _CACHE["models"] = plan.models()
        finally:
            plan.close()
    return _CACHE["models"]


@pytest.mark.parametrize("name", NAMES)
def test_model_structure(name):
    """The layout's promises and both structure sums within 16 eps, on every spectrum; U Ui = I and kappa as well."""
    lam, U, Ui, kappa = (x[NAMES.index(name)] for x in _models())
    pi = hp.floored_pi(ms.SPECTRA[name][0])
    rows, cols = ms.structure_sums(U[:, 1:], Ui[1:], Ui[0])
    print("structure %s: lam %s; sums in eps: rows of Ui %s ; columns of U %s" % (
        name, lam[1:], " ".join("%.3g" % v for v in rows), " ".join("%.3g" % v for v in cols)))
    assert lam[0] == 0.0 and np.all(U[:, 0] == 1.0) and np.allclose(Ui[0], pi, rtol=0, atol=1e-15)
    assert np.all(lam[1:] < 0)
    assert rows.max() <= 16.0 and cols.max() <= 16.0
    assert np.abs(U @ Ui - np.eye(4)).max() <= 64 * EPS / math.sqrt(pi.min())        # |U| |Ui| <= sqrt(1 / min pi)
    assert abs(kappa - hp.kappa(pi, ms.SPECTRA[name][1])) <= 8 * EPS * kappa


# ---- eval_columns ---------------------------------------------------------------------------------------------------

def _errors(f, g, h, F, G, H):
    return np.abs(f - F) / np.maximum(1.0, np.abs(F)), np.maximum(np.abs(g - G), np.abs(h - H)) / (1.0 + np.abs(H))


def _reference_case(oracle, tree, st, pi, exch):
    """The 40-digit curves [len(U_GRID), ncols] of one model, and the bound the oracle's own error on them sets."""
    F, G, H = hp.column_curves(st, *tree, pi, exch, U_GRID)
    of, og, oh = (np.empty_like(F) for _ in range(3))
    grid = np.array(U_GRID)
    for c in range(st.shape[1]):
        of[:, c], og[:, c], oh[:, c] = oracle.column_curve(st, *tree, pi, np.asarray(exch, float), c, grid)
    oef, oegh = _errors(of, og, oh, F, G, H)
    fb, gb = num.BOUNDS["gtr"]
    return dict(F=F, G=G, H=H, oef=oef.max(), oegh=oegh.max(), fb=max(fb, 10.0 * oef.max()), gb=max(gb, 10.0 * oegh.max()))


def _tree_inputs(tname):
    rng = np.random.default_rng(4000 + 13 * len(tname))         # one tree and one set of columns per tree, whatever the model
    parent, blen, leaf = num._tree(dict(num.TREES)[tname](), rng, tiny=0, long=1)
    ntaxa = int((leaf >= 0).sum())
    return (parent, blen, leaf), ntaxa, num._columns(ntaxa, rng)


def _gpu_curves(tname):
    """eval_columns of every spectrum on one tree: one plan, a locus per spectrum, one call per u.  [3, len(U_GRID), L, ncols]"""
    if ("gpu", tname) not in _CACHE:
        engine = num._engine()
        tree, ntaxa, st = _tree_inputs(tname)
        n, L = st.shape[1], len(NAMES)
        pi, exch = _spectrum_arrays(NAMES)
        plan = engine.Plan(ntaxa, *tree, np.arange(L + 1) * n, pi, exch, 10, [1], [[0, 1]], model="gtr")
        try:
            tiled = np.ascontiguousarray(np.tile(st, (1, L)))
            got = np.array([plan.eval_columns(tiled, np.full(L * n, u)) for u in U_GRID])     # [u, 3, L n]
        finally:
            plan.close()
        _CACHE["gpu", tname] = got.transpose(1, 0, 2).reshape(3, len(U_GRID), L, n)
    return _CACHE["gpu", tname]


def _curve_figures(oracle, name, tname):
    if ("curve", name, tname) not in _CACHE:
        tree, _, st = _tree_inputs(tname)
        pi, exch = hp.floored_pi(ms.SPECTRA[name][0]), ms.SPECTRA[name][1]
        ref = _reference_case(oracle, tree, st, pi, exch)
        f, g, h = _gpu_curves(tname)[:, :, NAMES.index(name), :]
        ef, _ = _errors(f, g, h, ref["F"], ref["G"], ref["H"])
        eg, eh = np.abs(g - ref["G"]) / (1.0 + np.abs(ref["H"])), np.abs(h - ref["H"]) / (1.0 + np.abs(ref["H"]))
        per_u = lambda e, b: " ".join("%.3g" % v for v in e.max(axis=1) / b)      # noqa: E731
        print("curves %s %s: error / bound per u  f %s ; g %s ; h %s   (bounds %.1e %.1e; oracle's largest error %.1e %.1e)" % (
            name, tname, per_u(ef, ref["fb"]), per_u(eg, ref["gb"]), per_u(eh, ref["gb"]), ref["fb"], ref["gb"], ref["oef"], ref["oegh"]))
        finite = bool(np.isfinite(f).all() and np.isfinite(g).all() and np.isfinite(h).all())
        _CACHE["curve", name, tname] = dict(finite=finite, ef=ef, eg=eg, eh=eh, fb=ref["fb"], gb=ref["gb"])
    return _CACHE["curve", name, tname]


# (spectrum, tree) -> the u at which h, and h alone, misses the bound: the ladder's curvature (module docstring)
RESIDUE = {("f81_ct_1e-9", "caterpillar17"): (-3.0,), ("cut_off_t", "caterpillar17"): (-3.0,)}


def _residue_rows(name, tname):
    return np.array([u in RESIDUE.get((name, tname), ()) for u in U_GRID])


@pytest.mark.parametrize("tname", CURVE_TREES)
@pytest.mark.parametrize("name", NAMES)
def test_model_curves(oracle, name, tname):
    """f, g, h at every u of U_GRID within max(BOUNDS, 10 x the oracle's own error) of the 40-digit reference.  On the
    (spectrum, tree, u) of RESIDUE h, and nothing else, is left to test_model_curves_residue."""
    r = _curve_figures(oracle, name, tname)
    held = ~_residue_rows(name, tname)
    assert r["finite"]
    assert r["ef"].max() <= r["fb"], (np.unravel_index(r["ef"].argmax(), r["ef"].shape), r["ef"].max(), r["fb"])
    assert r["eg"].max() <= r["gb"], (np.unravel_index(r["eg"].argmax(), r["eg"].shape), r["eg"].max(), r["gb"])
    assert r["eh"][held].max() <= r["gb"], (np.argwhere(r["eh"] > r["gb"]).tolist(), r["eh"][held].max(), r["gb"])


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="known: h = L''/L - g^2 on a ladder at u = -3 (DESIGN.md section 9, curvature on long ladders)")
@pytest.mark.parametrize("name,tname", list(RESIDUE))
def test_model_curves_residue(oracle, name, tname):
    """The same bound for h at the u of RESIDUE, where the kernel misses it on one random column of caterpillar17 at u = -3:
    by 3.4 under f81_ct_1e-9 (1.1e-11 against 3.3e-12; the model's bits are the ones from before the projection) and by 1.4
    under cut_off_t (7.6e-8 against 5.5e-8).  f and g are held there by test_model_curves."""
    r = _curve_figures(oracle, name, tname)
    rows = _residue_rows(name, tname)
    assert rows.any()
    assert r["eh"][rows].max() <= r["gb"], (r["eh"][rows].max(), r["gb"])


# ---- site_rates -----------------------------------------------------------------------------------------------------

def _rate_columns(rng):
    """17 taxa.  Columns that need transitions only: drawn from {A, G}, from {C, T}, in runs of 1 to 4 neighbouring taxa, half
    with a tenth of gaps.  Columns that need a transversion across the blocks: the first k taxa from one block and the others
    from the other one, one or two taxa of the other block, all four bases at random.  Then two columns of gaps but for two
    different bases on taxa 0 and 1, a cherry of two branches of 2e-5 (_rate_case): still uphill at the largest rate, one by a
    transition and one by a transversion.  In every other column taxon 1 repeats taxon 0 (the reason is in
    test_gpu_deep_tree_numerics._rate_columns)."""
    n, cols = 17, []
    for run in (1, 2, 4):
        for alphabet in ([1, 4], [2, 8]):
            for gaps in (False, True):
                col = np.repeat(rng.choice(alphabet, -(-n // run)), run)[:n].astype(np.uint8)
                if gaps:
                    col[rng.random(n) < 0.1] = 15
                cols.append(col)
    n_within = len(cols)
    for k in (2, 5, 9, 14):
        for left, right in (([1, 4], [2, 8]), ([8], [1]), ([2, 8], [4])):
            cols.append(np.concatenate([rng.choice(left, k), rng.choice(right, n - k)]).astype(np.uint8))
    for where in ([6], [3, 12]):
        col = rng.choice([1, 4], n).astype(np.uint8)
        col[where] = 2
        cols.append(col)
    cols += [rng.choice([1, 2, 4, 8], n).astype(np.uint8) for _ in range(2)]
    st = np.array(cols, np.uint8).T
    st[1] = st[0]
    pairs = np.full((n, 2), 15, np.uint8)
    pairs[0], pairs[1] = [1, 1], [4, 2]
    return np.ascontiguousarray(np.concatenate([st, pairs], axis=1)), n_within


def _rate_case(oracle, name):
    """As test_gpu_deep_tree_numerics._rate_case: the columns sent to the reference are chosen on the CPU with the oracle."""
    pi, exch = hp.floored_pi(ms.SPECTRA[name][0]), np.asarray(ms.SPECTRA[name][1], float)
    rng = np.random.default_rng(5000)
    parent, blen, leaf = num._tree(num._caterpillar(17), rng)
    assert leaf[0] == 0 and leaf[1] == 1 and parent[0] == parent[1]
    blen[0] = blen[1] = 2e-5
    st, n_within = _rate_columns(rng)
    ref = oracle.site_rates(st, parent, blen, leaf, pi, exch)
    interior = np.flatnonzero(ref["flag"] == 0)
    within, across = interior[interior < n_within], interior[interior >= n_within]
    assert within.size >= 5 and across.size >= 5, (name, np.bincount(ref["flag"]), within, across)
    pick = lambda a: a[np.linspace(0, a.size - 1, 5).astype(int)]      # noqa: E731
    saturated = np.array([st.shape[1] - 2, st.shape[1] - 1])
    assert np.all(ref["flag"][saturated] == 2)
    return dict(parent=parent, blen=blen, leaf=leaf, ntaxa=17, st=st, model="gtr", pi=pi, exch=exch, pi_ref=pi, oracle=ref,
                interior=np.concatenate([pick(within), pick(across)]), saturated=saturated, kappa=hp.kappa(pi, exch))


@pytest.mark.parametrize("name", ["blocks_e-7", "blocks_1e-4"])
def test_site_rates_on_block_models(oracle, name):
    """site_rates on caterpillar17 under the e^-7 and 1e-4 block models: every flag by the rule of
    test_gpu_deep_tree_numerics (its module docstring), against the 40-digit curve at the rate the kernel returned, on five
    interior columns that need transitions only, five that need a transversion across the blocks and two saturated ones."""
    engine = num._engine()
    case = _rate_case(oracle, name)
    ncols = case["st"].shape[1]
    plan = engine.Plan(17, case["parent"], case["blen"], case["leaf"], [0, ncols], [case["pi"]], [case["exch"]], 10, [1], [[0, 1]],
                       model="gtr")
    try:
        got = plan.site_rates(case["st"])
    finally:
        plan.close()
    deep._assert_rates(17, name, case, got)


# ---- the two quartet families -----------------------------------------------------------------------------------------

QUARTET_LOCI = ("hky", "blocks_e-7")
N_SITES = 12
EQUAL_Q = [gq.Q17[q] for q in gq.TWIN_Q]            # five (T, t_o)
UNEQUAL_Q = [guq.Q14[q] for q in guq.TWIN_Q[:5]]    # five (Ta, Tb, Tc, Td, t_o)


def _quartet_inputs():
    rng = np.random.default_rng(6000)
    n = N_SITES * len(QUARTET_LOCI)
    rates = 10.0 ** rng.uniform(-9, 3, n) * gq.CORRECTION
    nres = np.full(n, 5, np.int32)
    for a in range(0, n, N_SITES):
        rates[a], nres[a + 1], rates[a + 2], rates[a + 3] = 0.0, 2, 1e-9 * gq.CORRECTION, 1e3 * gq.CORRECTION
    return rates, nres, hp.finalize_rates(rates, -1, gq.CORRECTION, nres, 3)


def _quartet_figures(family):
    """The GPU's per-site planes of both loci against the twin at every (site, quartet) pair; the fp64 restatement's own error
    on the same pairs sets the bound."""
    engine = num._engine()
    rates, nres, fin = _quartet_inputs()
    pi, exch = _spectrum_arrays(QUARTET_LOCI)
    quartets = EQUAL_Q if family == "equal" else UNEQUAL_Q
    plan = engine.Plan(3, gq.PARENT, gq.BLEN, gq.LEAF, np.arange(len(QUARTET_LOCI) + 1) * N_SITES, pi, exch, 8, [], [],
                       correction=gq.CORRECTION, threshold=3, round_decimals=-1)
    try:
        got = plan.quartet_sites(rates, nres, quartets) if family == "equal" else plan.unequal_quartet_sites(rates, nres, quartets)
    finally:
        plan.close()
    out = {}
    for l, name in enumerate(QUARTET_LOCI):
        sl = slice(l * N_SITES, (l + 1) * N_SITES)
        e_rest, e_gpu, zeros_ok = 0.0, 0.0, True
        for q, row in enumerate(quartets):
            if family == "equal":
                rest = qr.site_values("gtr", pi[l], exch[l], fin[sl], *row)
                twin = qr.twin_values(pi[l], exch[l], fin[sl], *row)[:2]       # (y, x_ijij); x_ijji is the same by symmetry
            else:
                rest = ur.site_values("gtr", pi[l], exch[l], fin[sl], row[:4], row[4])
                twin = ur.twin_values(pi[l], exch[l], fin[sl], row[:4], row[4])
            for which in range(len(rest)):
                for c in range(N_SITES):
                    ref, g = twin[which][c], got[which, q, sl][c]
                    if ref == 0:
                        zeros_ok = zeros_ok and g == 0.0 and rest[which][c] == 0.0
                    else:
                        e_rest = max(e_rest, gq._relative(rest[which][c], ref))
                        e_gpu = max(e_gpu, gq._relative(g, ref))
        out[name] = (e_rest, max(16 * e_rest, 64 * EPS), e_gpu, zeros_ok)
    return out


@pytest.mark.parametrize("family", ["equal", "unequal"])
def test_quartet_sites_on_a_double_eigenvalue_and_on_blocks(family):
    """quartet_sites and unequal_quartet_sites on one plan with an HKY locus and an e^-7 block locus, 12 columns each (a zero
    rate, a culled column, 1e-9 and 1e3 among them), five quartets of the twin's sample of their own test files: relative,
    against the 40-digit twin, within 16 x the fp64 restatement's own error on the same pairs, at least 64 * 2^-52."""
    figures = _quartet_figures(family)
    for name, (e_rest, bound, e_gpu, zeros_ok) in figures.items():
        print("quartets %s %s: restatement against the twin %.3e, bound %.3e, GPU against the twin %.3e: error / bound = %.3f" % (
            family, name, e_rest, bound, e_gpu, e_gpu / bound))
    for name, (e_rest, bound, e_gpu, zeros_ok) in figures.items():
        assert zeros_ok, name
        assert e_gpu <= bound, (name, e_gpu, bound)


# ---- the product reaching the domain ----------------------------------------------------------------------------------

def _transition_locus():
    """60 hand-made columns on 5 taxa whose only differences are transitions: 30 constant ones, 15 over {A, G}, 15 over {C, T}."""
    cols = []
    for k in range(30):
        cols.append([1 << (k % 4)] * 5)
    for k in range(15):
        split = [(k >> i) & 1 for i in range(4)] + [1 - (k & 1)]
        cols.append([4 if s else 1 for s in split])
        cols.append([8 if s else 2 for s in split])
    return np.ascontiguousarray(np.array(cols, np.uint8).T)


def test_stage1_hands_stage2_a_nearly_reducible_model(oracle):
    """A locus whose only differences are transitions: stage 1 parks the transversion classes at the lower edge of its box, and
    the model-averaged exchangeabilities it hands to stage 2 are a block model.  eval_columns on the same plan under them, on
    test_gpu_numerics' 31 columns for 5 taxa and 29 of the locus' own, against the reference by the rule of test_model_curves."""
    from tapir_amd import synth
    engine = num._engine()
    pin = synth.plan_inputs(*synth.yule_tree(5, 23))            # the tree of test_gpu_stage1_models
    tree = (np.asarray(pin["parent"]), np.asarray(pin["blen"]), np.asarray(pin["leaf"]))
    locus = _transition_locus()
    assert locus.shape == (5, 60)
    resolved = locus[:, (locus != locus[0]).any(axis=0)]
    assert np.all(np.isin(resolved, [1, 4]).all(axis=0) | np.isin(resolved, [2, 8]).all(axis=0))     # transitions only
    generic = num._columns(5, np.random.default_rng(7000))
    st = np.ascontiguousarray(np.concatenate([generic, locus[:, generic.shape[1]:]], axis=1))
    plan = engine.Plan(5, *tree, [0, 60], [ms.PI], np.ones((1, 6)), pin["T"], [1], [[0, 1]], correction=pin["correction"])
    try:
        fit = plan.stage1_fit(locus)
        exch, pi = fit["exch"][0], hp.floored_pi(fit["pi"][0])
        ratio = exch[[0, 2, 3, 5]].max() / exch[[1, 4]].min()
        print("stage 1 on a transitions-only locus: averaged exchangeabilities %s, largest transversion / smallest transition %.3g"
              % (" ".join("%.6g" % v for v in exch), ratio))
        plan.set_models(exch=fit["exch"])
        got = np.array([plan.eval_columns(st, np.full(60, u)) for u in U_GRID])
        lam = plan.models()[0][0]
    finally:
        plan.close()
    assert np.allclose(pi, ms.PI, rtol=0, atol=1e-15)
    assert ratio <= 1e-2                                         # the premise: otherwise the case shows nothing new
    ref = _reference_case(oracle, tree, st, pi, exch)
    ef, egh = _errors(got[:, 0], got[:, 1], got[:, 2], ref["F"], ref["G"], ref["H"])
    print("curves under stage 1's model (lam %s): error / bound per u  f %s ; g, h %s   (bounds %.1e %.1e; oracle's largest error "
          "%.1e %.1e)" % (lam[1:], " ".join("%.3g" % v for v in ef.max(axis=1) / ref["fb"]),
                          " ".join("%.3g" % v for v in egh.max(axis=1) / ref["gb"]), ref["fb"], ref["gb"], ref["oef"], ref["oegh"]))
    assert np.isfinite(got).all()
    assert ef.max() <= ref["fb"] and egh.max() <= ref["gb"]

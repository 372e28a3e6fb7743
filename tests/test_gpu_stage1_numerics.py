"""The stage-1 likelihood and gradient kernels against a plain 40-digit reference (tests/hp_reference.py:
locus_reference, locus_dexch_reference), at the edges of their tiling, over the branch-length and rate domain, on every
kernel path.  Run with -m gpu on the MI355X box.

The CPU oracle restates U e^{Lambda t} U^-1, and the gradient was only ever compared with finite differences of that oracle
(noise floor 1e-9 .. 1e-6); the reference here shares nothing with either and its derivatives are analytic.

Paths (how a test reaches them):
  value_c1 / value_c2   locus_value_kernel<C, D>, TPHIP_VALUE_COLS = 1 / 2, register stack depth <= 5
  value_eigen           locus_loglik_kernel, TPHIP_VALUE_EIGENBASIS = 1, or a tree deeper than the register stack
  grad2                 locus_grad2_kernel<D>, the plan's device cache of the alignment, a binary tree
  grad                  locus_grad_kernel, no device cache; or a polytomy / a deeper tree with the cache

Error measures: |d lnL| / max(1, |lnL|); for dexch, dlogt, d2logt max|d| / max(1, max|ref|) over the array; sum_dlogt
against the sum of the reference's dlogt, relative to max(1, |sum|).

Bounds, with the largest error observed on one MI355X in parentheses (each bound is a round figure at most 10x its record;
no lnL bound above 1e-9, no first-derivative bound above 2e-6).  "ordinary": every case but the two below.  "extreme":
exchangeabilities six or more orders apart (MODELS[0] of test_gpu_numerics, and the optimiser's rate bounds e^-7 and e^9.2
side by side), where the fp64 eigen-system itself keeps fewer digits.
  ordinary      lnl              dexch            dlogt            d2logt           sum_dlogt
    value_c1    2e-14 (2.5e-15)
    value_c2    2e-14 (2.5e-15)
    value_eigen 2e-14 (2.7e-15)
    grad2       2e-14 (2.5e-15)  1e-12 (1.6e-13)  4e-13 (4.7e-14)  1e-12 (1.1e-13)  3e-13 (3.2e-14)
    grad        2e-14 (2.7e-15)  1e-12 (1.6e-13)  4e-13 (4.8e-14)  1e-12 (1.2e-13)  3e-13 (3.9e-14)
  extreme
    value_c1    4e-12 (4.2e-13)
    value_c2    4e-12 (4.2e-13)
    value_eigen 4e-12 (4.3e-13)
    grad2       4e-12 (4.2e-13)  1e-11 (1.3e-12)  8e-11 (8.6e-12)  7e-10 (7.5e-11)  9e-11 (9.5e-12)
    grad        4e-12 (4.3e-13)  1e-11 (1.4e-12)  8e-11 (8.6e-12)  7e-10 (7.5e-11)  9e-11 (9.5e-12)
Branches at the optimiser's lower bound (test_branches_at_the_lower_bound: three branches at t, the "ordinary" bounds): every
path misses them at every t and is xfail(strict).  Error of lnL, and the largest of any derivative, at
t = e^-23 / 1e-9 / 1e-8 / 1e-6:
    value_c1, value_c2   1.1e-7 / 1.1e-8 / 1.3e-9 / 1.3e-11
    value_eigen          1.1e-7 / 1.4e-8 / 1.2e-9 / 1.3e-11
    grad2                lnL as value_c1; derivatives 4.6e-6 / 4.2e-7 / 4.7e-8 / 4.5e-10
    grad                 lnL as value_eigen; derivatives 4.1e-6 / 4.9e-7 / 4.1e-8 / 4.8e-10
Forming P = I + U expm1(Lambda t) U^-1 in lik_pmat_kernel alone was tried: value_c1, value_c2 and grad2 then hold the bounds at
every t (1.6e-16; derivatives 4.3e-15), but the eigenbasis kernels cancel inside their main loops, and with one side exact
test_gpu_parity.test_locus_gradient_kernels_agree (1e-10 between the two gradient kernels, on branches down to 1e-7) no longer
holds: the four kernels have to change together.
The references are the slow side: about 9 s and 6 s of one CPU core for the two tiling trees (each distinct column once),
1 to 3 s for every other case.
"""
import math

import mpmath
import numpy as np
import pytest

import hp_reference as hp
from test_gpu_numerics import _arrays, _balanced, _caterpillar, _columns

pytestmark = pytest.mark.gpu

VALUE_PATHS = ("value_c1", "value_c2", "value_eigen")
GRAD_PATHS = ("grad2", "grad")
ALL_PATHS = VALUE_PATHS + GRAD_PATHS
OUTPUTS = ("lnl", "dexch", "dlogt", "d2logt", "sum_dlogt")
# bound per class of case, path and output.  "extreme": exchangeabilities six or more orders apart (the optimiser's rate bounds,
# MODELS[0] of test_gpu_numerics), where the eigen-system itself keeps fewer digits; "ordinary": everything else.
_G = ("lnl", "dexch", "dlogt", "d2logt", "sum_dlogt")
BOUNDS = {
    "ordinary": {
        "value_c1": {"lnl": 2e-14}, "value_c2": {"lnl": 2e-14}, "value_eigen": {"lnl": 2e-14},
        "grad2": dict(zip(_G, (2e-14, 1e-12, 4e-13, 1e-12, 3e-13))),
        "grad": dict(zip(_G, (2e-14, 1e-12, 4e-13, 1e-12, 3e-13))),
    },
    "extreme": {
        "value_c1": {"lnl": 4e-12}, "value_c2": {"lnl": 4e-12}, "value_eigen": {"lnl": 4e-12},
        "grad2": dict(zip(_G, (4e-12, 1e-11, 8e-11, 7e-10, 9e-11))),
        "grad": dict(zip(_G, (4e-12, 1e-11, 8e-11, 7e-10, 9e-11))),
    },
}
PI = np.array([0.1, 0.2, 0.3, 0.4])
EXCH = np.array([0.7, 1.0, 1.9, 0.4, 2.5, 1.1])


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


# ---- reference, column by column, each distinct column once ----------------------------------------------------------

_MEMO = {}


def _column_reference(parent, blen, leaf, pi, exch, cols, branches, want_dexch):
    """Per column of `cols` (mpf): log L, {b: g}, {b: h}, dexch [6] -- computed once per distinct column and parameter set."""
    parent, leaf = np.asarray(parent, np.int32), np.asarray(leaf, np.int32)
    blen, pi, exch = np.asarray(blen, np.float64), np.asarray(pi, np.float64), np.asarray(exch, np.float64)
    key = (parent.tobytes(), blen.tobytes(), leaf.tobytes(), pi.tobytes(), exch.tobytes(), tuple(branches), bool(want_dexch))
    memo = _MEMO.setdefault(key, {})
    cols = np.asarray(cols, np.uint8) & 15
    cols = np.where(cols == 0, 15, cols).astype(np.uint8)
    keys = [cols[:, c].tobytes() for c in range(cols.shape[1])]
    need = sorted(set(k for k in keys if k not in memo))
    if need:
        sub = np.ascontiguousarray(np.array([np.frombuffer(k, np.uint8) for k in need]).T)
        logl, g, h = hp.locus_reference_columns(sub, parent, blen, leaf, pi, exch, branches=branches)
        dex = hp.locus_dexch_reference_columns(sub, parent, blen, leaf, pi, exch) if want_dexch else None
        for i, k in enumerate(need):
            memo[k] = (logl[i], {b: g[b][i] for b in g}, {b: h[b][i] for b in h}, None if dex is None else [dex[q][i] for q in range(6)])
    return [memo[k] for k in keys]


def _reference(parent, blen, leaf, pi, exch, cols, weights, branches=None, want_dexch=True):
    """lnl, dexch [6] (or None), dlogt, d2logt (arrays over the nodes, NaN where not asked for) as floats."""
    parent = np.asarray(parent)
    nn = len(parent)
    if branches is None:
        branches = [int(b) for b in np.flatnonzero(parent >= 0)]
    g, h = np.full(nn, np.nan), np.full(nn, np.nan)
    if cols.shape[1] == 0:
        g[branches], h[branches] = 0.0, 0.0
        return 0.0, (np.zeros(6) if want_dexch else None), g, h
    per = _column_reference(parent, blen, leaf, pi, exch, cols, branches, want_dexch)
    w = [mpmath.mpf(1)] * len(per) if weights is None else [mpmath.mpf(float(x)) for x in weights]
    with mpmath.workdps(60):
        lnl = float(mpmath.fsum(wc * p[0] for wc, p in zip(w, per)))
        for b in branches:
            g[b] = float(mpmath.fsum(wc * p[1][b] for wc, p in zip(w, per)))
            h[b] = float(mpmath.fsum(wc * p[2][b] for wc, p in zip(w, per)))
        dex = np.array([float(mpmath.fsum(wc * p[3][q] for wc, p in zip(w, per))) for q in range(6)]) if want_dexch else None
    return lnl, dex, g, h


# ---- running one path ------------------------------------------------------------------------------------------------

def _plan(engine, monkeypatch, path, ntaxa, parent, blen, leaf, off, pi):
    monkeypatch.delenv("TPHIP_VALUE_COLS", raising=False)
    monkeypatch.delenv("TPHIP_VALUE_EIGENBASIS", raising=False)
    if path == "value_eigen":
        monkeypatch.setenv("TPHIP_VALUE_EIGENBASIS", "1")
    elif path in ("value_c1", "value_c2"):
        monkeypatch.setenv("TPHIP_VALUE_COLS", path[-1])
    L = len(off) - 1
    return engine.Plan(ntaxa, parent, blen, leaf, off, np.asarray(pi).reshape(L, 4), np.ones((L, 6)), 3, [1], [[0, 1]])


def _run(engine, monkeypatch, path, case, cache=None):
    """Outputs of one kernel path on a case: dict of arrays over the candidates.  cache: None = the path's own choice (grad2
    with the device cache, everything else without), True / False forces it."""
    plan = _plan(engine, monkeypatch, path, case["ntaxa"], case["parent"], case["blen"], case["leaf"], case["off"], case["pi"])
    if case.get("weights") is not None:
        plan.set_column_weights(case["weights"])
    use_cache = (path == "grad2") if cache is None else cache
    ch = plan.device_cache() if use_cache else None
    args = (case["st"], case["vecs"], case["cl"], case["ce"], case.get("cand_vec"), case.get("cand_scale"), case.get("cand_pidx"),
            case.get("cand_pfac"))
    out = {}
    if path in VALUE_PATHS:
        out["lnl"] = plan.locus_loglik(*args, cache=ch)
    else:
        out["lnl"], out["dexch"], out["dlogt"], out["sum_dlogt"], out["d2logt"] = plan.locus_gradient(*args, cache=ch, curvature=True)
    if ch is not None:
        ch.release()
    plan.close()
    return out


def _effective_blen(case, c):
    v = case["vecs"][c if case.get("cand_vec") is None else case["cand_vec"][c]].copy()
    if case.get("cand_scale") is not None:
        v = v * case["cand_scale"][c]
    if case.get("cand_pidx") is not None and case["cand_pidx"][c] >= 0:
        v[case["cand_pidx"][c]] *= case["cand_pfac"][c]
    return v


def _case_reference(case):
    """Per candidate (lnl, dexch, dlogt, d2logt) from the reference; kept on the case so that every path shares it."""
    if "ref" not in case:
        ref = []
        for c in range(len(case["cl"])):
            l = int(case["cl"][c])
            sl = slice(int(case["off"][l]), int(case["off"][l + 1]))
            w = None if case.get("weights") is None else case["weights"][sl]
            ref.append(_reference(case["parent"], _effective_blen(case, c), case["leaf"], np.asarray(case["pi"]).reshape(-1, 4)[l],
                                  case["ce"][c], case["st"][:, sl], w, case.get("branches"), case.get("want_dexch", True)))
        case["ref"] = ref
    return case["ref"]


def _errors(case, out):
    """The module docstring's error measures, the largest over the candidates; and whether everything was finite."""
    ref = _case_reference(case)
    br = case.get("branches")
    if br is None:
        br = np.flatnonzero(np.asarray(case["parent"]) >= 0)
    br = np.asarray(br, int)
    errs = {k: 0.0 for k in out}
    finite = all(bool(np.isfinite(v).all()) for v in out.values())
    for c, (lnl, dex, g, h) in enumerate(ref):
        errs["lnl"] = max(errs["lnl"], abs(out["lnl"][c] - lnl) / max(1.0, abs(lnl)))
        if "dlogt" not in out:
            continue
        if dex is not None:
            errs["dexch"] = max(errs["dexch"], np.abs(out["dexch"][c] - dex).max() / max(1.0, np.abs(dex).max()))
        else:
            errs.pop("dexch", None)
        errs["dlogt"] = max(errs["dlogt"], np.abs(out["dlogt"][c, br] - g[br]).max() / max(1.0, np.abs(g[br]).max()))
        errs["d2logt"] = max(errs["d2logt"], np.abs(out["d2logt"][c, br] - h[br]).max() / max(1.0, np.abs(h[br]).max()))
        if case.get("branches") is None:
            s = math.fsum(g[br])
            errs["sum_dlogt"] = max(errs["sum_dlogt"], abs(out["sum_dlogt"][c] - s) / max(1.0, abs(s)))
        else:
            errs.pop("sum_dlogt", None)
    if not finite:
        errs = {k: (v if np.isfinite(v) else math.inf) for k, v in errs.items()}
    return finite, errs


def _check(name, path, case, out, fails, bound_paths=None, cls="ordinary"):
    """Print the figures of one (case, path), then note every bound they miss in `fails` (asserted by the caller once all
    paths of the case are printed).  bound_paths: the kernels that may have run, when the test cannot choose (the largest
    of their bounds holds)."""
    finite, errs = _errors(case, out)
    print("stage1 %-28s %-11s %s%s" % (name, path, " ".join("%s=%.2e" % (k, errs[k]) for k in OUTPUTS if k in errs),
                                      "" if finite else " NON-FINITE"))
    if not finite:
        fails.append((name, path, "non-finite"))
    for k, v in errs.items():
        bound = max(BOUNDS[cls][p][k] for p in (bound_paths or (path,)))
        if not v <= bound:
            fails.append((name, path, k, float("%.3g" % v), bound))
    return errs


def _bits_differ(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a if k in b)


def _value_kernels_differ(engine, monkeypatch, case):
    """TPHIP_VALUE_EIGENBASIS=1 reaches another kernel than TPHIP_VALUE_COLS=2: over eight rescaled copies of the case's branch
    lengths the two values differ in bits (one candidate's two values may agree by chance)."""
    many = dict(case, vecs=case["vecs"][:1], cl=np.zeros(8, int), ce=np.tile(case["ce"][0], (8, 1)), cand_vec=np.zeros(8, int),
                cand_scale=np.linspace(0.6, 1.3, 8), cand_pidx=np.full(8, -1), cand_pfac=np.ones(8))
    return _bits_differ(_run(engine, monkeypatch, "value_c2", many), _run(engine, monkeypatch, "value_eigen", many))


def _simple_case(spec, st, blen, pi, exch, weights=None, branches=None, want_dexch=True):
    parent, leaf = _arrays(spec) if not isinstance(spec, tuple) else spec
    blen = np.asarray(blen, np.float64).copy()
    blen[parent < 0] = 0.0
    st = np.ascontiguousarray(st, dtype=np.uint8)
    return dict(ntaxa=int((leaf >= 0).sum()), parent=parent, leaf=leaf, blen=blen, off=np.array([0, st.shape[1]]), pi=[pi], st=st,
                vecs=blen[None, :], cl=np.array([0]), ce=np.asarray(exch, np.float64)[None, :], weights=weights, branches=branches,
                want_dexch=want_dexch)


def _pool(ntaxa, rng, n):
    """n columns: those of _columns() (constant, all-different, every IUPAC mask, gaps) with fresh random tails, zero bytes
    (read as gaps) and columns of random masks 0..15."""
    parts = [_columns(ntaxa, rng) for _ in range(3)]
    rnd = rng.choice(np.array([1, 2, 4, 8], np.uint8), (ntaxa, n))
    amb = rng.random(rnd.shape) < 0.1
    rnd[amb] = rng.integers(0, 16, int(amb.sum())).astype(np.uint8)
    st = np.concatenate(parts + [rnd], axis=1)[:, :n]
    st[1, 3] = 0
    st[ntaxa - 1, 4::29] = 0
    return np.ascontiguousarray(st)


# ---- column tiling ---------------------------------------------------------------------------------------------------

TILING_TREES = [("caterpillar9", lambda: _caterpillar(9)), ("balanced8", lambda: _balanced(list(range(8))))]
_TILING = {}


def _tiling_case(tname, spec, weighted):
    """Ragged loci of 0, 1, 17, 65, 129 and 257 columns in one plan (the value kernel's slice is 128 threads x C columns, a
    row of the gradient kernel's lane reduction 16 lanes, the wave 64), one candidate per locus, and a seventh candidate
    on the 65-column locus expressed through cand_vec / cand_scale / cand_pidx / cand_pfac.  The loci draw their columns
    from one pool of 257, so the reference sees each distinct column once."""
    if (tname, weighted) in _TILING:
        return _TILING[tname, weighted]
    rng = np.random.default_rng(len(tname))
    parent, leaf = _arrays(spec())
    nn, ntaxa = len(parent), int((leaf >= 0).sum())
    blen = np.exp(rng.uniform(np.log(0.01), np.log(1.0), nn))
    blen[parent < 0] = 0.0
    sizes = [0, 1, 17, 65, 129, 257]
    pool = _pool(ntaxa, rng, 257)
    st = np.concatenate([np.roll(pool, -37 * l, axis=1)[:, :n] for l, n in enumerate(sizes)], axis=1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    base = blen / 0.7
    base[5] /= 1.25
    case = dict(ntaxa=ntaxa, parent=parent, leaf=leaf, blen=blen, off=off, pi=[PI] * 6, st=np.ascontiguousarray(st),
                vecs=np.stack([blen, base]), cl=np.array([0, 1, 2, 3, 4, 5, 3]), ce=np.tile(EXCH, (7, 1)),
                cand_vec=np.array([0] * 6 + [1]), cand_scale=np.array([1.0] * 6 + [0.7]), cand_pidx=np.array([-1] * 6 + [5]),
                cand_pfac=np.array([1.0] * 6 + [1.25]),
                weights=(1.0 + np.arange(int(off[-1])) % 4) if weighted else None)
    _TILING[tname, weighted] = case
    return case


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weights1to4"])
@pytest.mark.parametrize("tname,spec", TILING_TREES, ids=[t[0] for t in TILING_TREES])
def test_column_tiling_edges(monkeypatch, tname, spec, weighted):
    engine = _engine()
    case = _tiling_case(tname, spec, weighted)
    fails, outs = [], {}
    for path in ALL_PATHS:
        outs[path] = _run(engine, monkeypatch, path, case)
        _check("tiling-%s-%s" % (tname, "w" if weighted else "u"), path, case, outs[path], fails)
    # which kernel ran: the eigenbasis value differs in bits from the transition-matrix one, the two gradient kernels differ
    assert _bits_differ(outs["value_eigen"], outs["value_c2"]) and _bits_differ(outs["grad2"], outs["grad"])
    for o in outs.values():      # the empty locus; the shared-vector candidate against the explicit vector's reference
        assert o["lnl"][0] == 0.0
    g = outs["grad2"]
    assert np.all(g["dexch"][0] == 0.0) and np.all(g["dlogt"][0] == 0.0) and np.all(g["d2logt"][0] == 0.0)
    assert not fails, fails


# ---- branch-length and rate domain -----------------------------------------------------------------------------------

_K = np.arange(6.0)
DOMAIN = [  # (name, pi, exch)
    ("random", PI, np.exp(np.random.default_rng(2).normal(0, 0.5, 6))),
    ("all_ones", PI, np.ones(6)),                                   # three equal eigenvalues under equal pi; F_kk limit
    ("all_ones_equal_pi", np.full(4, 0.25), np.ones(6)),
    ("near_equal_1e-7", np.full(4, 0.25), 1.0 + 1e-7 * _K),          # (lam_k - lam_l) t around the 1e-8 switch of expm1(x)/x
    ("near_equal_1e-4", np.full(4, 0.25), 1.0 + 1e-4 * _K),
    ("bounds_mixed", PI, np.array([1e-3, 1e3, 0.5, 20.0, 100.0, 3e-2])),
    ("rate_bounds", PI, np.array([math.exp(-7.0), 1.0, math.exp(9.2), 1.0, math.exp(-7.0), 3.0])),
    ("absent_base", np.array([0.3, 0.4, 0.3, 0.0]), np.array([1.0, 2.0, 0.5, 1.5, 3.0, 1.0])),
]


@pytest.mark.parametrize("mname,pi,exch", DOMAIN, ids=[m[0] for m in DOMAIN])
def test_branch_length_and_rate_domain(monkeypatch, mname, pi, exch):
    """8-taxon balanced tree, 40 columns, branch lengths log-uniform in [1e-3, 2] with one at 4.0 and one at e^4 (the
    optimiser's upper bound).  Near-equal rates 1 + 1e-7 k put (lam_k - lam_l) t between 2e-11 and 7e-6, on both sides of the
    1e-8 switch of grad2_ef_kernel's expm1(x) / x; 1 + 1e-4 k keeps it above."""
    engine = _engine()
    rng = np.random.default_rng(77)
    spec = _balanced(list(range(8)))
    parent, leaf = _arrays(spec)
    blen = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), len(parent)))
    blen[3], blen[9] = 4.0, math.exp(4.0)
    st = np.concatenate([_columns(8, rng), rng.choice(np.array([1, 2, 4, 8, 15, 5], np.uint8), (8, 10))], axis=1)
    for b in np.flatnonzero(np.asarray(pi) == 0.0):     # an absent base is nobody's only state (its frequency is 0)
        st[st == 1 << b] = 1 if b else 2
    cls = "extreme" if np.max(exch) / np.min(exch) >= 1e6 else "ordinary"
    case = _simple_case(spec, st, blen, pi, exch)
    fails, outs = [], {}
    for path in ALL_PATHS:
        outs[path] = _run(engine, monkeypatch, path, case)
        _check("domain-%s" % mname, path, case, outs[path], fails, cls=cls)
    assert _bits_differ(outs["grad2"], outs["grad"]) and _value_kernels_differ(engine, monkeypatch, case)
    assert not fails, fails


# ---- stack depth and rescaling ---------------------------------------------------------------------------------------

def _depths(parent):
    d = np.zeros(len(parent), int)
    for n in range(len(parent) - 2, -1, -1):
        d[n] = d[parent[n]] + 1
    return d


def _sample_branches(parent, leaf):
    """About 8 branches: the deepest tip, a child of the root, and six spread over the node order."""
    d = _depths(parent)
    tips = np.flatnonzero(leaf >= 0)
    root_kid = int(np.flatnonzero(parent == len(parent) - 1)[0])
    picks = {int(tips[d[tips].argmax()]), root_kid}
    picks.update(int(x) for x in np.linspace(0, len(parent) - 2, 6).astype(int))
    return sorted(picks)


@pytest.mark.parametrize("ntips", [64, 128])
def test_register_stack_depth_and_fallback(monkeypatch, ntips):
    """Balanced 64 tips: all five register slots of locus_value_kernel / locus_grad2_kernel and six parked adjoints (every
    branch checked).  Balanced 128 tips: deeper than the register stack, so the plan falls back to locus_loglik_kernel and
    locus_grad_kernel whatever is asked for (the default value is the eigenbasis value bit for bit); eight sampled branches."""
    engine = _engine()
    rng = np.random.default_rng(ntips)
    spec = _balanced(list(range(ntips)))
    parent, leaf = _arrays(spec)
    blen = np.exp(rng.uniform(np.log(0.01), np.log(0.5), len(parent)))
    st = _pool(ntips, rng, 24)
    fails = []
    if ntips == 64:
        case = _simple_case(spec, st, blen, PI, EXCH)
        outs = {}
        for path in ALL_PATHS:
            outs[path] = _run(engine, monkeypatch, path, case)
            _check("balanced64", path, case, outs[path], fails)
        assert _value_kernels_differ(engine, monkeypatch, case) and _bits_differ(outs["grad2"], outs["grad"])
    else:
        case = _simple_case(spec, st, blen, PI, EXCH, branches=_sample_branches(parent, leaf))
        eig = _run(engine, monkeypatch, "value_eigen", case)
        _check("balanced128", "value_eigen", case, eig, fails)
        for asked in ("value_c1", "value_c2"):
            assert np.array_equal(_run(engine, monkeypatch, asked, case)["lnl"], eig["lnl"]), asked
        for cache in (False, True):
            _check("balanced128-cache%d" % cache, "grad", case, _run(engine, monkeypatch, "grad", case, cache=cache), fails)
    assert not fails, fails


def test_rescaled_partials_on_300_taxa(monkeypatch):
    """A 300-taxon pure-birth tree (synth.yule_tree) with branch lengths in [0.05, 1] and 24 random columns: every column's
    likelihood is below 1e-200, so partials cross kLikRescaleBelow = 1e-100 on the way up; the reference does not rescale.
    Values and eight sampled branch derivatives only (the reference takes about 3 s on one CPU core for these; the six rate
    derivatives would take 20 s more).  Which kernels a random 300-taxon tree gets is the plan's choice (its stack depth
    decides), so the largest bound of the kernels that may have run holds."""
    engine = _engine()
    from tapir_amd import synth
    root, names = synth.yule_tree(300, 12)
    pin = synth.plan_inputs(root, names)
    parent, leaf = np.asarray(pin["parent"], np.int32), np.asarray(pin["leaf"], np.int32)
    rng = np.random.default_rng(300)
    blen = np.exp(rng.uniform(np.log(0.05), np.log(1.0), len(parent)))
    st = rng.choice(np.array([1, 2, 4, 8], np.uint8), (300, 24))
    case = _simple_case((parent, leaf), st, blen, PI, EXCH, branches=_sample_branches(parent, leaf), want_dexch=False)
    ref = _case_reference(case)
    assert ref[0][0] / 24 < math.log(1e-200)
    fails = []
    a = _run(engine, monkeypatch, "value_c2", case)
    _check("yule300", "value_c2", case, a, fails, bound_paths=("value_c2", "value_eigen"))
    b = _run(engine, monkeypatch, "value_eigen", case)
    _check("yule300", "value_eigen", case, b, fails)
    print("stage1 yule300: transition-matrix value kernel %s" % ("ran" if _bits_differ(a, b) else "did not run (fallback)"))
    for cache in (True, False):
        _check("yule300-cache%d" % cache, "grad2" if cache else "grad", case, _run(engine, monkeypatch, "grad", case, cache=cache), fails,
               bound_paths=GRAD_PATHS if cache else None)
    assert not fails, fails


# ---- a polytomy and two taxa -----------------------------------------------------------------------------------------

def test_polytomy_and_two_taxa(monkeypatch):
    """((a,b),(c,d),(e,f),g): not binary, so the gradient is locus_grad_kernel's with or without the cache.  (a,b): the
    smallest tree; lnL also against the closed form sum_c w_c log(pi_i expm(Q (t_a + t_b))_ij)."""
    engine = _engine()
    rng = np.random.default_rng(21)
    fails = []
    spec = [[0, 1], [2, 3], [4, 5], 6]
    parent, leaf = _arrays(spec)
    blen = np.exp(rng.uniform(np.log(0.02), np.log(1.5), len(parent)))
    case = _simple_case(spec, _pool(7, rng, 97), blen, PI, EXCH)
    for path in VALUE_PATHS:
        _check("polytomy", path, case, _run(engine, monkeypatch, path, case), fails)
    a = _run(engine, monkeypatch, "grad", case, cache=True)
    b = _run(engine, monkeypatch, "grad", case, cache=False)
    _check("polytomy-cache1", "grad", case, a, fails)
    _check("polytomy-cache0", "grad", case, b, fails)
    for k in a:    # one kernel both times
        assert np.max(np.abs(a[k] - b[k])) <= 1e-12 * max(1.0, np.abs(b[k]).max()), k
    # two taxa
    spec = [0, 1]
    ta, tb = 0.3, 0.045
    st = np.array([[1, 2, 4, 8, 1, 8, 2, 4], [1, 2, 8, 8, 4, 2, 2, 1]], np.uint8)
    w = np.array([3.0, 1.0, 2.0, 1.0, 1.0, 4.0, 2.0, 1.0])
    case = _simple_case(spec, st, [ta, tb, 0.0], PI, EXCH, weights=w)
    with mpmath.workdps(hp.DPS):
        Q, pim, _ = hp.rate_matrix(PI, EXCH)
        P = mpmath.expm(Q * (mpmath.mpf(ta) + mpmath.mpf(tb)), method="taylor")
        idx = {1: 0, 2: 1, 4: 2, 8: 3}
        closed = float(mpmath.fsum(w[c] * mpmath.log(pim[idx[st[0, c]]] * P[idx[st[0, c]], idx[st[1, c]]]) for c in range(st.shape[1])))
    assert abs(_case_reference(case)[0][0] - closed) <= 1e-15 * abs(closed)
    for path in ALL_PATHS:
        out = _run(engine, monkeypatch, path, case)
        _check("two-taxa", path, case, out, fails)
        if not abs(out["lnl"][0] - closed) <= BOUNDS["ordinary"][path]["lnl"] * max(1.0, abs(closed)):
            fails.append(("two-taxa closed form", path, out["lnl"][0], closed))
    assert not fails, fails


# ---- branches at the optimiser's lower bound -------------------------------------------------------------------------

TINY_T = [("e-23", math.exp(-23.0)), ("1e-9", 1e-9), ("1e-8", 1e-8), ("1e-6", 1e-6)]
# the (path, t) that miss the bounds on the MI355X, measured; everything else is a plain assert
TINY_KNOWN = {(path, tname) for path in ALL_PATHS for tname in ("e-23", "1e-9", "1e-8", "1e-6")}
TINY_REASON = ("known: P_b is formed as U e^{Lambda t} U^-1 (lik_pmat_kernel) or applied as U (e^{Lambda t} o U^-1 v) (the eigenbasis "
               "kernels), which cancels in fp64 for t << 1: a change probability of size q t carries the 1e-16 rounding of terms of "
               "size 1, and columns whose tips differ across such a branch lose those digits (DESIGN.md section 9)")
_TINY = {}


def _tiny_case(t):
    """Balanced 8 taxa; both branches of the cherry (0, 1), whose tips differ in most columns, and the internal branch above
    (2, 3), next to conflicting states, at t: the `nearly impossible columns` of DESIGN.md section 9."""
    if t not in _TINY:
        rng = np.random.default_rng(5)
        spec = _balanced(list(range(8)))
        parent, leaf = _arrays(spec)
        blen = np.exp(rng.uniform(np.log(0.02), np.log(0.5), len(parent)))
        blen[0] = blen[1] = blen[5] = t        # nodes 0, 1: tips 0 and 1; node 5: the parent of tips 2 and 3
        st = np.concatenate([_columns(8, rng), rng.choice(np.array([1, 2, 4, 8], np.uint8), (8, 10))], axis=1)
        assert (st[0] != st[1]).sum() >= 10
        _TINY[t] = _simple_case(spec, st, blen, PI, EXCH)
    return _TINY[t]


def _tiny_params():
    for path in ALL_PATHS:
        for tname, t in TINY_T:
            marks = [pytest.mark.xfail(strict=True, reason=TINY_REASON)] if (path, tname) in TINY_KNOWN else []
            yield pytest.param(path, tname, t, marks=marks, id="%s-t%s" % (path, tname))


@pytest.mark.parametrize("path,tname,t", list(_tiny_params()))
def test_branches_at_the_lower_bound(monkeypatch, path, tname, t):
    """Every path under the bounds of everything else with three branches at t = e^-23 (kLogBlenMin, where conserved loci
    end), 1e-9, 1e-8 and 1e-6.  One line per (path, t) makes the error table."""
    engine = _engine()
    case = _tiny_case(t)
    fails = []
    _check("tiny-t%s" % tname, path, case, _run(engine, monkeypatch, path, case), fails)
    assert not fails, fails


# ---- the fitted point ------------------------------------------------------------------------------------------------

def test_fitted_point_is_an_optimum_of_the_reference():
    """plan.stage1_fit on 2 loci x 60 columns x 6 taxa: at the general model's returned point the reference lnL is the
    engine's, and the REFERENCE gradient in (log r over the five free rates, log t) vanishes on every coordinate not at a
    bound, by the rule test_gpu_stage1.test_stage1_fullsize_properties applies to the kernel's own gradient
    (< 2e-6 max|lnL|; branches <= 2e-10 excluded); the likelihood sees only the sum of the two branches below the root."""
    engine = _engine()
    from tapir_amd import synth
    L, n, nt = 2, 60, 6
    d = synth.simulate(L, n, nt, 19, rate_mean=0.01)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    pi = np.asarray(d["pi"])
    parent, leaf = np.asarray(pin["parent"]), np.asarray(pin["leaf"])
    plan = engine.Plan(nt, parent, pin["blen"], leaf, d["locus_offsets"], pi, np.ones((L, 6)), pin["T"], [1], [[0, 1]],
                       correction=pin["correction"])
    fit = plan.stage1_fit(st)
    plan.close()
    root_kids = np.flatnonzero(parent == len(parent) - 1)
    assert len(root_kids) == 2
    bound = max(BOUNDS["ordinary"][p]["lnl"] for p in ALL_PATHS)
    refs = []
    for l in range(L):
        exch, blen = fit["model_exch"][l, 0], fit["grm_blen"][l]
        refs.append(_reference(parent, blen, leaf, pi[l], exch, st[:, l * n:(l + 1) * n], None))
    scale = max(abs(r[0]) for r in refs)
    for l, (lnl, dex, g, h) in enumerate(refs):
        exch, blen = fit["model_exch"][l, 0], fit["grm_blen"][l]
        err = abs(fit["lnl"][l, 0] - lnl) / max(1.0, abs(lnl))
        free_r = [q for q in (0, 2, 3, 4, 5) if -7.0 + 1e-6 < math.log(exch[q]) < 9.2 - 1e-6]
        grad = [dex[q] * exch[q] for q in free_r]
        for b in np.flatnonzero(parent >= 0):
            if b in root_kids or not 2e-10 < blen[b] < math.exp(4.0) * (1 - 1e-9):
                continue
            grad.append(g[b])
        s = blen[root_kids].sum()
        if 2e-10 < s < math.exp(4.0) * (1 - 1e-9):
            k = root_kids[np.argmax(blen[root_kids])]
            grad.append(g[k] * s / blen[k])          # d lnL / d log (t_1 + t_2)
        worst = np.abs(grad).max()
        print("stage1 fitted locus %d: |d lnL| %.2e, largest free reference gradient %.2e of %d (limit %.2e)"
              % (l, err, worst, len(grad), 2e-6 * scale))
        assert err <= bound, (l, err)
        assert exch[1] == 1.0 and len(grad) >= 8
        assert worst < 2e-6 * scale, (l, worst)

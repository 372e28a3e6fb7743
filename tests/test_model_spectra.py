"""The GTR eigen-system of stage 2 (gtr_setup_kernel, restated in tests/gtr_setup_emulation.py) on spectra the generic models
of the other tests never reach: exactly degenerate, nearly degenerate and nearly reducible ones.  No GPU is needed; the GPU
twin is tests/test_gpu_model_spectra.py, which takes SPECTRA from here.

The kernel puts the exact stationary pair (lam = 0, U[:, 0] = 1, Ui[0] = pi) beside three vectors of a Jacobi iteration.
Where a second eigenvalue comes near 0 (Q nearly reducible) Jacobi's stationary vector and its neighbour are each rotated
towards the other by about eps |S| / |lam_1|; replacing one of the pair and keeping the other leaves that much of sqrt(pi) in
the kept vector, and P(t) = 1 pi + U e^(Lambda t) U^-1 loses it on the entries across the blocks.  The kernel therefore removes
the component along sqrt(pi) from the kept vectors and re-orthonormalises them (leaving alone what is within 8 eps of its
own rounding scale, so that a well separated model keeps its bits); keep="jacobi" of the emulation is the form
before that, and the tests show that it, and not the emulation's other arithmetic, misses the bounds.

Structure (a condition, not a measurement: a projection leaves a few eps of the norm, the sums have four terms), k = 1..3:
  |sum_j Ui[k][j]| <= 16 eps sum_j |Ui[k][j]|      and      |sum_i pi_i U[i][k]| <= 16 eps sum_i pi_i |U[i][k]|
P(t), t in T_GRID: the largest relative error over the 16 entries against the 40-digit eigen-solver of hp_reference, held to
max(3e-13, 10 x the same figure of the CPU oracle's eigen-system), which keeps all four Jacobi vectors as a consistent set.
3e-13 is the product's bound on f for GTR (test_gpu_numerics.BOUNDS); 10 is the project's margin between a record and a bound.
Seen here, the largest error / bound over T_GRID per nearly reducible spectrum, kept vectors as Jacobi left them -> projected,
and the larger of the two structure sums in eps:
  blocks_1e-2   0.39 -> 0.39    1.5 -> 1.5        (inside either way, and below the 8 eps from which the kernel projects)
  blocks_e-7    2.1  -> 0.18    45  -> 1.3
  blocks_1e-4   31   -> 0.16    1.2e3 -> 0.6
  blocks_1e-6   110  -> 0.16    1.1e4 -> 0.6
  blocks_ac_gt  47   -> 0.38    4.7e2 -> 0.8
  cut_off_t     16   -> 0.23    4.6e2 -> 1.3
"""
import math

import mpmath
import numpy as np
import pytest

import gtr_setup_emulation as emu
import hp_reference as hp

EPS = 2.0 ** -52
PI4 = [0.25, 0.25, 0.25, 0.25]
PI = [0.1, 0.2, 0.3, 0.4]
E7 = math.exp(-7.0)          # where stage 1 parks a class rate the data never show
SCALE = np.array([0.5, 1.3, 2.0, 0.8, 0.7, 1.6])      # unequal factors in [.5, 2], one per exchangeability


def _blocks(ratio, within):
    """Two blocks of bases: the two exchangeabilities `within` of order 1, the four across at `ratio`, each times SCALE."""
    e = np.full(6, ratio)
    e[list(within)] = 1.0
    return (e * SCALE).tolist()


# name -> (pi, exchangeabilities AC AG AT CG CT GT); all are GTR plans
DEGENERATE = {
    "jc": (PI4, [1.0] * 6),
    "f81_as_gtr": (PI, [1.0] * 6),                                  # a triple eigenvalue
    "k80": (PI4, [1.0, 4.0, 1.0, 1.0, 4.0, 1.0]),
    "hky": (PI, [1.0, 4.0, 1.0, 1.0, 4.0, 1.0]),                    # a double eigenvalue
    "tn93": (PI, [1.0, 4.0, 1.0, 1.0, 2.5, 1.0]),
}
NEARLY_DEGENERATE = {
    "hky_ac_2^-40": (PI, [1.0 + 2.0 ** -40, 4.0, 1.0, 1.0, 4.0, 1.0]),
    "hky_cg_1e-9": (PI, [1.0, 4.0, 1.0, 1.0 + 1e-9, 4.0, 1.0]),
    "f81_at_2^-40": (PI, [1.0, 1.0, 1.0 + 2.0 ** -40, 1.0, 1.0, 1.0]),
    "f81_ct_1e-9": (PI, [1.0, 1.0, 1.0, 1.0, 1.0 + 1e-9, 1.0]),
}
NEARLY_REDUCIBLE = {
    "blocks_1e-2": (PI, _blocks(1e-2, (1, 4))),                     # {A,G} | {C,T}
    "blocks_e-7": (PI, _blocks(E7, (1, 4))),
    "blocks_1e-4": (PI, _blocks(1e-4, (1, 4))),
    "blocks_1e-6": (PI, _blocks(1e-6, (1, 4))),                     # the edge: smaller ratios are stage 1's "extreme" class
    "blocks_ac_gt": (PI, _blocks(E7, (0, 5))),                      # {A,C} | {G,T}
    "cut_off_t": (PI, (np.array([1.0, 1.0, 1e-4, 1.0, 1e-4, 1e-4]) * SCALE).tolist()),   # T nearly cut off
}
SPECTRA = {**DEGENERATE, **NEARLY_DEGENERATE, **NEARLY_REDUCIBLE}
# where the second eigenvalue is within e^-7 of the others: eps / |lam_1| is beyond 16 eps there
BROKEN_BEFORE = [n for n in NEARLY_REDUCIBLE if n != "blocks_1e-2"]
T_GRID = (1e-3, 1e-2, 0.1, 1.0, 10.0)
P_FLOOR = 3e-13


def structure_sums(U, Ui, pi):
    """The two sums of the module docstring for k = 1..3, each over its own scale, in units of eps: [3] and [3].
    U [4, 3], Ui [3, 4]: the kept slots only."""
    rows = np.array([abs(math.fsum(Ui[k])) / math.fsum(np.abs(Ui[k])) for k in range(3)])
    cols = np.array([abs(math.fsum(pi * U[:, k])) / math.fsum(pi * np.abs(U[:, k])) for k in range(3)])
    return rows / EPS, cols / EPS


def _relative_error(P, ref):
    return float(max(abs((mpmath.mpf(float(P[i, j])) - ref[i, j]) / ref[i, j]) for i in range(4) for j in range(4)))


_FIGURES = {}


def _figures(oracle, name):
    """Per spectrum, once: the structure sums of both forms, and per t the error of both forms and of the oracle's."""
    if name not in _FIGURES:
        pi, exch = SPECTRA[name]
        ref = hp._Model(pi, exch, "gtr")
        olam, oU, oUi, _ = oracle.gtr_eigen(np.array(pi), np.array(exch))
        models = {keep: emu.gtr_setup(pi, exch, keep) for keep in emu.KEEP}
        err = {keep: [] for keep in emu.KEEP + ("oracle",)}
        with mpmath.workdps(hp.DPS):
            for t in T_GRID:
                P = ref.matrices(mpmath.mpf(t), derivs=False)[0]
                for keep in emu.KEEP:
                    err[keep].append(_relative_error(emu.transition(models[keep], t), P))
                err["oracle"].append(_relative_error((oU * np.exp(olam * t)[None, :]) @ oUi, P))
        err = {k: np.array(v) for k, v in err.items()}
        bound = np.maximum(P_FLOOR, 10.0 * err["oracle"])
        sums = {keep: np.concatenate(structure_sums(m.U, m.Ui, m.pi)).max() for keep, m in models.items()}
        print("spectrum %s lam %s: error / bound per t  jacobi %s ; projected %s   structure sums (eps) %.3g -> %.3g" % (
            name, models["projected"].lam, " ".join("%.2g" % v for v in err["jacobi"] / bound),
            " ".join("%.2g" % v for v in err["projected"] / bound), sums["jacobi"], sums["projected"]))
        _FIGURES[name] = dict(models=models, err=err, bound=bound, sums=sums)
    return _FIGURES[name]


@pytest.mark.parametrize("name", list(SPECTRA))
def test_projected_system_on_every_spectrum(oracle, name):
    """The kernel's form: the layout's promises, both structure sums within 16 eps, U Ui = I - 1 pi, and P(t) within the
    bound of the module docstring at every t."""
    r = _figures(oracle, name)
    m = r["models"]["projected"]
    assert np.all(m.lam < 0) and abs(m.pi.sum() - 1.0) <= 2 * EPS
    assert r["sums"]["projected"] <= 16.0
    full = np.ones((4, 1)) * m.pi[None, :] + m.U @ m.Ui
    assert np.abs(full - np.eye(4)).max() <= 64 * EPS * (1.0 / np.sqrt(m.pi.min()))    # |U| |Ui| <= sqrt(1 / min pi)
    assert np.all(r["err"]["projected"] <= r["bound"]), (r["err"]["projected"], r["bound"])


@pytest.mark.parametrize("name", BROKEN_BEFORE)
def test_unprojected_vectors_are_the_cause(oracle, name):
    """With the kept vectors as Jacobi left them, and everything else the same, both structure sums exceed 16 eps and P(t)
    misses its bound, on every nearly reducible spectrum from e^-7 on."""
    r = _figures(oracle, name)
    assert r["sums"]["jacobi"] > 16.0
    assert np.any(r["err"]["jacobi"] > r["bound"]), (r["err"]["jacobi"], r["bound"])
    assert np.all(r["err"]["projected"] <= r["bound"])


def test_random_block_models(oracle):
    """pi from Dirichlet(5), transitions in [.3, 3], the four transversions near 1e-3 and near 1e-5 (each times a factor in
    [.5, 2]): the structure sums of the projected form stay within 16 eps, and P(0.1) within the bound."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for ratio in (1e-3, 1e-5):
        for _ in range(8):
            pi = rng.dirichlet([5.0] * 4)
            exch = ratio * rng.uniform(0.5, 2.0, 6)
            exch[[1, 4]] = rng.uniform(0.3, 3.0, 2)
            m = emu.gtr_setup(pi, exch)
            rows, cols = structure_sums(m.U, m.Ui, m.pi)
            assert max(rows.max(), cols.max()) <= 16.0
            olam, oU, oUi, _ = oracle.gtr_eigen(pi, exch)
            with mpmath.workdps(hp.DPS):
                P = hp._Model(pi, exch, "gtr").matrices(mpmath.mpf(0.1), derivs=False)[0]
                bound = max(P_FLOOR, 10.0 * _relative_error((oU * np.exp(olam * 0.1)[None, :]) @ oUi, P))
                err = _relative_error(emu.transition(m, 0.1), P)
            worst = max(worst, err / bound)
            assert err <= bound, (ratio, pi, exch, err, bound)
    print("random block models: largest error / bound %.3g" % worst)

"""The persistent mode's order of handing out a share's columns (slow columns first among the last 128 entries of every
segment, TPHIP_SITE_TAIL_ORDER) changes how many evaluation rounds the waves issue and nothing else."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("TPHIP_SITE_PERSISTENT", "TPHIP_SITE_MIXED", "TPHIP_SITE_WAVES", "TPHIP_SITE_GRID_MULT", "TPHIP_SITE_FIRST_FRACTION",
         "TPHIP_SITE_CHUNK", "TPHIP_SITE_TAIL_ORDER")
KEYS = ("rate", "subst", "lnl", "flag", "nres", "tables")
SEED_64 = 5   # see test_tail_order_lowers_the_rounds


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _replay():
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import share_replay
    return share_replay


def _run(engine, monkeypatch, env, ntaxa, st, off, d, pin):
    """One fused run under the given launch settings: outputs, evaluation count, rounds."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], d["exch"], pin["T"], [10], [[5, 15]],
                       correction=pin["correction"])
    got = plan.run_fused(st)
    got["evals"] = plan.last_eval_count()
    got["rounds"] = plan.last_round_count()
    plan.close()
    return got


def _same(got, ref, what):
    for key in KEYS:
        assert got[key].tobytes() == ref[key].tobytes(), (what, key)
    assert got["evals"] == ref["evals"], what


@pytest.fixture(scope="module")
def batch64():
    return _replay().share_order_batch(6, 2500, 64, SEED_64)


@pytest.mark.parametrize("shape", [(6, 2500, 64, SEED_64), (7, 3001, 24, 77)])
def test_outputs_do_not_depend_on_the_order(monkeypatch, shape, batch64):
    """An empty locus, a locus without optimiser work and a locus with fewer optimiser columns than a wave has lanes, under
    5 / 16 / 37 resident waves and three splits of the grid, with the tail order and without: every output, the PI table and
    the evaluation count equal the default (small-batch) run's to the byte."""
    engine = _engine()
    nloci, ncols, ntaxa, seed = shape
    st, off, d, pin = batch64 if shape[2] == 64 else _replay().share_order_batch(nloci, ncols, ntaxa, seed)
    ref = _run(engine, monkeypatch, {}, ntaxa, st, off, d, pin)
    ok = ref["flag"] == 0
    assert ok.sum() > 4000
    assert off[3] == off[2] and not ok[off[0]:off[1]].any() and 0 < ok[off[4]:off[5]].sum() < 64
    for waves in ("5", "16", "37"):
        for mult, frac in (("3", "0.8"), ("7", "0.33"), ("2", "0.999")):
            env = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES=waves, TPHIP_SITE_GRID_MULT=mult, TPHIP_SITE_FIRST_FRACTION=frac)
            _same(_run(engine, monkeypatch, env, ntaxa, st, off, d, pin), ref, env)
            env["TPHIP_SITE_TAIL_ORDER"] = "0"
            _same(_run(engine, monkeypatch, env, ntaxa, st, off, d, pin), ref, env)


def test_tail_order_lowers_the_rounds(monkeypatch, batch64):
    """16 resident waves, grid x 3, 80 % in the first round, on the 64-taxon batch: the rounds summed over the launch are
    strictly fewer with the tail order than with TPHIP_SITE_TAIL_ORDER=0, for the same evaluations.

    The seed is chosen so that the CPU replay (tools/share_replay.py --seed 5, oracle evaluation counts of this very batch)
    predicts at least 3 % fewer rounds: 376 rounds in list order, 360 with the tail order (4.26 % fewer) for 16 634
    evaluations (seeds 1-6 predict 3.8-5.5 %).  Observed on MI355X: 376 and 360 rounds, 16 634 evaluations both."""
    engine = _engine()
    st, off, d, pin = batch64
    env = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES="16", TPHIP_SITE_GRID_MULT="3", TPHIP_SITE_FIRST_FRACTION="0.8")
    on = _run(engine, monkeypatch, env, 64, st, off, d, pin)
    off_run = _run(engine, monkeypatch, dict(env, TPHIP_SITE_TAIL_ORDER="0"), 64, st, off, d, pin)
    print("rounds with the tail order %d, without %d, evaluations %d / %d" % (on["rounds"], off_run["rounds"], on["evals"], off_run["evals"]))
    _same(on, off_run, "tail order on / off")
    assert on["evals"] > 0 and 64 * on["rounds"] >= on["evals"]
    assert on["rounds"] < off_run["rounds"]


def test_small_batch_modes_ignore_the_switch(monkeypatch):
    """The ragged 12-taxon batch of test_gpu_parity.test_mixed_loci_mode_is_bit_identical (300 loci of 0-200 columns; the
    default mode there is the mixed-loci one), in the mixed-loci and the slice mode: the switch reaches neither -- rounds
    and outputs are identical with and without it."""
    engine = _engine()
    from tapir_amd import synth
    ntaxa, nloci = 12, 300
    rng = np.random.default_rng(77 + ntaxa)
    d = synth.simulate(nloci, 200, ntaxa, 900 + ntaxa)
    pin = synth.plan_inputs(d["root"], d["names"])
    lens = rng.integers(0, 201, size=nloci)
    tiny = rng.random(nloci) < 0.3
    lens[tiny] = rng.integers(0, 4, size=int(tiny.sum()))
    off = np.zeros(nloci + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    st = np.ascontiguousarray(d["states"].numpy()[:, : int(off[-1])])
    for env in ({}, dict(TPHIP_SITE_MIXED="0", TPHIP_SITE_PERSISTENT="0")):
        a = _run(engine, monkeypatch, env, ntaxa, st, off, d, pin)
        b = _run(engine, monkeypatch, dict(env, TPHIP_SITE_TAIL_ORDER="0"), ntaxa, st, off, d, pin)
        _same(a, b, env)
        assert a["rounds"] == b["rounds"] and a["rounds"] > 0, env

"""The persistent mode's shares by predicted work (TPHIP_SITE_SHARE_WORK: a reserved tail of easy columns per locus, the first
round's shares of equal predicted work, the later shares of equal column counts over the tails) change how many evaluation
rounds the waves issue and nothing else: every case compares with the same plan under TPHIP_SITE_SHARE_WORK=0."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("TPHIP_SITE_PERSISTENT", "TPHIP_SITE_MIXED", "TPHIP_SITE_WAVES", "TPHIP_SITE_GRID_MULT", "TPHIP_SITE_FIRST_FRACTION",
         "TPHIP_SITE_CHUNK", "TPHIP_SITE_TAIL_ORDER", "TPHIP_SITE_SHARE_WORK", "TPHIP_SITE_RESERVE", "TPHIP_SITE_CLASS_WEIGHTS",
         "TPHIP_DEDUP")
KEYS = ("rate", "subst", "lnl", "flag", "nres", "tables")
SEED_64 = 5
# the hand-out under test, spelled out so that the cases do not move with the library's defaults
WORK = dict(TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0.25", TPHIP_SITE_CLASS_WEIGHTS="2.9,2.04")
BASE = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES="16", TPHIP_SITE_GRID_MULT="3", TPHIP_SITE_FIRST_FRACTION="0.8")


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


def _run(engine, monkeypatch, env, ntaxa, st, off, d, pin, model="gtr"):
    """One fused run under the given launch settings: outputs, evaluation count, rounds."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nl = len(off) - 1
    plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"][:nl], None if model == "f81" else d["exch"][:nl],
                       pin["T"], [10], [[5, 15]], correction=pin["correction"], model=model)
    got = plan.run_fused(st)
    got["evals"] = plan.last_eval_count()
    got["rounds"] = plan.last_round_count()
    plan.close()
    return got


def _same(got, ref, what):
    for key in KEYS:
        assert got[key].tobytes() == ref[key].tobytes(), (what, key)
    assert got["evals"] == ref["evals"], what


def _old(env):
    return dict(env, TPHIP_SITE_SHARE_WORK="0")


@pytest.fixture(scope="module")
def batch64():
    return _replay().share_order_batch(6, 2500, 64, SEED_64)


def _edge_batch(ntaxa, ncols, seed):
    """Five loci of `ncols` columns: [0] as simulated, [1] constant columns only (nothing for the optimiser), [2] marked
    columns only (an empty reserved tail), [3] marked columns and three unmarked ones (fewer than a reserve of 0.25 asks
    whole columns of: the tail stays empty), [4] as simulated.  Returns (states, offsets, d, pin, marked, optimised)."""
    from tapir_amd import synth
    rp = _replay()
    d = synth.simulate(5, ncols, ntaxa, seed)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy().copy()
    off = d["locus_offsets"].copy()
    optimised, slow = rp.classify(st, pin["parent"], pin["leaf"])
    hard, easy = np.flatnonzero(slow), np.flatnonzero(optimised & ~slow)
    assert len(hard) >= 8 and len(easy) >= 8
    src = st.copy()
    st[:, off[1]:off[2]] = 1
    st[:, off[2]:off[3]] = src[:, np.resize(hard, ncols)]
    st[:, off[3]:off[4]] = src[:, np.resize(hard, ncols)]
    st[:, off[3] + 5:off[3] + 8] = src[:, easy[:3]]
    st = np.ascontiguousarray(st)
    optimised, slow = rp.classify(st, pin["parent"], pin["leaf"])
    return st, off, d, pin, slow, optimised


def test_base_case_bit_identical_and_rounds_as_replayed(monkeypatch, batch64):
    """6 loci x 2500 columns x 64 taxa (the batch of test_gpu_share_order), 16 resident waves, grid x 3: outputs, PI table and
    evaluation count equal the old hand-out's to the byte, and the rounds are what the CPU replay predicts from the oracle's
    evaluation counts of this very batch: `python tools/share_replay.py --seed 5 --reserve 0.25 --weights 2.9,2.04` prints
    360 rounds for the old hand-out (first fraction 0.8, tail order) and 336 for shares by predicted work, 16 634 evaluations."""
    engine = _engine()
    st, off, d, pin = batch64
    new = _run(engine, monkeypatch, dict(BASE, **WORK), 64, st, off, d, pin)
    old = _run(engine, monkeypatch, _old(BASE), 64, st, off, d, pin)
    print("rounds by predicted work %d, old hand-out %d, evaluations %d / %d" % (new["rounds"], old["rounds"], new["evals"], old["evals"]))
    _same(new, old, "share work on / off")
    assert new["evals"] == 16634
    assert old["rounds"] == 360
    assert new["rounds"] == 336


def test_edge_loci(monkeypatch):
    """A locus without optimiser work between working loci, a locus of marked columns only (empty reserved tail), a locus with
    fewer unmarked columns than the reserve takes a whole column of, under several grids, with and without the tail order:
    byte-equal to the old hand-out, and to the default (small-batch) run."""
    engine = _engine()
    st, off, d, pin, slow, optimised = _edge_batch(24, 700, 31)
    assert not optimised[off[1]:off[2]].any()
    assert optimised[off[2]:off[3]].all() and slow[off[2]:off[3]].all()
    assert (optimised & ~slow)[off[3]:off[4]].sum() == 3
    ref = _run(engine, monkeypatch, {}, 24, st, off, d, pin)
    for waves, mult in (("16", "3"), ("5", "7"), ("37", "2")):
        env = dict(BASE, TPHIP_SITE_WAVES=waves, TPHIP_SITE_GRID_MULT=mult, **WORK)
        _same(_run(engine, monkeypatch, env, 24, st, off, d, pin), ref, env)
        _same(_run(engine, monkeypatch, _old(env), 24, st, off, d, pin), ref, "old hand-out")
        env["TPHIP_SITE_TAIL_ORDER"] = "0"
        _same(_run(engine, monkeypatch, env, 24, st, off, d, pin), ref, env)
        env["TPHIP_SITE_RESERVE"] = "1.0"     # every unmarked column in the tails
        _same(_run(engine, monkeypatch, env, 24, st, off, d, pin), ref, env)


def test_single_locus_and_more_shares_than_columns(monkeypatch):
    """One locus; and 259 shares (37 waves x 7) for a work list of fewer columns than that, so that most shares are empty
    and leave at once."""
    engine = _engine()
    from tapir_amd import synth
    d = synth.simulate(1, 3000, 24, 11)
    pin = synth.plan_inputs(d["root"], d["names"])
    st, off = np.ascontiguousarray(d["states"].numpy()), d["locus_offsets"]
    ref = _run(engine, monkeypatch, {}, 24, st, off, d, pin)
    assert (ref["flag"] == 0).sum() > 1000
    env = dict(BASE, **WORK)
    _same(_run(engine, monkeypatch, env, 24, st, off, d, pin), ref, "single locus")
    # two loci of 90 columns
    d = synth.simulate(2, 90, 24, 12)
    pin = synth.plan_inputs(d["root"], d["names"])
    st, off = np.ascontiguousarray(d["states"].numpy()), d["locus_offsets"]
    ref = _run(engine, monkeypatch, {}, 24, st, off, d, pin)
    assert 0 < (ref["flag"] == 0).sum() < 180
    env = dict(BASE, TPHIP_SITE_WAVES="37", TPHIP_SITE_GRID_MULT="7", **WORK)
    got = _run(engine, monkeypatch, env, 24, st, off, d, pin)
    _same(got, ref, "more shares than columns")
    _same(_run(engine, monkeypatch, dict(env, TPHIP_SITE_RESERVE="0.9"), 24, st, off, d, pin), ref, "more shares than columns, reserve 0.9")


def test_reserve_zero_keeps_the_list(monkeypatch, batch64):
    """A reserved fraction of 0 leaves compact_kernel's list as it was, entry for entry.  The rounds depend on the order of
    the list, so they tell: with equal class weights and equal shares (grid x 1) the weighted boundaries are the old ones
    (floor(b W / N) / w = floor(b total / N) for W = w total), and the rounds must equal the old hand-out's; with the tail
    order off they depend on every entry's place."""
    engine = _engine()
    st, off, d, pin = batch64
    for tail in ("1", "0"):
        env = dict(BASE, TPHIP_SITE_WAVES="48", TPHIP_SITE_GRID_MULT="1", TPHIP_SITE_TAIL_ORDER=tail)
        env.pop("TPHIP_SITE_FIRST_FRACTION")
        new = _run(engine, monkeypatch, dict(env, TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0", TPHIP_SITE_CLASS_WEIGHTS="1,1"),
                   64, st, off, d, pin)
        old = _run(engine, monkeypatch, _old(env), 64, st, off, d, pin)
        _same(new, old, "reserve 0")
        assert new["rounds"] == old["rounds"] and new["rounds"] > 0, (tail, new["rounds"], old["rounds"])
    # grid x 3 with a reserve of 0: no later shares to take a tail, all 48 shares cut the list by predicted work
    env = dict(BASE, TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0")
    _same(_run(engine, monkeypatch, env, 64, st, off, d, pin), old, "reserve 0, grid x 3")


def test_16_taxa_and_f81(monkeypatch):
    """A 16-taxon batch (two packed words per column, the NW = 2 kernel) and an F81 plan, both forced into the persistent mode."""
    engine = _engine()
    st, off, d, pin = _replay().share_order_batch(6, 2500, 16, 21)
    ref = _run(engine, monkeypatch, {}, 16, st, off, d, pin)
    assert (ref["flag"] == 0).sum() > 3000
    env = dict(BASE, **WORK)
    new = _run(engine, monkeypatch, env, 16, st, off, d, pin)
    _same(new, ref, "16 taxa")
    _same(_run(engine, monkeypatch, _old(env), 16, st, off, d, pin), ref, "16 taxa, old hand-out")
    st, off, d, pin, _, _ = _edge_batch(24, 700, 31)
    ref = _run(engine, monkeypatch, {}, 24, st, off, d, pin, model="f81")
    _same(_run(engine, monkeypatch, env, 24, st, off, d, pin, model="f81"), ref, "F81")
    _same(_run(engine, monkeypatch, _old(env), 24, st, off, d, pin, model="f81"), ref, "F81, old hand-out")


def test_deduplication_on_and_off(monkeypatch):
    """De-duplication forced on (the work list holds one column per site pattern; dedup_resolve runs before compact_kernel):
    byte-equal to de-duplication off, under shares by predicted work and under the old hand-out."""
    engine = _engine()
    st, off, d, pin, _, _ = _edge_batch(24, 700, 31)
    st[:, off[4] + 100:off[4] + 400] = st[:, off[4]:off[4] + 300]    # repeated site patterns inside a locus
    st = np.ascontiguousarray(st)
    env = dict(BASE, **WORK)
    plain = _run(engine, monkeypatch, dict(env, TPHIP_DEDUP="0"), 24, st, off, d, pin)
    dedup = _run(engine, monkeypatch, dict(env, TPHIP_DEDUP="1"), 24, st, off, d, pin)
    for key in KEYS:
        assert dedup[key].tobytes() == plain[key].tobytes(), key
    assert 0 < dedup["evals"] < plain["evals"]
    _same(_run(engine, monkeypatch, _old(dict(env, TPHIP_DEDUP="1")), 24, st, off, d, pin), dedup, "de-duplication, old hand-out")

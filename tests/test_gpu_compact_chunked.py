"""The work list of long loci is built chunk-parallel (compact_count / compact_scan / compact_scatter kernels) instead of
by one workgroup per locus.  TPHIP_COMPACT_CHUNKED=0/1 forces either path on any shape; the list, its counts and class
counts and everything derived from them must be the same entry for entry, so every case compares the two paths to the
byte, and by the evaluation and round counts (the rounds follow the order of the list).

The batch is the one of tests/test_gpu_share_work.py (6 x 2500 x 64, with its empty, constant and nearly constant loci)
plus loci of 2049 (two chunks and one column), 1 and 0 columns, an all-constant locus and a locus in which every column
needs the optimiser, under that file's launch settings."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("TPHIP_SITE_PERSISTENT", "TPHIP_SITE_MIXED", "TPHIP_SITE_WAVES", "TPHIP_SITE_GRID_MULT", "TPHIP_SITE_FIRST_FRACTION",
         "TPHIP_SITE_CHUNK", "TPHIP_SITE_TAIL_ORDER", "TPHIP_SITE_SHARE_WORK", "TPHIP_SITE_RESERVE", "TPHIP_SITE_CLASS_WEIGHTS",
         "TPHIP_DEDUP", "TPHIP_COMPACT_CHUNKED")
KEYS = ("rate", "subst", "lnl", "flag", "nres", "tables")
BASE = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES="16", TPHIP_SITE_GRID_MULT="3", TPHIP_SITE_FIRST_FRACTION="0.8",
            TPHIP_SITE_CLASS_WEIGHTS="2.9,2.04")
NTAXA = 64


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


@pytest.fixture(scope="module")
def batch():
    rp = _replay()
    st, off, d, pin = rp.share_order_batch(6, 2500, NTAXA, 5)
    optimised, _ = rp.classify(st, pin["parent"], pin["leaf"])
    work = np.flatnonzero(optimised)
    assert len(work) > 2000
    extra = [st[:, off[5]:off[5] + 2049],                       # 2049 columns: two full chunks and one column
             st[:, work[7]:work[7] + 1],                        # one column
             st[:, :0],                                         # no column
             np.full((NTAXA, 1100), 1, dtype=st.dtype),         # constant columns only: nothing on the list
             st[:, np.resize(work, 1300)]]                      # every column needs the optimiser
    states = np.ascontiguousarray(np.concatenate([st] + extra, axis=1))
    offs = np.concatenate([off, off[-1] + np.cumsum([e.shape[1] for e in extra])]).astype(np.int64)
    pick = [1, 3, 5, 0, 1]
    pi = np.concatenate([d["pi"][:6], d["pi"][pick]])
    exch = np.concatenate([d["exch"][:6], d["exch"][pick]])
    optimised, _ = rp.classify(states, pin["parent"], pin["leaf"])
    assert not optimised[offs[9]:offs[10]].any() and optimised[offs[10]:offs[11]].all()
    assert offs[7] - offs[6] == 2049 and offs[8] - offs[7] == 1 and offs[9] == offs[8]
    return states, offs, pi, exch, pin


def _run(engine, monkeypatch, env, batch, ntaxa=NTAXA):
    states, offs, pi, exch, pin = batch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], offs, pi, exch, pin["T"], [10], [[5, 15]],
                       correction=pin["correction"])
    try:
        got = plan.run_fused(states)
        got["evals"] = plan.last_eval_count()
        got["rounds"] = plan.last_round_count()
    finally:
        plan.close()
    return got


@pytest.mark.parametrize("dedup", ["0", "1"])
@pytest.mark.parametrize("reserve", ["0", "0.15"])
@pytest.mark.parametrize("share_work", ["0", "1"])
def test_chunked_list_equals_one_workgroup_list(monkeypatch, batch, share_work, reserve, dedup):
    engine = _engine()
    env = dict(BASE, TPHIP_SITE_SHARE_WORK=share_work, TPHIP_SITE_RESERVE=reserve, TPHIP_DEDUP=dedup)
    old = _run(engine, monkeypatch, dict(env, TPHIP_COMPACT_CHUNKED="0"), batch)
    new = _run(engine, monkeypatch, dict(env, TPHIP_COMPACT_CHUNKED="1"), batch)
    print("share_work %s reserve %s dedup %s: evaluations %d / %d, rounds %d / %d" %
          (share_work, reserve, dedup, new["evals"], old["evals"], new["rounds"], old["rounds"]))
    assert (old["flag"] == 0).sum() > 2000 and old["evals"] > 0 and old["rounds"] > 0
    for key in KEYS:
        assert new[key].tobytes() == old[key].tobytes(), key
    assert new["evals"] == old["evals"]
    assert new["rounds"] == old["rounds"]


def test_short_loci_forced_onto_the_chunked_path(monkeypatch):
    """Loci below the switch (the <256> kernels' shapes), ragged and empty ones among them, forced onto the chunked path."""
    engine = _engine()
    from tapir_amd import synth
    d = synth.simulate(7, 300, 16, 5)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = np.ascontiguousarray(d["states"].numpy())
    offs = np.array([0, 300, 301, 301, 900, 1500, 2100], dtype=np.int64)   # 300, 1, 0, 599, 600, 600 columns
    small = (np.ascontiguousarray(st[:, :2100]), offs, d["pi"][:6], d["exch"][:6], pin)
    for env in (dict(BASE, TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0.15"), {}):
        old = _run(engine, monkeypatch, dict(env, TPHIP_COMPACT_CHUNKED="0"), small, 16)
        new = _run(engine, monkeypatch, dict(env, TPHIP_COMPACT_CHUNKED="1"), small, 16)
        for key in KEYS:
            assert new[key].tobytes() == old[key].tobytes(), (env, key)
        assert new["evals"] == old["evals"] and new["rounds"] == old["rounds"]

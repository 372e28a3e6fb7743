"""The later shares' cut of the reserved tails in whole lane-fills (TPHIP_SITE_TAIL_SHARES; tail_shares.hpp) changes how many
evaluation rounds the waves issue and nothing else: every case compares with the same plan under TPHIP_SITE_TAIL_SHARES=0,
the cut into equal column counts, and the rounds with the CPU replay's prediction from the oracle's evaluation counts of the
very batch (tools/share_replay.py).  The batches are test_gpu_share_work.py's."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("TPHIP_SITE_PERSISTENT", "TPHIP_SITE_MIXED", "TPHIP_SITE_WAVES", "TPHIP_SITE_GRID_MULT", "TPHIP_SITE_FIRST_FRACTION",
         "TPHIP_SITE_CHUNK", "TPHIP_SITE_TAIL_ORDER", "TPHIP_SITE_SHARE_WORK", "TPHIP_SITE_RESERVE", "TPHIP_SITE_CLASS_WEIGHTS",
         "TPHIP_SITE_TAIL_SHARES", "TPHIP_SITE_SPILL", "TPHIP_DEDUP")
KEYS = ("rate", "subst", "lnl", "flag", "nres", "tables")
WAVES, MULT, RESERVE, WEIGHTS = 16, 3, 0.25, (2.9, 2.04)
BASE = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES=str(WAVES), TPHIP_SITE_GRID_MULT=str(MULT), TPHIP_SITE_FIRST_FRACTION="0.8",
            TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE=str(RESERVE), TPHIP_SITE_CLASS_WEIGHTS="%g,%g" % WEIGHTS, TPHIP_DEDUP="0")


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


def _geometries():
    """2/2/2, 4/2/1 and the library's default, spelled out (this batch's later shares come from the knobs: left alone the
    library cuts them into equal column counts)."""
    rp = _replay()
    return ["2,2,2", "4,2,1", "%d,%d,%d,%g,%g" % (rp.DEFAULT_TAIL_FILLS + rp.DEFAULT_TAIL_FRACS)]


def _run(engine, monkeypatch, env, ntaxa, st, off, d, pin, model="gtr"):
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


class Batch:
    """A batch, the CPU's view of it (classification, the oracle's evaluations per column) and its run with later shares of
    equal column counts: computed once, shared by the cases."""

    def __init__(self, ntaxa, st, off, d, pin):
        rp = _replay()
        self.ntaxa, self.st, self.off, self.d, self.pin = ntaxa, st, off, d, pin
        self.optimised, self.slow = rp.classify(st, pin["parent"], pin["leaf"])
        self.ev = rp.column_evals(st, off, pin, d["pi"], d["exch"], self.optimised)
        self.ref = {}

    def n_easy(self):
        return [int((self.optimised & ~self.slow)[int(a):int(b)].sum()) for a, b in zip(self.off[:-1], self.off[1:])]

    def tails(self, q):
        return sum(int(_replay().reserved_before(n, q)) for n in self.n_easy())

    def predicted(self, reserve, tail, waves=WAVES):
        return _replay().replay_work(self.ev, self.slow, self.optimised, self.off, waves, MULT, reserve, WEIGHTS, 128, True, tail)

    def check(self, engine, monkeypatch, geometry, reserve=RESERVE, model="gtr"):
        """Outputs and evaluation count against equal column counts, rounds of both against the replay."""
        rp = _replay()
        env = dict(BASE, TPHIP_SITE_RESERVE=repr(reserve))
        key = (reserve, model)
        if key not in self.ref:
            self.ref[key] = _run(engine, monkeypatch, dict(env, TPHIP_SITE_TAIL_SHARES="0"), self.ntaxa, self.st, self.off, self.d, self.pin, model)
        ref = self.ref[key]
        got = _run(engine, monkeypatch, dict(env, TPHIP_SITE_TAIL_SHARES=geometry), self.ntaxa, self.st, self.off, self.d, self.pin, model)
        want, want_ref = self.predicted(reserve, rp.parse_tail_shares(geometry)), self.predicted(reserve, None)
        print("tail shares %s, reserve %r, %s: rounds %d (replay %d), equal column counts %d (replay %d), evaluations %d / %d"
              % (geometry, reserve, model, got["rounds"], want, ref["rounds"], want_ref, got["evals"], ref["evals"]))
        _same(got, ref, (geometry, reserve, model))
        if model == "gtr":     # (the oracle's evaluation counts are the GTR optimiser's)
            assert got["evals"] == int(self.ev.sum())
            assert ref["rounds"] == want_ref and got["rounds"] == want, (geometry, reserve)
        return got, ref


@pytest.fixture(scope="module")
def batch64():
    st, off, d, pin = _replay().share_order_batch(6, 2500, 64, 5)
    return Batch(64, st, off, d, pin)


@pytest.fixture(scope="module")
def edge_batch():
    """test_gpu_share_work.py's five loci of 700 columns x 24 taxa: [0] as simulated, [1] constant columns only, [2] marked
    columns only (an empty reserved tail), [3] marked columns and three unmarked ones (a reserve of 0.25 takes no whole
    column of them), [4] as simulated."""
    from tapir_amd import synth
    rp = _replay()
    ncols = 700
    d = synth.simulate(5, ncols, 24, 31)
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
    b = Batch(24, np.ascontiguousarray(st), off, d, pin)
    assert not b.optimised[off[1]:off[2]].any() and b.slow[off[2]:off[3]].all() and b.n_easy()[3] == 3
    return b


@pytest.mark.parametrize("which", range(3))
def test_base_batch(monkeypatch, batch64, which):
    """6 loci x 2500 columns x 64 taxa, 16 resident waves: 2/2/2, 4/2/1 and the default fills against equal column counts."""
    engine = _engine()
    got, ref = batch64.check(engine, monkeypatch, _geometries()[which])
    assert ref["rounds"] == 336           # what test_gpu_share_work.py pins for this hand-out
    assert got["rounds"] > 0


@pytest.mark.parametrize("which", range(3))
def test_edge_batch(monkeypatch, edge_batch, which):
    """An empty tail, a locus without optimiser work, a tail of no column at all beside two ordinary loci."""
    batch = edge_batch
    q = _replay().fixed(RESERVE, 16)
    assert 64 < batch.tails(q) and _replay().reserved_before(batch.n_easy()[3], q) == 0
    batch.check(_engine(), monkeypatch, _geometries()[which])


def _reserve_with(batch, accept, lo, hi):
    """A reserve (as the knob's text reads it) whose tails' total length the predicate accepts."""
    rp = _replay()
    for q in range(rp.fixed(lo, 16), rp.fixed(hi, 16)):
        reserve = float(repr(q / 65536.0))
        if rp.fixed(reserve, 16) == q and accept(batch.tails(q)):
            return reserve, batch.tails(q)
    raise AssertionError("no such reserve")


def test_tails_of_whole_fills_and_under_one_fill(monkeypatch, batch64):
    """The tails' total an exact multiple of 64 (the last share ends on a fill, nothing ragged), and under 64 (one share, the
    other later workgroups leave at once)."""
    engine = _engine()
    reserve, total = _reserve_with(batch64, lambda t: t % 64 == 0 and t >= 64 * 20, 0.15, 0.35)
    print("reserve %r: tails of %d columns" % (reserve, total))
    for geometry in _geometries()[1:]:
        batch64.check(engine, monkeypatch, geometry, reserve)
    reserve, total = _reserve_with(batch64, lambda t: 6 <= t < 64, 0.0005, 0.01)
    print("reserve %r: tails of %d columns" % (reserve, total))
    assert sum(1 for n in batch64.n_easy() if _replay().reserved_before(n, _replay().fixed(reserve, 16)) > 0) >= 2   # across loci
    for geometry in _geometries()[:2]:
        batch64.check(engine, monkeypatch, geometry, reserve)


def test_f81(monkeypatch, edge_batch):
    """The closed-form kernel's WORK instantiation: byte-equal to equal column counts."""
    edge_batch.check(_engine(), monkeypatch, "4,2,1", model="f81")


def test_default_geometry_and_short_tails(monkeypatch):
    """The library's own choice (no TPHIP_SITE_TAIL_SHARES) on a batch whose equal share is 1750 columns: 2 loci x 7000 columns x
    64 taxa on 8 waves take the default fills, and the rounds are the replay's for them.  The same batch with one locus made
    constant has tails of less than a fill per later workgroup (the case of loci whose columns repeat, after
    de-duplication): the cut stays the one into equal column counts, round for round."""
    import copy
    from tapir_amd import synth
    engine, rp = _engine(), _replay()
    waves = 8
    d = synth.simulate(2, 7000, 64, 23)
    pin = synth.plan_inputs(d["root"], d["names"])
    full = Batch(64, np.ascontiguousarray(d["states"].numpy()), d["locus_offsets"], d, pin)
    short = copy.copy(full)
    short.st = full.st.copy()
    short.st[:, full.off[1]:] = 1
    short.optimised, short.slow, short.ev = full.optimised.copy(), full.slow.copy(), full.ev.copy()
    short.optimised[full.off[1]:], short.slow[full.off[1]:], short.ev[full.off[1]:] = False, False, 0
    q = rp.fixed(0.15, 16)
    tail = rp.default_tail_shares(14000, waves, MULT, q)
    assert tail == rp.tail_shares(*rp.DEFAULT_TAIL_FILLS) + (64 * waves * (MULT - 1),)
    assert full.tails(q) >= tail[5] > short.tails(q) >= 64
    env = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_MIXED="0", TPHIP_SITE_WAVES=str(waves), TPHIP_DEDUP="0")
    for batch, whole_fills in ((full, True), (short, False)):
        got = _run(engine, monkeypatch, env, 64, batch.st, batch.off, d, pin)
        ref = _run(engine, monkeypatch, dict(env, TPHIP_SITE_TAIL_SHARES="0"), 64, batch.st, batch.off, d, pin)
        want, want_ref = batch.predicted(0.15, tail, waves), batch.predicted(0.15, None, waves)
        print("tails of %d columns: rounds %d (replay %d), equal column counts %d (replay %d)"
              % (batch.tails(q), got["rounds"], want, ref["rounds"], want_ref))
        _same(got, ref, whole_fills)
        assert got["evals"] == int(batch.ev.sum())
        assert (got["rounds"], ref["rounds"]) == (want, want_ref)
        if not whole_fills:
            assert got["rounds"] == ref["rounds"]


def test_spilled_stack_rows_follow_the_grid(monkeypatch):
    """256 taxa, 2.1 M columns in 21 long loci: the persistent kernel with the fourth parked partial in a global scratch row per
    workgroup (the variant needs 1000 columns per resident wave).  Single fills make thousands of later shares more than
    waves x 3: the grid and the scratch rows grow with them, and the outputs are the same bytes."""
    import torch
    from tapir_amd import synth
    _engine()
    from tapir_amd import engine
    nloci, ncols, ntaxa = 21, 100000, 256
    seed = synth.WORKLOAD_SEED["C5"]
    d = synth.simulate(nloci, ncols, ntaxa, seed, device="cuda", tree=synth.yule_tree(ntaxa, seed))
    pin = synth.plan_inputs(d["root"], d["names"])
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(TPHIP_SITE_GRID_MULT="3", TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0.25").items():
        monkeypatch.setenv(k, v)
    outs = {}
    for tail in ("0", "1,1,1"):
        monkeypatch.setenv("TPHIP_SITE_TAIL_SHARES", tail)
        plan = engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], d["pi"], d["exch"], pin["T"],
                           [10], [[5, 15]], correction=pin["correction"])
        assert plan.stack_depth == 4
        n, dev = plan.ncols, d["states"].device
        out = dict(rate=torch.empty(n, dtype=torch.float64, device=dev), subst=torch.empty(n, dtype=torch.float64, device=dev),
                   lnl=torch.empty(n, dtype=torch.float64, device=dev), flag=torch.empty(n, dtype=torch.uint8, device=dev),
                   nres=torch.empty(n, dtype=torch.int32, device=dev), tables=torch.empty((nloci, plan.width), dtype=torch.float64, device=dev))
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        plan.run_dev(d["states"], out["rate"], out["subst"], out["lnl"], out["flag"], out["nres"], out["tables"], ws,
                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs[tail] = (out, plan.workspace_bytes, plan.last_eval_count(), plan.last_round_count())
        plan.close()
        del ws
    print("workspace %d / %d bytes, rounds %d / %d" % (outs["0"][1], outs["1,1,1"][1], outs["0"][3], outs["1,1,1"][3]))
    # 6144 rows of 6144 bytes under equal column counts; 2048 + at least 8204 with a fill per share (525 000 columns at most)
    assert outs["1,1,1"][1] - outs["0"][1] >= (2048 + 8204 - 6144) * 6144
    assert outs["0"][2] == outs["1,1,1"][2] > 0
    for k in outs["0"][0]:
        assert torch.equal(outs["0"][0][k], outs["1,1,1"][0][k]), k
    del outs, d
    torch.cuda.empty_cache()

"""GPU: the PI partial sums in two kernels (pi_net_kernel + pi_interval_kernel, TPHIP_PI_SPLIT=1; the default for loci longer
than 2048 columns) against the fused pi_partial_kernel (TPHIP_PI_SPLIT=0).  Both pack a chunk's contributing rates the same
way and add in the same order, so the whole [L, W] table must be the same to the byte: no tolerance anywhere in the
comparisons between the two.

The cases are driven through tphip_pi_tables_dev (Plan.pi_tables_dev) with chosen rates and informative-cell counts, without
rounding (round_decimals = -1), so that a rate reaches the kernels as written here divided by the correction:
  * one plan with loci of 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025 and 2049 columns, a 1024-column locus with no
    contributing column, and two whose contributing counts are 128 (a multiple of 64) and 129;
  * dead columns by a rate of exactly 0 and by the cull (nres < threshold: NaN inside the kernels), in turns;
  * rates of 1e-9; a rate that takes the generic first panel on every interval; and for every half-length in use a pair of
    rates with 4 r hl just below and just at 30, next to each other in the packed list, so that the generic panel and the
    factored one run in the same wave;
  * T around the 16-time tile; n_i around pi_partial_kernel's 8-interval register tile and pi_interval_kernel's 4-interval
    one, with unequal half-lengths inside a tile and a repeated interval;
  * both integration modes.
One case goes through the fused step (run_dev) on 3 loci x 2500 columns x 16 taxa and compares all six outputs.

The split path is also held to what tests/test_gpu_pi_partial_slots.py holds the fused one to: that file's restatement of
the reference's worker, its rates and its tolerances, on a locus of a full chunk and a one-column chunk."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 1024, 1024, 1024]
DEAD_LOCUS, LIVE128, LIVE129 = 11, 12, 13
T_VALUES = [1, 15, 16, 17, 33]
NI_VALUES = [0, 1, 3, 4, 5, 8, 9, 17]
THRESHOLD = 3


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def intervals_for(n_i):
    """Lengths 10, 6, 10, 4 in turns (half-lengths 5, 3, 5, 2: unequal inside every tile of four); the third interval repeats
    the second; the fifth starts at t = 0."""
    out = []
    for k in range(n_i):
        a = 3 + 2 * k
        out.append([a, a + (10, 6, 10, 4)[k % 4]])
    if n_i >= 3:
        out[2] = list(out[1])
    if n_i >= 5:
        out[4] = [0, 10]
    return out


HALF_LENGTHS = (5.0, 3.0, 2.0)


@pytest.fixture(scope="module")
def batch():
    """(pin, raw rates, nres, locus offsets): the rates are raw ones, the kernels see raw / correction."""
    from tapir_amd import synth
    d = synth.simulate(1, 4, 16, 11)
    pin = synth.plan_inputs(d["root"], d["names"])
    corr = float(pin["correction"])
    rng = np.random.default_rng(14)
    special = [1e-9 * corr, 40.0 * corr]
    for hl in HALF_LENGTHS:
        at = 30.0 / (4.0 * hl)
        below, above = np.nextafter(at * corr, 0.0), at * corr
        while not 4.0 * (below / corr) * hl < 30.0:
            below = np.nextafter(below, 0.0)
        while not 4.0 * (above / corr) * hl >= 30.0:
            above = np.nextafter(above, np.inf)
        assert 4.0 * (below / corr) * hl > 29.999999
        special += [below, above]
    rates, nres = [], []
    for l, size in enumerate(SIZES):
        live = {DEAD_LOCUS: 0, LIVE128: 128, LIVE129: 129}.get(l, size - size // 5)
        r = np.zeros(size)
        n = np.full(size, 10, dtype=np.int32)
        where = np.sort(rng.permutation(size)[:live])
        r[where] = np.clip(rng.lognormal(-2.0, 1.2, live), 1e-4, 0.5) * corr
        if live >= 2 * len(special):
            r[where[3:3 + len(special)]] = special          # neighbours in the packed list: one wave
            r[where[-len(special):]] = special[::-1]
        dead = np.setdiff1d(np.arange(size), where)
        culled = dead[1::2]
        r[culled] = 0.0371 * corr                           # a fine rate, but too few informative cells
        n[culled] = rng.integers(0, THRESHOLD, culled.size)
        rates.append(r)
        nres.append(n)
        seen = r / corr
        assert int(((seen != 0) & (n >= THRESHOLD)).sum()) == live
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    return pin, np.concatenate(rates), np.concatenate(nres), offs


def _pi_tables_dev(engine, monkeypatch, split, pin, offs, rates, nres, T, intervals, integ_mode, round_decimals=-1):
    import torch
    monkeypatch.setenv("TPHIP_PI_SPLIT", split)
    L = len(offs) - 1
    pi = np.tile([0.3, 0.2, 0.2, 0.3], (L, 1))
    exch = np.tile([1.0, 2.0, 1.0, 1.0, 2.0, 1.0], (L, 1))
    times = [0, T - 1]
    plan = engine.Plan(16, pin["parent"], pin["blen"], pin["leaf"], offs, pi, exch, T, times, intervals,
                       correction=pin["correction"], threshold=THRESHOLD, round_decimals=round_decimals, integ_mode=integ_mode)
    try:
        d_rates = torch.from_numpy(rates).cuda()
        d_nres = torch.from_numpy(nres).cuda()
        d_tables = torch.full((L, plan.width), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device="cuda")
        plan.pi_tables_dev(d_rates, d_nres, d_tables, ws, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert plan.width == T + len(times) + 2 * len(intervals)
        return d_tables.cpu().numpy()
    finally:
        plan.close()


def _compare(engine, monkeypatch, batch, T, n_i, integ_mode):
    pin, rates, nres, offs = batch
    iv = intervals_for(n_i)
    fused = _pi_tables_dev(engine, monkeypatch, "0", pin, offs, rates, nres, T, iv, integ_mode)
    split = _pi_tables_dev(engine, monkeypatch, "1", pin, offs, rates, nres, T, iv, integ_mode)
    assert fused.shape == (len(SIZES), T + 2 + 2 * n_i)
    assert not np.isnan(fused).any(), "an entry of the table was not written"
    assert split.tobytes() == fused.tobytes(), np.argwhere(split.view(np.uint64) != fused.view(np.uint64))[:8]
    assert np.all(fused[DEAD_LOCUS] == 0.0)
    if T > 1:
        assert np.all(fused[LIVE128, 1:T] > 0.0)
    if n_i:
        assert np.all(fused[LIVE129, T + 2:T + 2 + n_i] > 0.0)
    return fused


@pytest.mark.parametrize("integ_mode", [0, 1])
@pytest.mark.parametrize("T", T_VALUES)
def test_time_tiles(monkeypatch, batch, T, integ_mode):
    _compare(_engine(), monkeypatch, batch, T, 5, integ_mode)


@pytest.mark.parametrize("integ_mode", [0, 1])
@pytest.mark.parametrize("n_i", NI_VALUES)
def test_interval_tiles(monkeypatch, batch, n_i, integ_mode):
    _compare(_engine(), monkeypatch, batch, 17, n_i, integ_mode)


def test_special_rates_take_the_paths_they_are_there_for(batch):
    """On the host: the pairs around 4 r hl = 30 lie on both sides for their half-length, and the half-lengths are in use."""
    pin, rates, nres, offs = batch
    corr = float(pin["correction"])
    seen = rates / corr
    for hl in HALF_LENGTHS:
        x = 4.0 * seen * hl
        assert ((x < 30.0) & (x > 29.999999)).any() and ((x >= 30.0) & (x < 30.000001)).any()
        assert any(0.5 * (b - a) == hl for a, b in intervals_for(17))
    assert np.isclose(seen, 1e-9, rtol=1e-12, atol=0).any() and np.isclose(seen, 40.0, rtol=1e-12, atol=0).any() and (seen == 0.0).any() and (nres < THRESHOLD).any()
    iv = intervals_for(17)
    assert iv[2] == iv[1] and iv[4][0] == 0


def test_split_path_against_the_restated_reference(monkeypatch):
    """pi_net_kernel + pi_interval_kernel alone against the float64 numpy / scipy restatement of the reference's worker, with
    the rates, the special columns and the tolerances of tests/test_gpu_pi_partial_slots.py."""
    import test_gpu_pi_partial_slots as slots
    engine = _engine()
    setup = slots.make_setup()
    pin, corr = setup["pin"], setup["corr"]
    rng = np.random.default_rng(21)
    rates, nres = slots._join([slots._chunk(rng, slots.CHUNK, 769, setup["special"], corr), slots._chunk(rng, 1, 1, (), corr)])
    T, times, iv = int(pin["T"]), [0, int(pin["T"]) - 1], slots.IV2
    offs = np.array([0, rates.size], dtype=np.int64)
    tab = _pi_tables_dev(engine, monkeypatch, "1", pin, offs, rates, nres, T, iv, 0, round_decimals=4)[0]
    net, integ, err, live = slots._expected(setup, rates, nres, T, times, iv)
    assert live == 770
    worst = [float(slots._rel(tab[1:T], net[1:]).max()), float(slots._rel(tab[T:T + 2], net[times]).max()),
             float(slots._rel(tab[T + 2:T + 4], integ).max()), float(slots._rel(tab[T + 4:], err).max())]
    print("split path: worst rel net %.2e disc %.2e integral %.2e error %.2e" % tuple(worst))
    assert tab[0] == 0.0
    assert worst[0] < slots.RTOL_PI and worst[1] < slots.RTOL_PI and worst[2] < slots.RTOL_PI, worst
    assert worst[3] < slots.RTOL_ERR, worst


def test_fused_step_both_ways(monkeypatch):
    """run_dev on 3 loci x 2500 columns x 16 taxa (longer than 2048: the split is this batch's default) under both knob values:
    rates, substitutions, log-likelihoods, flags, informative-cell counts and tables, byte for byte."""
    import torch
    from tapir_amd import synth
    engine = _engine()
    d = synth.simulate(3, 2500, 16, 9, device="cuda")
    pin = synth.plan_inputs(d["root"], d["names"])
    got = {}
    for split in ("0", "1", None):
        if split is None:
            monkeypatch.delenv("TPHIP_PI_SPLIT")
        else:
            monkeypatch.setenv("TPHIP_PI_SPLIT", split)
        plan = engine.Plan(16, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], d["pi"], d["exch"], pin["T"],
                           [10, 30], [[5, 15], [25, 35], [45, 55], [85, 95], [3, 9]], correction=pin["correction"])
        try:
            n, dev = plan.ncols, d["states"].device
            out = dict(rate=torch.empty(n, dtype=torch.float64, device=dev), subst=torch.empty(n, dtype=torch.float64, device=dev),
                       lnl=torch.empty(n, dtype=torch.float64, device=dev), flag=torch.empty(n, dtype=torch.uint8, device=dev),
                       nres=torch.empty(n, dtype=torch.int32, device=dev),
                       tables=torch.empty((3, plan.width), dtype=torch.float64, device=dev))
            ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
            plan.run_dev(d["states"], out["rate"], out["subst"], out["lnl"], out["flag"], out["nres"], out["tables"], ws,
                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got[split] = {k: v.cpu().numpy() for k, v in out.items()}
        finally:
            plan.close()
    assert (got["0"]["flag"] == 0).sum() > 1000 and np.all(got["0"]["tables"][:, 1:pin["T"]] > 0.0)
    for key in ("rate", "subst", "lnl", "flag", "nres", "tables"):
        assert got["1"][key].tobytes() == got["0"][key].tobytes(), key
        assert got[None][key].tobytes() == got["0"][key].tobytes(), key

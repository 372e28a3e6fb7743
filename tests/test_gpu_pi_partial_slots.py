"""GPU: the PI partial sums (pi_partial_kernel) at the edges of their work split.

A 1024-column chunk's contributing rates are packed to the front and handed to the workgroup's four waves in 64-column
slots (packed index j * 256 + thread, j = 0..3); the sums run in 16-time tiles and 8-interval register tiles.  The sums
have a fixed order, so a locus' row must be the same to the byte wherever its chunks sit -- behind 0, 1, 2 and 3
one-chunk filler loci -- and on a second call, and equal the float64 numpy/scipy restatement of the reference's worker
(the oracle module's get_townsend_pi and get_net_integral_for_epochs) to the tolerances of
tests/test_gpu_parity.py::test_pi_tables_vs_reference_outputs.

Driven through plan.pi_tables(rates, nres) on a 16-taxon plan, so that rates and culls are chosen exactly: a column is
dead by a rate of 0 or by too few informative cells, the others are live.  Two special rates ride along in every case with
room for them: one takes QUADPACK's generic first panel on every interval (4 r hl >= 30), one is not accepted after its
first panel on [3, 503] (the adaptive path), found with the CPU oracle before the GPU run.

sum(error) is held to 1e-6 relative.  scipy's own abserr supports that only where it does not come out of a cancellation:
with the integrand's exp perturbed by one ulp (scipy alone, on the CPU) the abserr of a panel that is accepted at its
50 eps resabs floor, and of a bisection whose panels all end there, does not move at all, while a panel accepted
while it still converges (|resk - resg| small against resk: r = 0.005 on [0, 500]) moves by 4e-6, a converged adaptive
result by up to 1e-5, and a huge rate on an interval that starts at t = 0 by 8e-2.  So the cases keep sum(error) away
from those terms: ordinary rates stay at or below 0.004 (every interval used here is accepted at the floor), the
adaptive rate is the first one rejected on [3, 503] (0.008: three panels, all at the floor), and no interval starts
before t = 3, where the huge rate's integrand is below 1e-39.  The byte comparisons need none of this.

There the generic panel adds ~1e-11 of the sums, so a wrong finite result of it would pass.  test_generic_panel_alone is
its value check: only huge rates are live, on intervals from t = 0, sum(integral) at 1e-12 and sum(error) loosely.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL_PI = 1e-12      # tests/test_gpu_parity.py: net PI, discrete PI, sum(integral)
RTOL_ERR = 1e-6      # ... sum(error)
CHUNK = 1024
LIVE_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 767, 768, 769, 1023, 1024]
LONG = [3, 503]
IV2 = [[5, 15], LONG]
R_MAX = 0.004         # ordinary rates as the kernels see them stay at or below this (see the module docstring)


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _rel(a, b, floor=1e-300):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def make_setup():
    """The plan inputs, the two special raw rates and the filler chunk."""
    from oracle import oracle as orc
    from tapir_amd import synth
    d = synth.simulate(1, 4, 16, 11)
    pin = synth.plan_inputs(d["root"], d["names"])
    corr = float(pin["correction"])
    generic = float("%.4f" % (8.0 * corr + 1.0))          # r >= 8: 4 r hl >= 30 for every half-length >= 1
    assert 4.0 * (generic / corr) * 1.0 >= 30.0
    adaptive = None
    for x in np.arange(1, 400) * 1e-3:                    # r = x: factored first panel on LONG (4 r 250 < 30), not accepted
        raw = float("%.4f" % (x * corr))
        r = raw / corr
        if raw > 0 and 4.0 * r * 250.0 < 30.0 and orc.quad_townsend(LONG[0], LONG[1], r)[2] > 21:
            adaptive = raw
            break
    assert adaptive is not None, "no rate found whose first panel on LONG is rejected"
    assert adaptive / corr > R_MAX
    rng = np.random.default_rng(5)
    filler = _chunk(rng, CHUNK, 809, (), corr)                  # the bench's share of live columns
    return dict(pin=pin, corr=corr, special=(generic, adaptive), filler=filler)


@pytest.fixture(scope="module")
def setup():
    return make_setup()


def _chunk(rng, size, live, special, corr):
    """(rates, nres) of `size` columns, exactly `live` of them contributing, at random places; the others are dead by a
    rate of 0 or by the cull, in turns."""
    rates = np.zeros(size)
    nres = np.full(size, 10, dtype=np.int32)
    where = rng.permutation(size)[:live]
    rates[where] = np.round(np.clip(rng.lognormal(-2.0, 1.2, live), 1e-4, R_MAX * corr), 4)
    if live >= 2 + len(special):
        rates[where[:len(special)]] = special
    dead = np.setdiff1d(np.arange(size), where)
    culled = dead[1::2]
    rates[culled] = 0.0371                                 # a fine rate, but too few informative cells
    nres[culled] = rng.integers(0, 3, culled.size)
    return rates, nres


def _plan(engine, pin, sizes, T, times, intervals):
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    L = len(sizes)
    pi = np.tile([0.3, 0.2, 0.2, 0.3], (L, 1))
    exch = np.tile([1.0, 2.0, 1.0, 1.0, 2.0, 1.0], (L, 1))
    return engine.Plan(16, pin["parent"], pin["blen"], pin["leaf"], offs, pi, exch, T, times, intervals,
                       correction=pin["correction"], threshold=3, round_decimals=4)


def _expected(setup, rates, nres, T, times, intervals):
    """bin/tapir_compute.py's worker on the rates as the PI stage sees them: 4 decimals, / correction, cull."""
    from oracle import oracle as orc
    r = orc.round_dp(rates, 4) / setup["corr"]
    r[nres < 3] = np.nan
    live = int((np.isfinite(r) & (r != 0)).sum())
    net = np.nansum(orc.get_townsend_pi(orc.get_time(0, T), r), axis=1) if r.size else np.zeros(T)
    # (a rate of exactly 0 adds exactly 0 to every sum: scipy's quad is spared those columns)
    integ, err = np.zeros(len(intervals)), np.zeros(len(intervals))
    if live:
        ep = orc.get_net_integral_for_epochs(r[np.isfinite(r) & (r != 0)], intervals)
        integ = np.array([ep["%d-%d" % (a, b)]["sum(integral)"] for a, b in intervals], dtype=np.float64)
        err = np.array([ep["%d-%d" % (a, b)]["sum(error)"] for a, b in intervals], dtype=np.float64)
    return net, integ, err, live


def _check(engine, setup, rates, nres, T=None, times=None, intervals=IV2, live=None, what="", rtol_err=RTOL_ERR):
    """The locus behind 0..3 filler chunks: each row equal to the locus alone and to a second call, and to the restatement."""
    pin = setup["pin"]
    T = int(pin["T"]) if T is None else T
    times = [0, T - 1] if times is None else times
    n_t, n_i = len(times), len(intervals)
    fr, fn = setup["filler"]
    rows = []
    for k in range(4):
        plan = _plan(engine, pin, [CHUNK] * k + [len(rates)], T, times, intervals)
        try:
            t1 = plan.pi_tables(np.concatenate([fr] * k + [rates]), np.concatenate([fn] * k + [nres]))
            t2 = plan.pi_tables(np.concatenate([fr] * k + [rates]), np.concatenate([fn] * k + [nres]))
        finally:
            plan.close()
        assert t1.shape == (k + 1, T + n_t + 2 * n_i)
        assert np.array_equal(_bits(t1), _bits(t2)), (what, k, "second call")
        rows.append(t1[k].copy())
        assert np.array_equal(_bits(rows[k]), _bits(rows[0])), (what, k, "behind %d filler chunks" % k)
    tab = rows[0]
    net, integ, err, n_live = _expected(setup, rates, nres, T, times, intervals)
    if live is not None:
        assert n_live == live, (what, n_live, live)
    got_net, got_disc = tab[:T], tab[T:T + n_t]
    got_integ, got_err = tab[T + n_t:T + n_t + n_i], tab[T + n_t + n_i:]
    worst = [float(_rel(got_net[1:], net[1:]).max()) if T > 1 else 0.0,
             float(_rel(got_disc, net[times]).max()) if n_t else 0.0,
             float(_rel(got_integ, integ).max()) if n_i else 0.0,
             float(_rel(got_err, err).max()) if n_i else 0.0]
    print("%s: live %d, worst rel net %.2e disc %.2e integral %.2e error %.2e" % ((what, n_live) + tuple(worst)))
    assert got_net[0] == 0.0
    assert worst[0] < RTOL_PI and worst[1] < RTOL_PI and worst[2] < RTOL_PI, (what, worst)
    assert worst[3] < rtol_err, (what, worst)
    if n_live == 0:
        assert np.all(tab == 0.0)


def _intervals(n_i, mixed):
    """n_i intervals: of equal length (the first-panel factors are built once per column and reused), or of lengths 6, 10,
    6, ... with LONG third (rebuilt at every change; the adaptive path on the long one)."""
    if not mixed:
        return [[3 + 2 * k, 7 + 2 * k] for k in range(n_i)]
    return [LONG if k == 2 else [3 + k, 3 + k + (6 if k % 2 == 0 else 10)] for k in range(n_i)]


# Every case of this module by key; make_case builds it.  tools/debug/pi_rows_dump.py walks the same list.
LIVE_KEYS = [("live", n) for n in LIVE_COUNTS]
SIZE_KEYS = [("size", 1, (1,)), ("size", 1, (0,)), ("size", 1025, (1023, 1)), ("size", 1025, (64, 0)),
             ("size", 3072 + 7, (65, 767, 1024, 5))]
TIME_KEYS = [("T", T) for T in (1, 15, 16, 17, 33, None, 128, 129, 257)]
INTERVAL_KEYS = [("n_i", 0, False)] + [("n_i", n, m) for n in (1, 4, 5, 8, 9, 32, 64, 65) for m in (False, True)]
GENERIC_KEYS = [("generic", 70)]
CASE_KEYS = LIVE_KEYS + SIZE_KEYS + TIME_KEYS + INTERVAL_KEYS + GENERIC_KEYS


def _join(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def make_case(setup, key):
    """dict(rates, nres, T, intervals, live, what, rtol_err) of one key of CASE_KEYS (T None: the plan's own)."""
    corr, special = setup["corr"], setup["special"]
    kind = key[0]
    case = dict(T=None, intervals=IV2, rtol_err=RTOL_ERR, what=" ".join(str(k) for k in key))
    if kind == "live":
        case["rates"], case["nres"] = _chunk(np.random.default_rng(100 + key[1]), CHUNK, key[1], special, corr)
        case["live"] = key[1]
    elif kind == "size":
        size, lives = key[1], key[2]
        rng = np.random.default_rng(size + sum(lives))
        case["rates"], case["nres"] = _join([_chunk(rng, min(CHUNK, size - c * CHUNK), lv, special, corr)
                                             for c, lv in enumerate(lives)])
        assert case["rates"].size == size
        case["live"] = sum(lives)
    elif kind == "T":
        rng = np.random.default_rng(7)
        case["rates"], case["nres"] = _join([_chunk(rng, CHUNK, 769, special, corr), _chunk(rng, 1, 1, (), corr)])
        case.update(T=key[1], intervals=[[5, 15]], live=770)
    elif kind == "n_i":
        rng = np.random.default_rng(11)
        case["rates"], case["nres"] = _join([_chunk(rng, CHUNK, 129, special, corr), _chunk(rng, 1, 1, (), corr)])
        case.update(intervals=_intervals(key[1], key[2]), live=130)
    elif kind == "generic":
        # every live column takes the generic panel on every interval (4 r hl >= 30 at hl = 1), and the intervals start at
        # t = 0, where these integrands live: each integral is ~1 and found by bisection towards t = 0
        rng = np.random.default_rng(13)
        rates, nres = _chunk(rng, CHUNK, key[1], (), corr)
        where = np.flatnonzero((rates != 0) & (nres >= 3))
        assert where.size == key[1]
        rates[where] = np.round(np.array([8.01, 12.5, 40.0, 200.0])[np.arange(where.size) % 4] * corr, 4)
        assert np.all(4.0 * (rates[where] / corr) * 1.0 >= 30.0)
        # sum(error) here is a sum of the terms scipy's own abserr moves by 8e-2 on under a one-ulp change of exp (module
        # docstring): held to six times that, not to RTOL_ERR
        case.update(rates=rates, nres=nres, intervals=[[0, 10], [0, 2]], live=key[1], rtol_err=0.5)
    else:
        raise KeyError(key)
    return case


def _run(setup, key):
    c = make_case(setup, key)
    _check(_engine(), setup, c["rates"], c["nres"], T=c["T"], intervals=c["intervals"], live=c["live"], what=c["what"],
           rtol_err=c["rtol_err"])


@pytest.mark.parametrize("key", LIVE_KEYS, ids=lambda k: str(k[1]))
def test_live_columns_at_slot_edges(setup, key):
    """One full chunk with `live` contributing columns: the edges of the 64-column wave-slots and of the 256-column j-slots."""
    _run(setup, key)


@pytest.mark.parametrize("key", SIZE_KEYS, ids=lambda k: "%d-%s" % (k[1], "_".join(map(str, k[2]))))
def test_locus_sizes(setup, key):
    """Loci of 1, 1025 (a full chunk and a 1-column chunk) and 3072 + 7 columns, each chunk with its own live count."""
    _run(setup, key)


@pytest.mark.parametrize("key", TIME_KEYS, ids=lambda k: str(k[1]))
def test_time_points(setup, key):
    """T around the 16-time tile, the plan's own T, and 128, 129 and 257 (eight tiles, one time point more, sixteen more)."""
    _run(setup, key)


@pytest.mark.parametrize("key", INTERVAL_KEYS, ids=lambda k: "%d-%s" % (k[1], "mixed" if k[2] else "equal"))
def test_interval_counts(setup, key):
    """n_i from none (the smallest a plan accepts) over the edges of the 8-interval register tile to 32, 64 and 65;
    130 live columns: three waves carry a slot, the third a ragged one."""
    _run(setup, key)


@pytest.mark.parametrize("key", GENERIC_KEYS, ids=lambda k: str(k[1]))
def test_generic_panel_alone(setup, key):
    """Only huge rates are live and the intervals start at t = 0: every term of sum(integral) comes from the generic panel
    (quad_townsend<false>) and its bisections, none from the factored one."""
    _run(setup, key)

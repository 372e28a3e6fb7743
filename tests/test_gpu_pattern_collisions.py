"""The integer kernels that decide which columns are evaluated and with what weight, at the inputs where they can go wrong
(run on the MI355X box with -m gpu): tphip_compress_columns (pattern_kernels.hpp, pattern_driver.hip) and the stage-2
de-duplication (dedup_kernels.hpp) under CONSTRUCTED hash collisions (tests/pattern_hash_emulation.py), compression at the
edges of its packing and of the locus table, and tphip_state_histogram on all sixteen codes.

Their contract is exactness, so every comparison is for equality: the references are np.unique(..., axis=1,
return_counts=True) and np.bincount on the normalised bytes (the low nibble, 0 read as 15), which share nothing with the
kernels; de-duplicated results are compared bit for bit with the results on all columns.  The one floating-point bound is
the stage-1 fit on patterns against the fit on raw columns: 1e-8 of lnL, the bound tests/test_gpu_stage1.py holds
compress_patterns to (the order of the column sum differs)."""
import functools
import tempfile

import numpy as np
import pytest

import pattern_hash_emulation as ph

pytestmark = pytest.mark.gpu

KEY_SEED, FULL_SEED, TREE_SEED = 1, 2, 5
K_COPIES = 6                    # further copies of each of the two colliding columns in a stage-2 locus
RTOL_STAGE1_LNL = 1e-8          # tests/test_gpu_stage1.py::test_stage1_patterns_and_frequencies_on_the_device


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _check_compression(engine, st, off):
    """tphip_compress_columns on (st, off) against np.unique locus by locus; two calls must agree.  Returns the outputs."""
    st = np.ascontiguousarray(st, np.uint8)
    off = np.asarray(off, np.int64)
    ntaxa, ncols = st.shape
    pst, poff, w, cmap = engine.compress_columns(st, off)
    norm = ph.normalise(st)
    assert pst.shape[0] == ntaxa and poff[0] == 0 and poff[-1] == pst.shape[1] == len(w) and len(poff) == len(off)
    assert w.sum() == ncols and np.all(w >= 1) and np.all(np.diff(poff) >= 0)
    for l in range(len(off) - 1):
        cols = norm[:, off[l]:off[l + 1]]
        pats = pst[:, poff[l]:poff[l + 1]]
        if cols.shape[1] == 0:
            assert pats.shape[1] == 0, l
            continue
        uniq, counts = np.unique(cols, axis=1, return_counts=True)
        assert pats.shape[1] == uniq.shape[1], (l, pats.shape[1], uniq.shape[1])     # never split ...
        order = np.lexsort(pats[::-1])                                             # np.unique sorts columns lexicographically
        assert np.array_equal(pats[:, order], uniq), l                               # ... never merged
        assert np.array_equal(w[poff[l]:poff[l + 1]][order], counts), l
        own = cmap[off[l]:off[l + 1]]
        assert np.all((own >= poff[l]) & (own < poff[l + 1])), l                     # loci do not mix
    assert np.array_equal(pst[:, cmap], norm)
    pst2, poff2, w2, cmap2 = engine.compress_columns(st, off)
    assert np.array_equal(pst, pst2) and np.array_equal(poff, poff2) and np.array_equal(w, w2) and np.array_equal(cmap, cmap2)
    return pst, poff, w, cmap


# ---- 1. tphip_compress_columns when two patterns of a locus share their 40-bit sort key ------------------------------------

@functools.lru_cache(maxsize=None)
def _key_pair():
    a, b, key = ph.find_key_collision(16, KEY_SEED)
    assert int(ph.compress_key(a)[0]) == int(ph.compress_key(b)[0]) == key and not np.array_equal(a, b)
    return a, b


def _filler(n, seed, ntaxa=16):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 16, size=(ntaxa, n), dtype=np.uint8)


def test_compress_columns_under_a_key_collision():
    """Columns A, B, A, B, A of one locus, A and B distinct with the same sort key (locus, 40 bits of hash 1): after a sort
    by the key alone they stay interleaved, and a head test against the predecessor only starts five patterns of weight 1
    where the header promises A x 3 and B x 2.  The locus alone, then as the middle one of three whose neighbours hold A and
    B as well; patterns, weights and map against np.unique, two calls alike."""
    engine = _engine()
    a, b = _key_pair()
    A, B = a[:, None], b[:, None]
    mid = np.concatenate([A, B, A, B, A, _filler(7, 11)], axis=1)
    pst, poff, w, cmap = _check_compression(engine, mid, [0, mid.shape[1]])
    assert pst.shape[1] == 9 and sorted(w.tolist()) == [1.0] * 7 + [2.0, 3.0]
    assert cmap[0] == cmap[2] == cmap[4] != cmap[1] == cmap[3]
    left = np.concatenate([_filler(3, 12), B, A, B, _filler(2, 13)], axis=1)
    right = np.concatenate([A, A, B, _filler(4, 14), B, A, B, A], axis=1)
    st = np.concatenate([left, mid, right], axis=1)
    off = np.cumsum([0, left.shape[1], mid.shape[1], right.shape[1]])
    pst, poff, w, cmap = _check_compression(engine, st, off)
    assert np.diff(poff).tolist() == [7, 9, 6]
    # the other interleavings of a tie: B first, runs of one pattern between the other's, a third column with its own key
    for seq in ("BABAB", "AABBAABB", "ABBA", "BAAAB", "ABxABxBA"):
        cols = [A if ch == "A" else B if ch == "B" else _filler(1, 15) for ch in seq]
        st = np.concatenate(cols + [_filler(5, 16)], axis=1)
        pst, poff, w, cmap = _check_compression(engine, st, [0, st.shape[1]])
        assert pst.shape[1] == 2 + 5 + ("x" in seq), seq


def test_stage1_fit_on_patterns_under_a_key_collision():
    """The same locus (A, B, A, B, A among 300 simulated columns of a 16-taxon tree) through tphip_stage1_fit with
    compress_patterns against the fit on the raw columns: the same likelihood, within the bound test_gpu_stage1.py uses."""
    engine = _engine()
    from tapir_amd import synth
    a, b = _key_pair()
    d = synth.simulate(1, 300, 16, 23)
    pin = synth.plan_inputs(d["root"], d["names"])
    fill = d["states"].numpy()
    st = np.ascontiguousarray(np.concatenate([fill[:, :100], a[:, None], b[:, None], a[:, None], fill[:, 100:200], b[:, None],
                                              a[:, None], fill[:, 200:]], axis=1))
    off = np.array([0, st.shape[1]], np.int64)
    pst, poff, w, cmap = _check_compression(engine, st, off)
    assert pst.shape[1] < st.shape[1] - 3                      # the simulated columns repeat too
    plan = engine.Plan(16, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], np.ones((1, 6)), pin["T"], [10], [[5, 15]],
                       correction=pin["correction"])
    try:
        comp = plan.stage1_fit(st, compress_patterns=True)
        raw = plan.stage1_fit(st, compress_patterns=False)
    finally:
        plan.close()
    gap = np.max(np.abs(comp["lnl"][:, 0] - raw["lnl"][:, 0]) / np.abs(raw["lnl"][:, 0]))
    print("stage-1 lnL on patterns %.12f, on raw columns %.12f: relative gap %.3g (bound %.1g)"
          % (comp["lnl"][0, 0], raw["lnl"][0, 0], gap, RTOL_STAGE1_LNL))
    assert np.isfinite(raw["lnl"][0, 0]) and gap < RTOL_STAGE1_LNL


# ---- 2. tphip_compress_columns at its edges ---------------------------------------------------------------------------------

def _tiny_loci(rng):
    sizes = rng.integers(0, 7, size=1025)
    sizes[[0, 1, 500, 501, 1024]] = 0                  # empty loci first and last, and two in a row (twice)
    sizes[[2, 3, 777, 1023]] = 1                       # one-column loci, next to each other and next to empty ones
    return sizes.tolist()


LAYOUTS = {
    "1 locus": lambda rng: [3000],
    "2 loci": lambda rng: [1, 2999],
    "3 loci, empty first and last": lambda rng: [0, 2500, 0],
    "3 loci, one column in the middle": lambda rng: [1200, 1, 1300],
    "1025 tiny loci": _tiny_loci,
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("ntaxa", [1, 7, 8, 9, 16, 17, 64, 65])
def test_compress_columns_at_the_edges(ntaxa, layout):
    """ntaxa around the eight-taxa word (a partial last word, exactly one and two words, nine words) x locus tables with one
    locus, with empty loci first, last and two in a row, with one-column loci and with 1025 tiny loci.  Columns are drawn from
    a pool of 60 (so that loci repeat columns, and adjacent loci hold identical ones) mixed with fresh random columns; the
    pool holds code 0 cells, bytes with high bits set, and all-gap columns written as 15, as 0 and as 0xf0."""
    engine = _engine()
    rng = np.random.default_rng(1000 * ntaxa + len(layout))
    sizes = LAYOUTS[layout](rng)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ncols = int(off[-1])
    assert 2000 <= ncols <= 5000
    pool = rng.integers(0, 16, size=(ntaxa, 60), dtype=np.uint8)
    pool[:, 0], pool[:, 1], pool[:, 2] = 15, 0, 0xF0                     # three spellings of the all-gap column
    pool[:, 3] = pool[:, 4]
    pool[rng.integers(0, ntaxa), 3] ^= 0x30                              # equal to column 4 once the high bits are dropped
    pool[:, 5] = np.where(pool[:, 6] == 15, 0, pool[:, 6])               # ... and once 0 reads as 15
    fresh = rng.integers(0, 16, size=(ntaxa, ncols), dtype=np.uint8)
    pick = rng.integers(0, 60, size=ncols)
    st = np.where(rng.random(ncols) < 0.7, pool[:, pick], fresh)
    b = off[len(off) // 2]
    if 0 < b < ncols:
        st[:, b] = st[:, b - 1]                                          # identical columns on both sides of a locus boundary
    pst, poff, w, cmap = _check_compression(engine, st, off)
    if ntaxa == 1:
        assert pst.shape[1] <= 15 * (len(off) - 1)
    assert pst.min() >= 1 and pst.max() <= 15


# ---- 3. stage-2 de-duplication when two patterns of a locus share the full 64-bit hash ------------------------------------

@functools.lru_cache(maxsize=None)
def _tree(ntaxa):
    from tapir_amd import synth
    root, names = synth.yule_tree(ntaxa, TREE_SEED)
    pin = synth.plan_inputs(root, names)
    order = ph.tip_order(pin["parent"], pin["blen"], pin["leaf"], ntaxa, tempfile.mkdtemp(prefix="tree_program"))
    pi, exch = synth.locus_parameters(1, 7)
    return pin, order, pi, exch


def _stage2_plan(engine, ntaxa, ncols, mode):
    pin, _, pi, exch = _tree(ntaxa)
    return engine.Plan(ntaxa, pin["parent"], pin["blen"], pin["leaf"], [0, ncols], pi, exch, pin["T"], [10, 30], [[5, 15]],
                       correction=pin["correction"], pattern_dedup=mode)


def _run(engine, ntaxa, st, mode):
    st = np.ascontiguousarray(st, np.uint8)
    plan = _stage2_plan(engine, ntaxa, st.shape[1], mode)
    try:
        return plan.run_fused(st), plan.last_eval_count()
    finally:
        plan.close()


@functools.lru_cache(maxsize=None)
def _full_pair(ntaxa):
    """The first constructed pair whose two columns the engine optimises (flag neither FLAT = 1 nor ZERO = 3) to different
    rates, by one run without de-duplication over all constructed pairs; with each column's own evaluation count from
    one-column plans, and whether those counts add up in a two-column plan."""
    engine = _engine()
    _, order, _, _ = _tree(ntaxa)
    pairs = ph.full_collisions(order, FULL_SEED)
    st = np.stack([c for p in pairs for c in p[:2]], axis=1)
    out, _ = _run(engine, ntaxa, st, engine.DEDUP_OFF)
    for i, (a, b, h) in enumerate(pairs):
        fa, fb = int(out["flag"][2 * i]), int(out["flag"][2 * i + 1])
        if fa not in (1, 3) and fb not in (1, 3) and out["rate"][2 * i] != out["rate"][2 * i + 1]:
            assert int(ph.classify_hash(a, order)[0]) == int(ph.classify_hash(b, order)[0]) == h
            ea = _run(engine, ntaxa, a[:, None], engine.DEDUP_OFF)[1]
            eb = _run(engine, ntaxa, b[:, None], engine.DEDUP_OFF)[1]
            eab = _run(engine, ntaxa, np.stack([a, b], axis=1), engine.DEDUP_OFF)[1]
            print("%d taxa: pair %d of %d, flags %d / %d, rates %.6g / %.6g; evaluations alone %d and %d, together %d"
                  % (ntaxa, i, len(pairs), fa, fb, out["rate"][2 * i], out["rate"][2 * i + 1], ea, eb, eab))
            return a, b, ea, eb, eab
    pytest.fail("none of the %d constructed pairs is a pair of work columns with different rates: flags %s, rates %s"
                % (len(pairs), out["flag"].tolist(), out["rate"].tolist()))


@functools.lru_cache(maxsize=None)
def _padding(ntaxa, n):
    """n distinct simulated columns on the tree of _tree(ntaxa) (fast enough to vary: most of them need the optimiser)."""
    from tapir_amd import synth
    root, names = synth.yule_tree(ntaxa, TREE_SEED)
    sim = synth.simulate(1, 3 * n + 200, ntaxa, 31 + ntaxa, tree=(root, names), rate_mean=0.02)["states"].numpy()
    _, first = np.unique(ph.normalise(sim), axis=1, return_index=True)
    first = np.sort(first)
    assert len(first) >= n
    return np.ascontiguousarray(sim[:, first[:n]])


def _collision_locus(ntaxa, ncols, first, second):
    """`first`, `second` at columns 3 and 4, then K_COPIES further copies of each, alternating, in one run across every
    1024-column boundary of the locus (in the middle of a short one), the rest distinct padding.  Returns the locus and
    the positions of the two patterns."""
    slots = [3, 4]
    bounds = [b for b in (1024, 2048) if b < ncols] or [ncols // 2 + 6]
    per = 2 * K_COPIES // len(bounds)
    for b in bounds:
        slots += list(range(b - per // 2, b + per // 2))
    assert len(slots) == 2 + 2 * K_COPIES and len(set(slots)) == len(slots) and max(slots) < ncols
    st = np.empty((ntaxa, ncols), np.uint8)
    pad = np.setdiff1d(np.arange(ncols), slots)
    st[:, pad] = _padding(ntaxa, len(pad))
    pos_first, pos_second = slots[0::2], slots[1::2]
    st[:, pos_first] = first[:, None]
    st[:, pos_second] = second[:, None]
    return st, np.array(pos_first), np.array(pos_second), pad


@pytest.mark.parametrize("lead", ["A first", "B first"])
@pytest.mark.parametrize("ncols", [40, 1100, 2100])
@pytest.mark.parametrize("ntaxa", [16, 70])
def test_stage2_dedup_under_a_full_hash_collision(ntaxa, ncols, lead):
    """A locus that holds two distinct columns with the same 64-bit classify hash, K_COPIES + 1 = 7 times each, among distinct
    padding: the table's representative of the hash is whichever comes first, and every copy of the other must find that its
    packed words differ and stay on the work list (dedup_resolve_kernel).  16 taxa (two words, both differ) and 70 (nine
    words, seven shared); loci of 40, 1100 and 2100 columns (the last takes dedup_estimate_kernel<1024> and the chunked
    compaction), the copies across the 1024-column boundaries; either column first.

    run_fused with de-duplication forced on equals the run without it in every bit of every output.  That the path ran is
    read from the engine's own outputs: (a) without de-duplication the two columns are work columns with different rates;
    (b) evaluation counts.  last_eval_count() is additive over columns -- a column's count depends on its packed words and its
    locus' model alone: the counts of one-column plans of A and B add up to the two-column plan's, and the run without
    de-duplication counts 7 e(A) + 7 e(B) + the padding's own run (both asserted below) -- so the run with de-duplication
    must count e(representative) + 7 e(other) + padding: one optimisation for the representative's seven columns, seven for
    the other's.  This additive form is the one that holds on the MI355X (16 taxa: 5 + 5 = 10 alone and together, 40
    columns off 172 = 7 x 10 + 102, on 142 = 5 + 7 x 5 + 102; 70 taxa: 6 + 6 = 12, off 144 = 7 x 12 + 60, on 108), so no
    control locus is needed.  The figures are printed before they are asserted.

    The same locus through eb_posterior and eb_fit_scale with and without site patterns: bit-identical, as test_gpu_eb.py
    requires of ordinary loci."""
    engine = _engine()
    from tapir_amd import eb
    a, b, ea, eb_, eab = _full_pair(ntaxa)
    print("%d taxa: evaluations of A alone %d, of B alone %d, of the two-column locus %d" % (ntaxa, ea, eb_, eab))
    assert ea > 0 and eb_ > 0 and eab == ea + eb_
    first, second, e_first, e_second = (a, b, ea, eb_) if lead == "A first" else (b, a, eb_, ea)
    st, pos_first, pos_second, pad = _collision_locus(ntaxa, ncols, first, second)
    assert pos_first[0] < pos_second[0]
    if ncols > 1024:
        assert pos_first.min() < 1024 <= pos_first.max() and pos_second.min() < 1024 <= pos_second.max()
    off_out, ev_off = _run(engine, ntaxa, st, engine.DEDUP_OFF)
    on_out, ev_on = _run(engine, ntaxa, st, engine.DEDUP_ON)
    ev_pad = _run(engine, ntaxa, st[:, pad], engine.DEDUP_OFF)[1]
    n = K_COPIES + 1
    print("%d taxa, %d columns, %s: evaluations off %d = %d x (%d + %d) + padding %d ?  on %d = %d + %d x %d + padding %d ?"
          % (ntaxa, ncols, lead, ev_off, n, e_first, e_second, ev_pad, ev_on, e_first, n, e_second, ev_pad))
    # (a) without de-duplication both are work columns, with different answers
    for pos in (pos_first, pos_second):
        assert all(int(f) not in (1, 3) for f in off_out["flag"][pos])
        assert len(set(off_out["rate"][pos].tolist())) == 1 and len(set(off_out["lnl"][pos].tolist())) == 1
    assert off_out["rate"][pos_first[0]] != off_out["rate"][pos_second[0]]
    # every output, bit for bit
    assert sorted(off_out) == ["flag", "lnl", "nres", "rate", "subst", "tables"]
    for k in off_out:
        assert np.array_equal(on_out[k], off_out[k], equal_nan=True), k
    # (b) the copies of the column that is not the representative were optimised one by one
    assert ev_off == n * (e_first + e_second) + ev_pad
    assert ev_on == e_first + n * e_second + ev_pad
    # empirical Bayes on site patterns: every column takes part, constant ones too
    pin, _, pi, exch = _tree(ntaxa)
    off = np.array([0, ncols], np.int64)
    start = eb.start_scales(st, off, pin["parent"], pin["blen"], pin["leaf"])
    rho, w = eb.gamma_tables([0.7], 4)
    plan = _stage2_plan(engine, ntaxa, ncols, engine.DEDUP_AUTO)
    try:
        raw = plan.eb_posterior(st, rho, w, start, use_patterns=False)
        pat = plan.eb_posterior(st, rho, w, start, use_patterns=True)
        fit_raw = plan.eb_fit_scale(st, rho, w, start, use_patterns=False)
        fit_pat = plan.eb_fit_scale(st, rho, w, start, use_patterns=True)
    finally:
        plan.close()
    assert raw["lnl"][pos_first[0]] != raw["lnl"][pos_second[0]] and raw["rate"][pos_first[0]] != raw["rate"][pos_second[0]]
    for k in ("rate", "sd", "lnl", "nres"):
        assert np.array_equal(raw[k], pat[k]), k
    for k in ("scale", "locus_lnl", "curvature"):
        assert np.array_equal(fit_raw[k], fit_pat[k]), k


# ---- 4. tphip_state_histogram on all sixteen codes --------------------------------------------------------------------------

@pytest.mark.parametrize("ntaxa", [1, 64, 65, 256])
def test_state_histogram_counts_every_code(ntaxa):
    """Loci of 0, 1, 3, 255, 256, 257 and 4097 columns in one call (the kernel strides a locus by its 256 threads), bytes over
    all 16 codes and some with high bits set: the counts are np.bincount of the normalised bytes -- code 0 is counted in bin
    15 and bin 0 stays empty."""
    engine = _engine()
    rng = np.random.default_rng(40 + ntaxa)
    sizes = [0, 1, 3, 255, 256, 257, 4097]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    st = rng.integers(0, 16, size=(ntaxa, int(off[-1])), dtype=np.uint8)
    st[rng.random(st.shape) < 0.1] |= 0x50
    hist = engine.state_histogram(st, off)
    assert hist.shape == (len(sizes), 16)
    norm = ph.normalise(st)
    for l, n in enumerate(sizes):
        blk = st[:, off[l]:off[l + 1]].ravel()
        want = np.bincount(np.where((blk & 15) == 0, 15, blk & 15), minlength=16)
        assert np.array_equal(want, np.bincount(norm[:, off[l]:off[l + 1]].ravel(), minlength=16))
        assert np.array_equal(hist[l], want), l
        assert hist[l, 0] == 0 and hist[l].sum() == n * ntaxa
    assert len(np.unique(st[:, off[-2]:] & 15)) == 16 and np.all(hist[-1, 1:] > 0)      # all 16 codes went in

"""GPU: a column's classification and a locus' PI row do not depend on where the locus sits in the batch.

classify_kernel gives each thread four consecutive columns and reads them as one dword when the locus starts on a
4-column boundary, byte by byte otherwise; a tree of more than 64 tips packs more than eight tip words per column.
pi_partial_kernel cuts every locus into 1024-column chunks that pi_reduce_kernel sums in chunk order.  Both are exact
integer / fixed-order work, so the required agreement is bit for bit: the same loci at 4-aligned and unaligned offsets,
next to 1-, 2- and 3-column and empty loci, give the same per-column outputs, with flags and informative-cell counts
equal to the CPU oracle's; a locus' PI row is the same alone, among neighbours of every chunk shape, and on a second
call of the same plan.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NTAXA = 70          # > 64 tips: nine packed words per column
NCOLS = 700


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _loci_states():
    """Two 700-column loci on a 70-taxon tree, with ambiguity codes, code 0 (nothing allowed), an all-gap column and
    a column of zeros mixed in; and the filler columns that go in front of or between them."""
    from tapir_amd import synth
    d = synth.simulate(2, NCOLS, NTAXA, 20261016)
    st = d["states"].numpy().copy()
    rng = np.random.default_rng(7)
    cells = rng.random(st.shape)
    st[cells < 0.03] = rng.choice(np.array([3, 5, 6, 9, 10, 12, 7, 11, 13, 14], np.uint8), size=int((cells < 0.03).sum()))
    st[(cells >= 0.03) & (cells < 0.045)] = 0
    st[:, 17] = 15                 # all gaps (locus 0)
    st[:, NCOLS + 400] = 15        # all gaps (locus 1)
    st[:, 333] = 0                 # nothing allowed anywhere: reads as all gaps
    filler = synth.simulate(1, 8, NTAXA, 99, tree=(d["root"], d["names"]))["states"].numpy()
    return d, st, filler


def _run(engine, pin, d, st, filler, layout):
    """layout: list of ('A' | 'B' | int k): the two loci or k filler columns (0 = an empty locus).  Returns the
    outputs and the column offset of each of A and B."""
    blocks, offs, pis, exs, where = [], [0], [], [], {}
    fcol = 0
    for item in layout:
        if item == "A" or item == "B":
            l = 0 if item == "A" else 1
            where[item] = offs[-1]
            blocks.append(st[:, l * NCOLS:(l + 1) * NCOLS])
            pis.append(d["pi"][l]); exs.append(d["exch"][l])
        else:
            blocks.append(filler[:, fcol:fcol + item])
            fcol += item
            pis.append(d["pi"][0]); exs.append(d["exch"][0])
        offs.append(offs[-1] + blocks[-1].shape[1])
    states = np.ascontiguousarray(np.concatenate(blocks, axis=1))
    plan = engine.Plan(NTAXA, pin["parent"], pin["blen"], pin["leaf"], offs, np.array(pis), np.array(exs), pin["T"],
                       [10, 30], [[5, 15], [25, 35]], correction=pin["correction"])
    try:
        out = plan.run_fused(states)
    finally:
        plan.close()
    return out, where, offs


def test_column_outputs_do_not_depend_on_locus_position():
    engine = _engine()
    from oracle import oracle as orc
    from tapir_amd import synth
    d, st, filler = _loci_states()
    pin = synth.plan_inputs(d["root"], d["names"])
    base, wb, _ = _run(engine, pin, d, st, filler, ["A", "B"])
    for l, name in enumerate("AB"):
        sl = slice(wb[name], wb[name] + NCOLS)
        ref = orc.site_rates(st[:, l * NCOLS:(l + 1) * NCOLS], pin["parent"], pin["blen"], pin["leaf"], d["pi"][l], d["exch"][l])
        assert np.array_equal(base["flag"][sl], ref["flag"]), name
        assert np.array_equal(base["nres"][sl], ref["nres"]), name
    layouts = [[1, "A", "B"], [2, "A", 0, "B"], [3, "A", 1, "B"], [0, 2, "B", 3, "A", 0]]
    for layout in layouts:
        out, w, offs = _run(engine, pin, d, st, filler, layout)
        for name in "AB":
            s0, s1 = slice(wb[name], wb[name] + NCOLS), slice(w[name], w[name] + NCOLS)
            for k in ("rate", "subst", "lnl", "flag", "nres"):
                assert np.array_equal(_bits(base[k][s0]), _bits(out[k][s1])), (layout, name, k)
            la, lb = layout.index(name), ["A", "B"].index(name)
            assert np.array_equal(_bits(base["tables"][lb]), _bits(out["tables"][la])), (layout, name, "PI row")


def _pi_plan(engine, pin, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    L = len(sizes)
    pi = np.tile([0.3, 0.2, 0.2, 0.3], (L, 1))
    exch = np.tile([1.0, 2.0, 1.0, 1.0, 2.0, 1.0], (L, 1))
    return engine.Plan(16, pin["parent"], pin["blen"], pin["leaf"], offs, pi, exch, pin["T"], [3, 10, 25],
                       [[2, 6], [5, 15], [20, 40]], correction=pin["correction"], threshold=3, round_decimals=4), offs


def test_pi_rows_do_not_depend_on_neighbours_or_chunking():
    engine = _engine()
    from tapir_amd import synth
    d = synth.simulate(1, 4, 16, 11)
    pin = synth.plan_inputs(d["root"], d["names"])
    # 1 chunk, several chunks with a ragged last one, a full chunk plus a 1-column chunk, an empty locus, 1 column
    sizes = [900, 2500, 1025, 0, 1, 3072, 7]
    rng = np.random.default_rng(3)
    n = int(np.sum(sizes))
    rates = rng.lognormal(-1.0, 1.5, n)
    rates[rng.random(n) < 0.2] = 0.0          # constant columns
    rates[rng.random(n) < 0.01] = 40.0        # huge rates: QUADPACK's generic panel
    nres = rng.integers(0, 40, n).astype(np.int32)   # some below the threshold: culled
    plan, offs = _pi_plan(engine, pin, sizes)
    try:
        t1 = plan.pi_tables(rates, nres)
        t2 = plan.pi_tables(rates, nres)      # the same plan again
    finally:
        plan.close()
    assert np.array_equal(_bits(t1), _bits(t2))
    assert np.all(t1[sizes.index(0)] == 0.0)
    for l, S in enumerate(sizes):
        if S == 0:
            continue
        alone, _ = _pi_plan(engine, pin, [S])
        try:
            ta = alone.pi_tables(rates[offs[l]:offs[l + 1]], nres[offs[l]:offs[l + 1]])
        finally:
            alone.close()
        assert np.array_equal(_bits(ta[0]), _bits(t1[l])), (l, S)

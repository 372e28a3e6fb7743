"""Site concordance factors on the GPU (tphip_concordance_counts, tphip_concordance_rows and their _dev twins; DESIGN.md section
3.12): the counts byte for byte against the enumeration of tests/concordance_reference.py, 64-bit per-column arithmetic, the
rows bit for bit against the plain-loop mirror, bit identity whatever surrounds a locus or a set, the refusals, the quartet
predictions of section 3.8 against simulated columns, and the command line on the bundled locus."""
import os
import sqlite3

import numpy as np
import pytest

import concordance_reference as cr
from concordance_reference import SHAPES, csr, shaped_sets, stored as _stored

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 1025]    # an empty locus, one column, a wave less one, a wave, a wave + 1, a workgroup + 1, 4 + 1
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


def _engine():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return engine


def _states(ntaxa, seed, ncols=int(OFFSETS[-1])):
    """Cells from all sixteen masks: four in five one base, the rest spread over the twelve other masks (0 included)."""
    weights = np.where(np.isin(np.arange(16), [1, 2, 4, 8]), 0.2, 0.2 / 12)
    return np.random.default_rng(seed).choice(16, size=(ntaxa, ncols), p=weights).astype(np.uint8)


@pytest.fixture(scope="module")
def batch70():
    """70 taxa on the ragged loci with the default sets of a 70-taxon tree (pooled sets and single quartets in one launch, 67
    internodes, more sets than one tile of the kernel), and the enumerated counts: computed once, never written to."""
    from tapir_amd import compute, newick, synth
    root, _ = synth.yule_tree(70, 11)
    names = [leaf.name for leaf in newick.leaves(root)]
    groups = compute.tree_concordance_groups(root)
    sets = compute.concordance_sets(groups, names)
    states = _states(70, 70)
    want = cr.counts_np(states, OFFSETS, sets["group_offsets"], sets["group_taxa"])
    want.setflags(write=False)
    return dict(states=states, sets=sets, want=want, groups=groups)


# ---- 1. the counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaxa", [5, 9, 70])
def test_counts_equal_the_enumeration_on_ragged_loci(ntaxa):
    engine = _engine()
    rng = np.random.default_rng(ntaxa)
    shapes = [s for s in SHAPES + [(2, 1, 1, 1), (1, 1, 2, 1), (1, 2, 2, 1)] if sum(s) <= ntaxa] + ([(5, 6, 7, 8)] if ntaxa == 70 else [])
    sets = shaped_sets(rng, ntaxa, shapes)
    assert len(sets) >= 3 and any(sum(len(g) for g in s) < ntaxa for s in sets)
    goff, taxa = csr(sets)
    states = _states(ntaxa, ntaxa)
    got = engine.concordance_counts(states, OFFSETS, goff, taxa)
    want = cr.counts_np(states, OFFSETS, goff, taxa) if ntaxa == 70 else np.array(cr.counts(states, OFFSETS, goff, taxa), dtype=np.uint64)
    assert got.dtype == np.uint64 and got.shape == (len(SIZES), len(sets), 3)
    assert np.array_equal(got, want)
    assert np.all(got[0] == 0) and np.all(want[-1].max(axis=0) > 0)


def test_counts_equal_the_enumeration_with_a_trees_default_sets(batch70):
    engine = _engine()
    sets = batch70["sets"]
    n_sets = int(sets["node_sets"][-1])
    assert n_sets > 1024 and len(batch70["groups"]) == 67 and not sets["enumerated"].all()
    got = engine.concordance_counts(batch70["states"], OFFSETS, sets["group_offsets"], sets["group_taxa"])
    assert np.array_equal(got, batch70["want"])


@pytest.mark.parametrize("rotation", [0, 1, 2])
def test_a_columns_numbers_are_formed_in_64_bits(rotation):
    """Four groups of 260 taxa, every column one base within two of them and another within the other two: 260^4 > 2^32 quartets
    a column, all for one of the three numbers."""
    engine = _engine()
    states = np.zeros((1040, 130), dtype=np.uint8)
    pair = [(0, 1), (0, 2), (0, 3)][rotation]                         # the groups that share A's base
    for g in range(4):
        states[260 * g:260 * (g + 1)] = 1 if g in pair else 4
    perm = np.random.default_rng(rotation).permutation(1040)         # the groups' taxa in no order
    rows = np.empty(1040, dtype=np.int64)
    rows[perm] = np.arange(1040)
    goff, taxa = csr([tuple(rows[260 * g:260 * (g + 1)].tolist() for g in range(4))])
    got = engine.concordance_counts(states[perm], [0, 130], goff, taxa)
    want = [0, 0, 0]
    want[rotation] = 130 * 260 ** 4
    assert 260 ** 4 > 2 ** 32 and got[0, 0].tolist() == want


def test_a_group_larger_than_the_packed_fields():
    """A group of 65540 taxa: more than a 16-bit field of the packed base counts holds."""
    engine = _engine()
    ntaxa = 65600
    states = _states(ntaxa, 3, ncols=3)
    states[:65540, 0] = 2                                             # one column where the whole group shows one base
    states[65540:65543, 0] = [2, 8, 8]
    goff, taxa = csr([(list(range(65540)), [65540], [65541], [65542])])
    got = engine.concordance_counts(states, [0, 1, 3], goff, taxa)
    assert got[0, 0].tolist() == [65540, 0, 0]
    assert np.array_equal(got, cr.counts_np(states, [0, 1, 3], goff, taxa))


# ---- 2. the rows -----------------------------------------------------------------------------------------------------------
def test_rows_equal_the_mirror_bit_for_bit(batch70):
    engine = _engine()
    sets = batch70["sets"]
    assert sets["enumerated"].any()                                   # an internode whose quartets are all listed
    counts = batch70["want"].copy()
    dead = int(np.flatnonzero(~sets["enumerated"])[0])
    counts[3, int(sets["node_sets"][dead]) + 2:int(sets["node_sets"][dead + 1])] = 0    # an internode without a decisive quartet
    got = engine.concordance_rows(counts, sets["node_sets"])
    want = cr.rows(counts.tolist(), sets["node_sets"])
    assert got.shape == (len(SIZES), 67, 12) and got.tobytes() == want.tobytes()
    assert np.all(np.isnan(got[3, dead, 6:10])) and got[3, dead, 10] == 0 and got[3, dead, 11] == 100
    assert np.all(np.isnan(got[0, :, 6:10])) and np.all(got[0, :, :6] == 0)              # the empty locus
    assert np.all((got[-1, :, 6:9] >= 0) & (got[-1, :, 6:9] <= 1)) and np.allclose(got[-1, :, 6:9].sum(axis=1), 1)
    # counts close to 2^53 convert exactly
    big = np.array([[[2 ** 53 - 1, 2 ** 52 + 1, 3], [2 ** 40 + 1, 0, 0], [2 ** 51 + 3, 2 ** 50 + 1, 5], [1, 2 ** 52 - 1, 0]]], dtype=np.uint64)
    assert engine.concordance_rows(big, [0, 4]).tobytes() == cr.rows(big.tolist(), [0, 4]).tobytes()


# ---- 3. bit identity -------------------------------------------------------------------------------------------------------
def test_counts_do_not_depend_on_what_surrounds_a_locus_or_a_set(batch70):
    import torch
    engine = _engine()
    states, sets, want = batch70["states"], batch70["sets"], batch70["want"]
    goff, taxa, nodes = sets["group_offsets"], sets["group_taxa"], sets["node_sets"]
    n_sets = int(nodes[-1])
    call = lambda st, off, **kw: engine.concordance_counts(st, off, goff, taxa, **kw)   # noqa: E731
    assert np.array_equal(call(states, OFFSETS), call(states, OFFSETS))                 # the same call twice
    order = [5, 0, 6, 2, 1, 4, 3]                                                       # the loci permuted
    moved = np.concatenate([states[:, OFFSETS[l]:OFFSETS[l + 1]] for l in order], axis=1)
    off = np.concatenate([[0], np.cumsum([SIZES[l] for l in order])])
    assert np.array_equal(call(moved, off), want[order])
    alone = np.ascontiguousarray(states[:, OFFSETS[5]:OFFSETS[6]])                      # a locus alone
    assert np.array_equal(call(alone, [0, SIZES[5]])[0], want[5])
    pitched = np.full((70, states.shape[1] + 77), 1, dtype=np.uint8)                    # rows longer than the batch
    pitched[:, :states.shape[1]] = states
    assert np.array_equal(call(pitched, OFFSETS, ncols_total=states.shape[1]), want)
    cut = int(nodes[31])                                                                # the sets in two calls
    first = engine.concordance_counts(states, OFFSETS, goff[:4 * cut + 1], taxa)
    second = engine.concordance_counts(states, OFFSETS, goff[4 * cut:], taxa)
    assert np.array_equal(np.concatenate([first, second], axis=1), want)
    # the _dev twins on device tensors, the rows rule included
    dev = torch.device("cuda", 0)
    d_states, d_off = torch.from_numpy(states).to(dev), torch.from_numpy(OFFSETS).to(dev)
    d_counts = torch.from_numpy(np.full((len(SIZES), n_sets, 3), -1, dtype=np.int64)).to(dev)   # (the call zeroes what it adds to)
    engine.concordance_counts_dev(d_states, states.shape[1], states.shape[1], 70, d_off, len(SIZES), goff, taxa, d_counts)
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint64), want)
    d_rows = torch.from_numpy(np.zeros((len(SIZES), len(nodes) - 1, 12))).to(dev)
    engine.concordance_rows_dev(d_counts, len(SIZES), n_sets, nodes, d_rows)
    assert d_rows.cpu().numpy().tobytes() == engine.concordance_rows(want, nodes).tobytes()


# ---- 4. the refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    import torch
    engine = _engine()
    dev = torch.device("cuda", 0)
    states = _states(6, 1, ncols=64)
    d_states, d_off = torch.from_numpy(states).to(dev), torch.tensor([0, 64], dtype=torch.int64, device=dev)
    d_counts = torch.from_numpy(np.full((1, 2, 3), 7, dtype=np.int64)).to(dev)
    good = ([0, 1, 2, 3, 4], [0, 1, 2, 3])
    cases = [(([0], []), 6, 64, "n_sets"), (good, 3, 64, "ntaxa"), (([0, 1, 1, 2, 3], [0, 1, 2]), 6, 64, "empty group"),
             ((good[0], [0, 1, 2, 6]), 6, 64, "out of range"), ((good[0], [0, 1, -1, 3]), 6, 64, "out of range"),
             (([0, 1, 3, 4, 5], [0, 1, 2, 3, 1]), 6, 64, "listed twice"),
             (([0, 1, 2, 3, 4, 5, 7, 8, 9], [0, 1, 2, 3, 0, 1, 2, 1, 3]), 6, 64, "listed twice"),   # (in the second set only)
             (good, 6, 63, "row_pitch")]
    for (goff, taxa), ntaxa, pitch, message in cases:
        with pytest.raises(engine.TphipError, match=message):
            engine.concordance_counts_dev(d_states, 64, pitch, ntaxa, d_off, 1, goff, taxa, d_counts)
        with pytest.raises(engine.TphipError, match=message):
            engine.concordance_counts(states[:ntaxa, :pitch], [0, pitch] if pitch < 64 else [0, 64], goff, taxa, ncols_total=64)
    d_rows = torch.from_numpy(np.full((1, 1, 12), 7.0)).to(dev)
    for nodes in ([0, 1], [0, 3], [1, 0]):                                # one set only, beyond the sets, decreasing
        with pytest.raises(engine.TphipError, match="node_sets"):
            engine.concordance_rows_dev(d_counts, 1, 2, nodes, d_rows)
    torch.cuda.synchronize()
    assert np.all(d_counts.cpu().numpy() == 7) and np.all(d_rows.cpu().numpy() == 7.0)
    # a taxon in two sets, and one in no group, are fine
    engine.concordance_counts_dev(d_states, 64, 64, 6, d_off, 1, [0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 3, 2, 1, 0], d_counts)
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint64),
                          np.array(cr.counts(states, [0, 64], [0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 3, 2, 1, 0]), dtype=np.uint64))


# ---- 5. prediction against observation ------------------------------------------------------------------------------------
N_SIM = 200000
SIM_TREES = {
    # unequal tips around the first internode the tree reports, the edge above (a, b): a long branch to a on its one side and to
    # c on the other, short ones to b and to d, so that ac|bd (long with long, short with short) draws far more noise than ad|bc
    5: "((a:60,b:6):10,(c:50,e:52):5,d:8);",
    9: "((a:60,b:6):10,(c:50,e:52):5,(d:8,(f:20,(g:30,(h:35,i:40):5):5):5):3);",
}
PI = [0.31, 0.19, 0.23, 0.27]
EXCH = [1.3, 3.1, 0.7, 0.9, 3.4, 1.0]


@pytest.mark.parametrize("model", ["gtr", "f81"])
@pytest.mark.parametrize("ntaxa", [5, 9])
def test_simulated_columns_show_the_counts_the_quartet_stage_predicts(ntaxa, model):
    """N columns simulated down the tree at one rate; the nearest-tip quartet of the first internode.  The observed counts are
    binomial(N, p) with p the per-site expectations of tphip_unequal_quartet_sites: each within 5 sd + 1 of N p.  With the two
    noise expectations exchanged the same bound fails (they are more than 12 sd apart: asserted first)."""
    engine = _engine()
    from tapir_amd import compute, newick
    root = newick.parse(SIM_TREES[ntaxa])
    names = [leaf.name for leaf in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, names)
    quartet = compute.tree_quartets(root)[0]
    groups = compute.tree_concordance_groups(root)[:1]
    sets = compute.concordance_sets(groups, names)
    rate = 0.012
    plan = engine.Plan(ntaxa, parent, blen, leaf, [0, N_SIM], [PI], None if model == "f81" else [EXCH], 10, [], [], correction=1.0,
                       threshold=0, round_decimals=-1, model=model)
    try:
        rates = np.full(N_SIM, rate)
        states = plan.simulate_columns(rates, None, replicate=0, seed=2020)
        p = plan.unequal_quartet_sites(rates, None, [list(quartet[2:7])])[:, 0, 0]
    finally:
        plan.close()
    assert np.isin(states, [1, 2, 4, 8]).all()                        # no missing cells
    counts = engine.concordance_counts(states, [0, N_SIM], sets["group_offsets"], sets["group_taxa"])
    near = engine.concordance_rows(counts, sets["node_sets"])[0, 0, 3:6]
    sd = np.sqrt(N_SIM * p * (1 - p))
    print("ntaxa %d %s: quartet %s, observed %s, expected %s, sd %s" % (ntaxa, model, quartet[2:7], near, N_SIM * p, sd))
    assert abs(p[1] - p[2]) * N_SIM > 12 * max(sd[1], sd[2])
    assert np.all(np.abs(near - N_SIM * p) <= 5 * sd + 1)
    swapped = p[[0, 2, 1]]
    assert not np.all(np.abs(near - N_SIM * swapped) <= 5 * np.sqrt(N_SIM * swapped * (1 - swapped)) + 1)


# ---- 6. the command line ---------------------------------------------------------------------------------------------------
def test_cli_on_the_bundled_locus(tmp_path, golden_dir):
    import shutil
    _engine()
    from tapir_amd import cli, compute, newick, nexus
    aln = tmp_path / "aln"
    aln.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln / "chr1_918.nex")
    tree = os.path.join(golden_dir, "Euteleost.tree")
    argv = [str(aln), tree, "--times", "10,30", "--intervals", "5-15,20-40", "--exchangeabilities", "1,1.2,0.8,0.9,1.5,1"]
    runs = []
    for name, extra in (("plain", []), ("flag", ["--site-concordance"])):
        out = tmp_path / name
        out.mkdir()
        runs.append(cli.main(argv + ["--output", str(out)] + extra))
    name = "phylogenetic-informativeness-concordance.sqlite"
    assert sorted(os.listdir(runs[1])) == sorted(os.listdir(runs[0]) + [name])
    main = "phylogenetic-informativeness.sqlite"
    assert open(os.path.join(runs[0], main), "rb").read() == open(os.path.join(runs[1], main), "rb").read()
    root = newick.read_tree(tree)
    names = [leaf.name for leaf in newick.leaves(root)]
    groups = compute.tree_concordance_groups(root)
    sets = compute.concordance_sets(groups, names)
    taxa, st = nexus.read_states(os.path.join(golden_dir, "chr1_918.nex"))
    st = st[[list(taxa).index(n) for n in names]]
    rows = cr.rows(cr.counts(st, [0, st.shape[1]], sets["group_offsets"], sets["group_taxa"]), sets["node_sets"])[0]
    con = sqlite3.connect(os.path.join(runs[1], name))
    got = con.execute("select * from concordance").fetchall()
    both = con.execute("select * from concordance_all").fetchall()
    con.close()
    assert len(groups) == 2 and [list(r)[1:] for r in got] == [[g[0]] + _stored(rows[i]) for i, g in enumerate(groups)]
    assert [list(r) for r in both] == [list(r)[1:] for r in got]          # one locus: all loci together is that locus
    assert sum(r[2] + r[3] + r[4] for r in got) > 0

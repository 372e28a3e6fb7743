"""The column simulation of the parametric bootstrap without a GPU: the CPU mirror (tests/simulate_reference.py) against the
distribution it must draw from, its edge cases, and the command line's refusals.  Every test prints its figures before it
asserts."""
import numpy as np
import pytest

import simulate_reference as sim

PI = np.array([0.10, 0.35, 0.15, 0.40])
EXCH = np.array([1.3, 1.0, 0.6, 0.9, 2.1, 0.7])
# two taxa under a root: leaves 0 and 1, both on branches of length T2
T2 = 0.7
PARENT2, BLEN2, LEAF2 = [2, 2, -1], [T2, T2, 0.0], [0, 1, -1]
N2 = 65536
Z_BOUND = 5.0


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_two_taxon_joint_frequencies(kind):
    """Leaves x, y of a two-taxon tree with branches t are distributed as pi_x P_xy(2 t) (reversibility).  65 536 columns at one
    rate, the 16 joint frequencies against scipy's expm: max |z| <= 5.  Seed 1 (the first one tried) gives max |z| = 2.18 for
    GTR and 1.66 for F81 on the CPU mirror, below the 4 above which another seed would have been taken."""
    model = sim.eigen_system(PI, EXCH) if kind == "gtr" else sim.f81_system(PI)
    r = 0.8 * model["kappa"]   # raw rate kappa * s with s = 0.8
    out = sim.simulate_locus(PARENT2, BLEN2, LEAF2, 2, model, np.full(N2, r), stream_id=3, b=0, seed=1)
    z, counts, expect = sim.joint_z(out["states"], model, 2 * T2 * r)
    print("%s: max |z| = %.3f over 16 cells, N = %d, undecided draws %d" % (kind, z, N2, out["undecided"]))
    assert out["undecided"] == 0
    assert z <= Z_BOUND


def test_zero_rate_nan_rate_and_mask():
    parent, blen, leaf = sim.caterpillar(5)
    model = sim.eigen_system(PI, EXCH)
    n = 200
    rates = np.zeros(n)
    rates[150:160] = np.nan
    rates[160:170] = -1.0
    rates[170:180] = np.inf
    out = sim.simulate_locus(parent, blen, leaf, 5, model, rates, stream_id=0, b=2, seed=5)
    st = out["states"]
    const = np.all(st[:, :150] == st[0:1, :150], axis=0) & np.isin(st[0, :150], [1, 2, 4, 8])
    print("r = 0: %d of 150 columns constant; root states seen: %s; bad-rate cells that are 15: %d of %d"
          % (const.sum(), sorted(set(st[0, :150].tolist())), (st[:, 150:180] == 15).sum(), 5 * 30))
    assert const.all()
    assert len(set(st[0, :150].tolist())) == 4          # the root's state still varies with the column
    assert np.all(st[:, 150:180] == 15)
    # masked cells pass through, every other cell is a single base; the draws are the same with and without the mask
    rng = np.random.default_rng(3)
    rates = np.full(n, 0.5)
    mask = rng.choice(np.array([1, 2, 4, 8, 15, 0, 5, 10, 14], np.uint8), size=(5, n))
    free = sim.simulate_locus(parent, blen, leaf, 5, model, rates, stream_id=7, b=1, seed=9)["states"]
    got = sim.simulate_locus(parent, blen, leaf, 5, model, rates, stream_id=7, b=1, seed=9, mask=mask)["states"]
    through = ~np.isin(mask, [1, 2, 4, 8])
    print("mask: %d cells copied through, %d simulated" % (through.sum(), (~through).sum()))
    assert np.array_equal(got[through], np.where(mask == 0, 15, mask)[through])
    assert np.array_equal(got[~through], free[~through])
    assert np.all(np.isin(free, [1, 2, 4, 8]))


def _argv(tmp_path, *extra):
    aln = tmp_path / "aln"
    aln.mkdir(exist_ok=True)
    tree = tmp_path / "tree.newick"
    tree.write_text("((a:1,b:1):1,c:2);\n")
    return [str(aln), str(tree), "--output", str(tmp_path), "--times", "1", "--intervals", "0-1"] + list(extra)


@pytest.mark.parametrize("extra, word", [
    (["--parametric-bootstrap", "8", "--site-rates"], "--site-rates"),
    (["--parametric-bootstrap", "8", "--rate-estimator", "eb"], "--rate-estimator eb"),
    (["--parametric-bootstrap", "8", "--gamma-categories", "4"], "--gamma-categories"),
    (["--parametric-bootstrap", "1"], "2..4096"),
    (["--parametric-bootstrap", "4097"], "2..4096"),
    (["--parametric-bootstrap-seed", "3"], "needs --parametric-bootstrap"),
    (["--parametric-bootstrap-level", "0.9"], "needs --parametric-bootstrap"),
    (["--parametric-bootstrap", "8", "--parametric-bootstrap-level", "1.0"], "(0, 1)"),
])
def test_parser_refuses(tmp_path, capsys, extra, word):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args(_argv(tmp_path, *extra))
    err = capsys.readouterr().err
    print("exit %s: %s" % (e.value.code, err.strip().splitlines()[-1]))
    assert e.value.code == 2
    assert word in err


def test_parser_accepts_and_fills_defaults(tmp_path):
    from tapir_amd import cli
    args = cli.get_args(_argv(tmp_path, "--parametric-bootstrap", "100", "--bootstrap", "50"))
    print(args.parametric_bootstrap, args.parametric_bootstrap_seed, args.parametric_bootstrap_level, args.bootstrap)
    assert (args.parametric_bootstrap, args.parametric_bootstrap_seed, args.parametric_bootstrap_level) == (100, 1, 0.95)
    assert args.bootstrap == 50   # the two bootstraps may be combined
    plain = cli.get_args(_argv(tmp_path))
    assert plain.parametric_bootstrap == 0 and plain.parametric_bootstrap_seed is None


@pytest.mark.parametrize("kind", ["gtr", "f81"])
def test_all_loci_together_equal_locus_by_locus(kind):
    """simulate_all_loci (what the byte comparison of the large trees uses) against simulate on the inputs of that comparison:
    yule70 with the loci, stream ids, rates and mask of the large trees, and the first of the large trees cut to its first four
    loci.  No draw is undecided in either, so the bytes must be the same."""
    import test_gpu_simulate as tgs
    c = tgs.byte_case("yule70", kind)
    big = tgs.byte_case("yule770", kind)
    cut = dict(big, off=big["off"][:5], models=big["models"][:4], rates=big["rates"][:int(big["off"][4])], ids=big["ids"][:4],
               mask=big["mask"][:, :int(big["off"][4])])
    for name, case, ids in (("yule70", c, c["ids"]), ("yule770, four loci", cut, cut["ids"])):
        for b, seed, m in [tgs.RUNS[k] for k in tgs.BIG_RUNS]:
            args = (case["parent"], case["blen"], case["leaf"], case["ntaxa"], case["off"], case["models"], case["rates"])
            kw = dict(locus_ids=ids, b=b, seed=seed, mask=case["mask"] if m else None)
            one, all_ = sim.simulate(*args, **kw), sim.simulate_all_loci(*args, **kw)
            print("%s %s b=%d mask=%s: %d cells, %d differ; undecided %d and %d of %d draws"
                  % (name, kind, b, m, one["states"].size, (one["states"] != all_["states"]).sum(), one["undecided"], all_["undecided"],
                     one["draws"]))
            assert one["undecided"] == 0 and all_["undecided"] == 0 and one["draws"] == all_["draws"]
            assert np.array_equal(one["states"], all_["states"]) and one["sure"].all() and all_["sure"].all()

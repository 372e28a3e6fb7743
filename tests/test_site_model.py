"""--site-model jc / f81 (Jukes-Cantor and F81 site-rate models) on the host side: command line, the C ABI's plan
descriptor as the ctypes binding mirrors it, and the pipeline end to end with the CPU stand-in engine."""
import json
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)


def _argv(tmp_path, golden_dir, *extra):
    aln = tmp_path / "aln"
    aln.mkdir(exist_ok=True)
    shutil.copy(os.path.join(golden_dir, "chr1_918.nex"), aln)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    return [str(aln), os.path.join(golden_dir, "Euteleost.tree"), "--output", str(out), "--times", "10,20,50",
            "--intervals", "0-10,10-15,20-100"] + list(extra)


def test_site_model_flag_parses(tmp_path, golden_dir):
    from tapir_amd import cli
    assert cli.get_args(_argv(tmp_path, golden_dir)).site_model == "locus"
    for m in ("locus", "jc", "f81"):
        assert cli.get_args(_argv(tmp_path, golden_dir, "--site-model", m)).site_model == m
    args = cli.get_args(_argv(tmp_path, golden_dir, "--site-model", "jc", "--gamma-categories", "4", "--reference-start",
                              "--full-precision-rates", "--integral-mode", "closed"))
    assert (args.site_model, args.gamma_categories, args.reference_start, args.full_precision_rates) == ("jc", 4, True, True)
    with pytest.raises(SystemExit) as e:
        cli.get_args(_argv(tmp_path, golden_dir, "--site-model", "hky"))
    assert e.value.code == 2


@pytest.mark.parametrize("model", ["jc", "f81"])
@pytest.mark.parametrize("conflict", [["--exchangeabilities", "1,1,1,1,1,1"], ["--subs-model", "x.tsv"], ["--site-rates"]])
def test_site_model_conflicts_are_argparse_errors(tmp_path, golden_dir, capsys, model, conflict):
    from tapir_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.get_args(_argv(tmp_path, golden_dir, "--site-model", model, *conflict))
    assert e.value.code == 2
    assert "--site-model" in capsys.readouterr().err
    cli.get_args(_argv(tmp_path, golden_dir, "--site-model", "locus", *conflict))   # the default combines with all of them


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "tphip.h"
#define F(name) printf("%s %zu\n", #name, offsetof(tphip_plan_desc, name));
int main(void) {
    printf("sizeof %zu\n", sizeof(tphip_plan_desc));
    F(struct_size) F(device) F(ntaxa) F(nnodes) F(parent) F(branch_len) F(leaf_taxon) F(nloci) F(locus_offsets) F(pi)
    F(exch) F(T) F(times) F(n_t) F(intervals) F(n_i) F(integ_mode) F(correction) F(threshold) F(round_decimals) F(ncat)
    F(cat_rate) F(cat_weight) F(start_rule) F(pattern_dedup) F(model)
    printf("TPHIP_MODEL_GTR %d\nTPHIP_MODEL_F81 %d\nTPHIP_VERSION %d\n", TPHIP_MODEL_GTR, TPHIP_MODEL_F81, TPHIP_VERSION);
    return 0;
}
"""


def test_plan_desc_ctypes_matches_header(tmp_path):
    """The ctypes PlanDesc against the C compiler's layout of include/tphip.h: every field in order, sizeof and the model
    constants."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to read include/tphip.h with")
    src = tmp_path / "probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    c = {k: int(v) for k, v in (ln.split() for ln in lines if ln.strip())}
    from tapir_amd import engine
    names = [f[0] for f in engine.PlanDesc._fields_]
    assert names[-1] == "model" and names[-2] == "pattern_dedup"
    assert ctypes_sizeof(engine.PlanDesc) == c["sizeof"]
    for n in names:
        assert getattr(engine.PlanDesc, n).offset == c[n], n
    assert [n for n in sorted(c, key=c.get) if n in names] == names   # declaration order
    assert engine.MODEL_GTR == c["TPHIP_MODEL_GTR"] == 0 and engine.MODEL_F81 == c["TPHIP_MODEL_F81"] == 1
    assert engine.MODELS == {"gtr": 0, "f81": 1}


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_plan_rejects_unknown_model_before_the_library():
    from tapir_amd import engine
    with pytest.raises(engine.TphipError):
        engine.Plan(2, [2, 2, -1], [0.1, 0.1, 0], [0, 1, -1], [0, 1], [[.25] * 4], None, 5, [1], [[0, 2]], model="hky")


def _read_outputs(outdir):
    doc = json.load(open(os.path.join(outdir, "chr1_918.nex.rates")))["sites"]
    conn = sqlite3.connect(os.path.join(outdir, "phylogenetic-informativeness.sqlite"))
    net = [p for _, p in conn.execute("select time, pi from net order by time")]
    disc = dict(conn.execute("select time, pi from discrete"))
    iv = {k: (p, e) for k, p, e in conn.execute("select interval, pi, error from interval")}
    conn.close()
    return doc, net, disc, iv


@pytest.mark.parametrize("model", ["jc", "f81"])
def test_cli_fixed_site_model_with_oracle_engine(golden_dir, tmp_path, oracle, capsys, model):
    """chr1_918 + Euteleost through the command line with --site-model: no stage 1, an F81 plan, a `.rates` header with the
    model actually used, and rates / sqlite rows equal to the oracle's (pi, exchangeabilities of 1) pushed through the
    same rounding, culling and PI."""
    import site_model_engine
    from tapir_amd import cli, compute, newick, nexus
    site_model_engine.PLANS.clear()
    outdir = cli.main(_argv(tmp_path, golden_dir, "--site-model", model), engine_mod=site_model_engine)
    assert site_model_engine.PLANS == ["f81"]
    doc, net, disc, iv = _read_outputs(outdir)
    names, st = nexus.read_states(os.path.join(golden_dir, "chr1_918.nex"))
    if model == "jc":
        pi = np.full(4, 0.25)
    else:
        pi = nexus.base_frequencies_from_histogram(oracle_engine_histogram(st))[0]
        assert not np.allclose(pi, 0.25)
    assert [doc["freqs"][b] for b in "ACGT"] == list(pi)
    assert [doc["subs_matrix"][k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")] == [1.0] * 6
    root = newick.read_tree(os.path.join(outdir, "Tree_100_174.0.newick"))
    leaf_names = [n.name for n in newick.leaves(root)]
    parent, blen, leaf = newick.to_arrays(root, leaf_names)
    st = st[[names.index(n) for n in leaf_names]]
    ref = oracle.site_rates(st, parent, blen, leaf, pi, np.ones(6))
    rate4 = compute.round_like_hyphy(ref["rate"], 4)
    rows = doc["rates"]
    assert [r["site"] for r in rows] == list(range(1, 227))
    assert np.array_equal(np.array([r["rate"] for r in rows]), rate4)
    assert np.array_equal(np.array([r["ll"] for r in rows]), compute.round_like_hyphy(ref["lnl"], 4))
    corrected = rate4 / 100
    assert np.array_equal(np.array([r["rate"] for r in doc["corrected_rates"]]), corrected)
    rates = corrected.copy()
    rates[ref["nres"] < 3] = np.nan
    pi_net, pi_times, pi_epochs = oracle.worker_tables(rates, 174, [10, 20, 50], [[0, 10], [10, 15], [20, 100]])
    assert np.allclose(net, pi_net, rtol=1e-12, atol=1e-300)
    assert set(disc) == {10, 20, 50} and all(abs(disc[t] - pi_times[t]) <= 1e-12 * abs(pi_times[t]) for t in disc)
    for k in ("0-10", "10-15", "20-100"):
        assert abs(iv[k][0] - pi_epochs[k]["sum(integral)"]) <= 1e-9 * pi_epochs[k]["sum(integral)"]
    # the model changes the answer: the locus' GTR model gives other rates
    gtr = oracle.site_rates(st, parent, blen, leaf, pi, [0.96, 1, 0.58, 0.36, 1.87, 0.51])
    assert np.abs(gtr["rate"] - ref["rate"]).max() > 1e-3


def oracle_engine_histogram(st):
    import oracle_engine
    return oracle_engine.state_histogram(st, [0, st.shape[1]])


def test_pipeline_rejects_model_with_exchangeabilities(golden_dir):
    import site_model_engine
    from tapir_amd import pipeline
    with pytest.raises(pipeline.PipelineError):
        pipeline.run_alignments([os.path.join(golden_dir, "chr1_918.nex")],
                                pipeline.Run(["a"], [1, -1], [0.1, 0], [0, -1], 5, [1], [[0, 2]], 1.0, 3), np.ones(6), engine_mod=site_model_engine, site_model="jc")
    with pytest.raises(pipeline.PipelineError):
        pipeline.run_alignments([os.path.join(golden_dir, "chr1_918.nex")],
                                pipeline.Run(["a"], [1, -1], [0.1, 0], [0, -1], 5, [1], [[0, 2]], 1.0, 3), None, engine_mod=site_model_engine, site_model="k80")

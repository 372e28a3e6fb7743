"""The output layout of the stage-1 gradient at its edges: lnl | sum_dlogt | dexch[6] | dlogt[nn]? | d2logt[nn]? (GradOutLayout,
csrc/locus_launch_plan.hpp), through both gradient kernels, with and without the column split, in the four call forms that ask for
dlogt and d2logt both, either alone, or neither.  Run with -m gpu on the MI355X box.

  host wrapper + the plan's alignment cache   locus_grad2_kernel, staged and unpacked with items = ncand
  locus_gradient_dev on the caller's tensor   locus_grad_kernel
  loci of 100 columns                         nsplit = 1: the kernels write the caller's arrays directly
  loci of 300 columns                         nsplit = 3: partial sums with items = ncand * nsplit, then split_sum_kernel

An optional output only adds stores, and the partial sums are added up in a fixed order, so every shared output is the same to the
bit whichever optional outputs are asked for (observed so at the commit before the layout got its single owner:
profiles/r15_locus_layout_parent.txt).  A slip in one copy of the offsets shows as a changed or untouched array: on the
device path every output starts as NaN.  The host wrapper's lnl is that of locus_loglik to the bit as well (locus_value_kernel: the same transition
matrices and the same forward sweep over the same slices), also observed at that commit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NTAXA, NLOCI, NCAND = 8, 3, 4
FORMS = {"both": (True, True), "dlogt": (True, False), "d2logt": (False, True), "neither": (False, False)}


def _run(cols):
    import torch
    from tapir_amd import engine, synth
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    d = synth.simulate(NLOCI, cols, NTAXA, 11)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy()
    plan = engine.Plan(NTAXA, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], d["pi"], d["exch"], pin["T"], [1], [[0, 1]],
                       correction=pin["correction"])
    nn = len(pin["parent"])
    base = np.asarray(pin["blen"]) / pin["correction"] * 0.01
    vecs = np.stack([base, base * 1.7])
    locus = np.array([0, 1, 2, 1], np.int32)
    exch = np.asarray(d["exch"])[locus] * np.array([1.0, 0.8, 1.3, 2.0])[:, None]
    vec = np.array([0, 1, 0, 1], np.int32)
    scale = np.array([1.0, 0.9, 1.2, 1.0])
    pidx = np.array([-1, 2, -1, 5], np.int32)
    pfac = np.array([1.0, 1.5, 1.0, 0.5])
    out = {"nn": nn}
    cache = plan.device_cache()
    for form, (want_dlogt, want_d2) in FORMS.items():
        r = plan.locus_gradient(st, vecs, locus, exch, vec, scale, pidx, pfac, cache=cache, per_branch=want_dlogt, curvature=want_d2)
        out["host", form] = dict(lnl=r[0], sum_dlogt=r[3], dexch=r[1], dlogt=r[2], d2logt=r[4] if want_d2 else None)
    out["host", "loglik"] = plan.locus_loglik(st, vecs, locus, exch, vec, scale, pidx, pfac, cache=cache)
    cache.release()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_st, d_vecs, d_locus, d_exch, d_vec, d_scale, d_pidx, d_pfac = (t(a) for a in (st, vecs, locus, exch, vec, scale, pidx, pfac))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)   # noqa: E731
    for form, (want_dlogt, want_d2) in FORMS.items():
        o = dict(lnl=nan(NCAND), sum_dlogt=nan(NCAND), dexch=nan(NCAND, 6), dlogt=nan(NCAND, nn) if want_dlogt else None,
                 d2logt=nan(NCAND, nn) if want_d2 else None)
        plan.locus_gradient_dev(d_st.data_ptr(), NCAND, d_locus, d_exch, d_vecs, d_vec, d_scale, d_pidx, d_pfac, o["lnl"], o["dexch"],
                                o["dlogt"], o["sum_dlogt"], o["d2logt"])
        torch.cuda.synchronize()
        out["dev", form] = {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}
    plan.close()
    return out


@pytest.fixture(scope="module")
def runs():
    return {cols: _run(cols) for cols in (100, 300)}


def _diff(a, b):
    """Largest |a - b| (NaN counts as infinite), printed before anything is asserted."""
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.where(np.isnan(d), np.inf, d).max())


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("cols", [100, 300])
def test_shared_outputs_do_not_depend_on_the_optional_ones(runs, cols, path):
    full = runs[cols][path, "both"]
    for k in ("lnl", "sum_dlogt", "dexch", "dlogt", "d2logt"):
        assert np.all(np.isfinite(full[k])), (cols, path, k)
    assert full["dlogt"].shape == full["d2logt"].shape == (NCAND, runs[cols]["nn"])
    for form in ("dlogt", "d2logt", "neither"):
        got = runs[cols][path, form]
        for k in ("lnl", "sum_dlogt", "dexch"):
            print("cols %d %s %s vs both: %s max|diff| %.3e" % (cols, path, form, k, _diff(got[k], full[k])))
            assert got[k].tobytes() == full[k].tobytes(), (cols, path, form, k)


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("cols", [100, 300])
def test_each_optional_output_with_and_without_the_other(runs, cols, path):
    full = runs[cols][path, "both"]
    for k in ("dlogt", "d2logt"):
        alone = runs[cols][path, k][k]
        print("cols %d %s: %s alone vs with the other: max|diff| %.3e" % (cols, path, k, _diff(alone, full[k])))
        assert alone.tobytes() == full[k].tobytes(), (cols, path, k)
    assert runs[cols][path, "dlogt"]["d2logt"] is None and runs[cols][path, "d2logt"]["dlogt"] is None
    # the two are different quantities: a slip that hands one array's offset to the other does not go unseen
    assert not np.array_equal(full["dlogt"], full["d2logt"])


@pytest.mark.parametrize("cols", [100, 300])
def test_host_gradient_lnl_is_locus_loglik(runs, cols):
    val = runs[cols]["host", "loglik"]
    for form in FORMS:
        lnl = runs[cols]["host", form]["lnl"]
        err = float(np.max(np.abs(lnl - val) / np.maximum(1.0, np.abs(val))))
        print("cols %d host %s: lnl vs locus_loglik: rel %.3e, byte-equal %s" % (cols, form, err, lnl.tobytes() == val.tobytes()))
        assert lnl.tobytes() == val.tobytes(), (cols, form, err)

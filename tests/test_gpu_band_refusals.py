"""What the three replicate-band families (site bootstrap, parametric bootstrap, posterior PI) refuse, with which code and in
which words: the C ABI's texts, pinned one by one.  One plan of 4 taxa with loci of 10 and 0 columns, T = 5, one interval; the
library is called through engine.load() with hand-built option structs where the Python wrapper cannot express the case (null
options, a struct_size of 8 or 24).  Every refusal is a host-side argument check that returns before any launch."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = 1, 4
FAMILIES = {
    # struct, least struct_size accepted, name in the texts, family in the texts, (code, text) of a workspace that is too small
    "bootstrap": ("BootstrapOpts", 24, "tphip_bootstrap_opts", "bootstrap",
                  (WORKSPACE, "workspace smaller than the minimum of tphip_bootstrap_workspace_bytes()")),
    "parametric": ("ParbootOpts", 24, "tphip_parboot_opts", "parametric bootstrap",
                   (INVALID, "workspace smaller than tphip_parboot_workspace_bytes()")),
    "posterior": ("PosteriorPiOpts", 40, "tphip_posterior_pi_opts", "posterior",
                  (WORKSPACE, "workspace smaller than the minimum of tphip_posterior_pi_workspace_bytes()")),
}
K = 4


@pytest.fixture(scope="module")
def setup():
    from tapir_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    parent, blen, leaf = [4, 4, 5, 5, 6, 6, -1], [0.1, 0.2, 0.3, 0.1, 0.05, 0.05, 0.0], [0, 1, 2, 3, -1, -1, -1]
    plan = engine.Plan(4, parent, blen, leaf, [0, 10, 10], np.full((2, 4), 0.25), np.ones((2, 6)), 5, [], [[1, 4]])
    yield engine, engine.load(), plan
    plan.close()


def make_opts(engine, family, struct_size=None, replicates=10, level=0.9, ids=None):
    cls = getattr(engine, FAMILIES[family][0])
    extra = dict(ncat=K) if family == "posterior" else {}
    return cls(struct_size=ctypes.sizeof(cls) if struct_size is None else struct_size, replicates=replicates, level=level, seed=3,
               locus_ids=None if ids is None else ids.ctypes.data, **extra)


def entry_points(lib, plan, family, opts):
    """The family's entry points that read the options, as calls with every array null: the options are checked first."""
    ref = None if opts is None else ctypes.byref(opts)
    h, n = plan._h, ctypes.c_size_t()
    if family == "bootstrap":     # (without options tphip_bootstrap_workspace_bytes answers for tphip_pi_resample_dev)
        sizes = [] if opts is None else [lambda: lib.tphip_bootstrap_workspace_bytes(h, ref, ctypes.byref(n), ctypes.byref(n))]
        return sizes + [lambda: lib.tphip_pi_bootstrap_dev(h, None, None, ref, None, None, None, 0, None),
                        lambda: lib.tphip_pi_bootstrap(h, None, None, ref, None, None)]
    if family == "parametric":
        return [lambda: lib.tphip_parboot_workspace_bytes(h, ref, ctypes.byref(n)),
                lambda: lib.tphip_pi_parametric_bootstrap_dev(h, None, None, ref, None, None, None, None, None, 0, None),
                lambda: lib.tphip_pi_parametric_bootstrap(h, None, None, ref, None, None, None, None)]
    return [lambda: lib.tphip_posterior_pi_workspace_bytes(h, ref, ctypes.byref(n), ctypes.byref(n)),
            lambda: lib.tphip_posterior_pi_dev(h, None, None, None, None, ref, None, None, None, None, None, None, 0, None),
            lambda: lib.tphip_posterior_pi(h, None, None, None, None, ref, None, None, None, None, None)]


def refused(lib, plan, family, opts, text):
    """Every entry point of the family that reads the options answers TPHIP_ERR_INVALID in exactly these words."""
    for call in entry_points(lib, plan, family, opts):
        rc, got = call(), lib.tphip_last_error().decode()
        print("%s: %d %s" % (family, rc, got))
        assert (rc, got) == (INVALID, text)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_options_are_refused_in_the_familys_words(setup, family):
    engine, lib, plan = setup
    _, least, struct, name, _ = FAMILIES[family]
    too_small = ("%s.struct_size is smaller than this library's struct" % struct if family == "posterior" else
                 "%s.struct_size is too small: set it to sizeof(%s)" % (struct, struct))
    refused(lib, plan, family, None, "null " + struct)
    refused(lib, plan, family, make_opts(engine, family, struct_size=8), too_small)
    refused(lib, plan, family, make_opts(engine, family, struct_size=least - 1), too_small)
    for replicates in (1, 4097):
        refused(lib, plan, family, make_opts(engine, family, replicates=replicates), "%s replicates must be in 2..4096" % name)
    for level in (0.0, 1.0, float("nan")):
        refused(lib, plan, family, make_opts(engine, family, level=level), "%s level must be in (0, 1)" % name)
    refused(lib, plan, family, make_opts(engine, family, replicates=1, level=0.0), "%s replicates must be in 2..4096" % name)
    if family == "posterior":
        for ncat in (1, 17):
            opts = make_opts(engine, family)
            opts.ncat = ncat
            refused(lib, plan, family, opts, "tphip_posterior_pi_opts.ncat must be in 2..16")
    else:      # through the end of the seed is enough
        n = ctypes.c_size_t()
        opts = make_opts(engine, family, struct_size=least)
        size_call = (lib.tphip_bootstrap_workspace_bytes(plan._h, ctypes.byref(opts), ctypes.byref(n), None) if family == "bootstrap" else
                     lib.tphip_parboot_workspace_bytes(plan._h, ctypes.byref(opts), ctypes.byref(n)))
        assert size_call == 0 and n.value > 0


def test_a_bootstrap_struct_of_24_bytes_ignores_the_ids(setup):
    engine, lib, plan = setup
    rates, ids = np.linspace(0.05, 0.5, 10), np.array([7, 9], np.int64)
    Wb = plan.bootstrap_width

    def run(opts):
        summary, rows = np.zeros((2, 4, Wb)), np.zeros((2, 10, Wb))
        assert lib.tphip_pi_bootstrap(plan._h, rates.ctypes.data, None, ctypes.byref(opts), summary.ctypes.data, rows.ctypes.data) == 0
        return rows
    short, plain = run(make_opts(engine, "bootstrap", struct_size=24, ids=ids)), run(make_opts(engine, "bootstrap"))
    with_ids = run(make_opts(engine, "bootstrap", ids=ids))
    assert np.array_equal(short, plain) and not np.array_equal(with_ids, plain)


def text_of(engine, fn):
    with pytest.raises(engine.TphipError) as e:
        fn()
    print(e.value)
    return str(e.value)


def test_one_byte_below_the_minimum_is_refused_and_the_plan_still_answers(setup):
    import torch
    engine, lib, plan = setup
    Wb, B = plan.bootstrap_width, 2
    rates, states = np.linspace(0.05, 0.5, 10), np.tile(np.array([[1], [2], [4], [8]], np.uint8), (1, 10))
    post, scale, cat = np.full((K, 10), 1.0 / K), np.ones(2), np.tile(np.array([0.2, 0.6, 1.2, 2.0]), (2, 1))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_rates, d_states, d_post, d_scale, d_cat = dev(rates), dev(states), dev(post), dev(scale), dev(cat)
    d_sum = torch.zeros((2, 4, Wb), dtype=torch.float64, device="cuda")
    d_an, d_ex = torch.zeros((2, 2, Wb), dtype=torch.float64, device="cuda"), torch.zeros((2, K), dtype=torch.float64, device="cuda")
    need = {"bootstrap": plan.bootstrap_workspace_bytes(B)[0], "parametric": plan.parboot_workspace_bytes(B),
            "posterior": plan.posterior_pi_workspace_bytes(K, B)[0]}
    d_ws = torch.zeros(max(need.values()), dtype=torch.uint8, device="cuda")
    calls = {
        "bootstrap": lambda n: plan.pi_bootstrap_dev(d_rates, None, d_sum, None, d_ws, B, ws_bytes=n),
        "parametric": lambda n: plan.pi_parametric_bootstrap_dev(d_rates, d_states, d_sum, None, None, None, d_ws, B, ws_bytes=n),
        "posterior": lambda n: plan.posterior_pi_dev(d_post, None, d_scale, d_cat, K, d_an, d_ex, d_sum, None, None, d_ws, B, ws_bytes=n),
    }
    for family in sorted(FAMILIES):
        code, text = FAMILIES[family][4]
        assert text_of(engine, lambda: calls[family](need[family] - 1)) == "libtphip error %d: %s" % (code, text)
    for family in sorted(FAMILIES):      # the plan still answers, at exactly the minimum
        calls[family](need[family])
        torch.cuda.synchronize()
        assert np.all(np.isfinite(d_sum.cpu().numpy()[0]))

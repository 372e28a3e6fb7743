"""The `_dev` entry points of include/tphip.h held to their buffer and stream contract ("the `_dev` boundary").

Every other GPU file hands them freshly allocated, over-aligned, padded torch tensors, a fresh workspace and the default
stream.  Here one case table names every `_dev` entry point; the PLAIN call of a case is that kind of call (separate tensors,
default stream, a zero-filled workspace), which the feature files pin to their references, and every variant below must equal
it bit for bit, with the arrays cut out of one device buffer between 4096-byte guard bands (tests/abi_arena.py):

  V1  extents: every array on a multiple of 256, outputs pre-filled with the band's pattern (zeroed where the header asks for
      zeros on entry), the workspace exactly the bytes the call's own size function states: no band byte changes;
  V2  workspace content: V1 with the workspace pre-filled with 0x00, 0xFF and 0xA5: the same bits three times;
  V3  natural alignment: every data array at the alignment of its element type and no better (address = itemsize mod 16, bytes
      at an odd address), the workspace at exactly the alignment the header states (16 for the plan workspace, 8 for the quartet
      calls, an odd address for the replicate-band calls, which round up inside min_bytes);
  V4  refusals: a call that states a workspace alignment gets one a byte off: TPHIP_ERR_INVALID naming the alignment, and
      every output still holds the pattern -- nothing was launched;
  V5  stream order: on a non-blocking side stream (the flag is read back), filler work, then the copies of the real inputs over
      poison (states 15, rates and planes NaN, nres 0), then the call, then clones of the outputs; the null stream stays idle.
      A launch, memset or copy the library put on the null stream runs before the inputs arrive and shows as poison in the
      result.  V5 catches such an operation ONLY WHEN IT OVERTAKES THE INPUTS: the filler (measured with events to be at least
      10 x the plain call, which is measured the same way) makes that near certain; it is not a proof.  Arrays whose values are
      indices, offsets or sizes (candidate indices, locus offsets, 16-bit counts) are uploaded beforehand and never poisoned: a
      mis-ordered kernel reads wrong values, never out-of-range ones.

Shapes: a 16-taxon Yule tree, T = 17, two times, five intervals; loci S4 = [64, 4, 1024, 60, 256, 2052] (every offset a
multiple of 4: classify_kernel's wide path in every full thread) and S1 = [1, 63, 65, 255, 1025, 2049] (the byte path, ragged
last threads); the last locus of each is longer than 2048 columns (the long-locus kernels).  The three plan-workspace calls run
under GTR and F81 with pattern de-duplication forced off and on; everything else under GTR.

V2 runs for the cases with a workspace, V4 for those whose call states an alignment for it (the table's WS_KIND says which
and why not the others); V1, V3 and V5 run for every case.  A sub-variant of V3 for the calls that run classify_kernel on the
caller's arrays keeps the states and the workspace aligned and puts only `flag`, only `nres` or both at natural alignment:
there the kernel's look at those two pointers decides between its wide stores and its byte path.

That the file bites was observed once on an MI355X with two builds that are not kept; both give wrong bytes inside memory the
test owns, and with each build every other test of the cases named passed:
  * concordance_rows_kernel launched without its stream argument (so on the null stream): V5 of concordance_rows failed on S4
    and S1, "output rows differs from the plain call" (the rows computed from the poisoned counts); its V1 and V3 passed;
  * quartet_partial_bytes, the layout total behind tphip_quartet_workspace_bytes AND behind the driver's own size check,
    returning 64 bytes fewer: V1, V2, V3 and V5 of quartet_tables failed with check() = [('ws', 896)] on S4 (8 chunks x 3
    quartets x 5 sums x 8 bytes = 960 stated as 896) and [('ws', 1016)] on S1 (1080 stated as 1016): the first guard byte.
    V4 passed: the refusal comes before any launch.
The unmutated build: all 377 tests pass in under 6 s; the smallest filler-to-call ratio of V5 seen was 21.9 (filler sized 2.5 x
the bound; 12.9 when it was sized 1.5 x)."""
import collections
import ctypes
import math

import numpy as np
import pytest

import abi_arena
from abi_arena import PATTERN, Arena

pytestmark = pytest.mark.gpu

LAYOUTS = {"S4": [64, 4, 1024, 60, 256, 2052], "S1": [1, 63, 65, 255, 1025, 2049]}
T17, TIMES, INTERVALS = 17, [3, 11], [[0, 2], [2, 5], [5, 9], [9, 13], [13, 16]]
Q3 = [(3.0, 1.0), (12.0, 2.5), (40.0, 6.0)]                                             # (T, t_o)
U3 = [(3.0, 4.0, 2.0, 5.0, 1.0), (12.0, 9.0, 14.0, 11.0, 2.5), (40.0, 35.0, 20.0, 44.0, 6.0)]   # (Ta, Tb, Tc, Td, t_o)
ORDERS = np.array([[0, 1, 2], [5, 3, 1], [2, 4, 0]], np.int32)                          # n_k = 3
CAP, B, K, NREP = 64, 5, 4, 3
NAN = float("nan")
FILLER_MARGIN = 10.0

A = collections.namedtuple("A", "name value dtype shape role poison")   # poison None: never poisoned (an index array, an output)


def _engine():
    from tapir_amd import engine
    engine.load()
    if engine.device_count() < 1:
        pytest.fail("no usable GPU: the engine has no CPU path")
    return engine


def _torch_dtype(np_dtype):
    import torch
    return {"uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64, "float64": torch.float64}[np.dtype(np_dtype).name]


def fin(name, value, poison):
    value = np.ascontiguousarray(value)
    return A(name, value, _torch_dtype(value.dtype), value.shape, "in", poison)


def fout(name, np_dtype, shape):
    return A(name, None, _torch_dtype(np_dtype), tuple(int(d) for d in shape), "out", None)


class Case:
    """arrays; call(T, ws, stream) -> dict of host results or None, T the arrays by name; ws_bytes and ws_align (16 or 8: the
    call refuses another base; 1: a replicate-band call, any base) or neither; zero: outputs the header wants zeroed on entry."""

    def __init__(self, arrays, call, ws_bytes=None, ws_align=None, zero=()):
        self.arrays, self.call, self.ws_bytes, self.ws_align, self.zero = arrays, call, ws_bytes, ws_align, set(zero)
        assert (ws_bytes is None) == (ws_align is None)
        self.outs = [a for a in arrays if a.role == "out"]
        self.plain = None      # (bits of the outputs, host results)
        self.plain_ms = None


# ---- the batch of a layout and everything the cases take as inputs, computed once on the host-pointer path ------------------
class World:
    def __init__(self, layout):
        from tapir_amd import eb, synth
        self.engine = _engine()
        self.layout = layout
        sizes = LAYOUTS[layout]
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n, self.L = int(self.off[-1]), len(sizes)
        root, names = synth.yule_tree(16, 20261021)
        self.pin = synth.plan_inputs(root, names)
        d = synth.simulate(1, self.n, 16, 77, tree=(root, names), rate_mean=0.02)
        st = d["states"].numpy().copy()
        rng = np.random.default_rng(5)
        lo, hi = int(self.off[-2]), int(self.off[-1])             # the long locus repeats its first 300 columns: patterns to find
        st[:, lo + 300:hi] = st[:, lo + rng.integers(0, 300, hi - lo - 300)]
        st[rng.integers(0, 16, 40), rng.integers(0, self.n, 40)] = rng.choice([3, 5, 10, 0], 40)   # IUPAC unions and 0 (= 15)
        self.states = np.ascontiguousarray(st)
        self.pi, self.exch = synth.locus_parameters(self.L, 31)
        self._plans, self._memo = {}, {}
        self.rho, self.wgt = eb.gamma_tables([0.7] * self.L, K)
        self.mu = eb.start_scales(self.states, self.off, self.pin["parent"], self.pin["blen"], self.pin["leaf"])

    def plan(self, model="gtr", dedup=None):
        e = self.engine
        dedup = e.DEDUP_AUTO if dedup is None else dedup
        if (model, dedup) not in self._plans:
            self._plans[model, dedup] = e.Plan(16, self.pin["parent"], self.pin["blen"], self.pin["leaf"], self.off, self.pi,
                                               None if model == "f81" else self.exch, T17, TIMES, INTERVALS,
                                               correction=self.pin["correction"], pattern_dedup=dedup, model=model)
        return self._plans[model, dedup]

    def close(self):
        for p in self._plans.values():
            p.close()

    def memo(self, key, make):
        if key not in self._memo:
            v = make()
            for a in (v.values() if isinstance(v, dict) else v if isinstance(v, (tuple, list)) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    @property
    def site(self):
        return self.memo("site", lambda: self.plan().run_fused(self.states))

    @property
    def table(self):
        return self.memo("table", lambda: self.plan().eb_posterior_table(self.states, self.rho, self.wgt, self.mu))

    @property
    def eq_sites(self):
        return self.memo("eq_sites", lambda: self.plan().quartet_sites(self.site["rate"], self.site["nres"], Q3))

    @property
    def un_sites(self):
        return self.memo("un_sites", lambda: self.plan().unequal_quartet_sites(self.site["rate"], self.site["nres"], U3))

    @property
    def eq_rows(self):
        return self.memo("eq_rows", lambda: self.plan().quartet_tables(self.site["rate"], self.site["nres"], Q3))

    @property
    def un_rows(self):
        return self.memo("un_rows", lambda: self.plan().unequal_quartet_tables(self.site["rate"], self.site["nres"], U3))

    @property
    def boot_rows(self):
        return self.memo("boot_rows", lambda: self.plan().pi_bootstrap(self.site["rate"], self.site["nres"], replicates=B, seed=3,
                                                                       return_rows=True)[1])

    @property
    def conc(self):
        def make():
            from tapir_amd import compute, newick, synth
            root, _ = synth.yule_tree(9, 3)
            names = [leaf.name for leaf in newick.leaves(root)]
            sets = compute.concordance_sets(compute.tree_concordance_groups(root), names)
            states9 = np.ascontiguousarray(self.states[:9])
            counts = self.engine.concordance_counts(states9, self.off, sets["group_offsets"], sets["group_taxa"])
            return dict(sets=sets, states=states9, counts=counts.view(np.int64))
        return self.memo("conc", make)


_WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def _worlds():
    yield
    for w in _WORLDS.values():
        w.close()
    _WORLDS.clear()
    _CASES.clear()


_FAULTED = []


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    """A HIP error is sticky: once a test has met one, the tests after it start nothing more on the device."""
    import torch
    if _FAULTED:
        pytest.fail("not run: an earlier test of this file met a HIP error (%s)" % _FAULTED[0])
    yield
    try:
        torch.cuda.synchronize()
    except Exception as exc:   # noqa: BLE001 (whatever the runtime raises, the device is not to be used again)
        _FAULTED.append(str(exc).splitlines()[0] if str(exc) else type(exc).__name__)
        raise


def world(layout):
    if layout not in _WORLDS:
        _WORLDS[layout] = World(layout)
    return _WORLDS[layout]


# ---- the case table ----------------------------------------------------------------------------------------------------------
def _percol_outs(n):
    return [fout("rate", np.float64, (n,)), fout("subst", np.float64, (n,)), fout("lnl", np.float64, (n,)), fout("flag", np.uint8, (n,)),
            fout("nres", np.int32, (n,))]


def c_site_rates(w, model, dedup):
    p = w.plan(model, dedup)
    return Case([fin("states", w.states, 15)] + _percol_outs(w.n),
                lambda T, ws, s: p.site_rates_dev(T["states"], T["rate"], T["subst"], T["lnl"], T["flag"], T["nres"], ws, s),
                ws_bytes=p.workspace_bytes, ws_align=16)


def c_pi_tables(w, model, dedup):
    p = w.plan(model, dedup)
    return Case([fin("rates", w.site["rate"], NAN), fin("nres", w.site["nres"], 0), fout("tables", np.float64, (w.L, p.width))],
                lambda T, ws, s: p.pi_tables_dev(T["rates"], T["nres"], T["tables"], ws, s), ws_bytes=p.workspace_bytes, ws_align=16)


def c_run(w, model, dedup):
    p = w.plan(model, dedup)
    return Case([fin("states", w.states, 15)] + _percol_outs(w.n) + [fout("tables", np.float64, (w.L, p.width))],
                lambda T, ws, s: p.run_dev(T["states"], T["rate"], T["subst"], T["lnl"], T["flag"], T["nres"], T["tables"], ws, s),
                ws_bytes=p.workspace_bytes, ws_align=16)


def c_corrected_rates(w):
    p = w.plan()
    return Case([fin("rates", w.site["rate"], NAN), fin("nres", w.site["nres"], 0), fout("out", np.float64, (w.n,))],
                lambda T, ws, s: p.corrected_rates_dev(T["rates"], T["nres"], T["out"], s))


def _lib_call(w, name, *args):
    e = w.engine
    e._check(getattr(e.load(), name)(*args))


def c_townsend_dense(w):
    rates = w.plan().corrected_rates(w.site["rate"], w.site["nres"])
    times = np.array([0.0, 1.0, 2.5, 16.0])
    return Case([fin("rates", rates, NAN), fin("times", times, NAN), fout("out", np.float64, (len(times), w.n))],
                lambda T, ws, s: _lib_call(w, "tphip_townsend_pi_dense_dev", 0, T["rates"].data_ptr(), w.n, T["times"].data_ptr(), len(times),
                                           T["out"].data_ptr(), s))


def c_quad_townsend(w):
    rates = w.plan().corrected_rates(w.site["rate"], w.site["nres"])
    return Case([fin("rates", rates, NAN), fout("integral", np.float64, (w.n,)), fout("abserr", np.float64, (w.n,))],
                lambda T, ws, s: _lib_call(w, "tphip_quad_townsend_dev", 0, T["rates"].data_ptr(), w.n, 2.0, 9.0, w.engine.INTEG_QUADPACK,
                                           T["integral"].data_ptr(), T["abserr"].data_ptr(), s))


def c_state_histogram(w):
    return Case([fin("states", w.states, 15), fin("offsets", w.off, None), fout("hist", np.int64, (w.L, 16))],
                lambda T, ws, s: _lib_call(w, "tphip_state_histogram_dev", 0, T["states"].data_ptr(), w.n, 16, T["offsets"].data_ptr(), w.L,
                                           T["hist"].data_ptr(), s))


def c_eval_columns(w):
    p = w.plan()
    u = np.random.default_rng(9).normal(-3.0, 1.0, w.n)
    return Case([fin("states", w.states, 15), fin("u", u, NAN)] + [fout(k, np.float64, (w.n,)) for k in "fgh"],
                lambda T, ws, s: p.eval_columns_dev(T["states"], T["u"], T["f"], T["g"], T["h"], s))


def _candidates(w):
    nn = len(w.pin["parent"])
    locus = np.array([0, 1, 2, 3, 4, 5, 2, 4], np.int32)
    ins = [fin("states", w.states, 15), fin("cand_locus", locus, None), fin("cand_exch", w.exch[locus], NAN),
           fin("blen_vecs", np.stack([w.pin["blen"] * 0.5, w.pin["blen"] * 1.25]), NAN),
           fin("cand_vec", np.array([0, 1, 0, 1, 0, 1, 1, 0], np.int32), None), fin("cand_scale", np.linspace(0.9, 1.1, 8), NAN),
           fin("cand_pidx", np.array([-1, -1, 3, -1, 7, -1, nn - 2, 0], np.int32), None), fin("cand_pfac", np.linspace(0.98, 1.03, 8), NAN)]
    return ins, 8, nn


def c_locus_loglik(w):
    p = w.plan()
    ins, n, nn = _candidates(w)
    return Case(ins + [fout("out", np.float64, (n,))],
                lambda T, ws, s: p.locus_loglik_dev(T["states"].data_ptr(), n, T["cand_locus"], T["cand_exch"], T["blen_vecs"], T["cand_vec"],
                                                    T["cand_scale"], T["cand_pidx"], T["cand_pfac"], T["out"], s))


def c_locus_gradient(w):
    p = w.plan()
    ins, n, nn = _candidates(w)
    outs = [fout("lnl", np.float64, (n,)), fout("dexch", np.float64, (n, 6)), fout("dlogt", np.float64, (n, nn)),
            fout("sum_dlogt", np.float64, (n,)), fout("d2logt", np.float64, (n, nn))]
    return Case(ins + outs,
                lambda T, ws, s: p.locus_gradient_dev(T["states"].data_ptr(), n, T["cand_locus"], T["cand_exch"], T["blen_vecs"], T["cand_vec"],
                                                      T["cand_scale"], T["cand_pidx"], T["cand_pfac"], T["lnl"], T["dexch"], T["dlogt"],
                                                      T["sum_dlogt"], T["d2logt"], s))


def c_stage1_fit(w):
    """outputs are host arrays: the device input alone is guarded; the call synchronises by contract"""
    p, e = w.plan(), w.engine
    nn = len(w.pin["parent"])

    def call(T, ws, s):
        opts = e.Stage1Opts(struct_size=ctypes.sizeof(e.Stage1Opts), maxit_grm=4, maxit_sub=2)
        out = dict(exch=np.empty((w.L, 6)), pi=np.empty((w.L, 4)), weights=np.empty((w.L, 203)), lnl=np.empty((w.L, 203)),
                   model_exch=np.empty((w.L, 203, 6)), grm_blen=np.empty((w.L, nn)), grm_iters=np.empty(w.L, np.int32),
                   sub_iters=np.empty((w.L, 202), np.int32), stats=np.zeros(8, np.int64))
        e._check(e.load().tphip_stage1_fit_dev(p._h, T["states"].data_ptr(), ctypes.byref(opts), *[out[k].ctypes.data for k in
                                               ("exch", "pi", "weights", "lnl", "model_exch", "grm_blen", "grm_iters", "sub_iters", "stats")], s))
        return out
    return Case([fin("states", w.states, 15)], call)


def c_eb_start_scale(w):
    p = w.plan()
    return Case([fin("states", w.states, 15)], lambda T, ws, s: dict(scale=p.eb_start_scale_dev(T["states"], stream=s)))


def c_eb_fit_scale(w):
    p = w.plan()
    return Case([fin("states", w.states, 15)], lambda T, ws, s: p.eb_fit_scale_dev(T["states"], w.rho, w.wgt, w.mu, maxit_scale=6, stream=s))


def _eb_outs(n):
    return [fout("rate", np.float64, (n,)), fout("sd", np.float64, (n,)), fout("lnl", np.float64, (n,)), fout("nres", np.int32, (n,))]


def c_eb_posterior(w):
    p = w.plan()
    return Case([fin("states", w.states, 15)] + _eb_outs(w.n),
                lambda T, ws, s: p.eb_posterior_dev(T["states"], w.rho, w.wgt, w.mu, T["rate"], T["sd"], T["lnl"], T["nres"], stream=s))


def c_eb_posterior_table(w):
    p = w.plan()
    return Case([fin("states", w.states, 15), fout("post", np.float64, (K, w.n))] + _eb_outs(w.n),
                lambda T, ws, s: p.eb_posterior_table_dev(T["states"], w.rho, w.wgt, w.mu, T["post"], T["rate"], T["sd"], T["lnl"], T["nres"],
                                                          stream=s))


IDS = np.array([7, 1 << 40, 3, 900, 2, 11], np.int64)   # stream ids: with them the band calls synchronise by contract


def c_posterior_pi(w, ids):
    p = w.plan()
    Wb = p.bootstrap_width
    arrays = [fin("post", w.table["post"], NAN), fin("nres", w.table["nres"], 0), fin("scale", w.mu, NAN), fin("cat_rate", w.rho, NAN),
              fout("analytic", np.float64, (w.L, 2, Wb)), fout("expected", np.float64, (w.L, K)), fout("summary", np.float64, (w.L, 4, Wb)),
              fout("rows", np.float64, (w.L, B, Wb)), fout("counts", np.int32, (w.L, B, K))]
    return Case(arrays, lambda T, ws, s: p.posterior_pi_dev(T["post"], T["nres"], T["scale"], T["cat_rate"], K, T["analytic"], T["expected"],
                                                            T["summary"], T["rows"], T["counts"], ws, B, seed=11,
                                                            locus_ids=IDS if ids else None, stream=s),
                ws_bytes=p.posterior_pi_workspace_bytes(K, B)[0], ws_align=1)


def c_pi_resample(w):
    p = w.plan()
    counts = np.random.default_rng(2).integers(0, 3, (NREP, w.n)).astype(np.int16)
    return Case([fin("rates", w.site["rate"], NAN), fin("nres", w.site["nres"], 0), fin("counts", counts, None),
                 fout("rows", np.float64, (w.L, NREP, p.bootstrap_width))],
                lambda T, ws, s: p.pi_resample_dev(T["rates"], T["nres"], T["counts"], NREP, T["rows"], ws, s),
                ws_bytes=p.resample_workspace_bytes()[0], ws_align=1)


def c_pi_bootstrap(w, ids):
    p = w.plan()
    Wb = p.bootstrap_width
    return Case([fin("rates", w.site["rate"], NAN), fin("nres", w.site["nres"], 0), fout("summary", np.float64, (w.L, 4, Wb)),
                 fout("rows", np.float64, (w.L, B, Wb))],
                lambda T, ws, s: p.pi_bootstrap_dev(T["rates"], T["nres"], T["summary"], T["rows"], ws, B, seed=5,
                                                    locus_ids=IDS if ids else None, stream=s),
                ws_bytes=p.bootstrap_workspace_bytes(B)[0], ws_align=1)


def c_simulate_columns(w):
    p = w.plan()
    return Case([fin("rates", w.site["rate"], NAN), fin("mask", w.states, 15), fout("states_out", np.uint8, (16, w.n))],
                lambda T, ws, s: p.simulate_columns_dev(T["rates"], T["mask"], T["states_out"], replicate=2, seed=9, stream=s))


def c_parametric_bootstrap(w):
    p = w.plan()
    Wb = p.bootstrap_width
    return Case([fin("rates", w.site["rate"], NAN), fin("states", w.states, 15), fout("summary", np.float64, (w.L, 4, Wb)),
                 fout("rows", np.float64, (w.L, B, Wb)), fout("rate_mean", np.float64, (w.n,)), fout("rate_sd", np.float64, (w.n,))],
                lambda T, ws, s: p.pi_parametric_bootstrap_dev(T["rates"], T["states"], T["summary"], T["rows"], T["rate_mean"], T["rate_sd"],
                                                               ws, B, seed=4, stream=s),
                ws_bytes=p.parboot_workspace_bytes(B), ws_align=1)


def c_summarize_rows(w):
    rows = w.boot_rows
    L, Bn, Wb = rows.shape
    return Case([fin("rows", rows, NAN), fout("summary", np.float64, (L, 4, Wb))],
                lambda T, ws, s: _lib_call(w, "tphip_summarize_rows_dev", 0, T["rows"].data_ptr(), L, Bn, Wb, 0.9, T["summary"].data_ptr(), s))


def c_quartet_tables(w, unequal):
    p = w.plan()
    q, width = (U3, 13) if unequal else (Q3, 8)
    fn = p.unequal_quartet_tables_dev if unequal else p.quartet_tables_dev
    need = p.unequal_quartet_workspace_bytes(q) if unequal else p.quartet_workspace_bytes(q)
    return Case([fin("rates", w.site["rate"], NAN), fin("nres", w.site["nres"], 0), fout("rows", np.float64, (w.L, 3, width))],
                lambda T, ws, s: fn(T["rates"], T["nres"], q, T["rows"], ws, s), ws_bytes=need, ws_align=8)


def c_quartet_sites(w, unequal):
    p = w.plan()
    q, planes = (U3, 3) if unequal else (Q3, 2)
    fn = p.unequal_quartet_sites_dev if unequal else p.quartet_sites_dev
    return Case([fin("rates", w.site["rate"], NAN), fin("nres", w.site["nres"], 0), fout("sites", np.float64, (planes, 3, w.n))],
                lambda T, ws, s: fn(T["rates"], T["nres"], q, T["sites"], s))


def _planes(w):
    s = w.un_sites
    return [fin("y", s[0], NAN), fin("x1", s[1], NAN), fin("x2", s[2], NAN)]


def c_quartet_exact(w):
    p = w.plan()
    return Case(_planes(w) + [fout("rows", np.float64, (w.L, 3, 6))],
                lambda T, ws, s: p.quartet_exact_dev(T["y"], T["x1"], T["x2"], 3, T["rows"], ws, window_cap=CAP, stream=s),
                ws_bytes=p.quartet_exact_workspace_bytes(3, CAP), ws_align=8)


def c_locus_set_rows(w, unequal):
    e = w.engine
    rows = w.un_rows if unequal else w.eq_rows
    return Case([fin("locus_rows", rows, NAN), fout("rows", np.float64, ORDERS.shape + (rows.shape[2],))],
                lambda T, ws, s: e.locus_set_rows_dev(T["locus_rows"], w.L, ORDERS, T["rows"], family=int(unequal), stream=s))


def c_locus_set_exact(w):
    p = w.plan()
    return Case(_planes(w) + [fout("rows", np.float64, ORDERS.shape + (6,))],
                lambda T, ws, s: p.locus_set_exact_dev(T["y"], T["x1"], T["x2"], ORDERS, T["rows"], ws, window_cap=CAP, stream=s),
                ws_bytes=p.locus_set_exact_workspace_bytes(3, 3, CAP), ws_align=8)


def c_concordance_counts(w):
    """the counts are zeroed on entry, as the header's sums over the columns start from them"""
    c, e = w.conc, w.engine
    sets = c["sets"]
    n_sets = int(sets["node_sets"][-1])
    return Case([fin("states", c["states"], 15), fin("offsets", w.off, None), fout("counts", np.int64, (w.L, n_sets, 3))],
                lambda T, ws, s: e.concordance_counts_dev(T["states"], w.n, w.n, 9, T["offsets"], w.L, sets["group_offsets"], sets["group_taxa"],
                                                          T["counts"], stream=s),
                zero=["counts"])


def c_concordance_rows(w):
    c, e = w.conc, w.engine
    nodes = c["sets"]["node_sets"]
    return Case([fin("counts", c["counts"], 0), fout("rows", np.float64, (w.L, len(nodes) - 1, 12))],
                lambda T, ws, s: e.concordance_rows_dev(T["counts"], w.L, int(nodes[-1]), nodes, T["rows"], stream=s))


def _table():
    t = collections.OrderedDict()
    for layout in LAYOUTS:
        for model in ("gtr", "f81"):
            for dedup in (1, 2):   # engine.DEDUP_OFF, engine.DEDUP_ON
                for name, fn in (("site_rates", c_site_rates), ("pi_tables", c_pi_tables), ("run", c_run)):
                    t["%s-%s-%s-dedup%s" % (name, layout, model, "on" if dedup == 2 else "off")] = (fn, layout, (model, dedup), 16)
        for name, fn, args in (
                ("corrected_rates", c_corrected_rates, ()), ("townsend_pi_dense", c_townsend_dense, ()), ("quad_townsend", c_quad_townsend, ()),
                ("state_histogram", c_state_histogram, ()), ("eval_columns", c_eval_columns, ()), ("locus_loglik", c_locus_loglik, ()),
                ("locus_gradient", c_locus_gradient, ()), ("stage1_fit", c_stage1_fit, ()), ("eb_start_scale", c_eb_start_scale, ()),
                ("eb_fit_scale", c_eb_fit_scale, ()), ("eb_posterior", c_eb_posterior, ()), ("eb_posterior_table", c_eb_posterior_table, ()),
                ("posterior_pi", c_posterior_pi, (False,)), ("posterior_pi_ids", c_posterior_pi, (True,)), ("pi_resample", c_pi_resample, ()),
                ("pi_bootstrap", c_pi_bootstrap, (False,)), ("pi_bootstrap_ids", c_pi_bootstrap, (True,)),
                ("simulate_columns", c_simulate_columns, ()), ("pi_parametric_bootstrap", c_parametric_bootstrap, ()),
                ("summarize_rows", c_summarize_rows, ()), ("quartet_tables", c_quartet_tables, (False,)),
                ("quartet_sites", c_quartet_sites, (False,)), ("unequal_quartet_tables", c_quartet_tables, (True,)),
                ("unequal_quartet_sites", c_quartet_sites, (True,)), ("quartet_exact", c_quartet_exact, ()),
                ("locus_set_rows", c_locus_set_rows, (False,)), ("locus_set_rows_unequal", c_locus_set_rows, (True,)),
                ("locus_set_exact", c_locus_set_exact, ()), ("concordance_counts", c_concordance_counts, ()),
                ("concordance_rows", c_concordance_rows, ())):
            t["%s-%s" % (name, layout)] = (fn, layout, args, WS_KIND.get(fn))
    return t


# The workspace a case's call takes: 16 or 8 = it states that alignment and refuses another base, 1 = a replicate-band call (any
# base, it rounds up inside min_bytes), absent = no workspace.  It decides which variants exist for a case, and why not:
#   V2 (workspace content) is not run for a case without a workspace;
#   V4 (refusals) is not run for a case without a workspace, nor for a band call, which states no alignment to refuse by;
#   V1, V3 and V5 run for every case (stage1_fit, eb_start_scale and eb_fit_scale return host arrays: their device input alone is guarded).
WS_KIND = {c_posterior_pi: 1, c_pi_resample: 1, c_pi_bootstrap: 1, c_parametric_bootstrap: 1, c_quartet_tables: 8, c_quartet_exact: 8,
           c_locus_set_exact: 8}


TABLE = _table()
WITH_WORKSPACE = [k for k, v in TABLE.items() if v[3] is not None]
STATES_ALIGNMENT = [k for k, v in TABLE.items() if v[3] in (8, 16)]
WIDE_STORES = [k for k, v in TABLE.items() if v[0] in (c_site_rates, c_run)]   # the calls that run classify_kernel on caller arrays
_CASES = {}


# ---- running a case ----------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _timed(fn):
    """fn() between two events on the current stream: (its result, milliseconds until the stream has passed the second event)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def _plain_call(c):
    """separate fresh tensors, the default stream, a zero-filled workspace of the stated size"""
    import torch
    T = {}
    for a in c.arrays:
        if a.role == "in":
            T[a.name] = torch.from_numpy(a.value).cuda()
        else:
            T[a.name] = (torch.zeros if a.name in c.zero else torch.empty)(a.shape, dtype=a.dtype, device="cuda")
    ws = None if c.ws_bytes is None else torch.zeros(c.ws_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host, ms = _timed(lambda: c.call(T, ws, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return ({a.name: _bits(T[a.name]) for a in c.outs}, host), ms


def case(case_id, monkeypatch):
    monkeypatch.delenv("TPHIP_DEDUP", raising=False)
    if case_id not in _CASES:
        fn, layout, args, ws_kind = TABLE[case_id]
        c = fn(world(layout), *args)
        assert c.ws_align == ws_kind, "the table's workspace kind of %s is not the case's" % case_id
        c.plain, _ = _plain_call(c)                 # (the first call of a kind may build what the plan makes on first use)
        again, c.plain_ms = _plain_call(c)
        _same(c, again, "the plain call, repeated")
        _CASES[case_id] = c
    return _CASES[case_id]


def _same(c, got, what):
    bits, host = got
    want_bits, want_host = c.plain
    for a in c.outs:
        assert bits[a.name] == want_bits[a.name], "%s: output %s differs from the plain call" % (what, a.name)
    for k in (want_host or {}):
        assert abi_arena.same_bits(host[k], want_host[k]), "%s: host result %s differs from the plain call" % (what, k)


def _poison(t, value):
    t.fill_(value)


def _in_arena(c, aligned, ws_mod=(256, 0), ws_fill=PATTERN, poison=False, natural=()):
    """The case's arrays cut out of one arena: inputs uploaded (or poisoned, the real values in staging tensors), outputs left
    holding the pattern (zeroed where the header says so), the workspace of exactly the stated size.  natural: the arrays that
    go to natural alignment although the others are aligned."""
    import torch
    specs = [(a.dtype, a.shape) for a in c.arrays] + ([c.ws_bytes] if c.ws_bytes is not None else [])
    arena = Arena(abi_arena.room(specs), device="cuda")
    T, staging = {}, {}
    for a in c.arrays:
        T[a.name] = arena.carve(a.name, a.dtype, a.shape, a.role, aligned=aligned and a.name not in natural)
        if a.role == "in":
            real = torch.from_numpy(a.value).cuda()
            if poison and a.poison is not None:
                _poison(T[a.name], a.poison)
                staging[a.name] = real
            else:
                T[a.name].copy_(real)
        elif a.name in c.zero:
            T[a.name].zero_()
    ws = None
    if c.ws_bytes is not None:
        ws = arena.carve("ws", torch.uint8, (c.ws_bytes,), "ws", address_mod=ws_mod)
        arena.fill("ws", ws_fill)
    torch.cuda.synchronize()
    return arena, T, ws, staging


def _run_in_arena(c, what, **kw):
    import torch
    arena, T, ws, _ = _in_arena(c, **kw)
    host = c.call(T, ws, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    found = arena.check()
    print("%s: %d guard bytes checked, worst offender %s" % (what, arena.guard_bytes, found[0] if found else None))
    assert found == [], "%s: wrote outside its arrays: (array, byte offset) %s" % (what, found)
    _same(c, ({a.name: _bits(T[a.name]) for a in c.outs}, host), what)
    return arena, T


@pytest.mark.parametrize("case_id", list(TABLE))
def test_v1_extents(case_id, monkeypatch):
    c = case(case_id, monkeypatch)
    _run_in_arena(c, "V1 %s" % case_id, aligned=True)


@pytest.mark.parametrize("case_id", WITH_WORKSPACE)
def test_v2_workspace_content(case_id, monkeypatch):
    c = case(case_id, monkeypatch)
    for byte in (0x00, 0xFF, PATTERN):
        _run_in_arena(c, "V2 %s workspace of 0x%02X" % (case_id, byte), aligned=True, ws_fill=byte)


@pytest.mark.parametrize("case_id", list(TABLE))
def test_v3_natural_alignment(case_id, monkeypatch):
    c = case(case_id, monkeypatch)
    mod = {None: (256, 0), 1: (2, 1), 8: (16, 8), 16: (32, 16)}[c.ws_align]
    arena, T = _run_in_arena(c, "V3 %s" % case_id, aligned=False, ws_mod=mod)
    for a in c.arrays:
        size = abi_arena.itemsize(a.dtype)
        assert arena.address(a.name) % (16 if size > 1 else 2) == size
    if c.ws_bytes is not None:
        assert arena.address("ws") % mod[0] == mod[1]
        print("V3 %s: workspace of %d bytes at an address = %d mod %d" % (case_id, c.ws_bytes, mod[1], mod[0]))


@pytest.mark.parametrize("odd", [("flag",), ("nres",), ("flag", "nres")], ids="+".join)
@pytest.mark.parametrize("case_id", WIDE_STORES)
def test_v3_wide_stores_look_at_their_own_pointers(case_id, odd, monkeypatch):
    """V3 puts the states at an odd address too, which alone sends classify_kernel down its byte path.  Here the states and
    the workspace keep the alignment its wide path asks of them (on S4 the column count and every locus offset as well) and only
    the flags (4-byte store, array at an odd address), the counts (16-byte store, array at 4 mod 16) or both are at natural
    alignment: what decides is the kernel's look at those pointers.  (`packed`, its third wide store, lies at a multiple of
    256 in a workspace that is refused unless 16-byte aligned: V4.)"""
    c = case(case_id, monkeypatch)
    arena, T = _run_in_arena(c, "V3 %s, only %s at natural alignment" % (case_id, " and ".join(odd)), aligned=True, ws_mod=(32, 16), natural=odd)
    assert arena.address("states") % 256 == 0 and arena.address("ws") % 32 == 16
    assert ("flag" not in odd) == (arena.address("flag") % 256 == 0) and ("nres" not in odd) == (arena.address("nres") % 256 == 0)
    assert ("flag" not in odd) or arena.address("flag") % 2 == 1
    assert ("nres" not in odd) or arena.address("nres") % 16 == 4


@pytest.mark.parametrize("case_id", STATES_ALIGNMENT)
def test_v4_refusals(case_id, monkeypatch):
    import torch
    c = case(case_id, monkeypatch)
    engine = _engine()
    arena, T, ws, _ = _in_arena(c, aligned=True, ws_mod=(256, 1))
    assert ws.data_ptr() % c.ws_align == 1
    with pytest.raises(engine.TphipError, match=r"libtphip error 1: .*%d-byte aligned" % c.ws_align) as err:
        c.call(T, ws, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    print("V4 %s: %s; %d guard bytes checked" % (case_id, err.value, arena.guard_bytes))
    assert arena.check() == []
    for a in c.outs:
        if a.name in c.zero:
            assert not bool(T[a.name].any().item()), "refused, yet %s was written" % a.name
        else:
            assert arena.holds_pattern(a.name), "refused, yet %s was written" % a.name
    assert arena.holds_pattern("ws")


# ---- V5 ---------------------------------------------------------------------------------------------------------------------
class _Filler:
    """Work for the side stream ahead of the inputs: products of two scratch matrices, as many as the time asked for takes."""

    def __init__(self):
        import torch
        self.a = torch.rand((2048, 2048), dtype=torch.float32, device="cuda")
        self.b = torch.rand((2048, 2048), dtype=torch.float32, device="cuda")
        self.c = torch.empty_like(self.a)
        self.run(2)
        torch.cuda.synchronize()
        _, ms = _timed(lambda: self.run(20))
        self.unit_ms = ms / 20.0

    def run(self, reps):
        import torch
        for _ in range(reps):
            torch.mm(self.a, self.b, out=self.c)

    def reps_for(self, ms):
        return int(math.ceil(2.5 * ms / self.unit_ms)) + 2   # (2.5: the unit was timed once, at whatever clock the device had then)


_FILLER = []


def _stream_is_non_blocking(engine, stream):
    hip = engine._preload_torch_hip_runtime() or ctypes.CDLL("libamdhip64.so")
    flags = ctypes.c_uint(0)
    assert hip.hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags)) == 0
    return bool(flags.value & 1)   # hipStreamNonBlocking


@pytest.mark.parametrize("case_id", list(TABLE))
def test_v5_stream_order(case_id, monkeypatch):
    import torch
    c = case(case_id, monkeypatch)
    engine = _engine()
    if not _FILLER:
        _FILLER.append(_Filler())
    filler = _FILLER[0]
    arena, T, ws, staging = _in_arena(c, aligned=True, poison=True)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0 and _stream_is_non_blocking(engine, side)
    reps = filler.reps_for(FILLER_MARGIN * c.plain_ms)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0.record()
        filler.run(reps)
        e1.record()
        for name, real in staging.items():
            T[name].copy_(real, non_blocking=True)
        host = c.call(T, ws, side.cuda_stream)
        clones = {a.name: T[a.name].clone() for a in c.outs}
    side.synchronize()
    filler_ms = e0.elapsed_time(e1)
    torch.cuda.synchronize()
    found = arena.check()
    print("V5 %s: filler %.3f ms (%d products), plain call %.3f ms, ratio %.1f; poisoned %s; %d guard bytes checked, worst offender %s"
          % (case_id, filler_ms, reps, c.plain_ms, filler_ms / c.plain_ms, sorted(staging), arena.guard_bytes, found[0] if found else None))
    assert staging, "a case without a value input has nothing for V5 to see"
    assert found == []
    _same(c, ({k: _bits(v) for k, v in clones.items()}, host), "V5 %s" % case_id)
    assert filler_ms >= FILLER_MARGIN * c.plain_ms, "the filler must outlast the plain call ten times: %.3f ms against %.3f ms" % (filler_ms, c.plain_ms)


def test_table_names_every_dev_entry_point():
    """every `_dev` function include/tphip.h declares is reached by a case (the quartet and band families through their wrappers)"""
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tphip.h")).read()
    declared = set(re.findall(r"\bint (tphip_\w+_dev)\(", header))
    reached = {"tphip_%s_dev" % k.split("-")[0] for k in TABLE}
    print(sorted(declared - reached), sorted(reached - declared))
    assert declared <= reached

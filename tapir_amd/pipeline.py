"""All loci at once: the batch replacement of `pis = Pool.map(worker, params)` (bin/tapir_compute.py:84-164).

worker() in the reference handles ONE locus: shell out to HyPhy, read its JSON back, cull, compute PI and
its sums and integrals.  Here every alignment column of every locus is flattened into one column-parallel
batch (taxon-major state masks + CSR locus offsets), one call into the HIP engine produces per-site
(rate, subst, lnL) and the per-locus PI tables, and the host only writes the reference's own artefacts:
`<alignment>.rates` JSON files (schema of models_and_rates.bf:1018-1104 plus `corrected_rates`,
tapir/compute.py:40-43) and worker()-shaped result tuples for tapir_amd.db.
"""
import contextlib
import dataclasses
import os
import sys

import numpy as np

from . import compute, nexus


class PipelineError(Exception):
    pass


def _read_one(path):
    return nexus.read_states(path)


def _peek_nchar(path):
    """NCHAR of a NEXUS file from its first block (None when the header does not say)."""
    import re
    with open(path) as fh:
        head = fh.read(4096)
    m = re.search(r"dimensions\s+[^;]*?nchar\s*=\s*(\d+)", head, flags=re.I)
    return int(m.group(1)) if m else None


_PARSE_VIEWS = {}


def _parse_into(job):
    """Pool worker: parse one alignment and put its rows, in the tree's leaf order, at its columns of the batch array the
    parent created in /dev/shm.  Returns None, or what went wrong (the parent raises)."""
    shared, ntaxa, total, path, c0, n, leaf_names = job
    arr = _PARSE_VIEWS.get(shared)
    if arr is None:
        _PARSE_VIEWS.clear()
        arr = _PARSE_VIEWS[shared] = np.memmap(shared, dtype=np.uint8, mode="r+", shape=(ntaxa, total))
    try:
        names, st = nexus.read_states(path)
    except Exception as e:   # reported by the parent with the file's name
        return ("error", "%s: %s" % (os.path.basename(path), e))
    if set(names) != set(leaf_names):
        return ("taxa", names)
    if st.shape[1] != n:
        return ("nchar", st.shape[1])
    arr[:, c0:c0 + n] = st[[names.index(x) for x in leaf_names]]
    return None


class HostPool:
    """Worker processes for the host-side text work of a run (NEXUS parsing, `.rates` JSON formatting) -- the part of
    `Pool(cpu_count() - 1).map(worker, params)` (bin/tapir_compute.py:159-164) that is still CPU work here.

    The pool is forked ONCE, by the caller, BEFORE the process touches the GPU (before torch.distributed /
    RCCL come up and before libtphip's first call): forking a process that holds a HIP context and RCCL's threads
    hands the children KFD file descriptors and possibly held locks.  Results that do not exist yet at fork time (the
    per-site arrays the writers format) reach the workers through files in /dev/shm that they map read-only."""

    def __init__(self, workers):
        import multiprocessing
        self.workers = int(workers)
        self._pool = multiprocessing.get_context("fork").Pool(self.workers)

    def parse(self, paths):
        return self._pool.map(_read_one, paths, chunksize=max(1, len(paths) // (8 * self.workers)))

    def parse_into(self, paths, leaf_names, alloc):
        """The batch array [ntaxa, total columns] filled by the workers themselves through a file in /dev/shm: returning
        50 000 parsed matrices through the pool's pipes (3.2 GB pickled) cost more than parsing them.  Returns
        (states, offsets), or None when this route does not apply (no /dev/shm, a header without NCHAR or one that
        disagrees with its matrix: the caller then takes the plain route, which also words the error messages)."""
        if _shared_dir() is None:
            return None
        chunk = max(1, len(paths) // (8 * self.workers))
        nchar = self._pool.map(_peek_nchar, paths, chunksize=chunk)
        if any(n is None or n <= 0 for n in nchar):
            return None
        offsets = np.concatenate([[0], np.cumsum(nchar)]).astype(np.int64)
        ntaxa, total = len(leaf_names), int(offsets[-1])
        shm = _shared_dir(ntaxa * total)
        if shm is None:
            return None
        import tempfile
        fd, shared = tempfile.mkstemp(prefix="tapir_amd_states_", dir=shm)
        os.close(fd)
        try:
            mm = np.memmap(shared, dtype=np.uint8, mode="w+", shape=(ntaxa, total))
            names = tuple(leaf_names)
            jobs = [(shared, ntaxa, total, p, int(offsets[i]), int(nchar[i]), names) for i, p in enumerate(paths)]
            res = self._pool.map(_parse_into, jobs, chunksize=chunk)
            if any(r is not None for r in res):
                return None
            states = alloc((ntaxa, total), np.uint8)
            states[...] = mm
            del mm
        finally:
            try:
                os.unlink(shared)
            except OSError:
                pass
        return states, offsets

    def write_rates_async(self, jobs):
        """Hand the jobs to the workers and return at once; .get() on the result waits (and raises what a worker raised)."""
        return self._pool.map_async(_write_job, jobs, chunksize=max(1, len(jobs) // (8 * self.workers)))

    def write_rates(self, jobs, progress=None):
        for _ in self._pool.imap_unordered(_write_job, jobs, chunksize=max(1, len(jobs) // (8 * self.workers))):
            if progress:
                progress()

    def close(self):
        if self._pool is not None:
            self._pool.close()
            self._pool.join()
            self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load_alignments(paths, leaf_names, pool=None, alloc=None):
    """Read NEXUS alignments and flatten them: returns (states uint8 [ntaxa, ncols_total], offsets int64[L+1]).
    Rows follow `leaf_names` (the tree's leaves); an alignment must hold exactly those taxa, as HyPhy
    requires of (siteFilter, siteTree).  pool: a HostPool parses the files in parallel (--multiprocessing).
    alloc(shape, dtype): where the flattened array lives (engine.pinned_empty: the H2D copy is then direct DMA)."""
    if pool is not None and len(paths) > 1:
        direct = pool.parse_into(paths, leaf_names, alloc or np.empty) if hasattr(pool, "parse_into") else None
        if direct is not None:
            return direct
        parsed = pool.parse(paths)
    else:
        parsed = [_read_one(p) for p in paths]
    blocks, offsets = [], [0]
    want = set(leaf_names)
    for p, (names, st) in zip(paths, parsed):
        have = set(names)
        if have != want:
            missing, extra = sorted(want - have), sorted(have - want)
            raise PipelineError("hyphy error: taxa of {0} do not match the tree (missing {1}, not in tree {2})".format(
                os.path.basename(p), missing, extra))
        order = [names.index(n) for n in leaf_names]
        blocks.append(st[order])
        offsets.append(offsets[-1] + st.shape[1])
    states = (alloc or np.empty)((len(leaf_names), offsets[-1]), np.uint8)
    for l, blk in enumerate(blocks):
        states[:, offsets[l]:offsets[l + 1]] = blk
    return states, np.asarray(offsets, dtype=np.int64)


def format_rates_json(freqs, exch, site, subst, rate, ll, corrected):
    """The per-locus site-rate document: HyPhy's writer (bf:1018-1031, 1040, 1091-1101) then tapir's
    parse_site_rates rewrite (tapir/compute.py:40-43).  subst/rate/ll carry 4 decimals (Format(x,0,4))."""
    r4 = lambda v: float("%.4f" % v)  # noqa: E731
    return {"sites": {
        "freqs": {"A": float(freqs[0]), "C": float(freqs[1]), "G": float(freqs[2]), "T": float(freqs[3])},
        "subs_matrix": {"AC": float(exch[0]), "AG": float(exch[1]), "AT": float(exch[2]), "CG": float(exch[3]),
                        "CT": float(exch[4]), "GT": float(exch[5])},
        "rates": [{"site": int(s), "subst": r4(a), "rate": r4(b), "ll": r4(c)} for s, a, b, c in zip(site, subst, rate, ll)],
        "corrected_rates": [{"site": int(s), "rate": float(v)} for s, v in zip(site, corrected)],
    }}


def _repr_rounded(arr, decimals=4):
    """[repr(float("%.4f" % v)) for v in arr] without a Python-level step per element: the rounding is compute.round_like_hyphy
    (the double nearest to the printf-rounded decimal, vectorised), repr runs over a plain list inside map().  Values too large
    for the vectorised rounding to be exact (|v| * 10^decimals beyond 2^52) and non-finite ones take the literal route."""
    from .compute import round_like_hyphy
    a = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1)
    out = list(map(repr, round_like_hyphy(a, decimals).tolist()))
    odd = np.flatnonzero(~(np.abs(a) < 2.0 ** 52 / 10.0 ** decimals))
    for k in odd.tolist():
        out[k] = repr(float("%.*f" % (decimals, a[k])))
    return out


_ROW = ('            {\n                "site": ', ',\n                "subst": ', ',\n                "rate": ',
        ',\n                "ll": ', '\n            },\n')
_CROW = ('            {\n                "site": ', ',\n                "rate": ', '\n            },\n')


_TEMPLATES = {}   # n -> the two arrays of a locus of n sites numbered 1..n with a %s for every number


def _rates_template(n):
    t = _TEMPLATES.get(n)
    if t is None:
        if len(_TEMPLATES) >= 32:   # ~150 bytes per site each; loci of one run mostly share a few lengths
            _TEMPLATES.clear()
        a, b, c, d, e = _ROW
        rows = "".join([a + str(i) + b + "%s" + c + "%s" + d + "%s" + e for i in range(1, n + 1)])[:-2]
        a, b, e = _CROW
        crow = "".join([a + str(i) + b + "%s" + e for i in range(1, n + 1)])[:-2]
        t = _TEMPLATES[n] = '        "rates": [\n%s\n        ],\n        "corrected_rates": [\n%s\n        ]\n' % (rows, crow)
    return t


def dumps_rates_json(freqs, exch, site, subst, rate, ll, corrected, sd=None, eb=None):
    """The text `json.dumps(format_rates_json(...), indent=4)` would produce, built by bulk string operations: the generic
    encoder spends ~30 us per site (it dominated the whole CLI), a formatted row per site ~2 us, this ~1.2 us, of which
    0.6 are the four float.__repr__ (every per-site step -- rounding, repr, placing the numbers in the fixed text -- runs
    inside numpy, map() or one `%` over a template cached per number of sites; sites not numbered 1..n: str.join route)."""
    from itertools import chain, repeat
    head = ('{\n    "sites": {\n        "freqs": {\n            "A": %s,\n            "C": %s,\n            "G": %s,\n'
            '            "T": %s\n        },\n        "subs_matrix": {\n            "AC": %s,\n            "AG": %s,\n'
            '            "AT": %s,\n            "CG": %s,\n            "CT": %s,\n            "GT": %s\n        },\n'
            % tuple(repr(float(x)) for x in list(freqs) + list(exch)))
    if eb is not None:   # empirical-Bayes rates: the prior's fit in the header, every row with the posterior sd
        head += ('        "estimator": "eb",\n        "gamma_alpha": %s,\n        "gamma_scale": %s,\n        "gamma_categories": %d,\n'
                 '        "locus_lnl": %s,\n' % (repr(float(eb["alpha"])), repr(float(eb["scale"])), int(eb["categories"]),
                                                 repr(float(eb["locus_lnl"]))))
        return head + _eb_rows(site, subst, rate, ll, corrected, sd) + "    }\n}"
    site = np.asarray(site).astype(np.int64).reshape(-1)
    n = site.size
    cor = map(repr, np.ascontiguousarray(corrected, dtype=np.float64).reshape(-1).tolist())   # json writes float.__repr__
    if n == 0:
        body = '        "rates": [],\n        "corrected_rates": []\n'
    elif site[0] == 1 and site[-1] == n and np.array_equal(site, np.arange(1, n + 1)):
        cols = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (subst, rate, ll)]
        vals = _repr_rounded(np.stack(cols, axis=1))   # subst, rate, ll of site 1, of site 2, ...
        vals.extend(cor)
        body = _rates_template(n) % tuple(vals)
    else:
        sub, rat, lls = _repr_rounded(subst), _repr_rounded(rate), _repr_rounded(ll)
        sites = list(map(str, site.tolist()))
        a, b, c, d, e = _ROW
        rows = "".join(chain.from_iterable(zip(repeat(a), sites, repeat(b), sub, repeat(c), rat, repeat(d), lls, repeat(e))))[:-2]
        a, b, e = _CROW
        crow = "".join(chain.from_iterable(zip(repeat(a), sites, repeat(b), cor, repeat(e))))[:-2]
        body = '        "rates": [\n%s\n        ],\n        "corrected_rates": [\n%s\n        ]\n' % (rows, crow)
    return head + body + "    }\n}"


_EROW = ('            {\n                "site": ', ',\n                "subst": ', ',\n                "rate": ',
         ',\n                "ll": ', ',\n                "sd": ', '\n            },\n')


def _eb_rows(site, subst, rate, ll, corrected, sd):
    """The two arrays of an empirical-Bayes `.rates` document: the rows of the maximum-likelihood one plus "sd"."""
    from itertools import chain, repeat
    site = np.asarray(site).astype(np.int64).reshape(-1)
    if site.size == 0:
        return '        "rates": [],\n        "corrected_rates": []\n'
    sub, rat, lls, sds = _repr_rounded(subst), _repr_rounded(rate), _repr_rounded(ll), _repr_rounded(sd)
    cor = map(repr, np.ascontiguousarray(corrected, dtype=np.float64).reshape(-1).tolist())
    sites = list(map(str, site.tolist()))
    a, b, c, d, e, f = _EROW
    rows = "".join(chain.from_iterable(zip(repeat(a), sites, repeat(b), sub, repeat(c), rat, repeat(d), lls, repeat(e), sds,
                                           repeat(f))))[:-2]
    a, b, e = _CROW
    crow = "".join(chain.from_iterable(zip(repeat(a), sites, repeat(b), cor, repeat(e))))[:-2]
    return '        "rates": [\n%s\n        ],\n        "corrected_rates": [\n%s\n        ]\n' % (rows, crow)


def _write_rates_file(path, freqs, exch, subst, rate4, lnl, corrected, sd=None, eb=None):
    n = len(subst)
    with open(path, "w") as fh:
        fh.write(dumps_rates_json(freqs, exch, np.arange(1, n + 1), subst, rate4, lnl, corrected, sd=sd, eb=eb))


_SHARED_VIEWS = {}


def _write_job(job):
    """Pool worker: format one locus' .rates file from the per-site arrays the parent left in a shared file."""
    path, shared, total, a, b, freqs, exch = job[:7]
    eb = job[7] if len(job) > 7 else None   # empirical-Bayes runs: the locus' fit, and a fifth row (sd) in the shared file
    arr = _SHARED_VIEWS.get(shared)
    if arr is None:
        _SHARED_VIEWS.clear()   # one run at a time: drop the mapping of a previous run
        arr = _SHARED_VIEWS[shared] = np.memmap(shared, dtype=np.float64, mode="r", shape=(4 if eb is None else 5, total))
    if eb is not None:
        _write_rates_file(path, freqs, exch, arr[0, a:b], arr[1, a:b], arr[2, a:b], arr[3, a:b], sd=arr[4, a:b], eb=eb)
    else:
        _write_rates_file(path, freqs, exch, arr[0, a:b], arr[1, a:b], arr[2, a:b], arr[3, a:b])
    return path


class _SideThread:
    """fn(make_arg()) on a second thread, the argument kept in .arg; join() returns its seconds and raises what it raised."""

    def __init__(self, fn, make_arg):
        import threading
        self.arg, self._make_arg, self._fn, self._exc, self._seconds = None, make_arg, fn, None, 0.0
        self._thread = threading.Thread(target=self._run, name="tapir_amd-side")
        self._thread.start()

    def _run(self):
        import time
        t0 = time.perf_counter()
        try:
            self.arg = self._make_arg()
            self._fn(self.arg)
        except BaseException as exc:   # handed to the joining thread
            self._exc = exc
        self._seconds = time.perf_counter() - t0

    def join(self):
        self._thread.join()
        if self._exc is not None:
            raise self._exc
        return self._seconds


def _shared_dir(need_bytes=0):
    """/dev/shm when it is there, writable and has room for `need_bytes` (a tmpfs that fills up under a memory map kills
    the writer with SIGBUS: containers often give it 64 MB), else None."""
    d = "/dev/shm"
    if not (os.path.isdir(d) and os.access(d, os.W_OK)):
        return None
    if need_bytes:
        import shutil
        try:
            if shutil.disk_usage(d).free < 1.2 * need_bytes + (64 << 20):
                return None
        except OSError:
            return None
    return d


STAGE1_BLOCK_LOCI = 16384  # loci fitted together by one tphip_stage1_fit call.  Bounds device memory (per locus ~0.5 MB of optimiser
                           # state and candidate arrays: 202 models x 9-point stencils) and nothing else: the optimisers' fixed cost per
                           # iteration is amortised over the block, and a block runs until its slowest locus has converged.


def model_averaged_exchangeabilities(eng, states, offsets, pi, ntaxa, parent, blen, leaf, T, times, intervals,
                                     correction, device=0, block_loci=None, return_pi=False):
    """Stage 1 of models_and_rates.bf (bf:405-897) for every locus -> [L, 6] AC, AG(=1), AT, CG, CT, GT.

    pi: [L, 4] base frequencies, or None = the empirical ones of each locus (HarvestFrequencies, bf:968), computed on the device
    from the same upload.  With return_pi the frequencies used come back as a second array.
    Loci are independent, so they are fitted in blocks of `block_loci` (bounds the optimiser's device memory).  With the
    real engine a block is ONE call: its column range of `states` goes up with a 2-D copy (no host copy; pinned `states` =
    direct DMA), the columns are collapsed into site patterns with counts on the device -- what HyPhy's likelihood function
    sums over (bf:960-963) -- and the 203 fits and the averaging run there (csrc/stage1_driver.hip)."""
    from . import stage1
    offsets = np.asarray(offsets, dtype=np.int64)
    L = len(offsets) - 1
    step = int(block_loci or _block_sizes()[0])
    out = np.empty((L, 6))
    pi_used = np.empty((L, 4))
    if pi is not None:
        pi = np.asarray(pi, dtype=np.float64).reshape(-1, 4)
    in_engine = hasattr(eng, "Plan") and hasattr(eng.Plan, "stage1_fit")
    if pi is None and not in_engine:
        pi = nexus.base_frequencies_from_histogram(eng.state_histogram(states, offsets, device=device))
    def open_plan(off, blk_pi):
        return eng.Plan(ntaxa, parent, blen, leaf, off, blk_pi, np.ones((len(blk_pi), 6)), T, times, intervals,
                        correction=correction, device=device)

    for l0 in range(0, L, step):
        l1 = min(L, l0 + step)
        off = offsets[l0:l1 + 1] - offsets[l0]
        if in_engine:
            cols = states[:, offsets[l0]:offsets[l1]]          # a view: rows are `states.strides[0]` bytes apart
            plan = open_plan(off, np.full((l1 - l0, 4), 0.25) if pi is None else pi[l0:l1])
            try:
                res = plan.stage1_fit(cols, details=False, compress_patterns=True, empirical_pi=pi is None)
            finally:
                plan.close()
            out[l0:l1], pi_used[l0:l1] = res["exch"], res["pi"]
            continue
        # an engine without the call (the tests' CPU stand-in): site patterns, then the host optimiser of stage1.py
        sub = np.ascontiguousarray(states[:, offsets[l0]:offsets[l1]])
        pstates, poffsets, weights, _ = eng.compress_columns(sub, off, device=device, want_map=False)
        plan = open_plan(poffsets, pi[l0:l1])
        try:
            plan.set_column_weights(weights)
            out[l0:l1] = stage1.model_averaged_exchangeabilities(plan, pstates, pi[l0:l1], parent,
                                                                 np.asarray(blen) / correction)["exch"]
            pi_used[l0:l1] = pi[l0:l1]
        finally:
            plan.close()
    return (out, pi_used) if return_pi else out


STREAM_BLOCK_LOCI = 8192   # loci per block of the streamed run (_run_streamed)


@dataclasses.dataclass(frozen=True)
class Run:
    """What one run fixes for every locus and every stage: the tree (blen already scaled by `correction`), the PI schedule,
    how raw rates become final rates, and what every plan of the run is opened with.  Nothing of the loci (offsets, models,
    rates) is in here."""
    leaf_names: list
    parent: list
    blen: list
    leaf: list
    T: int
    times: list
    intervals: list
    correction: float = 1.0
    threshold: int = 3
    round_decimals: int = 4
    integ_mode: int = 0
    device: int = 0
    start_rule: int = 0        # 1: every column starts at siteRate = 1 as in HyPhy (bf:1050) instead of at its parsimony rate
    cat_rates: list = None     # the optional rate mixture (more than one category)
    cat_weights: list = None

    @property
    def width(self):
        """Columns of a PI row: the net profile, the times, then integral and error of every interval."""
        return self.T + len(self.times) + 2 * len(self.intervals)

    @property
    def band_width(self):
        """Columns of a band row (the replicate stages): the net profile and the interval integrals."""
        return self.T + len(self.intervals)

    def plan(self, eng, offsets, pi, exch, times=None, start_rule=True, mixture=False, **model):
        """A plan with the run's correction, threshold and rounding (the main run and the stages that estimate rates again).
        times: [] for the band stages; start_rule False: never passed; mixture: the main run alone carries it; model=: the
        engine's own default applies where it is not given."""
        kw = dict(correction=self.correction, threshold=self.threshold, round_decimals=self.round_decimals,
                  integ_mode=self.integ_mode, device=self.device, **model)
        if mixture and self.cat_rates is not None and len(self.cat_rates) > 1:
            kw.update(cat_rates=self.cat_rates, cat_weights=self.cat_weights)
        if start_rule and self.start_rule:
            kw["start_rule"] = int(self.start_rule)
        return eng.Plan(len(self.leaf_names), self.parent, self.blen, self.leaf, offsets, pi, exch, self.T,
                        self.times if times is None else times, self.intervals, **kw)

    @contextlib.contextmanager
    def final_rates_plan(self, eng, per_locus, times=None, pi=None, exch=None, model=None):
        """The plan for already-final per-locus rates (NaN = culled) -- no rounding, no correction, no cull -- with the
        concatenated rates and the loci's offsets; closed on leaving.  The PI stages do not look at the models (model None:
        placeholders, the run's intervals and integ_mode); the quartet stages pass the loci's pi / exch / model as
        _locus_models returns them and have neither times nor intervals."""
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in per_locus])]).astype(np.int64)
        rates = np.concatenate(per_locus) if per_locus else np.zeros(0)
        L = len(per_locus)
        if model is None:
            pi, exch, intervals, kw = np.full((L, 4), 0.25), np.ones((L, 6)), self.intervals, dict(integ_mode=self.integ_mode)
            times = self.times if times is None else times
        else:
            times, intervals, kw = [], [], dict(model=model)
        plan = eng.Plan(len(self.leaf_names), self.parent, self.blen, self.leaf, offsets, pi, exch, self.T, times, intervals,
                        correction=1.0, threshold=0, round_decimals=-1, device=self.device, **kw)
        try:
            yield plan, rates, offsets
        finally:
            plan.close()

    def corrected(self, rate):
        """(rate rounded like HyPhy's JSON, that / correction): what tapir has after parse_site_rates."""
        rate4 = compute.round_like_hyphy(rate, self.round_decimals) if self.round_decimals >= 0 else rate
        return rate4, rate4 / self.correction

    def final_rates(self, rate, nres):
        """(rate4, corrected, culled): corrected() and the cull (bin/tapir_compute.py:100-102; NaN = culled)."""
        rate4, corrected = self.corrected(rate)
        return rate4, corrected, np.where(nres >= self.threshold, corrected, np.nan)

    def tuples(self, names, per_locus, tables):
        """worker()-shaped result tuples from the loci's final rates and PI rows."""
        T, n_t, n_i = self.T, len(self.times), len(self.intervals)
        out = []
        for l, name in enumerate(names):
            row = tables[l]
            rates = per_locus[l]
            fin = rates[~np.isnan(rates)]
            mean_rate = float(fin.mean()) if fin.size else float("nan")  # bin/tapir_compute.py:110 (never stored)
            pi_net = row[:T].copy()
            pi_times = dict(zip(self.times, row[T:T + n_t]))
            pi_epochs = {}
            for k, (a, b) in enumerate(self.intervals):
                pi_epochs["{0}-{1}".format(a, b)] = {"sum(integral)": row[T + n_t + k], "sum(error)": row[T + n_t + n_i + k]}
            out.append((name, rates, mean_rate, None, pi_net, pi_times, pi_epochs))
        return out


class _RatesShare:
    """The per-site arrays of the `.rates` files in one file the pool's workers map (they were forked before the arrays
    existed): rows subst, rate4, lnl, corrected, and sd under empirical Bayes.  jobs() are _write_job's plain tuples."""

    def __init__(self, total, eb):
        import tempfile
        self.total, self.eb = max(total, 1), eb
        fd, self.path = tempfile.mkstemp(prefix="tapir_amd_", suffix=".f64", dir=_shared_dir(32 * self.total))
        os.close(fd)
        self.arr = None

    def fill(self, a, b, subst, rate4, lnl, corrected, sd=None):
        if self.arr is None:
            self.arr = np.memmap(self.path, dtype=np.float64, mode="w+", shape=(5 if self.eb else 4, self.total))
        self.arr[0, a:b], self.arr[1, a:b], self.arr[2, a:b], self.arr[3, a:b] = subst, rate4, lnl, corrected
        if self.eb:
            self.arr[4, a:b] = sd

    def jobs(self, paths, offsets, l0, pi, exch, ebfit=None):
        """One job per path: the loci l0, l0 + 1, ... of `offsets`, `pi`, `exch` and of the fits."""
        jobs = [(p, self.path, self.total, int(offsets[l]), int(offsets[l + 1]), pi[l], exch[l])
                for l, p in enumerate(paths, l0)]
        if self.eb:
            jobs = [job + (_eb_meta(ebfit, l),) for l, job in enumerate(jobs, l0)]
        return jobs

    def close(self):
        self.arr = None
        try:
            os.unlink(self.path)
        except OSError:
            pass


def _eb_meta(fit, l):
    return dict(alpha=fit["alpha"][l], scale=fit["scale"][l], categories=fit["categories"], locus_lnl=fit["locus_lnl"][l])


def _eb_rates(run, plan, states, eb_options, tables=True):
    """The empirical-Bayes estimator in the place of the site-rate launch (tapir_amd/eb.py): the per-column arrays run_fused
    returns (rate = posterior mean, lnl = log marginal likelihood, subst = rate x tree length, flag = 0) plus sd and the
    per-locus fit; the PI tables come from the same tphip_pi_tables call, fed with these rates."""
    from . import eb
    est = eb.estimate(plan, states, ncat=eb_options["categories"], alpha=eb_options.get("alpha"),
                      alpha_bounds=eb_options.get("alpha_bounds") or eb.ALPHA_BOUNDS)
    length = float(np.asarray(run.blen, np.float64)[np.asarray(run.parent) >= 0].sum())
    out = dict(rate=est["rate"], subst=est["rate"] * length, lnl=est["lnl"], flag=np.zeros(len(est["rate"]), np.uint8),
               nres=est["nres"], sd=est["sd"],
               eb=dict(alpha=est["alpha"], scale=est["scale"], locus_lnl=est["locus_lnl"], categories=est["categories"]))
    if tables:
        out["tables"] = plan.pi_tables(out["rate"], out["nres"])
    return out


def _block_sizes():
    """(stage-1 block, stream block) in loci; TPHIP_STREAM_BLOCK=n sets both to n (tests: a streamed and an unstreamed run of
    the same small batch then fit the same loci together and must write the same bytes)."""
    env = os.environ.get("TPHIP_STREAM_BLOCK")
    if env:
        n = max(1, int(env))
        return n, n
    return STAGE1_BLOCK_LOCI, STREAM_BLOCK_LOCI


def _fixed_model_pi(eng, site_model, states, offsets, device):
    """[L, 4] base frequencies of a fixed site model: 1/4 each (jc) or the loci's empirical ones (f81, HarvestFrequencies)."""
    L = len(offsets) - 1
    if site_model == "jc":
        return np.full((L, 4), 0.25)
    return nexus.base_frequencies_from_histogram(eng.state_histogram(np.ascontiguousarray(states), offsets, device=device))


def _run_streamed(eng, run, states, offsets, alignments, pi, output_dir, pool, progress, table_sink, timings, lap,
                  site_model="locus", eb_options=None):
    """The whole pipeline block by block, host and device working at the same time.

    Block k of the loci: stage 1 (one tphip_stage1_fit call on the block's column range of the pinned batch array), its
    estimates into the same plan (tphip_plan_set_models), the per-site loop and the PI tables (tphip_run_fused_pitched) --
    and while the GPU does that for block k + 1, the pool's workers format block k's `.rates` files from a shared array and
    a second thread of this process inserts block k's PI rows into sqlite (`table_sink`).  At C4 scale the GPU needs ~8 s for
    the 50 000 loci and the host ~8 s for their 12 GB of text and 5.4 M rows: one after the other that is the sum, here close
    to the larger.  Results are those of the unstreamed run (loci are independent; every array is filled at the same places).
    A fixed site model (site_model jc / f81) has no stage 1: each block's plan carries the model from the start."""
    L = len(alignments)
    total = int(offsets[-1])
    new = getattr(eng, "pinned_empty", None) or np.empty
    out = dict(rate=new(total, np.float64), subst=new(total, np.float64), lnl=new(total, np.float64), flag=new(total, np.uint8),
               nres=new(total, np.int32), tables=new((L, run.width), np.float64))
    if eb_options is not None:   # the posterior sd is a fifth per-site array; the per-locus fits go into the .rates headers
        out["sd"] = np.empty(total)
        out["eb"] = dict(alpha=np.empty(L), scale=np.empty(L), locus_lnl=np.empty(L), categories=int(eb_options["categories"]))
    exch_all, pi_all = np.empty((L, 6)), np.empty((L, 4))
    per_locus = [None] * L
    paths = [os.path.join(output_dir, os.path.basename(a) + ".rates") for a in alignments]
    share = _RatesShare(total, eb_options is not None)
    pending = []
    sink_thread = None
    if table_sink is not None:
        import queue
        import threading
        q = queue.Queue()
        err = []

        def drain():
            try:
                while True:
                    item = q.get()
                    if item is None:
                        table_sink.close()   # (sqlite objects live and die on the thread that made them)
                        return
                    table_sink.add(*item)
            except BaseException as exc:   # handed to the main thread at the end
                err.append(exc)
        sink_thread = threading.Thread(target=drain, name="tapir_amd-sqlite")
        sink_thread.start()
    try:
        step = _block_sizes()[1]
        for l0 in range(0, L, step):
            l1 = min(L, l0 + step)
            a, b = int(offsets[l0]), int(offsets[l1])
            cols, off = states[:, a:b], offsets[l0:l1 + 1] - a
            if site_model != "locus":
                blk_pi, blk_exch, model = _fixed_model_pi(eng, site_model, cols, off, run.device), None, dict(model="f81")
                lap("base_frequencies")
                exch_all[l0:l1], pi_all[l0:l1] = 1.0, blk_pi
            else:
                blk_pi, blk_exch, model = np.full((l1 - l0, 4), 0.25) if pi is None else pi[l0:l1], np.ones((l1 - l0, 6)), {}
            plan = run.plan(eng, off, blk_pi, blk_exch, mixture=True, **model)
            try:
                if site_model == "locus":
                    res = plan.stage1_fit(cols, details=False, compress_patterns=True, empirical_pi=pi is None)
                    lap("stage1_model_averaging")
                    exch_all[l0:l1], pi_all[l0:l1] = res["exch"], res["pi"]
                    plan.set_models(exch=res["exch"])
                if eb_options is not None:
                    blk = _eb_rates(run, plan, np.ascontiguousarray(cols), eb_options)
                    for k in ("rate", "subst", "lnl", "flag", "nres", "sd"):
                        out[k][a:b] = blk[k]
                    out["tables"][l0:l1] = blk["tables"]
                    for k in ("alpha", "scale", "locus_lnl"):
                        out["eb"][k][l0:l1] = blk["eb"][k]
                    lap("eb_rates_and_pi_incl_pcie")
                else:
                    plan.run_fused_into(cols, out, col0=a, locus0=l0)
                    lap("site_rates_and_pi_incl_pcie")
            finally:
                plan.close()
            rate4, corrected, culled = run.final_rates(out["rate"][a:b], out["nres"][a:b])
            for l in range(l0, l1):
                per_locus[l] = culled[offsets[l] - a:offsets[l + 1] - a]
            share.fill(a, b, out["subst"][a:b], rate4, out["lnl"][a:b], corrected, out["sd"][a:b] if "sd" in out else None)
            lap("round_correct_cull")
            pending.append(pool.write_rates_async(share.jobs(paths[l0:l1], offsets, l0, pi_all, exch_all, out.get("eb"))))
            if sink_thread is not None:
                q.put((alignments[l0:l1], out["tables"][l0:l1].copy()))
        for res in pending:
            for _ in res.get():
                if progress:
                    progress()
        share.close()
        lap("write_rates_files")
        if sink_thread is not None:
            q.put(None)
            sink_thread.join()
            if err:
                raise err[0]
            out["during_write_done"] = True
            lap("sqlite_tail")
    finally:
        if sink_thread is not None and sink_thread.is_alive():
            q.put(None)
            sink_thread.join()
        share.close()
    out["timings"] = timings
    out["final_tables"] = out["tables"]
    out["streamed_blocks"] = (L + step - 1) // step
    out["models"] = dict(pi=pi_all, exch=exch_all, model="gtr" if site_model == "locus" else "f81")
    return run.tuples(alignments, per_locus, out["tables"]), out


def run_alignments(alignments, run, exch, pi=None, subsets=None, output_dir=None, engine_mod=None, progress=None, pool=None,
                   during_write=None, table_sink=None, site_model="locus", rate_estimator="ml", eb_options=None):
    """Site rates + PI for a list of NEXUS alignments.  Returns a list of worker()-shaped tuples
    (alignment, rates, mean_rate, None, pi_net, pi_times, pi_epochs) in the order of `alignments`.

    run: the Run (tree, PI schedule, correction / threshold / rounding, device, integral mode, start rule, rate mixture).

    during_write: callable(tuples) the caller would run next on the returned tuples (the command line: the sqlite
    inserts).  When the pool's workers write the `.rates` files it runs on a second thread of this process meanwhile
    (the parent only waits for the workers then; at C4 scale both take ~3 s) and out["during_write_done"] is True;
    an exception it raises is raised here.  Otherwise it is not called.

    exch: [6] or [L,6] exchangeabilities AC,AG,AT,CG,CT,GT, or None = HyPhy's stage 1 (model-averaged estimates per
    locus, tapir_amd/stage1.py); pi: None (empirical, HarvestFrequencies) or [L,4].
    site_model: "locus" (the GTR model above), or a fixed model without stage 1 that runs the engine's F81 kernel:
    "jc" (Jukes-Cantor: pi = 1/4, exchangeabilities 1) or "f81" (the loci's empirical pi, exchangeabilities 1); exch and pi
    must then be None.
    rate_estimator: "ml" (each column's maximum-likelihood rate) or "eb" (empirical Bayes under a discrete-gamma prior fitted
    per locus, tapir_amd/eb.py; eb_options: dict(categories, alpha or None, alpha_bounds)); under "eb" the `.rates` documents
    carry the fit and a posterior sd per site, everything downstream of the rates is the same code.
    pool: a HostPool created before the process touched the GPU (parallel parsing and .rates writing), or None."""
    if site_model not in ("locus", "jc", "f81"):
        raise PipelineError("unknown site model %r" % (site_model,))
    if rate_estimator not in ("ml", "eb"):
        raise PipelineError("unknown rate estimator %r" % (rate_estimator,))
    if rate_estimator == "eb":
        from . import eb as _eb
        eb_options = dict(eb_options or {})
        eb_options.setdefault("categories", _eb.DEFAULT_CATEGORIES)
        if not _eb.MIN_CATEGORIES <= int(eb_options["categories"]) <= _eb.MAX_CATEGORIES:
            raise PipelineError("the empirical-Bayes prior takes 2..16 categories")
        if run.cat_rates is not None and len(run.cat_rates) > 1:
            raise PipelineError("the empirical-Bayes estimator has its own prior: it cannot run on top of the rate mixture")
    else:
        if eb_options is not None:
            raise PipelineError("eb_options need rate_estimator='eb'")
    fixed = site_model != "locus"
    if fixed and (exch is not None or pi is not None):
        raise PipelineError("site model %s fixes the exchangeabilities and base frequencies" % site_model)
    eng = engine_mod
    if eng is None:
        from . import engine as eng
    subsets = subsets or {}
    import time
    timings = {}          # seconds per stage of this call (out["timings"]; tools/e2e_cli_timing.py prints them)
    t_mark = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        timings[name] = timings.get(name, 0.0) + now - t_mark[0]
        t_mark[0] = now

    pinned = getattr(eng, "pinned_empty", None)   # the real engine: I/O arrays in pinned memory
    states, offsets = load_alignments(alignments, run.leaf_names, pool, alloc=pinned)
    lap("parse_nexus")
    L = len(alignments)
    need_subset = any(os.path.basename(a) in subsets for a in alignments)
    if ((exch is None or fixed) and pool is not None and hasattr(pool, "write_rates_async") and output_dir is not None and not need_subset and
            L > _block_sizes()[1] and hasattr(eng, "Plan") and hasattr(eng.Plan, "run_fused_into") and
            _shared_dir(32 * max(int(offsets[-1]), 1)) is not None and os.environ.get("TPHIP_NO_STREAM") is None):
        if pi is not None:
            pi = np.asarray(pi, dtype=np.float64).reshape(L, 4)
        return _run_streamed(eng, run, states, offsets, alignments, pi, output_dir, pool, progress, table_sink, timings, lap,
                             site_model=site_model, eb_options=eb_options)
    if fixed:
        pi = _fixed_model_pi(eng, site_model, states, offsets, run.device)
        lap("base_frequencies")
        plan_exch, exch, model = None, np.ones((L, 6)), dict(model="f81")
    else:
        if pi is None and exch is not None:
            hist = eng.state_histogram(states, offsets, device=run.device)
            pi = nexus.base_frequencies_from_histogram(hist)
        lap("base_frequencies")
        if exch is None:   # HyPhy's stage 1; the empirical base frequencies (when none are given) come from the same upload
            exch, pi = model_averaged_exchangeabilities(eng, states, offsets, pi, len(run.leaf_names), run.parent, run.blen,
                                                        run.leaf, run.T, run.times, run.intervals, run.correction, run.device,
                                                        return_pi=True)
            lap("stage1_model_averaging")
        pi = np.asarray(pi, dtype=np.float64).reshape(L, 4)
        exch = np.asarray(exch, dtype=np.float64)
        if exch.ndim == 1:
            exch = np.tile(exch, (L, 1))
        plan_exch, model = exch, {}
    out = _run_plan(eng, run, states, offsets, pi, plan_exch, need_subset, pinned, eb_options, **model)
    lap("site_rates_and_pi_incl_pcie")
    tuples, out = _finish(eng, run, out, alignments, offsets, pi, exch, subsets, need_subset, output_dir, pool, progress,
                          during_write, timings, lap)
    # the loci's models, for stages that need them (quartet_tables)
    out["models"] = dict(pi=np.asarray(pi, dtype=np.float64), exch=exch, model=model.get("model", "gtr"))
    return tuples, out


def _run_plan(eng, run, states, offsets, pi, exch, need_subset, pinned, eb_options=None, **model):
    """One plan over the whole batch: per-site rates, and the PI tables unless a subset needs its own."""
    plan = run.plan(eng, offsets, pi, exch, mixture=True, **model)
    try:
        if eb_options is not None:
            return _eb_rates(run, plan, states, eb_options, tables=not need_subset)
        if need_subset:
            return plan.site_rates(states)
        return plan.run_fused(states, pinned=True) if pinned else plan.run_fused(states)
    finally:
        plan.close()


def _finish(eng, run, out, alignments, offsets, pi, exch, subsets, need_subset, output_dir, pool, progress, during_write,
            timings, lap):
    """Rounding, culling, the `.rates` files and the worker()-shaped tuples of run_alignments."""
    L = len(alignments)
    ebfit = out.get("eb")   # the per-locus fits of an empirical-Bayes run (None: maximum-likelihood rates)
    rate4, corrected, culled = run.final_rates(out["rate"], out["nres"])
    per_locus = []
    for l, a in enumerate(alignments):
        r = culled[offsets[l]:offsets[l + 1]]
        base = os.path.basename(a)
        if base in subsets:
            r = r[subsets[base][0]:subsets[base][1]]
        per_locus.append(r)
    lap("round_correct_cull")
    if output_dir is not None:
        paths = [os.path.join(output_dir, os.path.basename(a) + ".rates") for a in alignments]
        if pool is not None and L > 1:
            total = int(offsets[-1])
            share = _RatesShare(total, ebfit is not None)
            side = None
            try:
                share.fill(0, total, out["subst"], rate4, out["lnl"], corrected, out.get("sd"))
                share.arr.flush()
                jobs = share.jobs(paths, offsets, 0, pi, exch, ebfit)
                if during_write is not None and not need_subset:
                    side = _SideThread(during_write, lambda: run.tuples(alignments, per_locus, out["tables"]))
                pool.write_rates(jobs, progress)
            finally:
                share.close()
                if side is not None:
                    timings["during_write"] = side.join()
                    out["during_write_done"] = True
        else:
            for l in range(L):
                sl = slice(offsets[l], offsets[l + 1])
                _write_rates_file(paths[l], pi[l], exch[l], out["subst"][sl], rate4[sl], out["lnl"][sl], corrected[sl],
                                  sd=None if ebfit is None else out["sd"][sl], eb=None if ebfit is None else _eb_meta(ebfit, l))
                if progress:
                    progress()
    elif progress:
        for _ in alignments:
            progress()
    lap("write_rates_files")
    tables = _tables_for_rates(eng, run, per_locus) if need_subset else out["tables"]
    out["timings"] = timings
    out["final_tables"] = tables   # [L, W] rows as stored in sqlite (after any subset slicing)
    if out.get("during_write_done"):
        return side.arg, out
    return run.tuples(alignments, per_locus, tables), out


def run_rate_files(rate_files, run, subsets=None, engine_mod=None, progress=None, return_tables=False):
    """The --site-rates path (bin/tapir_compute.py:103-104, 153-158): re-read "rate" from each JSON, divide by
    the correction (again: the reference does not read `corrected_rates`), rewrite the file, NO culling."""
    eng = engine_mod
    if eng is None:
        from . import engine as eng
    subsets = subsets or {}
    per_locus = []
    for f in rate_files:
        r = compute.parse_site_rates(f, correction=run.correction)
        base = os.path.basename(f)
        if base in subsets:
            r = r[subsets[base][0]:subsets[base][1]]
        per_locus.append(r)
        if progress:
            progress()
    tables = _tables_for_rates(eng, run, per_locus)
    tuples = run.tuples(rate_files, per_locus, tables)
    return (tuples, tables) if return_tables else tuples


def _locus_models(L, pi, exch, model):
    """pi [L, 4] and exch [L, 6] (one row of six serves every locus) of the quartet stages' plans; exch None under "f81"."""
    if model not in ("gtr", "f81"):
        raise PipelineError("unknown model %r" % (model,))
    pi = np.asarray(pi, dtype=np.float64).reshape(L, 4)
    if model == "gtr":
        exch = np.asarray(exch, dtype=np.float64)
        exch = np.tile(exch, (L, 1)) if exch.ndim == 1 else exch.reshape(L, 6)
    else:
        exch = None
    return pi, exch


def _tables_for_rates(eng, run, per_locus):
    """PI tables for already-final rates (NaN = culled): tphip_pi_tables with no rounding/correction/cull."""
    with run.final_rates_plan(eng, per_locus) as (plan, rates, _):
        return plan.pi_tables(rates, None)


def bootstrap_tables(eng, per_locus, run, locus_ids, replicates, seed=1, level=0.95):
    """Site-bootstrap summaries [L, 4, T + n_i] (mean, sd, lo, hi of the net-PI profile and of the interval integrals) for
    already-final rates (NaN = culled), on a no-rounding plan exactly as _tables_for_rates: every path that ends in
    per-locus final rates (streamed or not, --subset-pi-map-file, --site-rates, --rate-estimator eb) is served without
    being touched.  locus_ids: the generator's stream id per locus -- the command line passes the global file indices, so
    a locus' bands do not depend on which rank, or which loci beside it, it was computed with.  The locus' model (and under
    eb the fitted prior) are held fixed: the bands are conditional on them."""
    if len(per_locus) == 0:
        return np.zeros((0, 4, run.band_width))
    with run.final_rates_plan(eng, per_locus, times=[]) as (plan, rates, _):
        return plan.pi_bootstrap(rates, None, replicates=replicates, seed=seed, level=level,
                                 locus_ids=np.asarray(locus_ids, dtype=np.int64))


def _band_models(models, L):
    """run_alignments' out["models"] as (model, pi [L, 4], exch [L, 6] or None under "f81")."""
    model = models["model"]
    pi = np.asarray(models["pi"], dtype=np.float64).reshape(L, 4)
    return model, pi, None if model == "f81" else np.asarray(models["exch"], dtype=np.float64).reshape(L, 6)


def _observed_blocks(run, alignments, per_locus, subsets, budget):
    """The loci's observed columns in blocks of at most `budget` columns (one locus at least): yields (l0, l1, states, offsets)
    with the alignments l0..l1 re-read, sliced as run_alignments slices the rates for `subsets`, and held against the
    lengths of the final rates."""
    L, l0 = len(alignments), 0
    while l0 < L:
        l1, cols = l0, 0
        while l1 < L and (l1 == l0 or cols + len(per_locus[l1]) <= budget):
            cols += len(per_locus[l1])
            l1 += 1
        states, off = load_alignments(alignments[l0:l1], run.leaf_names)
        blocks = []
        for k, a in enumerate(alignments[l0:l1]):
            blk = states[:, off[k]:off[k + 1]]
            base = os.path.basename(a)
            if base in subsets:
                blk = blk[:, subsets[base][0]:subsets[base][1]]
            if blk.shape[1] != len(per_locus[l0 + k]):
                raise PipelineError("{0}: {1} columns, but {2} final rates".format(base, blk.shape[1], len(per_locus[l0 + k])))
            blocks.append(blk)
        yield (l0, l1, np.ascontiguousarray(np.concatenate(blocks, axis=1)),
               np.concatenate([[0], np.cumsum([b.shape[1] for b in blocks])]).astype(np.int64))
        l0 = l1


PARBOOT_BLOCK_COLS = 1 << 24   # columns per plan of parametric_bootstrap_tables


def parametric_bootstrap_tables(eng, alignments, per_locus, models, run, locus_ids, replicates, seed=1, level=0.95, subsets=None,
                                output_dir=None):
    """Parametric bootstrap of the site rates and the PI rows: every column of every locus is
    simulated `replicates` times down the tree under the locus' model at its own rate, with the observed pattern of missing
    cells, its rate re-estimated and the PI row recomputed.  Returns the summaries [L, 4, T + n_i] (mean, sd, lo, hi) and,
    per locus, the (mean, sd) of every site's final rate over the replicates (NaN for culled sites); with output_dir the
    latter are also written as NAME.rates-bootstrap.json beside the `.rates` files.

    alignments: the loci's NEXUS files, re-read here and sliced as run_alignments slices the rates for `subsets`
    (--subset-pi-map-file).  per_locus: the run's final rates (rounded, / correction, NaN = culled); the raw rate of the
    simulation is final rate x correction, so a culled column comes out all missing and is culled again.  models:
    run_alignments' out["models"].  The plans carry the run's real correction, threshold, round_decimals and start rule.  The
    loci go through in blocks of at most 2^24 columns; a column's bytes do not depend on the loci beside it, so the blocking
    changes no bit.  locus_ids: the generator's stream ids -- the command line passes the global file indices.  The models and
    the tree are held fixed (no stage-1 refit per replicate): the bands are conditional on the fitted substitution model."""
    L = len(alignments)
    summary = np.zeros((L, 4, run.band_width))
    moments = []
    if L == 0:
        return summary, moments
    model, pi, exch = _band_models(models, L)
    ids = np.asarray(locus_ids, dtype=np.int64)
    for l0, l1, states, offsets in _observed_blocks(run, alignments, per_locus, subsets or {}, PARBOOT_BLOCK_COLS):
        raw = np.concatenate(per_locus[l0:l1]) * run.correction
        plan = run.plan(eng, offsets, pi[l0:l1], None if exch is None else exch[l0:l1], times=[], model=model)
        try:
            s, mean, sd = plan.pi_parametric_bootstrap(raw, states, replicates=replicates, seed=seed, level=level,
                                                       locus_ids=ids[l0:l1], return_rate_moments=True)
        finally:
            plan.close()
        summary[l0:l1] = s
        for k in range(l1 - l0):
            moments.append((mean[offsets[k]:offsets[k + 1]], sd[offsets[k]:offsets[k + 1]]))
    if output_dir is not None:
        for a, (mean, sd) in zip(alignments, moments):
            _write_rate_moments_file(os.path.join(output_dir, os.path.basename(a) + ".rates-bootstrap.json"), mean, sd)
    return summary, moments


# posterior_pi_tables works through the loci in blocks whose category posterior ([K][columns] doubles) stays within this many
# bytes of device memory
POSTERIOR_PI_BYTES = 256 << 20


def posterior_pi_tables(eng, alignments, per_locus, models, ebfit, run, locus_ids, replicates, seed=1, level=0.95, subsets=None):
    """The empirical-Bayes rate posterior carried into the PI rows, beside bootstrap_tables: per locus
    the analytic mean and sd of the net-PI profile and of the interval integrals under the posterior of the sites' rate
    categories, and the band [lo, hi] of `replicates` posterior draws.  Returns dict(bands [L, 4, T + n_i] = mean, sd, lo, hi;
    category_rate [L, K] = the categories' final rates; expected_sites [L, K] = the informative sites expected in each).

    alignments: the loci's NEXUS files, re-read here and sliced for `subsets` as parametric_bootstrap_tables does (a column's
    posterior depends on the column and the locus' fit only).  per_locus: the run's final rates (their lengths are checked).
    models: run_alignments' out["models"]; ebfit: its out["eb"] (alpha, scale, categories).  The plans carry the run's real
    correction, threshold and round_decimals.  The loci go through in blocks whose [K][columns] table fits
    POSTERIOR_PI_BYTES; a locus' results depend on nothing beside it, so the blocking changes no bit.  locus_ids: the
    generator's stream ids -- the command line passes the global file indices.  Everything is conditional on the fitted
    (scale, alpha), the model and the tree: the bands carry the posterior of the sites' rates, not the uncertainty of the fit."""
    from . import eb
    L = len(alignments)
    K = int(ebfit["categories"]) if L else 0
    out = dict(bands=np.zeros((L, 4, run.band_width)), category_rate=np.zeros((L, K)), expected_sites=np.zeros((L, K)))
    if L == 0:
        return out
    model, pi, exch = _band_models(models, L)
    alpha = np.asarray(ebfit["alpha"], dtype=np.float64).reshape(L)
    scale = np.asarray(ebfit["scale"], dtype=np.float64).reshape(L)
    ids = np.asarray(locus_ids, dtype=np.int64)
    for l0, l1, states, offsets in _observed_blocks(run, alignments, per_locus, subsets or {}, max(1, POSTERIOR_PI_BYTES // (8 * K))):
        plan = run.plan(eng, offsets, pi[l0:l1], None if exch is None else exch[l0:l1], times=[], start_rule=False, model=model)
        try:
            table = eb.posterior_table(plan, states, alpha[l0:l1], scale[l0:l1], ncat=K)
            res = eb.posterior_pi(plan, table, alpha[l0:l1], scale[l0:l1], replicates, seed=seed, level=level, locus_ids=ids[l0:l1])
            kappa = np.asarray(plan.models()[3], dtype=np.float64)
        finally:
            plan.close()
        out["bands"][l0:l1, :2] = res["analytic"]
        out["bands"][l0:l1, 2:] = res["summary"][:, 2:]
        out["expected_sites"][l0:l1] = res["expected_counts"]
        out["category_rate"][l0:l1] = run.corrected((kappa * scale[l0:l1])[:, None] * eb.gamma_tables(alpha[l0:l1], K)[0])[1]
    return out


def _write_rate_moments_file(path, mean, sd):
    """NAME.rates-bootstrap.json: mean and sd of every site's final rate over the parametric replicates, null for culled sites."""
    import json
    clean = lambda v: [None if x != x else x for x in np.asarray(v, dtype=np.float64).tolist()]   # noqa: E731
    with open(path, "w") as fh:
        json.dump({"mean": clean(mean), "sd": clean(sd)}, fh)


def quartet_tables(eng, per_locus, pi, exch, run, quartets, model="gtr"):
    """Quartet signal and noise rows [L, n_q, 8] (Y, X, Yy, Xx, XY, p_correct, p_incorrect, p_polytomy; DESIGN.md section
    3.6) for already-final rates (NaN = culled), on a no-rounding plan exactly as bootstrap_tables: every path that ends in
    per-locus final rates is served without being touched.  Unlike the PI stage this one needs the loci's models: pi [L, 4]
    and exch [L, 6] (model "gtr"), or pi alone with exch None (model "f81": exchangeabilities of 1; Jukes-Cantor is pi = 1/4).
    quartets: [n_q, 2] rows (T, t_o) in the tree's original time units, the units of --times.  A locus' rows depend on its
    rates, its model and the quartets only, so they do not depend on which rank, or which loci beside it, it was computed
    with."""
    quartets = np.asarray(quartets, dtype=np.float64).reshape(-1, 2)
    L = len(per_locus)
    if L == 0:
        return np.zeros((0, len(quartets), 8))
    pi, exch = _locus_models(L, pi, exch, model)
    with run.final_rates_plan(eng, per_locus, pi=pi, exch=exch, model=model) as (plan, rates, _):
        return plan.quartet_tables(rates, None, quartets)


def unequal_quartet_tables(eng, per_locus, pi, exch, run, quartets, model="gtr"):
    """Rows [L, n_q, 13] of quartets with unequal tips (the sums of y, x1, x2, y^2, x1^2, x2^2, y x1, y x2, x1 x2, then
    p_correct, p_ac, p_ad, p_polytomy) for already-final rates, on a no-rounding plan exactly as
    quartet_tables.  quartets: [n_q, 5] rows (Ta, Tb, Tc, Td, t_o) in the tree's original time units; a list longer than
    the engine's 256 goes through in calls of at most 256.  A locus' rows depend on its rates, its model and the quartet
    only, so neither the split nor the rank or the loci beside it change them."""
    quartets = np.asarray(quartets, dtype=np.float64).reshape(-1, 5)
    L = len(per_locus)
    if L == 0 or len(quartets) == 0:
        return np.zeros((L, len(quartets), 13))
    pi, exch = _locus_models(L, pi, exch, model)
    with run.final_rates_plan(eng, per_locus, pi=pi, exch=exch, model=model) as (plan, rates, _):
        return np.concatenate([plan.unequal_quartet_tables(rates, None, quartets[q0:q0 + 256])
                               for q0 in range(0, len(quartets), 256)], axis=1)


# exact_quartet_tables works through the quartets in tiles: the dense per-site planes of a tile ([2 or 3][tile][ncols] doubles)
# and the exact call's workspace each stay within this many bytes of device memory
EXACT_QUARTET_BYTES = 256 << 20


def exact_quartet_tile(L, ncols, n_q, planes, window_cap):
    """Quartets per tile: the most (up to the engine's 256) for which the planes and the workspace of the exact call (32 bytes
    per (locus, quartet) pair and 24 per pair and tile of 512 frequencies at the cap) each fit EXACT_QUARTET_BYTES, and the
    call's pairs its limit of 2^24; at least one."""
    tiles = (window_cap * (window_cap // 2 + 1) + 511) // 512
    fit = min(EXACT_QUARTET_BYTES // max(1, 8 * planes * ncols), EXACT_QUARTET_BYTES // max(1, L * (32 + 24 * tiles)),
              (1 << 24) // max(1, L))
    return int(max(1, min(256, n_q, fit)))


def _exact_quartet_tables(eng, per_locus, pi, exch, run, quartets, model, window_cap, unequal):
    L, n_q, device = len(per_locus), len(quartets), run.device
    if L == 0 or n_q == 0:
        return np.zeros((L, n_q, 6))
    pi, exch = _locus_models(L, pi, exch, model)
    with run.final_rates_plan(eng, per_locus, pi=pi, exch=exch, model=model) as (plan, rates, offsets):
        ncols, planes = int(offsets[-1]), 3 if unequal else 2
        tile = exact_quartet_tile(L, ncols, n_q, planes, window_cap)
        stream = eng.device_stream(device)
        d_rates = eng.device_array(rates, device)
        d_flat = eng.device_empty((planes * tile * ncols,), device)
        d_ws = eng.device_empty((plan.quartet_exact_workspace_bytes(tile, window_cap),), device, np.uint8)
        out = np.zeros((L, n_q, 6))
        for q0 in range(0, n_q, tile):
            part = quartets[q0:q0 + tile]
            k = len(part)
            d_sites = d_flat[:planes * k * ncols].reshape(planes, k, ncols)   # (a view: the last tile may be shorter)
            (plan.unequal_quartet_sites_dev if unequal else plan.quartet_sites_dev)(d_rates, None, part, d_sites, stream)
            d_rows = eng.device_empty((L, k, 6), device)
            plan.quartet_exact_dev(d_sites[0], d_sites[1], d_sites[planes - 1], k, d_rows, d_ws, window_cap, 0.0, stream)
            out[:, q0:q0 + k] = eng.host_array(d_rows)
        return out


def exact_quartet_tables(eng, per_locus, pi, exch, run, quartets, model="gtr", window_cap=128):
    """Exact resolution probabilities beside quartet_tables: rows [L, n_q, 6] (p_correct, p_ac, p_ad, p_polytomy, window,
    tail_bound) from the same final rates on the same no-rounding plan.  Per tile of quartets
    (exact_quartet_tile) the per-site planes are written by quartet_sites_dev and read by quartet_exact_dev where they lie;
    only the rows leave the device.  With equal tips p_ac = p_ad up to rounding (one noise plane serves both).  A pair whose
    law does not fit window_cap has NaN probabilities and window 0.  A locus' rows depend on its rates, its model, the
    quartet and window_cap only."""
    return _exact_quartet_tables(eng, per_locus, pi, exch, run, np.asarray(quartets, dtype=np.float64).reshape(-1, 2), model,
                                 window_cap, False)


def exact_unequal_quartet_tables(eng, per_locus, pi, exch, run, quartets, model="gtr", window_cap=128):
    """exact_quartet_tables for quartets [n_q, 5] (Ta, Tb, Tc, Td, t_o) beside unequal_quartet_tables; a list longer than the
    engine's 256 goes through in tiles like any other."""
    return _exact_quartet_tables(eng, per_locus, pi, exch, run, np.asarray(quartets, dtype=np.float64).reshape(-1, 5), model,
                                 window_cap, True)


# ---- locus-set accumulation curves ----------------------------------------------------------------
def locus_set_order(rows, names, order_file=None, max_k=None):
    """The order of the loci per quartet, int32 [n_q, K].  rows: the per-locus normal rows [L, n_q, 8] (quartet_tables) or
    [L, n_q, 13] (unequal_quartet_tables); names: the loci's names, in the rows' order.  Default: per quartet, descending
    per-locus normal-approximation p_correct, ties by ascending locus index (a stable argsort of -p_correct: the order never
    depends on the exact rows).  order_file: one locus name per line (blank lines skipped), the same order for every quartet;
    a name that is unknown or repeated is an error, loci that are not named are left out.  Then the order is cut to max_k."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 3 or rows.shape[2] not in (8, 13) or rows.shape[0] != len(names):
        raise PipelineError("locus_set_order: rows must be [L, n_q, 8] or [L, n_q, 13] with one row per name")
    L, n_q = rows.shape[:2]
    if max_k is not None and int(max_k) < 1:
        raise PipelineError("locus_set_order: max_k must be at least 1")
    if order_file is None:
        order = np.argsort(-rows[:, :, 5 if rows.shape[2] == 8 else 9].T, axis=1, kind="stable")
    else:
        index = {n: l for l, n in enumerate(names)}
        if len(index) != L:
            raise PipelineError("locus_set_order: the loci's names are not distinct, so an order file cannot name them")
        with open(order_file) as fh:
            listed = [line.strip() for line in fh if line.strip()]
        if not listed:
            raise PipelineError("{0} names no locus".format(order_file))
        for n in listed:
            if n not in index:
                raise PipelineError("{0}: unknown locus {1!r}".format(order_file, n))
        if len(set(listed)) != len(listed):
            raise PipelineError("{0}: a locus is named more than once".format(order_file))
        order = np.tile(np.array([index[n] for n in listed], dtype=np.int64), (n_q, 1))
    if max_k is not None:
        order = order[:, :int(max_k)]
    return np.ascontiguousarray(order, dtype=np.int32)


def locus_set_tables(eng, rows, order, device=0):
    """The normal rows of the sets order[q, :k], k = 1..K: [n_q, K, 8 or 13] in the per-locus rows' layout (their sums added
    left to right in the order given, the family's probability rule on those sums; engine.locus_set_rows).  rows: all loci's
    per-locus rows [L, n_q, 8 or 13].  A list longer than the engine's 256 quartets, or than 2^24 (locus, quartet) pairs, goes
    through in slices; a quartet's rows do not depend on the others, so the split changes nothing."""
    rows, order = np.asarray(rows, dtype=np.float64), np.asarray(order, dtype=np.int32)
    if order.size == 0:
        return np.zeros(order.shape + (rows.shape[2],))
    L, n_q = rows.shape[:2]
    step = int(max(1, min(256, (1 << 24) // max(1, L))))
    return np.concatenate([eng.locus_set_rows(rows[:, q0:q0 + step], order[q0:q0 + step], device)
                           for q0 in range(0, n_q, step)], axis=0)


def locus_set_tile(L, ncols, n_q, n_k, planes, window_cap):
    """(quartets per tile, n_head): the most quartets (up to the engine's 256) for which the per-site planes and the exact
    call's workspace at n_head = 1 (per quartet 48 bytes a locus, 36 a prefix, 2048 for the alignment of its five arrays, 24 a computed prefix and tile of 512
    frequencies at the cap) each fit EXACT_QUARTET_BYTES, and then the most prefixes per quartet that keep the workspace
    there; at least one of each."""
    tiles = (window_cap * (window_cap // 2 + 1) + 511) // 512
    fixed = 48 * L + 36 * n_k + 2048
    fit = min(EXACT_QUARTET_BYTES // max(1, 8 * planes * ncols), EXACT_QUARTET_BYTES // (fixed + 24 * tiles), (1 << 24) // max(1, L))
    tile = int(max(1, min(256, n_q, fit)))
    n_head = (EXACT_QUARTET_BYTES // tile - fixed) // (24 * tiles)
    return tile, int(max(1, min(n_k, n_head)))


def exact_locus_set_tables(eng, per_locus, pi, exch, run, quartets, order, model="gtr", window_cap=128, unequal=False):
    """The exact rows of the sets order[q, :k]: [n_q, K, 6] (p_correct, p_ac, p_ad, p_polytomy, window, tail_bound) on the
    torus M = window_cap, from the final rates of `per_locus` on a no-rounding plan exactly as exact_quartet_tables.
    quartets [n_q, 2] (T, t_o), or [n_q, 5] (Ta, Tb, Tc, Td, t_o) with unequal=True; order indexes per_locus.  Quartets go
    through in tiles (locus_set_tile): the planes are written by *_quartet_sites_dev and read by locus_set_exact_dev where
    they lie; only the rows leave the device.  A prefix that does not fit the cap, or lies beyond the tile's n_head, has NaN
    probabilities and window 0."""
    quartets = np.asarray(quartets, dtype=np.float64).reshape(-1, 5 if unequal else 2)
    order = np.ascontiguousarray(order, dtype=np.int32)
    L, n_q, device = len(per_locus), len(quartets), run.device
    if order.ndim != 2 or order.shape[0] != n_q:
        raise PipelineError("exact_locus_set_tables: order must be [n_q, K]")
    n_k = order.shape[1]
    if L == 0 or n_q == 0 or n_k == 0:
        return np.zeros((n_q, n_k, 6))
    pi, exch = _locus_models(L, pi, exch, model)
    with run.final_rates_plan(eng, per_locus, pi=pi, exch=exch, model=model) as (plan, rates, offsets):
        ncols, planes = int(offsets[-1]), 3 if unequal else 2
        tile, n_head = locus_set_tile(L, ncols, n_q, n_k, planes, window_cap)
        stream = eng.device_stream(device)
        d_rates = eng.device_array(rates, device)
        d_flat = eng.device_empty((planes * tile * ncols,), device)
        d_ws = eng.device_empty((plan.locus_set_exact_workspace_bytes(tile, n_k, window_cap, n_head),), device, np.uint8)
        out = np.zeros((n_q, n_k, 6))
        for q0 in range(0, n_q, tile):
            part = quartets[q0:q0 + tile]
            k = len(part)
            d_sites = d_flat[:planes * k * ncols].reshape(planes, k, ncols)   # (a view: the last tile may be shorter)
            (plan.unequal_quartet_sites_dev if unequal else plan.quartet_sites_dev)(d_rates, None, part, d_sites, stream)
            d_rows = eng.device_empty((k, n_k, 6), device)
            plan.locus_set_exact_dev(d_sites[0], d_sites[1], d_sites[planes - 1], order[q0:q0 + k], d_rows, d_ws, window_cap, 0.0,
                                     n_head, stream)
            out[q0:q0 + k] = eng.host_array(d_rows)
        return out


# concordance_tables works through the loci in blocks of at most this many columns whose counts ([loci][sets][3] 64-bit integers)
# stay within this many bytes
CONCORDANCE_BLOCK_COLS = 1 << 24
CONCORDANCE_COUNT_BYTES = 256 << 20


def concordance_tables(eng, alignments, per_locus, run, sets, subsets=None):
    """Site concordance factors of the loci at the tree's internodes: what the alignments show where
    the quartet stages predict.  Returns (rows [L, n_nodes, 12], totals uint64 [n_sets, 3]): per locus and internode pooled_c,
    pooled_1, pooled_2, near_c, near_1, near_2, sCF, sDF1, sDF2, sN, n_decisive, n_quartets (engine.concordance_rows), and
    the integer sum of the counts over these loci, from which the rows of all loci analysed as one alignment follow.

    alignments: the loci's NEXUS files, re-read here and sliced for `subsets` as parametric_bootstrap_tables does; every
    column of a locus counts, culled or not.  per_locus: the run's final rates (their lengths are checked).  sets:
    compute.concordance_sets' tables, the same for every locus.  The loci go through in blocks of at most
    CONCORDANCE_BLOCK_COLS columns whose counts fit CONCORDANCE_COUNT_BYTES; a locus' counts depend on nothing beside it, so
    the blocking changes no bit.  A locus and internode with ncols * |A||B||C||D| >= 2^53 is refused: its counts might not
    convert to fp64 exactly."""
    L = len(alignments)
    node_sets = np.asarray(sets["node_sets"], dtype=np.int64)
    n_nodes, n_sets = len(node_sets) - 1, int(node_sets[-1])
    rows = np.zeros((L, n_nodes, 12))
    totals = np.zeros((n_sets, 3), dtype=np.uint64)
    if L == 0 or n_nodes == 0:
        return rows, totals
    most = max(int(np.prod([int(v) for v in s])) for s in sets["sizes"])
    for a, r in zip(alignments, per_locus):
        if len(r) * most >= 2 ** 53:
            raise PipelineError("{0}: {1} columns times {2} quartets around an internode reach 2^53: the concordance counts "
                                "would not convert exactly".format(os.path.basename(a), len(r), most))
    step = max(1, CONCORDANCE_COUNT_BYTES // (24 * n_sets))
    for l0, l1, states, offsets in _observed_blocks(run, alignments, per_locus, subsets or {}, CONCORDANCE_BLOCK_COLS):
        for k0 in range(0, l1 - l0, step):
            k1 = min(l1 - l0, k0 + step)
            part = states if (k0, k1) == (0, l1 - l0) else np.ascontiguousarray(states[:, offsets[k0]:offsets[k1]])
            counts = eng.concordance_counts(part, offsets[k0:k1 + 1] - offsets[k0], sets["group_offsets"], sets["group_taxa"],
                                            device=run.device)
            rows[l0 + k0:l0 + k1] = eng.concordance_rows(counts, node_sets, device=run.device)
            totals += counts.sum(axis=0, dtype=np.uint64)
    return rows, totals


def dot_progress():
    sys.stdout.write(".")
    sys.stdout.flush()

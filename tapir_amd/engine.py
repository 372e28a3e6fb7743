"""ctypes binding of libtphip.so (include/tphip.h) -- the MI355X site-rate + PI engine.

This replaces, for every locus at once, what `worker()` does per locus in the reference
(bin/tapir_compute.py:84-123): the HyPhy subprocess (Popen + JSON file round trip) and the numpy/scipy
PI arithmetic.  There is deliberately no CPU fallback: if the shared library is missing, or no GPU is
visible, every entry point raises.
"""
import collections
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TPHIP_LIB: another build of the library (same-box A/B comparisons of kernel variants, tools/ only)
LIB_PATH = os.environ.get("TPHIP_LIB") or os.path.join(_HERE, "libtphip.so")

FLAG_OK, FLAG_FLAT, FLAG_SATURATED, FLAG_ZERO, FLAG_MAXIT = 0, 1, 2, 3, 4
START_AUTO, START_REFERENCE, START_PARSIMONY = 0, 1, 2
DEDUP_AUTO, DEDUP_OFF, DEDUP_ON = 0, 1, 2
INTEG_QUADPACK, INTEG_CLOSED = 0, 1
MODEL_GTR, MODEL_F81 = 0, 1
MODELS = {"gtr": MODEL_GTR, "f81": MODEL_F81}

_vp = ctypes.c_void_p
_i32, _i64, _f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double


class TphipError(Exception):
    """An error reported by libtphip (message from tphip_last_error)."""


class PlanDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", _i32), ("ntaxa", _i32), ("nnodes", _i32), ("parent", _vp), ("branch_len", _vp),
                ("leaf_taxon", _vp), ("nloci", _i64), ("locus_offsets", _vp), ("pi", _vp), ("exch", _vp),
                ("T", _i32), ("times", _vp), ("n_t", _i32), ("intervals", _vp), ("n_i", _i32),
                ("integ_mode", _i32), ("correction", _f64), ("threshold", _i32), ("round_decimals", _i32),
                ("ncat", _i32), ("cat_rate", _vp), ("cat_weight", _vp), ("start_rule", _i32),
                ("pattern_dedup", _i32), ("model", _i32)]


class Stage1Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("maxit_grm", _i32), ("maxit_sub", _i32), ("no_prune", _i32),
                ("fd_step", _f64), ("free_root_pair", _i32), ("compress_patterns", _i32), ("empirical_pi", _i32),
                ("row_pitch", _i64)]


class EbOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("ncat", _i32), ("maxit_scale", _i32), ("use_patterns", _i32),
                ("tol_scale", _f64)]


class BootstrapOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("replicates", _i32), ("level", _f64), ("seed", ctypes.c_uint64),
                ("locus_ids", _vp)]


class PosteriorPiOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("replicates", _i32), ("level", _f64), ("seed", ctypes.c_uint64),
                ("locus_ids", _vp), ("ncat", _i32)]


class QuartetOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_q", _i32), ("tip", _vp), ("internode", _vp)]


class UnequalQuartetOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_q", _i32), ("tips", _vp), ("internode", _vp)]


class QuartetExactOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_q", _i32), ("window_cap", _i32), ("tail_tolerance", _f64)]


class LocusSetOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_q", _i32), ("n_k", _i32), ("family", _i32), ("window_cap", _i32),
                ("tail_tolerance", _f64), ("n_head", _i32), ("order", _vp)]


class SimulateOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("replicate", _i32), ("seed", ctypes.c_uint64), ("locus_ids", _vp)]


class ParbootOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("replicates", _i32), ("level", _f64), ("seed", ctypes.c_uint64),
                ("locus_ids", _vp)]


class ConcordanceSets(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_sets", _i64), ("group_offsets", _vp), ("group_taxa", _vp)]


# every symbol include/tphip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("tphip_version", ctypes.c_int, []),
    ("tphip_last_error", ctypes.c_char_p, []),
    ("tphip_device_count", ctypes.c_int, []),
    ("tphip_plan_create", ctypes.c_int, [ctypes.POINTER(PlanDesc), ctypes.POINTER(_vp)]),
    ("tphip_plan_destroy", ctypes.c_int, [_vp]),
    ("tphip_plan_table_width", _i32, [_vp]),
    ("tphip_plan_ncols", _i64, [_vp]),
    ("tphip_plan_workspace_bytes", ctypes.c_size_t, [_vp]),
    ("tphip_plan_chrono_length", _f64, [_vp]),
    ("tphip_plan_stack_depth", _i32, [_vp]),
    ("tphip_plan_op_counts", ctypes.c_int, [_vp, _vp]),
    ("tphip_plan_cherry_count", _i32, [_vp]),
    ("tphip_plan_get_models", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("tphip_site_rates_dev", ctypes.c_int, [_vp] * 8 + [ctypes.c_size_t, _vp]),
    ("tphip_pi_tables_dev", ctypes.c_int, [_vp] * 5 + [ctypes.c_size_t, _vp]),
    ("tphip_run_dev", ctypes.c_int, [_vp] * 9 + [ctypes.c_size_t, _vp]),
    ("tphip_townsend_pi_dense_dev", ctypes.c_int, [_i32, _vp, _i64, _vp, _i32, _vp, _vp]),
    ("tphip_quad_townsend_dev", ctypes.c_int, [_i32, _vp, _i64, _f64, _f64, _i32, _vp, _vp, _vp]),
    ("tphip_locus_loglik_dev", ctypes.c_int, [_vp, _vp, _i64] + [_vp] * 9),
    ("tphip_locus_gradient_dev", ctypes.c_int, [_vp, _vp, _i64] + [_vp] * 13),
    ("tphip_state_histogram_dev", ctypes.c_int, [_i32, _vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    ("tphip_profile_enable", ctypes.c_int, [_vp, _i32]),
    ("tphip_profile_read", ctypes.c_int, [_vp, ctypes.POINTER(_f64), ctypes.POINTER(_f64), ctypes.POINTER(_i64), _i32]),
    ("tphip_last_eval_count", ctypes.c_int, [_vp, ctypes.POINTER(_i64)]),
    ("tphip_last_round_count", ctypes.c_int, [_vp, ctypes.POINTER(_i64)]),
    ("tphip_host_alloc", _vp, [ctypes.c_size_t]),
    ("tphip_host_free", ctypes.c_int, [_vp]),
    ("tphip_site_rates", ctypes.c_int, [_vp] * 7),
    ("tphip_pi_tables", ctypes.c_int, [_vp] * 4),
    ("tphip_run_fused", ctypes.c_int, [_vp] * 8),
    ("tphip_run_fused_pitched", ctypes.c_int, [_vp, _vp, _i64] + [_vp] * 6),
    ("tphip_townsend_pi_dense", ctypes.c_int, [_i32, _vp, _i64, _vp, _i32, _vp]),
    ("tphip_quad_townsend", ctypes.c_int, [_i32, _vp, _i64, _f64, _f64, _i32, _vp, _vp]),
    ("tphip_state_histogram", ctypes.c_int, [_i32, _vp, _i64, _i32, _vp, _i64, _vp]),
    ("tphip_eval_columns", ctypes.c_int, [_vp] * 6),
    ("tphip_eval_columns_dev", ctypes.c_int, [_vp] * 7),
    ("tphip_corrected_rates_dev", ctypes.c_int, [_vp] * 5),
    ("tphip_corrected_rates", ctypes.c_int, [_vp] * 4),
    ("tphip_locus_loglik", ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), _i64, _vp, _i64] + [_vp] * 7),
    ("tphip_plan_set_column_weights", ctypes.c_int, [_vp, _vp]),
    ("tphip_compress_columns", ctypes.c_int, [ctypes.c_int32, _vp, _i64, ctypes.c_int32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("tphip_locus_gradient", ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), _i64, _vp, _i64] + [_vp] * 11),
    ("tphip_free_device", ctypes.c_int, [_vp, _vp]),
    ("tphip_stage1_fit_dev", ctypes.c_int, [_vp, _vp, ctypes.POINTER(Stage1Opts)] + [_vp] * 10),
    ("tphip_stage1_fit", ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(Stage1Opts)] + [_vp] * 9),
    ("tphip_plan_set_models", ctypes.c_int, [_vp, _vp, _vp]),
    ("tphip_eb_start_scale", ctypes.c_int, [_vp, _vp, _vp]),
    ("tphip_eb_start_scale_dev", ctypes.c_int, [_vp, _vp, _vp, _vp]),
    ("tphip_eb_fit_scale", ctypes.c_int, [_vp, _vp, ctypes.POINTER(EbOpts), _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tphip_eb_fit_scale_dev", ctypes.c_int, [_vp, _vp, ctypes.POINTER(EbOpts), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tphip_eb_posterior", ctypes.c_int, [_vp, _vp, ctypes.POINTER(EbOpts), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tphip_eb_posterior_dev", ctypes.c_int, [_vp, _vp, ctypes.POINTER(EbOpts), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tphip_eb_posterior_table", ctypes.c_int, [_vp, _vp, ctypes.POINTER(EbOpts)] + [_vp] * 8),
    ("tphip_eb_posterior_table_dev", ctypes.c_int, [_vp, _vp, ctypes.POINTER(EbOpts)] + [_vp] * 9),
    ("tphip_posterior_pi_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(PosteriorPiOpts), ctypes.POINTER(ctypes.c_size_t),
                                                          ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_posterior_pi_dev", ctypes.c_int, [_vp] * 5 + [ctypes.POINTER(PosteriorPiOpts)] + [_vp] * 6 + [ctypes.c_size_t, _vp]),
    ("tphip_posterior_pi", ctypes.c_int, [_vp] * 5 + [ctypes.POINTER(PosteriorPiOpts)] + [_vp] * 5),
    ("tphip_bootstrap_width", _i32, [_vp]),
    ("tphip_bootstrap_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(BootstrapOpts), ctypes.POINTER(ctypes.c_size_t),
                                                       ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_pi_resample_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, ctypes.c_size_t, _vp]),
    ("tphip_pi_bootstrap_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(BootstrapOpts), _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("tphip_pi_resample", ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _vp]),
    ("tphip_pi_bootstrap", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(BootstrapOpts), _vp, _vp]),
    ("tphip_bootstrap_counts", ctypes.c_int, [_i32, ctypes.c_uint64, _i64, _i64, _i64, _i32, _vp]),
    ("tphip_quartet_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(QuartetOpts), ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_quartet_tables_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(QuartetOpts), _vp, _vp, ctypes.c_size_t, _vp]),
    ("tphip_quartet_sites_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(QuartetOpts), _vp, _vp]),
    ("tphip_quartet_tables", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(QuartetOpts), _vp]),
    ("tphip_quartet_sites", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(QuartetOpts), _vp]),
    ("tphip_unequal_quartet_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(UnequalQuartetOpts), ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_unequal_quartet_tables_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(UnequalQuartetOpts), _vp, _vp, ctypes.c_size_t, _vp]),
    ("tphip_unequal_quartet_sites_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(UnequalQuartetOpts), _vp, _vp]),
    ("tphip_unequal_quartet_tables", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(UnequalQuartetOpts), _vp]),
    ("tphip_unequal_quartet_sites", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(UnequalQuartetOpts), _vp]),
    ("tphip_quartet_exact_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(QuartetExactOpts), ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_quartet_exact_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(QuartetExactOpts), _vp, _vp, ctypes.c_size_t, _vp]),
    ("tphip_quartet_exact", ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(QuartetExactOpts), _vp]),
    ("tphip_locus_set_rows_dev", ctypes.c_int, [_i32, _vp, _i64, ctypes.POINTER(LocusSetOpts), _vp, _vp]),
    ("tphip_locus_set_rows", ctypes.c_int, [_i32, _vp, _i64, ctypes.POINTER(LocusSetOpts), _vp]),
    ("tphip_locus_set_exact_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(LocusSetOpts), ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_locus_set_exact_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(LocusSetOpts), _vp, _vp, ctypes.c_size_t, _vp]),
    ("tphip_locus_set_exact", ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(LocusSetOpts), _vp]),
    ("tphip_simulate_columns_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(SimulateOpts), _vp, _vp]),
    ("tphip_simulate_columns", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(SimulateOpts), _vp]),
    ("tphip_parboot_workspace_bytes", ctypes.c_int, [_vp, ctypes.POINTER(ParbootOpts), ctypes.POINTER(ctypes.c_size_t)]),
    ("tphip_pi_parametric_bootstrap_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ParbootOpts), _vp, _vp, _vp, _vp, _vp,
                                                         ctypes.c_size_t, _vp]),
    ("tphip_pi_parametric_bootstrap", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ParbootOpts), _vp, _vp, _vp, _vp]),
    ("tphip_summarize_rows_dev", ctypes.c_int, [_i32, _vp, _i64, _i32, _i32, _f64, _vp, _vp]),
    ("tphip_summarize_rows", ctypes.c_int, [_i32, _vp, _i64, _i32, _i32, _f64, _vp]),
    ("tphip_concordance_counts_dev", ctypes.c_int, [_i32, _vp, _i64, _i64, _i32, _vp, _i64, ctypes.POINTER(ConcordanceSets), _vp, _vp]),
    ("tphip_concordance_counts", ctypes.c_int, [_i32, _vp, _i64, _i64, _i32, _vp, _i64, ctypes.POINTER(ConcordanceSets), _vp]),
    ("tphip_concordance_rows_dev", ctypes.c_int, [_i32, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    ("tphip_concordance_rows", ctypes.c_int, [_i32, _vp, _i64, _i64, _vp, _i64, _vp]),
]

_lib = None


def _preload_torch_hip_runtime():
    """Make sure the process ends up with ONE HIP/ROCr runtime whatever the import order.

    A process can host one ROCr: a second copy fails to acquire the GPU's VM from KFD and its hipGetDeviceCount
    reports no devices.  PyTorch-ROCm wheels bundle their own runtime (torch/lib/libamdhip64.so, SONAME
    libamdhip64.so.7) and request it by the UN-versioned file name; libtphip.so requests `libamdhip64.so.7`.  When
    torch is imported first the loader satisfies libtphip's request by SONAME from torch's copy; when libtphip.so is
    loaded first it binds /opt/rocm's copy, torch's later request for "libamdhip64.so" matches neither that name nor
    that SONAME, a second runtime is mapped, and torch then raises "No HIP GPUs are available" (seen in round 1 when
    GPU tests touched the engine before torch).  Loading torch's copy by path first makes both orders the first one.
    torch itself is not imported here."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load libtphip.so (built in-tree by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TphipError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(the engine has no CPU fallback)" % LIB_PATH)
        _preload_torch_hip_runtime()
        lib = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc):
    if rc != 0:
        raise TphipError("libtphip error %d: %s" % (rc, load().tphip_last_error().decode("utf-8", "replace")))


def device_count():
    return load().tphip_device_count()


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    """Device pointer of a torch tensor, host pointer of a numpy array, or None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise TphipError("array passed to libtphip is not C-contiguous")
        return a.ctypes.data
    if not a.is_contiguous():   # the library sees only the pointer: a strided tensor would be read as garbage
        raise TphipError("tensor passed to libtphip is not contiguous")
    return a.data_ptr()


def _nbytes(t):
    """Byte size of a device tensor (a workspace)."""
    return t.numel() * t.element_size()


def _size_out(fn, *args):
    """fn(*args, &n) of a *_workspace_bytes entry point: n."""
    n = ctypes.c_size_t()
    _check(fn(*args, ctypes.byref(n)))
    return n.value


def _size_pair(fn, *args):
    """fn(*args, &min, &preferred) of a *_workspace_bytes entry point that blocks over its workspace: (min, preferred)."""
    mn, pf = ctypes.c_size_t(), ctypes.c_size_t()
    _check(fn(*args, ctypes.byref(mn), ctypes.byref(pf)))
    return mn.value, pf.value


def _ws_nbytes(d_ws, ws_bytes):
    """How much of the workspace d_ws a call may use: ws_bytes, by default all of it."""
    return _nbytes(d_ws) if ws_bytes is None else int(ws_bytes)


def _candidates(blen_vecs, cand_locus, cand_exch, cand_vec, cand_scale, cand_pidx, cand_pfac):
    """The candidate arrays of locus_loglik / locus_gradient as the library reads them, defaults filled in: (bv, cl, ce, cv, cs, ci, cf)."""
    bv = _np(blen_vecs, np.float64)
    bv = bv.reshape(-1, bv.shape[-1])
    cl = _np(cand_locus, np.int32).reshape(-1)
    n = len(cl)
    ce = _np(cand_exch, np.float64).reshape(n, 6)
    cv = _np(np.arange(n) if cand_vec is None else cand_vec, np.int32).reshape(n)
    cs = _np(np.ones(n) if cand_scale is None else cand_scale, np.float64).reshape(n)
    ci = _np(np.full(n, -1) if cand_pidx is None else cand_pidx, np.int32).reshape(n)
    cf = _np(np.ones(n) if cand_pfac is None else cand_pfac, np.float64).reshape(n)
    return bv, cl, ce, cv, cs, ci, cf


class _Pinned:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                load().tphip_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """numpy array in pinned host memory (tphip_host_alloc): the host-pointer calls then copy by direct DMA and overlap
    the result copies with the PI kernels.  Falls back to ordinary memory when pinning fails."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    ptr = load().tphip_host_alloc(max(n, 1))
    if not ptr:
        return np.empty(shape, dtype)
    holder = _Pinned(ptr)
    buf = (ctypes.c_char * max(n, 1)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    _PINNED_HOLDERS[id(buf)] = holder   # keep the allocation alive as long as the ctypes buffer (= the array's base) lives
    import weakref
    weakref.finalize(buf, _PINNED_HOLDERS.pop, id(buf), None)
    return arr


_PINNED_HOLDERS = {}


# Device buffers for callers that chain `_dev` calls without holding torch themselves (pipeline.exact_quartet_tables): torch
# tensors on the plan's device, in torch's current stream there.
def device_empty(shape, device, dtype=np.float64):
    import torch
    return torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=torch.device("cuda", int(device)))


def device_array(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", int(device)))


def host_array(t):
    """numpy copy of a device buffer (waits for the work enqueued on its stream)."""
    return t.cpu().numpy()


def device_stream(device):
    import torch
    return torch.cuda.current_stream(int(device)).cuda_stream


class Plan:
    """Tree program + per-locus GTR models + PI schedule on one device (tphip_plan_*).

    parent / branch_len / leaf_taxon: post-order tree arrays (branch lengths already / correction).
    locus_offsets: [L+1] column ranges; pi [L,4]; exch [L,6] in AC,AG,AT,CG,CT,GT order.
    times / intervals: the --times and --intervals of bin/tapir_compute.py:27-33.
    model: "gtr" (the locus' GTR model) or "f81" (exchangeabilities of 1, closed-form site-rate kernel; exch must be
    None -- Jukes-Cantor is "f81" with pi = 1/4 each).
    """

    def __init__(self, ntaxa, parent, branch_len, leaf_taxon, locus_offsets, pi, exch, T, times, intervals,
                 correction=1.0, threshold=3, round_decimals=4, integ_mode=INTEG_QUADPACK, device=0, cat_rates=None,
                 cat_weights=None, start_rule=START_AUTO, pattern_dedup=DEDUP_AUTO, model="gtr"):
        if model not in MODELS:
            raise TphipError("model must be one of %s" % sorted(MODELS))
        lib = load()
        self._lib = lib
        self._h = _vp()
        self._keep = dict(parent=_np(parent, np.int32), blen=_np(branch_len, np.float64),
                          leaf=_np(leaf_taxon, np.int32), off=_np(locus_offsets, np.int64),
                          pi=_np(pi, np.float64).reshape(-1),
                          exch=None if exch is None else _np(exch, np.float64).reshape(-1),
                          times=_np(times, np.int32).reshape(-1), iv=_np(intervals, np.int32).reshape(-1))
        k = self._keep
        ncat = 0 if cat_rates is None else len(cat_rates)
        if ncat > 1:   # opt-in rate mixture on top of the site rate (not in the reference; see include/tphip.h)
            k["cr"] = _np(cat_rates, np.float64).reshape(-1)
            k["cw"] = _np(np.full(ncat, 1.0 / ncat) if cat_weights is None else cat_weights, np.float64).reshape(-1)
            if k["cw"].size != ncat:
                raise TphipError("cat_weights must match cat_rates")
        self.nloci = len(k["off"]) - 1
        if k["pi"].size != 4 * self.nloci or (k["exch"] is not None and k["exch"].size != 6 * self.nloci):
            raise TphipError("pi must be [L,4] and exch [L,6] for L = len(locus_offsets) - 1")
        if k["iv"].size % 2:
            raise TphipError("intervals must be (start, stop) pairs")
        d = PlanDesc(struct_size=ctypes.sizeof(PlanDesc), device=device, ntaxa=ntaxa, nnodes=len(k["parent"]), parent=k["parent"].ctypes.data,
                     branch_len=k["blen"].ctypes.data, leaf_taxon=k["leaf"].ctypes.data, nloci=self.nloci,
                     locus_offsets=k["off"].ctypes.data, pi=k["pi"].ctypes.data, exch=_ptr(k["exch"]), T=int(T),
                     times=k["times"].ctypes.data, n_t=k["times"].size, intervals=k["iv"].ctypes.data,
                     n_i=k["iv"].size // 2, integ_mode=integ_mode, correction=float(correction),
                     threshold=int(threshold), round_decimals=int(round_decimals),
                     ncat=ncat if ncat > 1 else 0, cat_rate=k["cr"].ctypes.data if ncat > 1 else None,
                     cat_weight=k["cw"].ctypes.data if ncat > 1 else None, start_rule=int(start_rule),
                     pattern_dedup=int(pattern_dedup), model=MODELS[model])
        _check(lib.tphip_plan_create(ctypes.byref(d), ctypes.byref(self._h)))
        self.device = device
        self.ntaxa = ntaxa
        self.model = model
        self.T, self.n_t, self.n_i = int(T), k["times"].size, k["iv"].size // 2
        self.ncols = lib.tphip_plan_ncols(self._h)
        self.width = lib.tphip_plan_table_width(self._h)
        self.workspace_bytes = lib.tphip_plan_workspace_bytes(self._h)
        self.chrono_length = lib.tphip_plan_chrono_length(self._h)
        self.stack_depth = lib.tphip_plan_stack_depth(self._h)
        oc = np.zeros(5, np.int32)
        _check(lib.tphip_plan_op_counts(self._h, oc.ctypes.data))
        self.op_counts = dict(zip(("tip_set", "tip_mul", "branch", "push", "pop_mul"), oc.tolist()))
        self.op_counts["cherry"] = int(lib.tphip_plan_cherry_count(self._h))

    def _rates_nres(self, rates, nres=None):
        """rates as float64 [ncols] and nres as int32 (or None): what the calls on per-column rates take."""
        rates = _np(rates, np.float64)
        assert rates.shape == (self.ncols,)
        return rates, None if nres is None else _np(nres, np.int32)

    def close(self):
        if self._h:
            self._lib.tphip_plan_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-pointer path (numpy in, numpy out; the library does the PCIe copies) -------------
    def site_rates(self, states):
        """states: uint8 [ntaxa, ncols] masks.  Returns dict(rate, subst, lnl, flag, nres)."""
        states = _np(states, np.uint8)
        assert states.shape == (self.ntaxa, self.ncols), (states.shape, self.ntaxa, self.ncols)
        n = self.ncols
        out = dict(rate=np.empty(n), subst=np.empty(n), lnl=np.empty(n), flag=np.empty(n, np.uint8),
                   nres=np.empty(n, np.int32))
        _check(self._lib.tphip_site_rates(self._h, states.ctypes.data, out["rate"].ctypes.data, out["subst"].ctypes.data,
                                          out["lnl"].ctypes.data, out["flag"].ctypes.data, out["nres"].ctypes.data))
        return out

    def pi_tables(self, rates, nres=None):
        """rates: float64 [ncols] raw rates (rounding, /correction and cull are applied by the kernel).
        Returns tables [L, W]."""
        rates, nres = self._rates_nres(rates, nres)
        tables = np.empty((self.nloci, self.width))
        _check(self._lib.tphip_pi_tables(self._h, rates.ctypes.data, _ptr(nres), tables.ctypes.data))
        return tables

    def run_fused(self, states, pinned=False):
        """pinned=True: the result arrays live in pinned memory (direct DMA, copies overlapped with the PI kernels; when
        `states` is pinned too -- pinned_empty -- a big batch runs as a pipeline of locus groups, upload under compute)."""
        states = _np(states, np.uint8)
        assert states.shape == (self.ntaxa, self.ncols), (states.shape, self.ntaxa, self.ncols)
        n = self.ncols
        new = pinned_empty if pinned else np.empty
        out = dict(rate=new(n, np.float64), subst=new(n, np.float64), lnl=new(n, np.float64), flag=new(n, np.uint8),
                   nres=new(n, np.int32), tables=new((self.nloci, self.width), np.float64))
        _check(self._lib.tphip_run_fused(self._h, states.ctypes.data, out["rate"].ctypes.data, out["subst"].ctypes.data,
                                         out["lnl"].ctypes.data, out["flag"].ctypes.data, out["nres"].ctypes.data,
                                         out["tables"].ctypes.data))
        return out

    def run_fused_into(self, states, out, col0=0, locus0=0):
        """tphip_run_fused_pitched: `states` may be a column range of a bigger C-contiguous [ntaxa, N] array (a view
        states[:, a:b]); the results go into the caller's arrays `out` (rate, subst, lnl, flag, nres: 1-D over the big batch;
        tables [loci, W]) at column `col0` and locus `locus0` -- how pipeline.py streams a batch block by block."""
        if states.dtype != np.uint8 or states.ndim != 2 or states.strides[1] != 1:
            states = _np(states, np.uint8)
        assert states.shape == (self.ntaxa, self.ncols), (states.shape, self.ntaxa, self.ncols)
        pitch = int(states.strides[0]) if self.ntaxa > 1 else self.ncols
        a, b = int(col0), int(col0) + self.ncols
        views = [out[k][a:b] for k in ("rate", "subst", "lnl", "flag", "nres")] + [out["tables"][locus0:locus0 + self.nloci]]
        for v, dt in zip(views, (np.float64, np.float64, np.float64, np.uint8, np.int32, np.float64)):
            if v.dtype != dt or not v.flags["C_CONTIGUOUS"]:
                raise TphipError("output arrays must be C-contiguous with the documented dtypes")
        assert len(views[0]) == self.ncols and views[5].shape == (self.nloci, self.width)
        _check(self._lib.tphip_run_fused_pitched(self._h, states.ctypes.data, pitch, *[v.ctypes.data for v in views]))

    def eval_columns(self, states, u):
        """Diagnostic: (f, g, h) = log L and its u-derivatives for every column at u[ncols]."""
        states = _np(states, np.uint8)
        u = _np(u, np.float64)
        assert u.shape == (self.ncols,)
        f, g, h = np.empty(self.ncols), np.empty(self.ncols), np.empty(self.ncols)
        _check(self._lib.tphip_eval_columns(self._h, states.ctypes.data, u.ctypes.data, f.ctypes.data, g.ctypes.data,
                                            h.ctypes.data))
        return f, g, h

    def eval_columns_dev(self, d_states, d_u, d_f, d_g, d_h, stream=0):
        _check(self._lib.tphip_eval_columns_dev(self._h, _ptr(d_states), _ptr(d_u), _ptr(d_f), _ptr(d_g), _ptr(d_h), stream))

    def _eb_args(self, cat_rate, cat_weight, scale, use_patterns, maxit_scale=0, tol_scale=0.0):
        cr = _np(cat_rate, np.float64)
        cw = _np(cat_weight, np.float64)
        if cr.ndim != 2 or cr.shape[0] != self.nloci or cw.shape != cr.shape:
            raise TphipError("cat_rate and cat_weight must be [nloci][ncat]")
        sc = np.array(scale, dtype=np.float64).reshape(-1)   # a copy: the fit writes into it
        if sc.shape != (self.nloci,):
            raise TphipError("scale must be [nloci]")
        opts = EbOpts(ctypes.sizeof(EbOpts), int(cr.shape[1]), int(maxit_scale), 1 if use_patterns else 0, float(tol_scale))
        return opts, cr, cw, sc

    def eb_start_scale(self, states):
        """Start of the scale fit per locus (tphip_eb_start_scale): the locus' mean parsimony start rate."""
        states = _np(states, np.uint8)
        sc = np.empty(self.nloci)
        _check(self._lib.tphip_eb_start_scale(self._h, states.ctypes.data, sc.ctypes.data))
        return sc

    def eb_start_scale_dev(self, d_states, stream=0):
        sc = np.empty(self.nloci)
        _check(self._lib.tphip_eb_start_scale_dev(self._h, _ptr(d_states), sc.ctypes.data, stream))
        return sc

    def eb_fit_scale(self, states, cat_rate, cat_weight, scale, use_patterns=True, maxit_scale=0, tol_scale=0.0):
        """Empirical-Bayes inner problem (tphip_eb_fit_scale): for every locus the scale mu that maximises
        sum_c log sum_k w_k L_c(mu rho_k), by Newton iteration in log mu from scale[nloci].
        Returns dict(scale, locus_lnl, curvature, iters); iters < 0 marks a locus that hit the iteration limit."""
        states = _np(states, np.uint8)
        opts, cr, cw, sc = self._eb_args(cat_rate, cat_weight, scale, use_patterns, maxit_scale, tol_scale)
        lnl, curv, it = np.empty(self.nloci), np.empty(self.nloci), np.zeros(self.nloci, dtype=np.int32)
        _check(self._lib.tphip_eb_fit_scale(self._h, states.ctypes.data, ctypes.byref(opts), cr.ctypes.data, cw.ctypes.data,
                                            sc.ctypes.data, lnl.ctypes.data, curv.ctypes.data, it.ctypes.data))
        return dict(scale=sc, locus_lnl=lnl, curvature=curv, iters=it)

    def eb_posterior(self, states, cat_rate, cat_weight, scale, use_patterns=True):
        """Per column (tphip_eb_posterior): rate = kappa mu E[rho | column], sd, lnl = log m_c, nres."""
        states = _np(states, np.uint8)
        opts, cr, cw, sc = self._eb_args(cat_rate, cat_weight, scale, use_patterns)
        rate, sd, lnl = np.empty(self.ncols), np.empty(self.ncols), np.empty(self.ncols)
        nres = np.empty(self.ncols, dtype=np.int32)
        _check(self._lib.tphip_eb_posterior(self._h, states.ctypes.data, ctypes.byref(opts), cr.ctypes.data, cw.ctypes.data,
                                            sc.ctypes.data, rate.ctypes.data, sd.ctypes.data, lnl.ctypes.data, nres.ctypes.data))
        return dict(rate=rate, sd=sd, lnl=lnl, nres=nres)

    def eb_fit_scale_dev(self, d_states, cat_rate, cat_weight, scale, use_patterns=True, maxit_scale=0, tol_scale=0.0, stream=0):
        """eb_fit_scale with the alignment already on the device (d_states: device pointer or tensor)."""
        opts, cr, cw, sc = self._eb_args(cat_rate, cat_weight, scale, use_patterns, maxit_scale, tol_scale)
        lnl, curv, it = np.empty(self.nloci), np.empty(self.nloci), np.zeros(self.nloci, dtype=np.int32)
        _check(self._lib.tphip_eb_fit_scale_dev(self._h, _ptr(d_states), ctypes.byref(opts), cr.ctypes.data, cw.ctypes.data,
                                                sc.ctypes.data, lnl.ctypes.data, curv.ctypes.data, it.ctypes.data, stream))
        return dict(scale=sc, locus_lnl=lnl, curvature=curv, iters=it)

    def eb_posterior_dev(self, d_states, cat_rate, cat_weight, scale, d_rate, d_sd, d_lnl, d_nres, use_patterns=True, stream=0):
        opts, cr, cw, sc = self._eb_args(cat_rate, cat_weight, scale, use_patterns)
        _check(self._lib.tphip_eb_posterior_dev(self._h, _ptr(d_states), ctypes.byref(opts), cr.ctypes.data, cw.ctypes.data,
                                                sc.ctypes.data, _ptr(d_rate), _ptr(d_sd), _ptr(d_lnl), _ptr(d_nres), stream))

    # ---- the EB rate posterior carried into the PI rows (csrc/posterior_pi_driver.hip) ----
    def eb_posterior_table(self, states, cat_rate, cat_weight, scale, use_patterns=True):
        """eb_posterior with the category posterior besides (tphip_eb_posterior_table): post [K, ncols], p_ck."""
        states = _np(states, np.uint8)
        opts, cr, cw, sc = self._eb_args(cat_rate, cat_weight, scale, use_patterns)
        post = np.zeros((cr.shape[1], self.ncols))
        rate, sd, lnl = np.empty(self.ncols), np.empty(self.ncols), np.empty(self.ncols)
        nres = np.empty(self.ncols, dtype=np.int32)
        _check(self._lib.tphip_eb_posterior_table(self._h, states.ctypes.data, ctypes.byref(opts), cr.ctypes.data, cw.ctypes.data,
                                                  sc.ctypes.data, post.ctypes.data, rate.ctypes.data, sd.ctypes.data,
                                                  lnl.ctypes.data, nres.ctypes.data))
        return dict(post=post, rate=rate, sd=sd, lnl=lnl, nres=nres)

    def eb_posterior_table_dev(self, d_states, cat_rate, cat_weight, scale, d_post, d_rate, d_sd, d_lnl, d_nres, use_patterns=True,
                               stream=0):
        opts, cr, cw, sc = self._eb_args(cat_rate, cat_weight, scale, use_patterns)
        _check(self._lib.tphip_eb_posterior_table_dev(self._h, _ptr(d_states), ctypes.byref(opts), cr.ctypes.data, cw.ctypes.data,
                                                      sc.ctypes.data, _ptr(d_post), _ptr(d_rate), _ptr(d_sd), _ptr(d_lnl),
                                                      _ptr(d_nres), stream))

    def posterior_pi_workspace_bytes(self, ncat, replicates, seed=1, level=0.95):
        """(min, preferred) bytes of device workspace for posterior_pi_dev; any size >= min gives the same bits."""
        opts, _ = self._band_opts(PosteriorPiOpts, replicates, seed, level, None, ncat=int(ncat))
        return _size_pair(self._lib.tphip_posterior_pi_workspace_bytes, self._h, ctypes.byref(opts))

    def posterior_pi(self, post, nres, scale, cat_rate, replicates=200, seed=1, level=0.95, locus_ids=None, return_rows=False,
                     return_counts=False):
        """The EB rate posterior carried into the PI rows (tphip_posterior_pi), conditional on the fitted scale and prior.
        post [K, ncols] from eb_posterior_table, nres [ncols] or None (no cull), scale [L], cat_rate [L, K].
        Returns dict(analytic [L, 2, Wb] = mean, sd; expected_counts [L, K]; summary [L, 4, Wb] = mean, sd, lo, hi over the
        `replicates` draws) and, on request, rows [L, B, Wb] and counts int32 [L, B, K]."""
        cr = _np(cat_rate, np.float64)
        if cr.ndim != 2 or cr.shape[0] != self.nloci:
            raise TphipError("cat_rate must be [nloci][ncat]")
        K = int(cr.shape[1])
        post = _np(post, np.float64)
        if post.shape != (K, self.ncols):
            raise TphipError("post must be [ncat, ncols]")
        sc = _np(scale, np.float64).reshape(-1)
        if sc.shape != (self.nloci,):
            raise TphipError("scale must be [nloci]")
        if nres is not None:
            nres = _np(nres, np.int32)
            if nres.shape != (self.ncols,):
                raise TphipError("nres must be [ncols]")
        opts, ids = self._band_opts(PosteriorPiOpts, replicates, seed, level, locus_ids, ncat=K)
        Wb, B = self.bootstrap_width, int(replicates)
        out = dict(analytic=np.zeros((self.nloci, 2, Wb)), expected_counts=np.zeros((self.nloci, K)),
                   summary=np.zeros((self.nloci, 4, Wb)))
        if return_rows:
            out["rows"] = np.zeros((self.nloci, max(B, 0), Wb))
        if return_counts:
            out["counts"] = np.zeros((self.nloci, max(B, 0), K), dtype=np.int32)
        _check(self._lib.tphip_posterior_pi(self._h, post.ctypes.data, _ptr(nres), sc.ctypes.data, cr.ctypes.data, ctypes.byref(opts),
                                            out["analytic"].ctypes.data, out["expected_counts"].ctypes.data,
                                            out["summary"].ctypes.data, _ptr(out.get("rows")), _ptr(out.get("counts"))))
        return out

    def posterior_pi_dev(self, d_post, d_nres, d_scale, d_cat_rate, ncat, d_analytic, d_expected, d_summary, d_rows, d_counts, d_ws,
                         replicates, seed=1, level=0.95, locus_ids=None, stream=0, ws_bytes=None):
        """tphip_posterior_pi_dev on device tensors (d_nres / d_rows / d_counts may be None); ws_bytes: use only that much of d_ws."""
        opts, ids = self._band_opts(PosteriorPiOpts, replicates, seed, level, locus_ids, ncat=int(ncat))
        _check(self._lib.tphip_posterior_pi_dev(self._h, _ptr(d_post), _ptr(d_nres), _ptr(d_scale), _ptr(d_cat_rate), ctypes.byref(opts),
                                                _ptr(d_analytic), _ptr(d_expected), _ptr(d_summary), _ptr(d_rows), _ptr(d_counts),
                                                _ptr(d_ws), _ws_nbytes(d_ws, ws_bytes), stream))

    def corrected_rates(self, rates, nres=None):
        """parse_site_rates (+ cull when nres is given) as the PI stage applies them: round4(rate) / correction."""
        rates, nres = self._rates_nres(rates, nres)
        out = np.empty(self.ncols)
        _check(self._lib.tphip_corrected_rates(self._h, rates.ctypes.data, _ptr(nres), out.ctypes.data))
        return out

    def corrected_rates_dev(self, d_rates, d_nres, d_out, stream=0):
        _check(self._lib.tphip_corrected_rates_dev(self._h, _ptr(d_rates), _ptr(d_nres), _ptr(d_out), stream))

    def locus_loglik(self, states, blen_vecs, cand_locus, cand_exch, cand_vec=None, cand_scale=None, cand_pidx=None,
                     cand_pfac=None, cache=None):
        """Sum over columns of log L (site rate 1) for candidate parameter sets (tphip_locus_loglik).
        Branch lengths of candidate c = blen_vecs[cand_vec[c]] * cand_scale[c], with branch cand_pidx[c]
        additionally multiplied by cand_pfac[c].  Defaults: vec = arange, scale = 1, no perturbation.
        cache: device_cache() object that keeps the alignment on the device between calls."""
        states = _np(states, np.uint8)
        bv, cl, ce, cv, cs, ci, cf = _candidates(blen_vecs, cand_locus, cand_exch, cand_vec, cand_scale, cand_pidx, cand_pfac)
        n = len(cl)
        out = np.empty(n)
        ref = ctypes.byref(cache.ptr) if cache is not None else None
        _check(self._lib.tphip_locus_loglik(self._h, states.ctypes.data, ref, bv.shape[0], bv.ctypes.data, n, cl.ctypes.data,
                                            ce.ctypes.data, cv.ctypes.data, cs.ctypes.data, ci.ctypes.data, cf.ctypes.data,
                                            out.ctypes.data))
        return out

    def locus_loglik_dev(self, d_states_ptr, ncand, d_cand_locus, d_cand_exch, d_blen_vecs, d_cand_vec, d_cand_scale,
                         d_cand_pidx, d_cand_pfac, d_out, stream=0):
        """tphip_locus_loglik_dev: every array is a device tensor (int32 / float64), nothing is copied or synchronised.
        d_states_ptr: device address of the alignment (int, e.g. the pointer a device_cache() holds)."""
        _check(self._lib.tphip_locus_loglik_dev(self._h, d_states_ptr, int(ncand), _ptr(d_cand_locus), _ptr(d_cand_exch),
                                                _ptr(d_blen_vecs), _ptr(d_cand_vec), _ptr(d_cand_scale), _ptr(d_cand_pidx),
                                                _ptr(d_cand_pfac), _ptr(d_out), stream))

    def locus_gradient_dev(self, d_states_ptr, ncand, d_cand_locus, d_cand_exch, d_blen_vecs, d_cand_vec, d_cand_scale,
                           d_cand_pidx, d_cand_pfac, d_lnl, d_dexch, d_dlogt, d_sum_dlogt, d_d2logt, stream=0):
        """tphip_locus_gradient_dev on device tensors (d_dlogt / d_d2logt may be None); nothing is copied or synchronised."""
        _check(self._lib.tphip_locus_gradient_dev(self._h, d_states_ptr, int(ncand), _ptr(d_cand_locus), _ptr(d_cand_exch),
                                                  _ptr(d_blen_vecs), _ptr(d_cand_vec), _ptr(d_cand_scale), _ptr(d_cand_pidx),
                                                  _ptr(d_cand_pfac), _ptr(d_lnl), _ptr(d_dexch), _ptr(d_dlogt),
                                                  _ptr(d_sum_dlogt), _ptr(d_d2logt), stream))

    def locus_gradient(self, states, blen_vecs, cand_locus, cand_exch, cand_vec=None, cand_scale=None, cand_pidx=None,
                       cand_pfac=None, cache=None, per_branch=True, curvature=False):
        """locus_loglik plus its derivatives (tphip_locus_gradient): returns (lnl[n], dexch[n, 6], dlogt[n, nnodes] or
        None, sum_dlogt[n]) and, with curvature=True, a fifth item d2logt[n, nnodes]; dexch holds branch lengths
        fixed, dlogt is d lnL / d log t_b, d2logt the matching second derivatives (Hessian diagonal)."""
        states = _np(states, np.uint8)
        bv, cl, ce, cv, cs, ci, cf = _candidates(blen_vecs, cand_locus, cand_exch, cand_vec, cand_scale, cand_pidx, cand_pfac)
        n = len(cl)
        lnl, dex, st = np.empty(n), np.empty((n, 6)), np.empty(n)
        dlt = np.empty((n, bv.shape[1])) if per_branch else None
        d2 = np.empty((n, bv.shape[1])) if curvature else None
        ref = ctypes.byref(cache.ptr) if cache is not None else None
        _check(self._lib.tphip_locus_gradient(self._h, states.ctypes.data, ref, bv.shape[0], bv.ctypes.data, n, cl.ctypes.data,
                                              ce.ctypes.data, cv.ctypes.data, cs.ctypes.data, ci.ctypes.data, cf.ctypes.data,
                                              lnl.ctypes.data, dex.ctypes.data, dlt.ctypes.data if per_branch else None,
                                              st.ctypes.data, d2.ctypes.data if curvature else None))
        return (lnl, dex, dlt, st, d2) if curvature else (lnl, dex, dlt, st)

    def stage1_fit(self, states, cache=None, details=True, maxit_grm=0, maxit_sub=0, prune_models=True, fd_step=0.0,
                   free_root_pair=False, compress_patterns=False, empirical_pi=False):
        """HyPhy's stage 1 for every locus of the plan in one engine call (tphip_stage1_fit): model-averaged
        exchangeabilities [L, 6], the base frequencies used [L, 4] and, with details, weights / lnl [L, 203], model_exch
        [L, 203, 6], grm_blen [L, nnodes], iteration counts and counters.  The optimisers run on the device
        (csrc/stage1_opt_kernels.hpp).  `states` may be a column range of a bigger C-contiguous [ntaxa, N] array (a view
        states[:, a:b]): it is uploaded with one 2-D copy, not copied on the host.  compress_patterns: collapse the columns
        into site patterns with counts on the device first (HyPhy's dupInfo); empirical_pi: HarvestFrequencies on the device."""
        if states.dtype != np.uint8 or states.ndim != 2 or states.strides[1] != 1:
            states = _np(states, np.uint8)
        assert states.shape == (self.ntaxa, self.ncols), (states.shape, self.ntaxa, self.ncols)
        pitch = int(states.strides[0]) if self.ntaxa > 1 else self.ncols
        if pitch != self.ncols and cache is not None:
            raise ValueError("a device cache cannot hold a column range of a bigger array")
        L, nn = self.nloci, len(self._keep["parent"])
        opts = Stage1Opts(struct_size=ctypes.sizeof(Stage1Opts), maxit_grm=int(maxit_grm), maxit_sub=int(maxit_sub),
                          no_prune=0 if prune_models else 1, fd_step=float(fd_step),
                          free_root_pair=1 if free_root_pair else 0, compress_patterns=1 if compress_patterns else 0,
                          empirical_pi=1 if empirical_pi else 0, row_pitch=0 if pitch == self.ncols else pitch)
        out = dict(exch=np.empty((L, 6)), pi=np.empty((L, 4)))
        if details:
            out.update(weights=np.empty((L, 203)), lnl=np.empty((L, 203)), model_exch=np.empty((L, 203, 6)),
                       grm_blen=np.empty((L, nn)), grm_iters=np.empty(L, np.int32), sub_iters=np.empty((L, 202), np.int32))
        stats = np.zeros(8, np.int64)
        ref = ctypes.byref(cache.ptr) if cache is not None else None
        g = lambda k: out[k].ctypes.data if k in out else None  # noqa: E731
        _check(self._lib.tphip_stage1_fit(self._h, states.ctypes.data, ref, ctypes.byref(opts), out["exch"].ctypes.data,
                                          out["pi"].ctypes.data, g("weights"), g("lnl"), g("model_exch"), g("grm_blen"),
                                          g("grm_iters"), g("sub_iters"), stats.ctypes.data))
        out["stats"] = dict(zip(("nevals", "ngrads", "grm_evals", "grm_grads", "pruned", "fitted", "grm_outer_iterations",
                                 "sub_outer_iterations"), stats.tolist()))
        return out

    def set_models(self, pi=None, exch=None):
        """Replace the per-locus base frequencies [L, 4] and / or exchangeabilities [L, 6] of the plan (tphip_plan_set_models;
        an F81 plan takes pi only)."""
        a = None if pi is None else _np(pi, np.float64).reshape(-1)
        b = None if exch is None else _np(exch, np.float64).reshape(-1)
        if (a is not None and a.size != 4 * self.nloci) or (b is not None and b.size != 6 * self.nloci):
            raise TphipError("pi must be [L,4] and exch [L,6]")
        _check(self._lib.tphip_plan_set_models(self._h, _ptr(a), _ptr(b)))

    def set_column_weights(self, weights):
        """Column multiplicities for locus_loglik / locus_gradient (site-pattern counts); None removes them."""
        if weights is None:
            _check(self._lib.tphip_plan_set_column_weights(self._h, None))
            return
        w = _np(weights, np.float64).reshape(-1)
        if w.size != self.ncols:
            raise ValueError("weights must have one entry per column of the plan")
        _check(self._lib.tphip_plan_set_column_weights(self._h, w.ctypes.data))

    def device_cache(self):
        """Holder that keeps the alignment on the device across locus_loglik calls; release() frees it."""
        return _DeviceCache(self)

    def models(self):
        L = self.nloci
        lam, U, Ui, kappa = np.empty((L, 4)), np.empty((L, 4, 4)), np.empty((L, 4, 4)), np.empty(L)
        _check(self._lib.tphip_plan_get_models(self._h, lam.ctypes.data, U.ctypes.data, Ui.ctypes.data, kappa.ctypes.data))
        return lam, U, Ui, kappa

    # ---- device-pointer path (torch tensors resident in HBM; nothing is copied or synchronised) --
    def run_dev(self, d_states, d_rate, d_subst, d_lnl, d_flag, d_nres, d_tables, d_ws, stream=0):
        _check(self._lib.tphip_run_dev(self._h, _ptr(d_states), _ptr(d_rate), _ptr(d_subst), _ptr(d_lnl), _ptr(d_flag),
                                       _ptr(d_nres), _ptr(d_tables), _ptr(d_ws), _nbytes(d_ws), stream))

    def site_rates_dev(self, d_states, d_rate, d_subst, d_lnl, d_flag, d_nres, d_ws, stream=0):
        _check(self._lib.tphip_site_rates_dev(self._h, _ptr(d_states), _ptr(d_rate), _ptr(d_subst), _ptr(d_lnl),
                                              _ptr(d_flag), _ptr(d_nres), _ptr(d_ws), _nbytes(d_ws), stream))

    def pi_tables_dev(self, d_rates, d_nres, d_tables, d_ws, stream=0):
        _check(self._lib.tphip_pi_tables_dev(self._h, _ptr(d_rates), _ptr(d_nres), _ptr(d_tables), _ptr(d_ws), _nbytes(d_ws), stream))

    # ---- site bootstrap of the PI rows (csrc/bootstrap_driver.hip) ------------------------------
    @property
    def bootstrap_width(self):
        """Wb = T + n_i: net PI at t = 0..T-1, then one integral per interval."""
        return int(self._lib.tphip_bootstrap_width(self._h))

    def bootstrap_workspace_bytes(self, replicates, seed=1, level=0.95):
        """(min, preferred) bytes of device workspace for pi_bootstrap_dev; any size >= min gives the same bits."""
        opts, _ = self._band_opts(BootstrapOpts, replicates, seed, level, None)
        return _size_pair(self._lib.tphip_bootstrap_workspace_bytes, self._h, ctypes.byref(opts))

    def resample_workspace_bytes(self):
        """(min, preferred) bytes of device workspace for pi_resample_dev (per-site integrals only; any nrep)."""
        return _size_pair(self._lib.tphip_bootstrap_workspace_bytes, self._h, None)

    def pi_bootstrap(self, rates, nres=None, replicates=200, seed=1, level=0.95, locus_ids=None, return_rows=False):
        """Site bootstrap of the PI rows (tphip_pi_bootstrap): `replicates` resamples of every locus' columns with
        replacement, the locus' model held fixed.  rates / nres as for pi_tables.  Returns summary [L, 4, Wb] (mean, sd,
        lo, hi; [lo, hi] covers `level`) and, with return_rows, the replicate rows [L, B, Wb] as a second array.
        locus_ids: the generator's stream id per locus (default: the plan's locus index); a locus gives the same rows
        whatever plan it is part of as long as its id, the seed and its rates are the same."""
        rates, nres = self._rates_nres(rates, nres)
        opts, ids = self._band_opts(BootstrapOpts, replicates, seed, level, locus_ids)
        Wb = self.bootstrap_width
        summary = np.zeros((self.nloci, 4, Wb))
        rows = np.zeros((self.nloci, int(replicates), Wb)) if return_rows else None
        _check(self._lib.tphip_pi_bootstrap(self._h, rates.ctypes.data, _ptr(nres), ctypes.byref(opts), summary.ctypes.data,
                                            _ptr(rows)))
        return (summary, rows) if return_rows else summary

    def pi_resample(self, rates, nres, counts):
        """The weighted-sum core on caller-supplied counts (tphip_pi_resample): counts uint16 [nrep, ncols] over the plan's
        columns -> rows [L, nrep, Wb], rows[l, b] = sum over the locus' columns of counts[b, i] * (site i's PI values)."""
        rates, nres = self._rates_nres(rates, nres)
        counts = _np(counts, np.uint16)
        if counts.ndim != 2 or counts.shape[1] != self.ncols:
            raise TphipError("counts must be uint16 [nrep, ncols]")
        rows = np.zeros((self.nloci, counts.shape[0], self.bootstrap_width))
        _check(self._lib.tphip_pi_resample(self._h, rates.ctypes.data, _ptr(nres), counts.ctypes.data, counts.shape[0],
                                           rows.ctypes.data))
        return rows

    def pi_bootstrap_dev(self, d_rates, d_nres, d_summary, d_rows, d_ws, replicates, seed=1, level=0.95, locus_ids=None,
                         stream=0, ws_bytes=None):
        """tphip_pi_bootstrap_dev on device tensors (d_nres / d_rows may be None); ws_bytes: use only that much of d_ws."""
        opts, ids = self._band_opts(BootstrapOpts, replicates, seed, level, locus_ids)
        _check(self._lib.tphip_pi_bootstrap_dev(self._h, _ptr(d_rates), _ptr(d_nres), ctypes.byref(opts), _ptr(d_summary),
                                                _ptr(d_rows), _ptr(d_ws), _ws_nbytes(d_ws, ws_bytes), stream))

    def pi_resample_dev(self, d_rates, d_nres, d_counts, nrep, d_rows, d_ws, stream=0):
        """tphip_pi_resample_dev on device tensors: d_counts int16/uint16 [nrep, ncols], d_rows [L, nrep, Wb]."""
        _check(self._lib.tphip_pi_resample_dev(self._h, _ptr(d_rates), _ptr(d_nres), _ptr(d_counts), int(nrep), _ptr(d_rows),
                                               _ptr(d_ws), _nbytes(d_ws), stream))

    # ---- quartet signal and noise: equal tips (csrc/quartet_driver.hip), unequal tips (csrc/unequal_quartet_driver.hip) ----
    # One implementation per kind of call over a family `fam` (_QuartetFamily below: options builder, symbol prefix, row width,
    # per-site planes); the public methods name the family.
    @staticmethod
    def _quartet_opts(quartets):
        """quartets: [n_q, 2] rows (T, t_o).  Returns the options and the arrays they point into (keep them alive)."""
        q = _np(quartets, np.float64).reshape(-1, 2)
        tip, internode = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])
        opts = QuartetOpts(struct_size=ctypes.sizeof(QuartetOpts), n_q=len(q), tip=tip.ctypes.data, internode=internode.ctypes.data)
        return opts, (tip, internode)

    @staticmethod
    def _unequal_quartet_opts(quartets):
        """quartets: [n_q, 5] rows (Ta, Tb, Tc, Td, t_o).  Returns the options and the arrays they point into (keep them alive)."""
        q = _np(quartets, np.float64).reshape(-1, 5)
        tips, internode = np.ascontiguousarray(q[:, :4]), np.ascontiguousarray(q[:, 4])
        opts = UnequalQuartetOpts(struct_size=ctypes.sizeof(UnequalQuartetOpts), n_q=len(q), tips=tips.ctypes.data,
                                  internode=internode.ctypes.data)
        return opts, (tips, internode)

    def _quartet_workspace_bytes(self, fam, quartets):
        opts, keep = fam.opts(quartets)
        return _size_out(getattr(self._lib, fam.prefix + "_workspace_bytes"), self._h, ctypes.byref(opts))

    def _quartet_tables(self, fam, rates, nres, quartets):
        rates, nres = self._rates_nres(rates, nres)
        opts, keep = fam.opts(quartets)
        rows = np.zeros((self.nloci, opts.n_q, fam.row))
        _check(getattr(self._lib, fam.prefix + "_tables")(self._h, rates.ctypes.data, _ptr(nres), ctypes.byref(opts), rows.ctypes.data))
        return rows

    def _quartet_sites(self, fam, rates, nres, quartets):
        rates, nres = self._rates_nres(rates, nres)
        opts, keep = fam.opts(quartets)
        sites = np.zeros((fam.planes, opts.n_q, self.ncols))
        _check(getattr(self._lib, fam.prefix + "_sites")(self._h, rates.ctypes.data, _ptr(nres), ctypes.byref(opts), sites.ctypes.data))
        return sites

    def _quartet_tables_dev(self, fam, d_rates, d_nres, quartets, d_rows, d_ws, stream):
        opts, keep = fam.opts(quartets)
        _check(getattr(self._lib, fam.prefix + "_tables_dev")(self._h, _ptr(d_rates), _ptr(d_nres), ctypes.byref(opts), _ptr(d_rows),
                                                              _ptr(d_ws), _nbytes(d_ws), stream))

    def _quartet_sites_dev(self, fam, d_rates, d_nres, quartets, d_sites, stream):
        opts, keep = fam.opts(quartets)
        _check(getattr(self._lib, fam.prefix + "_sites_dev")(self._h, _ptr(d_rates), _ptr(d_nres), ctypes.byref(opts), _ptr(d_sites), stream))

    def quartet_workspace_bytes(self, quartets):
        """bytes of device workspace for quartet_tables_dev with these quartets."""
        return self._quartet_workspace_bytes(_EQUAL_TIPS, quartets)

    def quartet_tables(self, rates, nres, quartets):
        """Signal and noise of the quartets ((a:T, b:T), (c:T, d:T)) with internode t_o under the plan's models
        (tphip_quartet_tables).  rates / nres as for pi_tables; quartets [n_q, 2] rows (T, t_o) in the tree's original time
        units.  Returns rows [L, n_q, 8]: Y, X, Yy, Xx, XY, p_correct, p_incorrect, p_polytomy."""
        return self._quartet_tables(_EQUAL_TIPS, rates, nres, quartets)

    def quartet_sites(self, rates, nres, quartets):
        """The per-site values behind quartet_tables (tphip_quartet_sites): [2, n_q, ncols], signal y then noise x; exactly
        0 for a culled or zero-rate column."""
        return self._quartet_sites(_EQUAL_TIPS, rates, nres, quartets)

    def quartet_tables_dev(self, d_rates, d_nres, quartets, d_rows, d_ws, stream=0):
        """tphip_quartet_tables_dev on device tensors (d_nres may be None): d_rows [L, n_q, 8]; enqueues, does not synchronise."""
        self._quartet_tables_dev(_EQUAL_TIPS, d_rates, d_nres, quartets, d_rows, d_ws, stream)

    def quartet_sites_dev(self, d_rates, d_nres, quartets, d_sites, stream=0):
        """tphip_quartet_sites_dev on device tensors: d_sites [2, n_q, ncols]; enqueues, does not synchronise."""
        self._quartet_sites_dev(_EQUAL_TIPS, d_rates, d_nres, quartets, d_sites, stream)

    def unequal_quartet_workspace_bytes(self, quartets):
        """bytes of device workspace for unequal_quartet_tables_dev with these quartets."""
        return self._quartet_workspace_bytes(_UNEQUAL_TIPS, quartets)

    def unequal_quartet_tables(self, rates, nres, quartets):
        """Signal and noise of the quartets ((a:Ta, b:Tb), (c:Tc, d:Td)) with internode t_o under the plan's models
        (tphip_unequal_quartet_tables).  rates / nres as for pi_tables; quartets [n_q, 5] rows (Ta, Tb, Tc, Td, t_o) in the
        tree's original time units.  Returns rows [L, n_q, 13]: the sums of y, x1, x2, y^2, x1^2, x2^2, y x1, y x2, x1 x2, then
        p_correct, p_ac, p_ad, p_polytomy."""
        return self._quartet_tables(_UNEQUAL_TIPS, rates, nres, quartets)

    def unequal_quartet_sites(self, rates, nres, quartets):
        """The per-site values behind unequal_quartet_tables (tphip_unequal_quartet_sites): [3, n_q, ncols], signal y, then
        the noise x1 (pattern ijij) and x2 (ijji); exactly 0 for a culled or zero-rate column."""
        return self._quartet_sites(_UNEQUAL_TIPS, rates, nres, quartets)

    def unequal_quartet_tables_dev(self, d_rates, d_nres, quartets, d_rows, d_ws, stream=0):
        """tphip_unequal_quartet_tables_dev on device tensors (d_nres may be None): d_rows [L, n_q, 13]; enqueues, does not
        synchronise."""
        self._quartet_tables_dev(_UNEQUAL_TIPS, d_rates, d_nres, quartets, d_rows, d_ws, stream)

    def unequal_quartet_sites_dev(self, d_rates, d_nres, quartets, d_sites, stream=0):
        """tphip_unequal_quartet_sites_dev on device tensors: d_sites [3, n_q, ncols]; enqueues, does not synchronise."""
        self._quartet_sites_dev(_UNEQUAL_TIPS, d_rates, d_nres, quartets, d_sites, stream)

    # ---- exact quartet resolution probabilities (csrc/exact_quartet_driver.hip) -------------------
    @staticmethod
    def _quartet_exact_opts(n_q, window_cap, tail_tolerance):
        return QuartetExactOpts(struct_size=ctypes.sizeof(QuartetExactOpts), n_q=int(n_q), window_cap=int(window_cap),
                                tail_tolerance=float(tail_tolerance))

    def quartet_exact_workspace_bytes(self, n_q, window_cap=128):
        """bytes of device workspace for quartet_exact_dev with n_q quartets and this cap."""
        opts = self._quartet_exact_opts(n_q, window_cap, 0.0)
        return _size_out(self._lib.tphip_quartet_exact_workspace_bytes, self._h, ctypes.byref(opts))

    def quartet_exact(self, y, x1, x2, window_cap=128, tail_tolerance=0.0):
        """The exact law of the quartet counts from the per-site planes (tphip_quartet_exact): y, x1, x2 [n_q, ncols] as
        unequal_quartet_sites returns them; an equal-tip quartet passes quartet_sites' x for both (the same array: it is then
        uploaded once).  Returns rows [L, n_q, 6]: p_correct, p_ac, p_ad, p_polytomy, window, tail_bound; a pair whose law
        does not fit a window of window_cap (a power of two in 16..512) within tail_tolerance (0: 1e-12) has NaN in the four
        probabilities and window 0."""
        same = x2 is x1
        y, x1 = _np(y, np.float64), _np(x1, np.float64)
        x2 = x1 if same else _np(x2, np.float64)
        if y.ndim != 2 or y.shape[1] != self.ncols or x1.shape != y.shape or x2.shape != y.shape:
            raise TphipError("y, x1 and x2 must be [n_q, ncols] planes of one shape")
        opts = self._quartet_exact_opts(y.shape[0], window_cap, tail_tolerance)
        rows = np.zeros((self.nloci, y.shape[0], 6))
        _check(self._lib.tphip_quartet_exact(self._h, y.ctypes.data, x1.ctypes.data, x2.ctypes.data, ctypes.byref(opts),
                                             rows.ctypes.data))
        return rows

    def quartet_exact_dev(self, d_y, d_x1, d_x2, n_q, d_rows, d_ws, window_cap=128, tail_tolerance=0.0, stream=0):
        """tphip_quartet_exact_dev on device tensors: d_y, d_x1, d_x2 [n_q, ncols] (views of a *_sites_dev buffer), d_rows
        [L, n_q, 6]; enqueues, does not synchronise."""
        opts = self._quartet_exact_opts(n_q, window_cap, tail_tolerance)
        _check(self._lib.tphip_quartet_exact_dev(self._h, _ptr(d_y), _ptr(d_x1), _ptr(d_x2), ctypes.byref(opts), _ptr(d_rows),
                                                 _ptr(d_ws), _nbytes(d_ws), stream))

    # ---- locus-set accumulation curves, exact rows (csrc/locus_set_driver.hip) ---------------------
    def locus_set_exact_workspace_bytes(self, n_q, n_k, window_cap=128, n_head=0):
        """bytes of device workspace for locus_set_exact_dev with n_q quartets, orders of n_k loci, this cap and n_head."""
        opts, _ = _locus_set_opts(np.zeros((int(n_q), int(n_k)), np.int32), window_cap=window_cap, n_head=n_head)
        return _size_out(self._lib.tphip_locus_set_exact_workspace_bytes, self._h, ctypes.byref(opts))

    def locus_set_exact(self, y, x1, x2, order, window_cap=128, tail_tolerance=0.0, n_head=0):
        """The exact law of the quartet counts of the sets of loci order[q, :k], k = 1..K, analysed together
        (tphip_locus_set_exact): y, x1, x2 [n_q, ncols] as for quartet_exact, order int [n_q, K] distinct locus indices per
        quartet.  Returns rows [n_q, K, 6]: p_correct, p_ac, p_ad, p_polytomy, window, tail_bound, all on the torus
        M = window_cap; a prefix whose law does not fit it within tail_tolerance (0: 1e-12), or beyond n_head (0: K), has NaN
        in the four probabilities and window 0."""
        same = x2 is x1
        y, x1 = _np(y, np.float64), _np(x1, np.float64)
        x2 = x1 if same else _np(x2, np.float64)
        if y.ndim != 2 or y.shape[1] != self.ncols or x1.shape != y.shape or x2.shape != y.shape:
            raise TphipError("y, x1 and x2 must be [n_q, ncols] planes of one shape")
        opts, order = _locus_set_opts(order, window_cap=window_cap, tail_tolerance=tail_tolerance, n_head=n_head)
        if order.shape[0] != y.shape[0]:
            raise TphipError("order must have one row per quartet of the planes")
        rows = np.zeros(order.shape + (6,))
        _check(self._lib.tphip_locus_set_exact(self._h, y.ctypes.data, x1.ctypes.data, x2.ctypes.data, ctypes.byref(opts),
                                               rows.ctypes.data))
        return rows

    def locus_set_exact_dev(self, d_y, d_x1, d_x2, order, d_rows, d_ws, window_cap=128, tail_tolerance=0.0, n_head=0, stream=0):
        """tphip_locus_set_exact_dev on device tensors: d_y, d_x1, d_x2 [n_q, ncols] (views of a *_sites_dev buffer), order a
        host array [n_q, K], d_rows [n_q, K, 6]; enqueues, does not synchronise (the order travels as kernel arguments)."""
        opts, order = _locus_set_opts(order, window_cap=window_cap, tail_tolerance=tail_tolerance, n_head=n_head)
        _check(self._lib.tphip_locus_set_exact_dev(self._h, _ptr(d_y), _ptr(d_x1), _ptr(d_x2), ctypes.byref(opts), _ptr(d_rows),
                                                   _ptr(d_ws), _nbytes(d_ws), stream))

    # ---- parametric bootstrap of site rates and PI rows (csrc/simulate_driver.hip) ---------------
    def _ids(self, locus_ids):
        ids = None if locus_ids is None else _np(locus_ids, np.int64).reshape(-1)
        if ids is not None and ids.size != self.nloci:
            raise TphipError("locus_ids must have one entry per locus of the plan")
        return ids

    def _band_opts(self, cls, replicates, seed, level, locus_ids, **extra):
        """The options of a replicate-band family (BootstrapOpts, ParbootOpts, PosteriorPiOpts with ncat=) and the id array
        they point into (keep it alive)."""
        ids = self._ids(locus_ids)
        return cls(struct_size=ctypes.sizeof(cls), replicates=int(replicates), level=float(level), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                   locus_ids=_ptr(ids), **extra), ids

    def _simulate_opts(self, replicate, seed, locus_ids):
        ids = self._ids(locus_ids)
        return SimulateOpts(struct_size=ctypes.sizeof(SimulateOpts), replicate=int(replicate), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                            locus_ids=_ptr(ids)), ids

    def simulate_columns(self, rates, mask=None, replicate=0, seed=1, locus_ids=None):
        """Alignment columns simulated down the plan's tree (tphip_simulate_columns): column c under its locus' model at the
        raw rate rates[c] (kappa * s, the unit of site_rates()["rate"]; NaN, negative or infinite: a column of 15s).  mask:
        uint8 [ntaxa, ncols] observed alignment whose cells that are not a single base (gaps, ambiguity codes) are copied
        through.  Returns uint8 [ntaxa, ncols].  A column's bytes depend on seed, its locus' stream id (locus_ids, default the
        locus index), its index in the locus, replicate, its rate, the model, the tree and its mask only."""
        rates, _ = self._rates_nres(rates)
        if mask is not None:
            mask = _np(mask, np.uint8)
            assert mask.shape == (self.ntaxa, self.ncols), (mask.shape, self.ntaxa, self.ncols)
        opts, ids = self._simulate_opts(replicate, seed, locus_ids)
        out = np.empty((self.ntaxa, self.ncols), np.uint8)
        _check(self._lib.tphip_simulate_columns(self._h, rates.ctypes.data, _ptr(mask), ctypes.byref(opts), out.ctypes.data))
        return out

    def simulate_columns_dev(self, d_rates, d_mask, d_states_out, replicate=0, seed=1, locus_ids=None, stream=0):
        """tphip_simulate_columns_dev on device tensors (d_mask may be None); enqueues on `stream`."""
        opts, ids = self._simulate_opts(replicate, seed, locus_ids)
        _check(self._lib.tphip_simulate_columns_dev(self._h, _ptr(d_rates), _ptr(d_mask), ctypes.byref(opts), _ptr(d_states_out),
                                                    stream))

    def parboot_workspace_bytes(self, replicates, seed=1, level=0.95):
        """bytes of device workspace for pi_parametric_bootstrap_dev."""
        opts, _ = self._band_opts(ParbootOpts, replicates, seed, level, None)
        return _size_out(self._lib.tphip_parboot_workspace_bytes, self._h, ctypes.byref(opts))

    def pi_parametric_bootstrap(self, rates, states, replicates=100, seed=1, level=0.95, locus_ids=None, return_rows=False,
                                return_rate_moments=False):
        """Parametric bootstrap of the site rates and the PI rows (tphip_pi_parametric_bootstrap): `replicates` times every
        column is simulated at its raw rate rates[c] with the missing cells of `states` (the observed alignment), its rate
        re-estimated and the PI row recomputed; the locus' model and the tree are held fixed.  Returns summary [L, 4, Wb]
        (mean, sd, lo, hi); with return_rows the replicate rows [L, B, Wb]; with return_rate_moments (rate_mean, rate_sd) of
        every column's final rate over the replicates, NaN for culled columns -- in that order."""
        rates, _ = self._rates_nres(rates)
        if states is not None:
            states = _np(states, np.uint8)
            assert states.shape == (self.ntaxa, self.ncols), (states.shape, self.ntaxa, self.ncols)
        opts, ids = self._band_opts(ParbootOpts, replicates, seed, level, locus_ids)
        Wb = self.bootstrap_width
        summary = np.zeros((self.nloci, 4, Wb))
        rows = np.zeros((self.nloci, int(replicates), Wb)) if return_rows else None
        mean = np.empty(self.ncols) if return_rate_moments else None
        sd = np.empty(self.ncols) if return_rate_moments else None
        _check(self._lib.tphip_pi_parametric_bootstrap(self._h, rates.ctypes.data, _ptr(states), ctypes.byref(opts),
                                                       summary.ctypes.data, _ptr(rows), _ptr(mean), _ptr(sd)))
        out = (summary,)
        if return_rows:
            out += (rows,)
        if return_rate_moments:
            out += (mean, sd)
        return out if len(out) > 1 else summary

    def pi_parametric_bootstrap_dev(self, d_rates, d_states, d_summary, d_rows, d_rate_mean, d_rate_sd, d_ws, replicates, seed=1,
                                    level=0.95, locus_ids=None, stream=0, ws_bytes=None):
        """tphip_pi_parametric_bootstrap_dev on device tensors (d_rows / d_rate_mean / d_rate_sd may be None)."""
        opts, ids = self._band_opts(ParbootOpts, replicates, seed, level, locus_ids)
        _check(self._lib.tphip_pi_parametric_bootstrap_dev(self._h, _ptr(d_rates), _ptr(d_states), ctypes.byref(opts), _ptr(d_summary),
                                                           _ptr(d_rows), _ptr(d_rate_mean), _ptr(d_rate_sd), _ptr(d_ws),
                                                           _ws_nbytes(d_ws, ws_bytes), stream))

    def profile_enable(self, on=True):
        _check(self._lib.tphip_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, reset=True):
        a, b, n = _f64(), _f64(), _i64()
        _check(self._lib.tphip_profile_read(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), 1 if reset else 0))
        return a.value, b.value, n.value

    def last_eval_count(self):
        n = _i64()
        _check(self._lib.tphip_last_eval_count(self._h, ctypes.byref(n)))
        return n.value

    def last_round_count(self):
        """Evaluation rounds of the last site-rate launch summed over its wavefronts: last_eval_count() / (64 * rounds) is
        the share of the issued lane-evaluations that carried a column."""
        n = _i64()
        _check(self._lib.tphip_last_round_count(self._h, ctypes.byref(n)))
        return n.value


# what Plan's five calls of a signal / noise family differ in
_QuartetFamily = collections.namedtuple("_QuartetFamily", "opts prefix row planes")
_EQUAL_TIPS = _QuartetFamily(Plan._quartet_opts, "tphip_quartet", 8, 2)
_UNEQUAL_TIPS = _QuartetFamily(Plan._unequal_quartet_opts, "tphip_unequal_quartet", 13, 3)


class _DeviceCache:
    def __init__(self, plan):
        self.plan, self.ptr = plan, _vp()

    def release(self):
        if self.ptr:
            _check(self.plan._lib.tphip_free_device(self.plan._h, self.ptr))
            self.ptr = _vp()


def bootstrap_counts(n, rep0=0, nrep=1, seed=1, locus_id=0, device=0):
    """The bootstrap's draw kernel alone (tphip_bootstrap_counts): uint16 [nrep, n], row k = how often each of the n columns
    of a locus with stream id `locus_id` is drawn in replicate rep0 + k."""
    out = np.zeros((int(nrep), int(n)), np.uint16)
    _check(load().tphip_bootstrap_counts(device, int(seed) & 0xFFFFFFFFFFFFFFFF, int(locus_id), int(n), int(rep0), int(nrep),
                                         out.ctypes.data))
    return out


def summarize_rows(rows, level=0.95, device=0):
    """The bootstrap's summary kernel on any replicate rows [L, B, Wb] (tphip_summarize_rows): [L, 4, Wb] = mean, sd (B - 1 in
    the denominator), and the quantiles at (1 - level) / 2 and 1 - (1 - level) / 2 by numpy's default rule."""
    rows = _np(rows, np.float64)
    if rows.ndim != 3:
        raise TphipError("rows must be [L, B, Wb]")
    L, B, Wb = rows.shape
    summary = np.zeros((L, 4, Wb))
    _check(load().tphip_summarize_rows(device, rows.ctypes.data, L, B, Wb, float(level), summary.ctypes.data))
    return summary


LOCUS_SET_EQUAL, LOCUS_SET_UNEQUAL = 0, 1


def _locus_set_opts(order, family=LOCUS_SET_EQUAL, window_cap=128, tail_tolerance=0.0, n_head=0):
    """order: int [n_q, K].  Returns the options and the array they point into (keep it alive)."""
    order = _np(order, np.int32)
    if order.ndim != 2:
        raise TphipError("order must be [n_q, K]")
    opts = LocusSetOpts(struct_size=ctypes.sizeof(LocusSetOpts), n_q=order.shape[0], n_k=order.shape[1], family=int(family),
                        window_cap=int(window_cap), tail_tolerance=float(tail_tolerance), n_head=int(n_head), order=order.ctypes.data)
    return opts, order


def locus_set_rows(locus_rows, order, device=0):
    """The normal-approximation rows of the sets of loci order[q, :k], k = 1..K (tphip_locus_set_rows): locus_rows [L, n_q, 8]
    as quartet_tables returns them or [L, n_q, 13] as unequal_quartet_tables does, order int [n_q, K] distinct locus indices
    per quartet.  Returns [n_q, K, 8 or 13] in the per-locus layout: the sums added left to right in the order given, the
    probabilities by the family's own rule; row k = 1 is the per-locus row of locus order[q, 0] bit for bit."""
    locus_rows = _np(locus_rows, np.float64)
    if locus_rows.ndim != 3 or locus_rows.shape[2] not in (8, 13):
        raise TphipError("locus_rows must be [L, n_q, 8] or [L, n_q, 13]")
    opts, order = _locus_set_opts(order, LOCUS_SET_EQUAL if locus_rows.shape[2] == 8 else LOCUS_SET_UNEQUAL)
    if order.shape[0] != locus_rows.shape[1]:
        raise TphipError("order must have one row per quartet of locus_rows")
    rows = np.zeros(order.shape + (locus_rows.shape[2],))
    _check(load().tphip_locus_set_rows(int(device), locus_rows.ctypes.data, locus_rows.shape[0], ctypes.byref(opts), rows.ctypes.data))
    return rows


def locus_set_rows_dev(d_locus_rows, nloci, order, d_rows, family=LOCUS_SET_EQUAL, device=0, stream=0):
    """tphip_locus_set_rows_dev on device tensors: d_locus_rows [L, n_q, 8 or 13], order a host array [n_q, K], d_rows
    [n_q, K, 8 or 13]."""
    opts, order = _locus_set_opts(order, family)
    _check(load().tphip_locus_set_rows_dev(int(device), _ptr(d_locus_rows), int(nloci), ctypes.byref(opts), _ptr(d_rows), stream))


def state_histogram(states, locus_offsets, device=0):
    """Per-locus histogram [L, 16] of the state masks (HarvestFrequencies, bf:968), counted on the GPU."""
    states = _np(states, np.uint8)
    off = _np(locus_offsets, np.int64)
    ntaxa, ncols = states.shape
    hist = np.empty((len(off) - 1, 16), np.int64)
    _check(load().tphip_state_histogram(device, states.ctypes.data, ncols, ntaxa, off.ctypes.data, len(off) - 1,
                                        hist.ctypes.data))
    return hist


def _concordance_sets(group_offsets, group_taxa):
    """The set tables of the concordance calls: the struct and the arrays it points into (keep them alive)."""
    goff, taxa = _np(group_offsets, np.int64).reshape(-1), _np(group_taxa, np.int32).reshape(-1)
    if len(goff) % 4 != 1:
        raise TphipError("group_offsets must have 4 * n_sets + 1 entries")
    if len(goff) and len(taxa) < goff.max():   # (what the offsets say is the library's to judge; what they reach must exist)
        raise TphipError("group_offsets reach beyond group_taxa")
    sets = ConcordanceSets(struct_size=ctypes.sizeof(ConcordanceSets), n_sets=len(goff) // 4, group_offsets=goff.ctypes.data,
                           group_taxa=taxa.ctypes.data if len(taxa) else None)
    return sets, goff, taxa


def concordance_counts(states, locus_offsets, group_offsets, group_taxa, ncols_total=None, device=0):
    """Site concordance counts (tphip_concordance_counts): uint64 [L, n_sets, 3] = per locus and set of four taxon groups
    A, B | C, D the quartets of A x B x C x D its columns support as ab|cd, ac|bd and ad|bc, over cells of exactly one base.
    states uint8 [ntaxa, pitch]; ncols_total: the columns of the batch when the rows are longer than it (default: all of them).
    group_offsets int64 [4 * n_sets + 1] into group_taxa (taxon rows): groups A, B, C, D of set s are 4s .. 4s + 3."""
    states = _np(states, np.uint8)
    off = _np(locus_offsets, np.int64)
    ntaxa, pitch = states.shape
    ncols = pitch if ncols_total is None else int(ncols_total)
    sets, goff, taxa = _concordance_sets(group_offsets, group_taxa)
    counts = np.zeros((len(off) - 1, sets.n_sets, 3), np.uint64)
    _check(load().tphip_concordance_counts(int(device), states.ctypes.data, ncols, pitch, ntaxa, off.ctypes.data, len(off) - 1,
                                           ctypes.byref(sets), counts.ctypes.data))
    return counts


def concordance_counts_dev(d_states, ncols_total, row_pitch, ntaxa, d_locus_offsets, nloci, group_offsets, group_taxa, d_counts,
                           device=0, stream=0):
    """tphip_concordance_counts_dev on device tensors: d_states uint8 [ntaxa, row_pitch], d_locus_offsets int64 [nloci + 1],
    d_counts [nloci, n_sets, 3] of 64-bit integers; the set tables are host arrays.  Waits for its kernels."""
    sets, goff, taxa = _concordance_sets(group_offsets, group_taxa)
    _check(load().tphip_concordance_counts_dev(int(device), _ptr(d_states), int(ncols_total), int(row_pitch), int(ntaxa),
                                               _ptr(d_locus_offsets), int(nloci), ctypes.byref(sets), _ptr(d_counts), stream))


def concordance_rows(counts, node_sets, device=0):
    """The per-internode rows of the concordance counts (tphip_concordance_rows): counts uint64 [L, n_sets, 3], node_sets int64
    [n_nodes + 1] (internode i owns the sets node_sets[i] .. node_sets[i + 1] - 1: pooled, nearest-tip quartet, sampled
    quartets).  Returns [L, n_nodes, 12] = pooled_c, pooled_1, pooled_2, near_c, near_1, near_2, sCF, sDF1, sDF2, sN,
    n_decisive, n_quartets."""
    counts = _np(counts, np.uint64)
    if counts.ndim != 3 or counts.shape[2] != 3:
        raise TphipError("counts must be [L, n_sets, 3]")
    nodes = _np(node_sets, np.int64).reshape(-1)
    rows = np.zeros((counts.shape[0], len(nodes) - 1, 12))
    _check(load().tphip_concordance_rows(int(device), counts.ctypes.data, counts.shape[0], counts.shape[1], nodes.ctypes.data,
                                         len(nodes) - 1, rows.ctypes.data))
    return rows


def concordance_rows_dev(d_counts, nloci, n_sets, node_sets, d_rows, device=0, stream=0):
    """tphip_concordance_rows_dev on device tensors: d_counts [nloci, n_sets, 3], d_rows [nloci, n_nodes, 12]; node_sets is a
    host array.  Waits for its kernel."""
    nodes = _np(node_sets, np.int64).reshape(-1)
    _check(load().tphip_concordance_rows_dev(int(device), _ptr(d_counts), int(nloci), int(n_sets), nodes.ctypes.data, len(nodes) - 1,
                                             _ptr(d_rows), stream))


def compress_columns(states, locus_offsets, device=0, want_map=True):
    """Unique site patterns per locus (tphip_compress_columns): returns (pattern_states [ntaxa, P] uint8,
    pattern_offsets int64[L+1], weights float64[P], column -> pattern map int64[ncols] or None)."""
    states = _np(states, np.uint8)
    off = _np(locus_offsets, np.int64)
    ntaxa, ncols = states.shape
    buf = np.empty(ntaxa * max(ncols, 1), np.uint8)
    new_off = np.empty(len(off), np.int64)
    w = np.empty(max(ncols, 1))
    cmap = np.empty(max(ncols, 1), np.int64) if want_map else None
    npat = _i64()
    _check(load().tphip_compress_columns(device, states.ctypes.data, ncols, ntaxa, off.ctypes.data, len(off) - 1,
                                         buf.ctypes.data, new_off.ctypes.data, w.ctypes.data,
                                         cmap.ctypes.data if want_map else None, ctypes.byref(npat)))
    P = npat.value
    return buf[:ntaxa * P].reshape(ntaxa, P).copy(), new_off, w[:P].copy(), (cmap[:ncols] if want_map else None)


def townsend_pi_dense(times, rates, device=0):
    """tapir/compute.py:46-48 for a vector of times and a vector of rates -> (n_times, n) matrix (GPU)."""
    rates = _np(rates, np.float64).reshape(-1)
    times = _np(times, np.float64).reshape(-1)
    out = np.empty((times.size, rates.size))
    _check(load().tphip_townsend_pi_dense(device, rates.ctypes.data, rates.size, times.ctypes.data, times.size,
                                          out.ctypes.data))
    return out


def quad_townsend(a, b, rates, integ_mode=INTEG_QUADPACK, device=0):
    """tapir/compute.py:50-52 over a vector of rates -> (integral[n], abserr[n]) (GPU, dqagse emulation)."""
    rates = _np(rates, np.float64).reshape(-1)
    integral, abserr = np.empty(rates.size), np.empty(rates.size)
    _check(load().tphip_quad_townsend(device, rates.ctypes.data, rates.size, float(a), float(b), integ_mode,
                                      integral.ctypes.data, abserr.ctypes.data))
    return integral, abserr

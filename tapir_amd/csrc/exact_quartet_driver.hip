// exact_quartet_driver.hip -- the exact quartet resolution probabilities: the C entry points
// tphip_quartet_exact / tphip_quartet_exact_dev and tphip_quartet_exact_workspace_bytes.  The kernels are in
// exact_quartet_kernels.hpp, the window rule in exact_quartet_window.hpp.
//
// The options are plain numbers and travel as kernel arguments; the window of a pair is chosen on the device and the
// spectrum kernel's grid is sized for the cap, so the _dev call copies nothing, never synchronises and can be captured.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "exact_quartet_kernels.hpp"
#include "tphip_internal.hpp"

namespace {

constexpr int32_t kEqMaxQuartets = 256;
constexpr int64_t kEqMaxPairs = (int64_t)1 << 24;   // pairs of one call
constexpr int64_t kEqPairsPerLaunch = 65535;        // the grid's second dimension

struct EqOpts {
    int32_t n_q, cap;
    double tol;
};

int eq_read_opts(const tphip_plan* p, const tphip_quartet_exact_opts* o, EqOpts* out) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_quartet_exact_opts");
    if (o->struct_size < offsetof(tphip_quartet_exact_opts, tail_tolerance) + sizeof(double))
        return fail(TPHIP_ERR_INVALID, "tphip_quartet_exact_opts.struct_size is too small: set it to sizeof(tphip_quartet_exact_opts)");
    if (o->n_q < 1 || o->n_q > kEqMaxQuartets) return fail(TPHIP_ERR_INVALID, "n_q must be in 1..256");
    const int32_t cap = o->window_cap == 0 ? kEqDefaultWindow : o->window_cap;
    if (!exact_window_valid(cap)) return fail(TPHIP_ERR_INVALID, "window_cap must be a power of two in 16..512 (0: 128)");
    const double tol = o->tail_tolerance == 0.0 ? kEqDefaultTail : o->tail_tolerance;
    if (!(tol > 0.0) || !(tol < 1.0)) return fail(TPHIP_ERR_INVALID, "tail_tolerance must be in (0, 1) (0: 1e-12)");
    if (p->nloci * (int64_t)o->n_q > kEqMaxPairs)
        return fail(TPHIP_ERR_INVALID, "nloci * n_q exceeds 2^24 pairs: call with fewer quartets at a time");
    out->n_q = o->n_q;
    out->cap = cap;
    out->tol = tol;
    return TPHIP_OK;
}

inline size_t eq_moment_bytes(int64_t pairs) { return align_up(sizeof(EqMoment) * (size_t)pairs, 256); }

inline size_t eq_workspace_bytes(const tphip_plan* p, const EqOpts& o) {
    const int64_t pairs = p->nloci * (int64_t)o.n_q;
    return std::max<size_t>(eq_moment_bytes(pairs) + sizeof(double) * 3 * (size_t)exact_tiles(o.cap) * (size_t)pairs, 256);
}

}  // namespace

extern "C" {

int tphip_quartet_exact_workspace_bytes(const tphip_plan* p, const tphip_quartet_exact_opts* opts, size_t* bytes) {
    EqOpts o;
    int rc = eq_read_opts(p, opts, &o);
    if (rc) return rc;
    if (bytes) *bytes = eq_workspace_bytes(p, o);
    return TPHIP_OK;
}

int tphip_quartet_exact_dev(tphip_plan* p, const double* d_y, const double* d_x1, const double* d_x2,
                            const tphip_quartet_exact_opts* opts, double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    EqOpts o;
    int rc = eq_read_opts(p, opts, &o);
    if (rc) return rc;
    if (p->nloci == 0) return TPHIP_OK;
    if (!d_rows || !ws || (p->ncols && (!d_y || !d_x1 || !d_x2))) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (((uintptr_t)ws & 7u) != 0) return fail(TPHIP_ERR_INVALID, "workspace must be 8-byte aligned");
    if (ws_bytes < eq_workspace_bytes(p, o)) return fail(TPHIP_ERR_INVALID, "ws_bytes: workspace smaller than tphip_quartet_exact_workspace_bytes()");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    EqParams P;
    P.y = d_y; P.x1 = d_x1; P.x2 = d_x2;
    P.locus_offsets = p->d_offsets.p;
    P.ncols = p->ncols;
    P.pairs = p->nloci * (int64_t)o.n_q;
    P.pair0 = 0;
    P.n_q = o.n_q;
    P.cap = o.cap;
    P.tiles_cap = exact_tiles(o.cap);
    P.tol = o.tol;
    P.mom = (EqMoment*)ws;
    P.partial = (double*)((char*)ws + eq_moment_bytes(P.pairs));
    P.rows = d_rows;
    exact_moment_kernel<<<dim3((unsigned)P.pairs), dim3(kEqMomentBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    const size_t lds = sizeof(double) * (size_t)(4 * kEqSiteTile + 2 * kEqWeights * o.cap + 6);
    for (int64_t p0 = 0; p0 < P.pairs; p0 += kEqPairsPerLaunch) {
        P.pair0 = p0;
        const int64_t np = std::min<int64_t>(kEqPairsPerLaunch, P.pairs - p0);
        exact_spectrum_kernel<<<dim3((unsigned)std::min<int32_t>(P.tiles_cap, kEqGridTiles), (unsigned)np), dim3(kEqBlock), lds, st>>>(P);
        HIP_TRY(hipGetLastError());
    }
    P.pair0 = 0;
    exact_finalise_kernel<<<dim3((unsigned)((P.pairs + kEqFinalBlock - 1) / kEqFinalBlock)), dim3(kEqFinalBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int tphip_quartet_exact(tphip_plan* p, const double* y, const double* x1, const double* x2, const tphip_quartet_exact_opts* opts,
                        double* rows) {
    EqOpts o;
    int rc = eq_read_opts(p, opts, &o);
    if (rc) return rc;
    const size_t plane = (size_t)o.n_q * (size_t)p->ncols, nrows = (size_t)p->nloci * (size_t)o.n_q * kEqRow;
    if (nrows == 0) return TPHIP_OK;
    if (!rows || (plane && (!y || !x1 || !x2))) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const size_t ws_bytes = eq_workspace_bytes(p, o);
    const double* d_y = S.in(y, plane);
    const double* d_x1 = S.in(x1, plane);
    const double* d_x2 = x2 == x1 ? d_x1 : S.in(x2, plane);   // an equal-tip quartet: one noise plane serves both
    double* d_rows = S.out(rows, nrows);
    char* ws = S.scratch<char>(ws_bytes);
    if (S.rc) return S.rc;
    rc = tphip_quartet_exact_dev(p, d_y, d_x1, d_x2, opts, d_rows, ws, ws_bytes, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

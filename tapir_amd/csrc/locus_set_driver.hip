// locus_set_driver.hip -- locus-set accumulation curves: the C entry points tphip_locus_set_rows /
// tphip_locus_set_rows_dev (the normal rows of the sets o_q[0..k)) and tphip_locus_set_exact / tphip_locus_set_exact_dev with
// tphip_locus_set_exact_workspace_bytes (their exact rows).  The kernels are in locus_set_kernels.hpp.
//
// The order is a host array: it is validated here (distinct indices in range, per quartet).  The exact call hands it to the
// device as kernel arguments, so nothing is copied; everything after that is decided on the device -- the head of a quartet,
// which prefixes are point laws -- and the spectrum kernel's grid is sized for the cap: the exact _dev call never synchronises
// and can be captured.  The rows call has no workspace: it copies the order into a buffer of its own and waits before it frees it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "locus_set_kernels.hpp"
#include "tphip_internal.hpp"

namespace {

constexpr int32_t kLsMaxQuartets = 256;
constexpr int64_t kLsMaxPairs = (int64_t)1 << 24;   // (locus, quartet) pairs of one call

struct LsOpts {
    int32_t n_q, n_k, n_head, family, cap;
    double tol;
    const int32_t* order;
};

// Everything but the order's contents; exact: the fields of the exact rows too.
int ls_read_opts(const tphip_locus_set_opts* o, int64_t nloci, bool exact, LsOpts* out) {
    if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_locus_set_opts");
    if (o->struct_size < offsetof(tphip_locus_set_opts, order) + sizeof(const int32_t*))
        return fail(TPHIP_ERR_INVALID, "tphip_locus_set_opts.struct_size is too small: set it to sizeof(tphip_locus_set_opts)");
    if (nloci < 0) return fail(TPHIP_ERR_INVALID, "negative nloci");
    if (o->n_q < 1 || o->n_q > kLsMaxQuartets) return fail(TPHIP_ERR_INVALID, "n_q must be in 1..256");
    if (o->n_k < 1 || (int64_t)o->n_k > nloci) return fail(TPHIP_ERR_INVALID, "n_k must be in 1..nloci");
    if (nloci * (int64_t)o->n_q > kLsMaxPairs)
        return fail(TPHIP_ERR_INVALID, "nloci * n_q exceeds 2^24 pairs: call with fewer quartets at a time");
    out->n_q = o->n_q;
    out->n_k = o->n_k;
    out->family = o->family;
    out->order = o->order;
    out->n_head = o->n_k;
    out->cap = kEqDefaultWindow;
    out->tol = kEqDefaultTail;
    if (!exact) {
        if (o->family != TPHIP_LOCUS_SET_EQUAL && o->family != TPHIP_LOCUS_SET_UNEQUAL)
            return fail(TPHIP_ERR_INVALID, "family must be TPHIP_LOCUS_SET_EQUAL or TPHIP_LOCUS_SET_UNEQUAL");
        return TPHIP_OK;
    }
    out->cap = o->window_cap == 0 ? kEqDefaultWindow : o->window_cap;
    if (!exact_window_valid(out->cap)) return fail(TPHIP_ERR_INVALID, "window_cap must be a power of two in 16..512 (0: 128)");
    out->tol = o->tail_tolerance == 0.0 ? kEqDefaultTail : o->tail_tolerance;
    if (!(out->tol > 0.0) || !(out->tol < 1.0)) return fail(TPHIP_ERR_INVALID, "tail_tolerance must be in (0, 1) (0: 1e-12)");
    if (o->n_head < 0 || o->n_head > o->n_k) return fail(TPHIP_ERR_INVALID, "n_head must be in 1..n_k (0: n_k)");
    if (o->n_head) out->n_head = o->n_head;
    return TPHIP_OK;
}

// every quartet's order: n_k distinct indices in 0..nloci-1
int ls_check_order(const LsOpts& o, int64_t nloci) {
    if (!o.order) return fail(TPHIP_ERR_INVALID, "null order");
    std::vector<int32_t> seen((size_t)nloci, -1);
    for (int32_t q = 0; q < o.n_q; ++q)
        for (int32_t k = 0; k < o.n_k; ++k) {
            const int32_t l = o.order[(size_t)q * o.n_k + k];
            if (l < 0 || (int64_t)l >= nloci) return fail(TPHIP_ERR_INVALID, "order: a locus index is out of range");
            if (seen[l] == q) return fail(TPHIP_ERR_INVALID, "order: a locus index is repeated within a quartet");
            seen[l] = q;
        }
    return TPHIP_OK;
}

// the exact call's workspace: order, per-pair sums, per-prefix records, heads, partial sums
struct LsLayout {
    size_t order, sums, prefix, head, partial, total;
};

LsLayout ls_layout(int64_t nloci, const LsOpts& o) {
    LsLayout L;
    size_t at = 0;
    L.order = at;
    at += align_up(sizeof(int32_t) * (size_t)o.n_q * (size_t)o.n_k, 256);
    L.sums = at;
    at += align_up(sizeof(LsSums) * (size_t)nloci * (size_t)o.n_q, 256);
    L.prefix = at;
    at += align_up(sizeof(LsPrefix) * (size_t)o.n_q * (size_t)o.n_k, 256);
    L.head = at;
    at += align_up(sizeof(int32_t) * (size_t)o.n_q, 256);
    L.partial = at;
    at += align_up(sizeof(double) * 3 * (size_t)exact_tiles(o.cap) * (size_t)o.n_q * (size_t)o.n_head, 256);
    L.total = at;
    return L;
}

}  // namespace

extern "C" {

int tphip_locus_set_rows_dev(int32_t device, const double* d_locus_rows, int64_t nloci, const tphip_locus_set_opts* opts,
                             double* d_rows, void* stream) {
    LsOpts o;
    int rc = ls_read_opts(opts, nloci, false, &o);
    if (rc) return rc;
    rc = ls_check_order(o, nloci);
    if (rc) return rc;
    if (!d_locus_rows || !d_rows) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch S;   // freed on return: hipFree waits for the kernels that read it
    const size_t n_order = (size_t)o.n_q * (size_t)o.n_k;
    int32_t* d_order = S.get<int32_t>(n_order);
    if (!d_order) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpyAsync(d_order, o.order, sizeof(int32_t) * n_order, hipMemcpyHostToDevice, st));
    LsRowsParams P;
    P.locus_rows = d_locus_rows;
    P.order = d_order;
    P.n_q = o.n_q;
    P.n_k = o.n_k;
    P.sums = o.family == TPHIP_LOCUS_SET_EQUAL ? kLsEqualSums : kLsUnequalSums;
    P.row = o.family == TPHIP_LOCUS_SET_EQUAL ? kLsEqualRow : kLsUnequalRow;
    P.rows = d_rows;
    locus_set_sums_kernel<<<dim3((unsigned)((o.n_q * P.sums + kLsBlock - 1) / kLsBlock)), dim3(kLsBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    locus_set_probabilities_kernel<<<dim3((unsigned)((n_order + kLsBlock - 1) / kLsBlock)), dim3(kLsBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // the caller's order and d_order have been read
    return TPHIP_OK;
}

int tphip_locus_set_rows(int32_t device, const double* locus_rows, int64_t nloci, const tphip_locus_set_opts* opts, double* rows) {
    LsOpts o;
    int rc = ls_read_opts(opts, nloci, false, &o);
    if (rc) return rc;
    rc = ls_check_order(o, nloci);
    if (rc) return rc;
    if (!locus_rows || !rows) return fail(TPHIP_ERR_INVALID, "null host pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    const size_t w = o.family == TPHIP_LOCUS_SET_EQUAL ? kLsEqualRow : kLsUnequalRow;
    Staging S;
    const double* d_in = S.in(locus_rows, (size_t)nloci * (size_t)o.n_q * w);
    double* d_out = S.out(rows, (size_t)o.n_q * (size_t)o.n_k * w);
    if (S.rc) return S.rc;
    rc = tphip_locus_set_rows_dev(device, d_in, nloci, opts, d_out, nullptr);
    return rc ? rc : S.finish();
}

int tphip_locus_set_exact_workspace_bytes(const tphip_plan* p, const tphip_locus_set_opts* opts, size_t* bytes) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    LsOpts o;
    int rc = ls_read_opts(opts, p->nloci, true, &o);
    if (rc) return rc;
    if (bytes) *bytes = ls_layout(p->nloci, o).total;
    return TPHIP_OK;
}

int tphip_locus_set_exact_dev(tphip_plan* p, const double* d_y, const double* d_x1, const double* d_x2,
                              const tphip_locus_set_opts* opts, double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    LsOpts o;
    int rc = ls_read_opts(opts, p->nloci, true, &o);
    if (rc) return rc;
    rc = ls_check_order(o, p->nloci);
    if (rc) return rc;
    if (!d_rows || !ws || (p->ncols && (!d_y || !d_x1 || !d_x2))) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (((uintptr_t)ws & 7u) != 0) return fail(TPHIP_ERR_INVALID, "workspace must be 8-byte aligned");
    const LsLayout L = ls_layout(p->nloci, o);
    if (ws_bytes < L.total) return fail(TPHIP_ERR_INVALID, "ws_bytes: workspace smaller than tphip_locus_set_exact_workspace_bytes()");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    // The order travels as kernel arguments, kLsOrderBatch indices a launch (as the quartets' lengths do in sections 3.6 and
    // 3.8): they are read at the launch, so the caller's array need not outlive the call, nothing is copied and nothing waits.
    const int64_t n_order = (int64_t)o.n_q * o.n_k;
    for (int64_t at = 0; at < n_order; at += kLsOrderBatch) {
        LsOrderBatch B = {};
        const int32_t n = (int32_t)std::min<int64_t>(kLsOrderBatch, n_order - at);
        std::copy(o.order + at, o.order + at + n, B.v);
        locus_set_order_kernel<<<dim3((unsigned)((n + kLsBlock - 1) / kLsBlock)), dim3(kLsBlock), 0, st>>>((int32_t*)(base + L.order), at, n, B);
        HIP_TRY(hipGetLastError());
    }
    LsParams P;
    P.y = d_y; P.x1 = d_x1; P.x2 = d_x2;
    P.locus_offsets = p->d_offsets.p;
    P.ncols = p->ncols;
    P.pairs = p->nloci * (int64_t)o.n_q;
    P.n_q = o.n_q;
    P.n_k = o.n_k;
    P.n_head = o.n_head;
    P.cap = o.cap;
    P.tiles_cap = exact_tiles(o.cap);
    P.tol = o.tol;
    P.order = (const int32_t*)(base + L.order);
    P.sums = (LsSums*)(base + L.sums);
    P.prefix = (LsPrefix*)(base + L.prefix);
    P.head = (int32_t*)(base + L.head);
    P.partial = (double*)(base + L.partial);
    P.rows = d_rows;
    locus_set_moment_kernel<<<dim3((unsigned)P.pairs), dim3(kEqMomentBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    locus_set_head_kernel<<<dim3((unsigned)((o.n_q + kLsBlock - 1) / kLsBlock)), dim3(kLsBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    const size_t lds = sizeof(double) * (size_t)(4 * kEqSiteTile + 2 * kEqWeights * o.cap + 6);
    locus_set_spectrum_kernel<<<dim3((unsigned)std::min<int32_t>(P.tiles_cap, kEqGridTiles), (unsigned)o.n_q), dim3(kEqBlock), lds, st>>>(P);
    HIP_TRY(hipGetLastError());
    const int64_t nrows = (int64_t)o.n_q * o.n_k;
    locus_set_finalise_kernel<<<dim3((unsigned)((nrows + kLsBlock - 1) / kLsBlock)), dim3(kLsBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int tphip_locus_set_exact(tphip_plan* p, const double* y, const double* x1, const double* x2, const tphip_locus_set_opts* opts,
                          double* rows) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    LsOpts o;
    int rc = ls_read_opts(opts, p->nloci, true, &o);
    if (rc) return rc;
    rc = ls_check_order(o, p->nloci);
    if (rc) return rc;
    const size_t plane = (size_t)o.n_q * (size_t)p->ncols, nrows = (size_t)o.n_q * (size_t)o.n_k * kEqRow;
    if (!rows || (plane && (!y || !x1 || !x2))) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const size_t ws_bytes = ls_layout(p->nloci, o).total;
    const double* d_y = S.in(y, plane);
    const double* d_x1 = S.in(x1, plane);
    const double* d_x2 = x2 == x1 ? d_x1 : S.in(x2, plane);   // an equal-tip quartet: one noise plane serves both
    double* d_rows = S.out(rows, nrows);
    char* ws = S.scratch<char>(ws_bytes);
    if (S.rc) return S.rc;
    rc = tphip_locus_set_exact_dev(p, d_y, d_x1, d_x2, opts, d_rows, ws, ws_bytes, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

// quartet_driver.hip -- quartet signal and noise probabilities for per-locus site rates: the C entry
// points tphip_quartet_tables / tphip_quartet_sites (+ _dev) and tphip_quartet_workspace_bytes.  The kernels are in
// quartet_kernels.hpp.
//
// The quartets' lengths travel as kernel arguments, kQtBatch quartets per launch, so the _dev calls copy nothing and never
// synchronise.  A (locus, quartet) entry is computed by the same code from the locus' own columns whatever the batch, so
// neither the list around a quartet nor the loci around a locus change a bit of its row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "quartet_kernels.hpp"
#include "tphip_internal.hpp"

namespace {

constexpr int32_t kQtMaxQuartets = 256;

int qt_read_opts(const tphip_quartet_opts* o, int32_t* n_q) {
    if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_quartet_opts");
    if (o->struct_size < offsetof(tphip_quartet_opts, internode) + sizeof(const double*))
        return fail(TPHIP_ERR_INVALID, "tphip_quartet_opts.struct_size is too small: set it to sizeof(tphip_quartet_opts)");
    if (o->n_q < 1 || o->n_q > kQtMaxQuartets) return fail(TPHIP_ERR_INVALID, "n_q must be in 1..256");
    if (!o->tip || !o->internode) return fail(TPHIP_ERR_INVALID, "null quartet lengths");
    for (int32_t q = 0; q < o->n_q; ++q) {
        if (!(o->tip[q] >= 0.0) || !std::isfinite(o->tip[q]))
            return fail(TPHIP_ERR_INVALID, "quartet " + std::to_string(q) + ": the tip length T must be finite and >= 0");
        if (!(o->internode[q] > 0.0) || !std::isfinite(o->internode[q]))
            return fail(TPHIP_ERR_INVALID, "quartet " + std::to_string(q) + ": the internode length t_o must be finite and > 0");
    }
    *n_q = o->n_q;
    return TPHIP_OK;
}

inline size_t qt_partial_bytes(const tphip_plan* p, int32_t n_q) {
    return sizeof(double) * (size_t)p->n_pi_chunks * (size_t)n_q * kQtSums;
}

// kernel(P, batch) over the plan's chunks for every batch of the list
template <typename Kernel>
int qt_launch_batches(const tphip_plan* p, QuartetParams P, const tphip_quartet_opts* o, Kernel kernel, hipStream_t st) {
    if (p->n_pi_chunks == 0) return TPHIP_OK;
    for (int32_t q0 = 0; q0 < P.n_q; q0 += kQtBatch) {
        QuartetBatch B;
        P.q0 = q0;
        P.nq = std::min<int32_t>(kQtBatch, P.n_q - q0);
        for (int32_t k = 0; k < kQtBatch; ++k) {
            B.tip[k] = k < P.nq ? o->tip[q0 + k] : 0.0;
            B.internode[k] = k < P.nq ? o->internode[q0 + k] : 0.0;
        }
        kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(kQtBlock), 0, st>>>(P, B);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

QuartetParams qt_params(const tphip_plan* p, const double* d_rates, const int32_t* d_nres, int32_t n_q) {
    QuartetParams P;
    P.pi = plan_pi_params(p, d_rates, d_nres);
    P.models = p->d_models.p;
    P.f81 = p->model == TPHIP_MODEL_F81 ? 1 : 0;
    P.n_q = n_q; P.q0 = 0; P.nq = 0;
    P.partial = nullptr; P.sites = nullptr;
    P.ncols = p->ncols;
    return P;
}

}  // namespace

extern "C" {

int tphip_quartet_workspace_bytes(const tphip_plan* p, const tphip_quartet_opts* opts, size_t* bytes) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = qt_read_opts(opts, &n_q);
    if (rc) return rc;
    if (bytes) *bytes = std::max<size_t>(qt_partial_bytes(p, n_q), 256);
    return TPHIP_OK;
}

int tphip_quartet_tables_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_quartet_opts* opts,
                             double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = qt_read_opts(opts, &n_q);
    if (rc) return rc;
    if (p->nloci == 0) return TPHIP_OK;
    if (!d_rows || !ws || (p->ncols && !d_rates)) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (((uintptr_t)ws & 7u) != 0) return fail(TPHIP_ERR_INVALID, "workspace must be 8-byte aligned");
    if (ws_bytes < qt_partial_bytes(p, n_q)) return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than tphip_quartet_workspace_bytes()");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    QuartetParams P = qt_params(p, d_rates, d_nres, n_q);
    P.partial = (double*)ws;
    rc = qt_launch_batches(p, P, opts, quartet_partial_kernel, st);
    if (rc) return rc;
    quartet_reduce_kernel<<<dim3((unsigned)p->nloci), dim3(kQtReduceBlock), 0, st>>>(P.partial, p->d_locus_pichunk_offsets.p, n_q, d_rows);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int tphip_quartet_sites_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_quartet_opts* opts,
                            double* d_sites, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = qt_read_opts(opts, &n_q);
    if (rc) return rc;
    if (p->ncols == 0) return TPHIP_OK;
    if (!d_sites || !d_rates) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    QuartetParams P = qt_params(p, d_rates, d_nres, n_q);
    P.sites = d_sites;
    return qt_launch_batches(p, P, opts, quartet_sites_kernel, (hipStream_t)stream);
}

int tphip_quartet_tables(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_quartet_opts* opts, double* rows) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = qt_read_opts(opts, &n_q);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, nrows = (size_t)p->nloci * (size_t)n_q * kQtRow;
    if (nrows == 0) return TPHIP_OK;
    if (!rows || (n && !rates)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    const size_t ws_bytes = std::max<size_t>(qt_partial_bytes(p, n_q), 256);
    double* d_r = S.get<double>(n);
    int32_t* d_n = nres ? S.get<int32_t>(n) : nullptr;
    double* d_rows = S.get<double>(nrows);
    char* ws = S.get<char>(ws_bytes);
    if (!d_r || (nres && !d_n) || !d_rows || !ws) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    if (n) {
        HIP_TRY(hipMemcpy(d_r, rates, sizeof(double) * n, hipMemcpyHostToDevice));
        if (nres) HIP_TRY(hipMemcpy(d_n, nres, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    }
    rc = tphip_quartet_tables_dev(p, d_r, d_n, opts, d_rows, ws, ws_bytes, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(rows, d_rows, sizeof(double) * nrows, hipMemcpyDeviceToHost));
    return TPHIP_OK;
}

int tphip_quartet_sites(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_quartet_opts* opts, double* sites) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = qt_read_opts(opts, &n_q);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, total = 2 * (size_t)n_q * n;
    if (total == 0) return TPHIP_OK;
    if (!sites || !rates) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    double* d_r = S.get<double>(n);
    int32_t* d_n = nres ? S.get<int32_t>(n) : nullptr;
    double* d_sites = S.get<double>(total);
    if (!d_r || (nres && !d_n) || !d_sites) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_r, rates, sizeof(double) * n, hipMemcpyHostToDevice));
    if (nres) HIP_TRY(hipMemcpy(d_n, nres, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    rc = tphip_quartet_sites_dev(p, d_r, d_n, opts, d_sites, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(sites, d_sites, sizeof(double) * total, hipMemcpyDeviceToHost));
    return TPHIP_OK;
}

}  // extern "C"

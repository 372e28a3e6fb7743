// quartet_driver_common.hpp -- the host side that quartet_driver.hip and unequal_quartet_driver.hip
// (section 3.8) share: the five entry points of a signal / noise family as function templates over its traits F.
//
//   F::Opts, F::Params, F::Batch          the options of the C ABI and the kernels' two arguments
//   F::kBatch, kBlock, kReduceBlock       quartets per launch and the workgroup sizes
//   F::kSums, kRow, kPlanes               sums per (chunk, quartet), numbers per row, per-site planes
//   F::partial_kernel, sites_kernel, reduce_kernel
//   F::read_opts(opts, &n_q)              validation, with the family's own messages
//   F::fill_batch(B, opts, q0, nq)        the lengths of quartets q0 .. q0 + nq - 1, 0 beyond them
//   F::workspace_too_small()              fail() with the family's code and message
//
// The quartets' lengths travel as kernel arguments, kBatch quartets per launch, so the _dev calls copy nothing and never
// synchronise.  A (locus, quartet) entry is computed by the same code from the locus' own columns whatever the batch, so
// neither the list around a quartet nor the loci around a locus change a bit of its row.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "tphip_internal.hpp"

template <typename F>
inline size_t quartet_partial_bytes(const tphip_plan* p, int32_t n_q) {
    return sizeof(double) * (size_t)p->n_pi_chunks * (size_t)n_q * F::kSums;
}

template <typename F>
inline size_t quartet_ws_bytes(const tphip_plan* p, int32_t n_q) { return std::max<size_t>(quartet_partial_bytes<F>(p, n_q), 256); }

// kernel(P, batch) over the plan's chunks for every batch of the list
template <typename F, typename Kernel>
int quartet_launch_batches(const tphip_plan* p, typename F::Params P, const typename F::Opts* o, Kernel kernel, hipStream_t st) {
    if (p->n_pi_chunks == 0) return TPHIP_OK;
    for (int32_t q0 = 0; q0 < P.n_q; q0 += F::kBatch) {
        typename F::Batch B;
        P.q0 = q0;
        P.nq = std::min<int32_t>(F::kBatch, P.n_q - q0);
        F::fill_batch(B, o, q0, P.nq);
        kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(F::kBlock), 0, st>>>(P, B);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

template <typename F>
typename F::Params quartet_params(const tphip_plan* p, const double* d_rates, const int32_t* d_nres, int32_t n_q) {
    typename F::Params P;
    P.pi = plan_pi_params(p, d_rates, d_nres);
    P.models = p->d_models.p;
    P.f81 = p->model == TPHIP_MODEL_F81 ? 1 : 0;
    P.n_q = n_q; P.q0 = 0; P.nq = 0;
    P.partial = nullptr; P.sites = nullptr;
    P.ncols = p->ncols;
    return P;
}

template <typename F>
int quartet_workspace_bytes(const tphip_plan* p, const typename F::Opts* opts, size_t* bytes) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = F::read_opts(opts, &n_q);
    if (rc) return rc;
    if (bytes) *bytes = quartet_ws_bytes<F>(p, n_q);
    return TPHIP_OK;
}

template <typename F>
int quartet_tables_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const typename F::Opts* opts, double* d_rows,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = F::read_opts(opts, &n_q);
    if (rc) return rc;
    if (p->nloci == 0) return TPHIP_OK;
    if (!d_rows || !ws || (p->ncols && !d_rates)) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (((uintptr_t)ws & 7u) != 0) return fail(TPHIP_ERR_INVALID, "workspace must be 8-byte aligned");
    if (ws_bytes < quartet_partial_bytes<F>(p, n_q)) return F::workspace_too_small();
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    typename F::Params P = quartet_params<F>(p, d_rates, d_nres, n_q);
    P.partial = (double*)ws;
    rc = quartet_launch_batches<F>(p, P, opts, F::partial_kernel, st);
    if (rc) return rc;
    F::reduce_kernel<<<dim3((unsigned)p->nloci), dim3(F::kReduceBlock), 0, st>>>(P.partial, p->d_locus_pichunk_offsets.p, n_q, d_rows);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

template <typename F>
int quartet_sites_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const typename F::Opts* opts, double* d_sites,
                      void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = F::read_opts(opts, &n_q);
    if (rc) return rc;
    if (p->ncols == 0) return TPHIP_OK;
    if (!d_sites || !d_rates) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    typename F::Params P = quartet_params<F>(p, d_rates, d_nres, n_q);
    P.sites = d_sites;
    return quartet_launch_batches<F>(p, P, opts, F::sites_kernel, (hipStream_t)stream);
}

template <typename F>
int quartet_tables(tphip_plan* p, const double* rates, const int32_t* nres, const typename F::Opts* opts, double* rows) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = F::read_opts(opts, &n_q);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, nrows = (size_t)p->nloci * (size_t)n_q * F::kRow;
    if (nrows == 0) return TPHIP_OK;
    if (!rows || (n && !rates)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const size_t ws_bytes = quartet_ws_bytes<F>(p, n_q);
    const double* d_r = S.in(rates, n);
    const int32_t* d_n = S.in(nres, n);
    double* d_rows = S.out(rows, nrows);
    char* ws = S.scratch<char>(ws_bytes);
    if (S.rc) return S.rc;
    rc = quartet_tables_dev<F>(p, d_r, d_n, opts, d_rows, ws, ws_bytes, nullptr);
    return rc ? rc : S.finish();
}

template <typename F>
int quartet_sites(tphip_plan* p, const double* rates, const int32_t* nres, const typename F::Opts* opts, double* sites) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    int32_t n_q = 0;
    int rc = F::read_opts(opts, &n_q);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, total = F::kPlanes * (size_t)n_q * n;
    if (total == 0) return TPHIP_OK;
    if (!sites || !rates) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const double* d_r = S.in(rates, n);
    const int32_t* d_n = S.in(nres, n);
    double* d_sites = S.out(sites, total);
    if (S.rc) return S.rc;
    rc = quartet_sites_dev<F>(p, d_r, d_n, opts, d_sites, nullptr);
    return rc ? rc : S.finish();
}

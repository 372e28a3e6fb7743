// site_posterior_params.hpp -- launch parameters of the empirical-Bayes kernels, shared by
// site_rate_launch.hip (the per-column mixture kernels of site_posterior_kernel.hpp) and eb_driver.hip (reduction, scale step, C entry points).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "site_rate_params.hpp"

namespace tphip {

constexpr int kEbMaxCat = 16;          // the mixture's limit (tphip_plan_desc.ncat)
constexpr int kEbReduceBlock = 256;    // threads of locus_marginal_reduce_kernel: part of the summation order

// Per column (or site pattern): the K-category mixture m = sum_k w_k L(mu rho_k) at the locus' scale mu.
struct PosteriorParams {
    SiteParams S;               // packed tip words, fused op stream, models, site chunk tables; S.work_cols / S.work_count
                                // (may be null: every column) list the columns to evaluate, per locus at locus_offsets[l]
    int32_t ncat;               // K, 2..kEbMaxCat
    const double* cat_rate;     // [nloci][K] rho_k
    const double* cat_logw;     // [nloci][K] log w_k
    const double* log_scale;    // [nloci] u = log mu
    const int32_t* done;        // [nloci] or null: loci whose fit has converged are skipped
    double* f;                  // [ncols] log m
    double* g;                  // [ncols] d log m / du
    double* h;                  // [ncols] d2 log m / du2
    double* mean;               // [ncols] posterior mean of rho
    double* second;             // [ncols] posterior second moment of rho
};

// The posterior-table variant stores, besides the moments, each category's f_k + log w_k.
struct PosteriorTableParams : PosteriorParams {
    double* logp;               // [K][ncols] category-major
};

// variant: 2 / 8 = packed words in registers, kStreamWords = streamed words (more than 64 tips)
hipError_t launch_site_posterior_kernel(int variant, int model, dim3 grid, size_t lds_bytes, hipStream_t st, const PosteriorParams& E);
hipError_t launch_site_posterior_table_kernel(int variant, int model, dim3 grid, size_t lds_bytes, hipStream_t st,
                                              const PosteriorTableParams& E);

}  // namespace tphip

// site_rate_launch.hip -- the translation unit of the site-rate kernels and of the empirical-Bayes mixture kernels
// (site_posterior_kernel.hpp: the same interpreter, instantiated as further eval_columns_kernel overloads).
//
// This file is one of the three units compiled with `-mllvm -structurizecfg-skip-uniform-regions` (see
// __graft_entry__.build): the op interpreter of site_rate_kernel branches on wave-uniform op codes, and structurizing
// those branches adds Flow blocks whose phis keep the 12-double accumulator alive on every path (8-36 v_mov_b64 per op,
// DESIGN section 8 r1 v7).  The option is off by default in LLVM's AMDGPU pipeline for a reason: in round 2 it
// miscompiled classify_kernel as soon as that kernel got a wave-uniform branch inside a divergent if / else (two stores
// tail-merged across the paths with the address register of one path holding the other path's temporary: found with
// rocgdb, precise-memory mode).  So only interpreter kernels are built with it (tools/flag_containment.py checks which); whatever
// changes in site_rate_kernel.hpp is covered by the GPU-vs-oracle parity tests, which exercise every op and scheduling mode of
// these kernels, and the mixture kernels by tests/test_gpu_eb.py up to 256 taxa (the streamed-words path).
#include <hip/hip_runtime.h>

#include "site_rate_kernel.hpp"
#include "site_posterior_kernel.hpp"

namespace tphip {

// MODEL is a template parameter of every variant: F81 plans run the closed-form instantiations (distinct kernel names).
template <int MODEL>
static hipError_t launch_site_rate_model(int variant, dim3 grid, size_t lds_bytes, hipStream_t st, const SiteParams& S) {
    const dim3 block(kSiteBlock);
    if (S.share_work) {   // shares by predicted work: the instantiations that walk the list through part_prefix / part_start
        if (variant == 2) site_rate_kernel<2, false, false, MODEL, true><<<grid, block, lds_bytes, st>>>(S);
        else if (variant == 8) site_rate_kernel<8, false, false, MODEL, true><<<grid, block, lds_bytes, st>>>(S);
        else if (variant == kStreamWords) site_rate_kernel<kStreamWords, false, false, MODEL, true><<<grid, block, lds_bytes, st>>>(S);
        else if (variant == kStreamWordsSpill) site_rate_kernel<kStreamWords, true, false, MODEL, true><<<grid, block, lds_bytes, st>>>(S);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (variant == 2) site_rate_kernel<2, false, false, MODEL><<<grid, block, lds_bytes, st>>>(S);
    else if (variant == 8) site_rate_kernel<8, false, false, MODEL><<<grid, block, lds_bytes, st>>>(S);
    else if (variant == kMixedVariant + 2) site_rate_kernel<2, false, true, MODEL><<<grid, block, lds_bytes, st>>>(S);
    else if (variant == kMixedVariant + 8) site_rate_kernel<8, false, true, MODEL><<<grid, block, lds_bytes, st>>>(S);
    else if (variant == kStreamWords) site_rate_kernel<kStreamWords, false, false, MODEL><<<grid, block, lds_bytes, st>>>(S);
    else if (variant == kStreamWordsSpill) site_rate_kernel<kStreamWords, true, false, MODEL><<<grid, block, lds_bytes, st>>>(S);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <int MODEL>
static hipError_t site_rate_occupancy_model(int variant, size_t lds_bytes, int* blocks_per_cu) {
    if (variant == 2) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, site_rate_kernel<2, false, false, MODEL>, kSiteBlock, lds_bytes);
    if (variant == 8) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, site_rate_kernel<8, false, false, MODEL>, kSiteBlock, lds_bytes);
    if (variant == kMixedVariant + 2) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, site_rate_kernel<2, false, true, MODEL>, kSiteBlock, lds_bytes);
    if (variant == kMixedVariant + 8) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, site_rate_kernel<8, false, true, MODEL>, kSiteBlock, lds_bytes);
    if (variant == kStreamWords)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, site_rate_kernel<kStreamWords, false, false, MODEL>, kSiteBlock, lds_bytes);
    if (variant == kStreamWordsSpill)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, site_rate_kernel<kStreamWords, true, false, MODEL>, kSiteBlock, lds_bytes);
    return hipErrorInvalidValue;
}

hipError_t launch_site_rate_kernel(int variant, int model, dim3 grid, size_t lds_bytes, hipStream_t st, const SiteParams& S) {
    if (model == TPHIP_MODEL_F81) return launch_site_rate_model<TPHIP_MODEL_F81>(variant, grid, lds_bytes, st, S);
    if (model == TPHIP_MODEL_GTR) return launch_site_rate_model<TPHIP_MODEL_GTR>(variant, grid, lds_bytes, st, S);
    return hipErrorInvalidValue;
}

hipError_t site_rate_kernel_occupancy(int variant, int model, size_t lds_bytes, int* blocks_per_cu) {
    if (model == TPHIP_MODEL_F81) return site_rate_occupancy_model<TPHIP_MODEL_F81>(variant, lds_bytes, blocks_per_cu);
    if (model == TPHIP_MODEL_GTR) return site_rate_occupancy_model<TPHIP_MODEL_GTR>(variant, lds_bytes, blocks_per_cu);
    return hipErrorInvalidValue;
}

hipError_t launch_eval_columns_kernel(int model, dim3 grid, size_t lds_bytes, hipStream_t st, const EvalParams& E) {
    if (model == TPHIP_MODEL_F81) {
        EvalParamsF81 F;
        static_cast<EvalParams&>(F) = E;
        eval_columns_kernel<<<grid, dim3(kSiteBlock), lds_bytes, st>>>(F);
    } else if (model == TPHIP_MODEL_GTR) eval_columns_kernel<<<grid, dim3(kSiteBlock), lds_bytes, st>>>(E);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// The empirical-Bayes mixture kernels (site_posterior_kernel.hpp): eval_columns_kernel overloads, one per (words, model).
template <int NW, int MODEL>
static hipError_t launch_posterior(dim3 grid, size_t lds_bytes, hipStream_t st, const PosteriorParams& E) {
    PosteriorArgs<NW, MODEL> A;
    static_cast<PosteriorParams&>(A) = E;
    eval_columns_kernel<<<grid, dim3(kSiteBlock), lds_bytes, st>>>(A);
    return hipGetLastError();
}

template <int MODEL>
static hipError_t launch_posterior_model(int variant, dim3 grid, size_t lds_bytes, hipStream_t st, const PosteriorParams& E) {
    if (variant == 2) return launch_posterior<2, MODEL>(grid, lds_bytes, st, E);
    if (variant == 8) return launch_posterior<8, MODEL>(grid, lds_bytes, st, E);
    if (variant == kStreamWords) return launch_posterior<kStreamWords, MODEL>(grid, lds_bytes, st, E);
    return hipErrorInvalidValue;
}

hipError_t launch_site_posterior_kernel(int variant, int model, dim3 grid, size_t lds_bytes, hipStream_t st, const PosteriorParams& E) {
    if (model == TPHIP_MODEL_F81) return launch_posterior_model<TPHIP_MODEL_F81>(variant, grid, lds_bytes, st, E);
    if (model == TPHIP_MODEL_GTR) return launch_posterior_model<TPHIP_MODEL_GTR>(variant, grid, lds_bytes, st, E);
    return hipErrorInvalidValue;
}

// The posterior-table variant of the mixture kernels: six more eval_columns_kernel overloads.
template <int NW, int MODEL>
static hipError_t launch_posterior_table(dim3 grid, size_t lds_bytes, hipStream_t st, const PosteriorTableParams& E) {
    PosteriorTableArgs<NW, MODEL> A;
    static_cast<PosteriorTableParams&>(A) = E;
    eval_columns_kernel<<<grid, dim3(kSiteBlock), lds_bytes, st>>>(A);
    return hipGetLastError();
}

template <int MODEL>
static hipError_t launch_posterior_table_model(int variant, dim3 grid, size_t lds_bytes, hipStream_t st, const PosteriorTableParams& E) {
    if (variant == 2) return launch_posterior_table<2, MODEL>(grid, lds_bytes, st, E);
    if (variant == 8) return launch_posterior_table<8, MODEL>(grid, lds_bytes, st, E);
    if (variant == kStreamWords) return launch_posterior_table<kStreamWords, MODEL>(grid, lds_bytes, st, E);
    return hipErrorInvalidValue;
}

hipError_t launch_site_posterior_table_kernel(int variant, int model, dim3 grid, size_t lds_bytes, hipStream_t st,
                                              const PosteriorTableParams& E) {
    if (model == TPHIP_MODEL_F81) return launch_posterior_table_model<TPHIP_MODEL_F81>(variant, grid, lds_bytes, st, E);
    if (model == TPHIP_MODEL_GTR) return launch_posterior_table_model<TPHIP_MODEL_GTR>(variant, grid, lds_bytes, st, E);
    return hipErrorInvalidValue;
}

hipError_t launch_scan_counts_kernel(hipStream_t st, const int32_t* count, int64_t nloci, int32_t chunk_cols, int64_t* prefix,
                                     int64_t* slice_prefix, const ScanClasses* C) {
    if (C) scan_classes_kernel<<<dim3(1), dim3(1024), 0, st>>>(count, nloci, chunk_cols, prefix, slice_prefix, *C);
    else scan_counts_kernel<<<dim3(1), dim3(1024), 0, st>>>(count, nloci, chunk_cols, prefix, slice_prefix);
    return hipGetLastError();
}

}  // namespace tphip

// band_driver_common.hpp -- the host side that the replicate-band drivers share: bootstrap_driver.hip,
// simulate_driver.hip (3.7) and posterior_pi_driver.hip (3.10).  Their options begin with the same four fields, they stage the
// generator's stream ids the same way, they cut the caller's workspace by the rules of band_blocks.hpp, and each ends in
// bootstrap_summary_kernel on its replicate rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "band_blocks.hpp"
#include "tphip_internal.hpp"

struct BandOpts { int32_t replicates = 0; double level = 0.0; uint64_t seed = 0; const int64_t* locus_ids = nullptr; };

// what a family accepts and how it refuses: the least struct_size, the struct_size from which locus_ids is read, its messages
struct BandOptsRules { size_t min_size, ids_size; const char *null_opts, *too_small, *replicates, *level; };

template <typename Abi>
int band_read_opts(const Abi* o, const BandOptsRules& R, BandOpts* out) {
    static_assert(offsetof(Abi, replicates) == offsetof(tphip_bootstrap_opts, replicates) &&
                      offsetof(Abi, level) == offsetof(tphip_bootstrap_opts, level) &&
                      offsetof(Abi, seed) == offsetof(tphip_bootstrap_opts, seed) &&
                      offsetof(Abi, locus_ids) == offsetof(tphip_bootstrap_opts, locus_ids),
                  "the band families' options share their first four fields");
    if (!o) return fail(TPHIP_ERR_INVALID, R.null_opts);
    if (o->struct_size < R.min_size) return fail(TPHIP_ERR_INVALID, R.too_small);
    out->replicates = o->replicates; out->level = o->level; out->seed = o->seed;
    out->locus_ids = o->struct_size >= R.ids_size ? o->locus_ids : nullptr;
    if (out->replicates < 2 || out->replicates > kBandMaxReplicates) return fail(TPHIP_ERR_INVALID, R.replicates);
    if (!(out->level > 0.0 && out->level < 1.0)) return fail(TPHIP_ERR_INVALID, R.level);
    return TPHIP_OK;
}
// an options struct through the end of its seed, and through its locus_ids
template <typename Abi> constexpr size_t band_seed_end() { return offsetof(Abi, seed) + sizeof(uint64_t); }
template <typename Abi> constexpr size_t band_ids_end() { return offsetof(Abi, locus_ids) + sizeof(const int64_t*); }

// stream ids to the device at dst (read now: the caller's array need not outlive the call, so the stream is synchronised
// once); *d_ids = null without ids
inline int band_stage_ids(int64_t* dst, const int64_t* host_ids, int64_t nloci, hipStream_t st, const int64_t** d_ids) {
    *d_ids = nullptr;
    if (!host_ids) return TPHIP_OK;
    HIP_TRY(hipMemcpyAsync(dst, host_ids, sizeof(int64_t) * (size_t)nloci, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    *d_ids = dst;
    return TPHIP_OK;
}

// the caller's workspace from its first aligned byte on
inline char* band_ws_base(void* ws, size_t ws_bytes, size_t* usable = nullptr) {
    const BandBase b = band_base((uintptr_t)ws, ws_bytes);
    if (usable) *usable = b.usable;
    return (char*)b.base;
}

// bootstrap_summary_kernel on [nloci][B][Wb] rows at coverage `level`, B and level already checked; in bootstrap_driver.hip,
// where the __global__ lives
__attribute__((visibility("hidden"))) int band_summarize(const double* d_rows, int64_t nloci, int32_t B, int32_t Wb, double level,
                                                         double* d_summary, hipStream_t st);

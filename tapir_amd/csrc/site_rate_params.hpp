// site_rate_params.hpp -- launch parameters and constants of the site-rate kernels, shared by the two translation
// units of libtphip.so: site_rate_launch.hip (compiles site_rate_kernel.hpp, the only code built with
// -structurizecfg-skip-uniform-regions) and site_driver.hip (the stage-2 launches, built without that flag, as everything else is);
// eb_driver.hip fills a SiteParams too (plan_site_params in tphip_internal.hpp is the common part).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gtr_model.hpp"
#include "launch_constants.hpp"   // kSiteBlock, the LDS headers, the launcher variants, ...
#include "tail_shares.hpp"
#include "tree_program.hpp"

namespace tphip {

constexpr double kUMin = -23.025850929940457;  // log(1e-10)
constexpr double kUMax = 9.210340371976184;    // log(1e4)
constexpr double kStepMax = 2.0;
constexpr double kStepTol = 3e-4;       // accept when the step is this small: applied with a third-order correction
constexpr double kHermiteSpan = 3e-4;   // ... while |step| * |distance between the two points| stays below this
constexpr double kHermiteTol = 2e-3;    // final step from the two-point quartic model of f' accepted below this size
                                        // (calibration of the two bounds: tools/debug/two_point_experiment.py)
constexpr double kHermiteT2D3 = 1.5e-8;  // step^2 * |distance of the far point|^3 below this (the quartic's error term)
constexpr double kHermiteGuard = 0.005;  // the quartic's higher-order terms at the step, relative to |h|
constexpr double kHermiteRegular = 0.25; // curvature |h| from which the two exits apply (below: iterate until the step is below 1e-6)
constexpr double kHermiteNoise = 5.3e-5; // 30 * (8 * 2.2e-16) / 1e-9: rounding of the two values vs curvature (site_rate_kernel.hpp)
constexpr double kHalleySpan = 1.0;      // the two curvatures behind the Halley step of a weakly curved point lie this close
constexpr double kStepTolFirst = 1e-6;  // ... except at the first evaluation (no second point yet)
constexpr int kMaxIt = 100;
constexpr double kFlatEps = 1e-10;  // |g| and |h| below this: log L flat to fp64 resolution -> saturated
// A maximum found at a large rate may be nothing but rounding noise on the plateau log L reaches as s -> infinity (where
// the flatness rule above fires, or not, depending on the last bits).  So an optimum at s >= kCheckRate is confirmed
// by value: if log L at the largest rate is not lower by more than kSatTol (relative), the column is saturated.
constexpr double kUCheck = 2.995732273553991;   // log(20)
constexpr double kSatTol = 1e-10;
constexpr double kPlateauStride = 0.5;
constexpr int kTailWindow = 2 * kSiteBlock;   // persistent mode: entries at the end of a segment that are put in slow-first order (SiteParams::tail_order)
#ifndef TPHIP_EXP_TABLE
#define TPHIP_EXP_TABLE 1
#endif
constexpr bool kUseExpTable = TPHIP_EXP_TABLE != 0;

struct SiteParams {
    const uint8_t* states;       // [ntaxa][ncols_total]
    int64_t ncols_total;
    const LocusModel* models;    // [nloci]
    const TreeOp* ops;
    int32_t nops;
    int32_t stack_depth;
    double chrono_length;
    const int64_t* locus_offsets;  // [nloci+1]
    const int32_t* chunk_locus;    // [nchunks]  work slices of chunk_cols columns, never straddling loci
    const int32_t* chunk_index;    // [nchunks]  index of the slice inside its locus
    int32_t chunk_cols;            // target columns per slice
    const uint32_t* packed;        // [nwords][ncols_total] 8 tip masks per word, tips in program order (classify_kernel)
    int32_t nwords;                // ceil(ntips / 8)
    const int32_t* work_cols;      // [ncols_total] compacted column ids, per locus at locus_offsets[l]
    int32_t* work_cols2;           // [ncols_total] scratch of the same shape, or null: in the small-batch mode every wave
                                   // rewrites its slice of the list there with the columns predicted to be slow first
    const int32_t* work_count;     // [nloci]
    const int64_t* work_prefix;    // [nloci+1] exclusive scan of work_count (scan_counts_kernel)
    const int64_t* slice_prefix;   // [nloci+1] exclusive scan of the per-locus slice counts (non-persistent mode)
    int64_t nloci;
    int32_t persistent;            // 1: grid = resident waves (x grid multiplier), shares of the global work list; 0: grid = slices
                                   // (the mixed-loci variants are launched with 1 and equal shares)
    int32_t first_round;           // persistent: the first `first_round` workgroups (one per resident wave) share
    double first_fraction;         //   this fraction of the work equally, the others the rest (see site_rate_kernel)
    int32_t tail_order = 0;        // persistent, one locus at a time: before a wave starts a segment of its share it moves the
                                   //   columns classify_kernel marked as slow to the front of the segment's last kTailWindow entries
    int32_t share_work = 0;        // persistent, one locus at a time: shares by predicted work.  compact_kernel put a fixed fraction of
                                   //   every locus' easy (unmarked) columns into a reserved tail of the locus' part of the list; the
                                   //   first `main_shares` workgroups cut the main parts into equal predicted work (work_wprefix), the
                                   //   others cut the reserved tails in whole lane-fills (tail_shares, below) or into equal column
                                   //   counts.  0: shares as above
    int32_t main_shares = 0;
    const int64_t* work_wprefix = nullptr;   // [nloci+1] exclusive scan of the main parts' predicted work (scan_classes_kernel)
    const int64_t* part_prefix = nullptr;    // [nloci+1][2] exclusive scans of the column counts of the main parts / the reserved tails
    const int64_t* part_start = nullptr;     // [nloci][2] where the locus' main part / reserved tail begins in work_cols
                                             //   (both written by scan_classes_kernel, read by the WORK instantiations only)
    int32_t mixed_few_waves;       // mixed-loci mode: with fewer than mixed_switch_cols columns on the work list only this many
    int64_t mixed_switch_cols;     //   workgroups take shares (one wave per SIMD), the others leave at once
    int32_t ncat;                  // > 1: discrete rate mixture on top of the site rate (tphip_plan_desc.ncat)
    const double* cat;             // [2 * ncat]: category rate multipliers, then log weights
    double* rate;
    double* subst;
    double* lnl;
    uint8_t* flag;
    unsigned long long* eval_counter;
    double* spill;                 // SPILL variant: [grid waves][stack_depth - lds_depth][12][64] parked partials beyond the LDS stack
    int32_t lds_depth;             // parked partials kept in LDS (= stack_depth unless the SPILL variant runs)
    TailShares tail_shares;        // share_work: the later shares' cut of the reserved tails (tail_shares.hpp); fills_big = 0: equal
                                   //   column counts over the gridDim.x - main_shares later workgroups.  (Last: the WORK
                                   //   instantiations alone read it, and the other fields keep their places.)
};

// Slices a locus with `count` optimiser columns is cut into in the non-persistent mode: about chunk_cols each.
__host__ __device__ __forceinline__ int site_slices(int count, int chunk_cols) {
    if (count <= 0) return 0;
    const int ns = (count + chunk_cols / 2) / chunk_cols;
    return ns < 1 ? 1 : ns;
}

// Of the first r easy columns of a locus (in list order), how many go to the locus' reserved tail: the column of rank r
// is reserved when this count steps from r to r + 1.  The rule sees the locus' own columns only, so which columns are
// reserved does not depend on the other loci of the batch (or on how a batch is sharded).
__host__ __device__ __forceinline__ int32_t reserved_before(int64_t r, int32_t reserve_q) {
    return (int32_t)((r * (int64_t)reserve_q) >> kReserveShift);
}


// Diagnostic launch: evaluate f = log L, g = df/du, h = d2f/du2 at a caller-chosen u for EVERY column.
struct EvalParams {
    SiteParams S;
    const double* u;
    double* f;
    double* g;
    double* h;
};

// ---- launchers defined in site_rate_launch.hip ------------------------------------------------------------------
// variant: 2 / 8 = packed words in registers, kStreamWords = streamed words (> 64 tips),
// kStreamWordsSpill = the same with the deepest parked partials in global scratch (S.spill, S.lds_depth);
// model: TPHIP_MODEL_GTR (eigen-system messages) or TPHIP_MODEL_F81 (closed-form messages)
hipError_t launch_site_rate_kernel(int variant, int model, dim3 grid, size_t lds_bytes, hipStream_t st, const SiteParams& S);
hipError_t site_rate_kernel_occupancy(int variant, int model, size_t lds_bytes, int* blocks_per_cu);
hipError_t launch_eval_columns_kernel(int model, dim3 grid, size_t lds_bytes, hipStream_t st, const EvalParams& E);
// scan_classes_kernel's view of the classes: cls [nloci][2] = slow / easy work-list columns per locus (compact_classes_kernel)
struct ScanClasses {
    const int32_t* cls = nullptr;
    const int64_t* locus_offsets = nullptr;
    int32_t reserve_q = 0, w_slow = 0, w_easy = 0;
    int64_t* wprefix = nullptr;       // SiteParams::work_wprefix
    int64_t* part_prefix = nullptr;   // SiteParams::part_prefix
    int64_t* part_start = nullptr;    // SiteParams::part_start
};
hipError_t launch_scan_counts_kernel(hipStream_t st, const int32_t* count, int64_t nloci, int32_t chunk_cols, int64_t* prefix,
                                     int64_t* slice_prefix, const ScanClasses* C);   // C null: the two plain scans

}  // namespace tphip

// site_launch_plan.hpp -- how the site-rate stage of a plan will run, decided on the host from a handful of numbers: the
// batch shape, the tree's word count and stack depth, the CU count, two or three occupancy figures and the tuning knobs.
// Plain integer and floating-point arithmetic with no HIP header: tphip.hip calls it from tphip_plan_create, site_driver.hip
// takes every launch's arguments from it, and tests/native/site_launch_dump.cpp compiles it with g++ so that every decision
// is checked without a GPU (tests/test_site_launch.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <utility>
#include <vector>

#include "launch_constants.hpp"
#include "tail_shares.hpp"
#include "tphip.h"

namespace tphip {

// LDS of one site-rate workgroup that keeps `depth` parked partials there: one locus at a time / the mixed-loci mode
inline size_t site_lds_bytes(int depth) { return (kSiteLdsHeader + (size_t)depth * 12 * kSiteBlock) * sizeof(double); }
inline size_t mixed_lds_bytes(int depth) { return (kMixedLdsHeader + (size_t)depth * 12 * kSiteBlock) * sizeof(double); }

// The tuning, A/B and test knobs of plan creation; an empty optional = not set.  Switches keep the first character of
// their text (each has its own reading of it, below), numbers what atol / atof / atoi made of it.
struct PlanKnobs {
    std::optional<long> site_chunk, site_waves, site_grid_mult;
    std::optional<char> site_spill, site_persistent, site_mixed, site_tail_order, site_share_work, compact_chunked, pi_split, dedup;
    std::optional<double> site_first_fraction, site_reserve;
    std::optional<std::pair<double, double>> site_class_weights;   // "slow,easy"; text that does not parse = not set
    // "big,mid,small[,frac_big,frac_mid]": lane-fills per later share in the three bands of the reserved tails and the fractions
    // of the tails that the first two bands take (tail_shares.hpp); "0" = later shares of equal column counts; text that
    // holds neither = not set
    struct TailSharesKnob { int big = 0, mid = 0, small = 0; double frac_big = -1.0, frac_mid = -1.0; };
    std::optional<TailSharesKnob> site_tail_shares;
    std::optional<int> host_split;
    // stage 1 (locus_launch_plan.hpp): columns per thread of locus_value_kernel, 1 or 2 (text below 2 = 1); the eigenbasis value
    // kernel instead of it whenever the variable is set, whatever its text
    std::optional<int> value_cols;
    bool value_eigenbasis = false;
};

constexpr const char* kPlanKnobNames[] = {
    "TPHIP_SITE_CHUNK", "TPHIP_SITE_SPILL", "TPHIP_SITE_PERSISTENT", "TPHIP_SITE_MIXED", "TPHIP_SITE_WAVES",
    "TPHIP_SITE_FIRST_FRACTION", "TPHIP_SITE_GRID_MULT", "TPHIP_SITE_TAIL_ORDER", "TPHIP_SITE_SHARE_WORK", "TPHIP_SITE_RESERVE",
    "TPHIP_SITE_CLASS_WEIGHTS", "TPHIP_SITE_TAIL_SHARES", "TPHIP_COMPACT_CHUNKED", "TPHIP_PI_SPLIT", "TPHIP_DEDUP", "TPHIP_HOST_SPLIT",
    "TPHIP_VALUE_COLS", "TPHIP_VALUE_EIGENBASIS"};

// One knob from its text (an environment variable's value).  False: no knob of that name.
inline bool set_plan_knob(PlanKnobs* k, const char* name, const char* text) {
    const auto is = [name](const char* n) { return strcmp(name, n) == 0; };
    if (is("TPHIP_SITE_CHUNK")) k->site_chunk = atol(text);
    else if (is("TPHIP_SITE_SPILL")) k->site_spill = text[0];
    else if (is("TPHIP_SITE_PERSISTENT")) k->site_persistent = text[0];
    else if (is("TPHIP_SITE_MIXED")) k->site_mixed = text[0];
    else if (is("TPHIP_SITE_WAVES")) k->site_waves = atol(text);
    else if (is("TPHIP_SITE_FIRST_FRACTION")) k->site_first_fraction = atof(text);
    else if (is("TPHIP_SITE_GRID_MULT")) k->site_grid_mult = atol(text);
    else if (is("TPHIP_SITE_TAIL_ORDER")) k->site_tail_order = text[0];
    else if (is("TPHIP_SITE_SHARE_WORK")) k->site_share_work = text[0];
    else if (is("TPHIP_SITE_RESERVE")) k->site_reserve = atof(text);
    else if (is("TPHIP_SITE_CLASS_WEIGHTS")) {
        double a = 0, b = 0;
        if (sscanf(text, "%lf,%lf", &a, &b) == 2) k->site_class_weights = std::make_pair(a, b);
    }
    else if (is("TPHIP_SITE_TAIL_SHARES")) {
        PlanKnobs::TailSharesKnob t;
        const int n = sscanf(text, "%d,%d,%d,%lf,%lf", &t.big, &t.mid, &t.small, &t.frac_big, &t.frac_mid);
        if (n == 1 && t.big == 0) k->site_tail_shares = PlanKnobs::TailSharesKnob();
        else if (n == 3 || n == 5) k->site_tail_shares = t;
    }
    else if (is("TPHIP_COMPACT_CHUNKED")) k->compact_chunked = text[0];
    else if (is("TPHIP_PI_SPLIT")) k->pi_split = text[0];
    else if (is("TPHIP_DEDUP")) k->dedup = text[0];
    else if (is("TPHIP_HOST_SPLIT")) k->host_split = atoi(text);
    else if (is("TPHIP_VALUE_COLS")) k->value_cols = atoi(text) >= 2 ? 2 : 1;
    else if (is("TPHIP_VALUE_EIGENBASIS")) k->value_eigenbasis = true;
    else return false;
    return true;
}

// What the decision sees of a batch and its tree.
struct SiteShape {
    int64_t ncols = 0, nloci = 0, max_locus_cols = 0;
    int32_t ntaxa = 0;
    int32_t nwords = 0;         // packed tip words per column: ceil(tips / 8)
    int32_t stack_depth = 0;    // TreeProgram::stack_depth
    int32_t model = 0;          // TPHIP_MODEL_*
    int32_t ncat = 0;           // rate categories (tphip_plan_desc.ncat)
    int32_t start_rule = 0;     // TPHIP_START_*, as in the descriptor
    int32_t pattern_dedup = 0;  // TPHIP_DEDUP_*, as in the descriptor
    int32_t T = 0, n_i = 0;
};

// How launch_site_rates (site_driver.hip) runs a plan's site-rate stage.
struct SiteLaunch {
    int32_t start_rule = 0;   // TPHIP_START_PARSIMONY or _REFERENCE (AUTO resolved)
    int32_t dedup_mode = 0;   // DEDUP_* (launch_constants.hpp)
    int32_t chunk_cols = kSiteBlock;  // columns per site_rate_kernel work slice (multiple of 64)
    int32_t waves = 0;        // persistent grid of site_rate_kernel = resident waves on the device
    int32_t persistent = 1;
    int32_t mixed_few_waves = 0;   // mixed-loci mode: workgroups that take shares when the work list is short (SiteParams)
    int64_t mixed_switch_cols = 0;
    int32_t mixed = 0;        // small batches: waves carry columns of several loci (site_rate_kernel<NW, false, true>)
    int32_t grid_mult = 1;    // persistent grid = resident waves x this
    int32_t lds_depth = 0;    // parked partials kept in LDS by site_rate_kernel (< stack depth: SPILL variant)
    double first_fraction = 0.0;   // share of the work the first round of shares takes (0 = equal shares)
    int32_t tail_order = 1;   // persistent mode: slow columns first in the last 128 entries of every segment (SiteParams::tail_order)
    // persistent mode, one locus at a time: shares by predicted work (SiteParams::share_work).  reserve_q / 2^16 of every locus'
    // easy columns go to a reserved tail that the later, small shares cut into equal column counts; the first round's shares
    // cut the rest into equal predicted work, a slow column weighing w_slow / 2^10 evaluations and an easy one w_easy / 2^10
    int32_t share_work = 0, reserve_q = 0, w_slow = 0, w_easy = 0;
    // how the later shares cut the reserved tails (tail_shares.hpp; fills_big = 0: into equal column counts) and how many of
    // them the longest tails this shape can have would need
    TailShares tail_shares;
    int64_t tail_share_bound = 0;
    int32_t compact_chunked = 0;   // long loci: the work list by the chunk-parallel count / scan / scatter kernels (pi_kernels.hpp)
    int32_t pi_split = 0;          // long loci: the PI partial sums by pi_net_kernel + pi_interval_kernel instead of pi_partial_kernel
};

// Workgroups of the site-rate launch.  Later shares in whole lane-fills: the resident waves and every later share that the
// longest possible tails need.  decide_site_launch sizes the shares to fit waves x grid_mult; only shares spelled out by the
// knob make the grid larger.  The workgroups that the real tails leave without a share are the last of the grid.
inline int64_t site_grid(const SiteLaunch& s, int64_t n_site_chunks) {
    if (s.mixed) return s.waves;
    if (!s.persistent) return n_site_chunks;
    return std::max((int64_t)s.waves * s.grid_mult, s.waves + s.tail_share_bound);
}

// The launcher variant by the tree's packed tip words alone: the words in registers (<= 16 / <= 64 tips) or streamed one word
// ahead (more than 64 tips).  The spill and the mixed-loci variants build on it (site_kernel_args).
inline int site_variant(int32_t nwords) { return nwords <= 2 ? 2 : nwords <= 8 ? 8 : kStreamWords; }

// What a site_rate_kernel launch takes from the plan's SiteLaunch besides pointers: the launcher's arguments and the
// scheduling members of SiteParams (launch_site_rates in site_driver.hip).
struct SiteKernelArgs {
    int variant = 0;          // launch_site_rate_kernel's: site_variant, the spill variant of the streamed words, or kMixedVariant +
    size_t lds_bytes = 0;
    int64_t grid = 0;
    int32_t persistent = 0, first_round = 0, tail_order = 0, share_work = 0, main_shares = 0;   // SiteParams members of these names
    double first_fraction = 1.0;
    bool spill = false;        // the deepest parked partials go to the workspace's scratch rows (SiteParams::spill)
    bool second_list = false;  // the kernel gets the second work list (SiteParams::work_cols2): the layout has it whenever !persistent
};

inline SiteKernelArgs site_kernel_args(const SiteLaunch& s, int32_t nwords, int32_t stack_depth, int64_t n_site_chunks) {
    SiteKernelArgs a;
    a.spill = s.lds_depth < stack_depth;
    a.second_list = !s.persistent;
    a.persistent = (s.persistent || s.mixed) ? 1 : 0;   // the mixed-loci variants are launched as persistent, with equal shares
    a.first_round = s.waves;
    a.tail_order = (s.persistent && !s.mixed && s.tail_order) ? 1 : 0;
    a.first_fraction = (s.first_fraction > 0.0) ? s.first_fraction : 1.0 / (double)s.grid_mult;
    a.share_work = s.share_work;
    a.main_shares = (s.reserve_q > 0) ? s.waves : s.waves * s.grid_mult;
    a.grid = site_grid(s, n_site_chunks);
    a.variant = (a.spill && nwords > 8) ? kStreamWordsSpill : site_variant(nwords);
    a.lds_bytes = site_lds_bytes(s.lds_depth);   // (lds_depth = the stack depth unless the spill variant runs)
    if (s.mixed) {   // equal shares: first_round = grid
        a.first_fraction = 1.0;
        a.variant += kMixedVariant;
        a.lds_bytes = mixed_lds_bytes(stack_depth);
    }
    return a;
}

// Target slice length of the non-persistent mode (small batches) and of the eval diagnostic: needs no device, and the
// chunk tables want it before anything else is decided.
inline int32_t site_chunk_cols(const PlanKnobs& knobs) {
    int64_t cc = 512;
    if (knobs.site_chunk && *knobs.site_chunk >= kSiteBlock) cc = *knobs.site_chunk;   // tuning knob for experiments
    return (int32_t)cc;
}

// `occupancy(variant, lds_bytes)`: resident workgroups per CU of that site_rate_kernel variant (for shape.model), 0 when the
// query failed.  Asked for the base variant always, for the spill and the mixed variant only where they are candidates.
template <typename Occupancy>
SiteLaunch decide_site_launch(const SiteShape& shape, int num_cus, const PlanKnobs& knobs, Occupancy&& occupancy) {
    SiteLaunch s;
    const int64_t ncols = shape.ncols;
    const int nwords = shape.nwords, stack_depth = shape.stack_depth;
    // TPHIP_START_AUTO: HyPhy's own start where the parsimony start was ever seen to end on another local optimum (small trees)
    // (the rate mixture is an extension without a HyPhy counterpart to start like: it keeps the parsimony start)
    s.start_rule = shape.start_rule == TPHIP_START_AUTO
                       ? ((shape.ntaxa >= kFirstStepMinTaxa || shape.ncat > 1) ? TPHIP_START_PARSIMONY : TPHIP_START_REFERENCE)
                       : shape.start_rule;
    s.chunk_cols = site_chunk_cols(knobs);
    // persistent grid: exactly the waves the device keeps resident for this LDS footprint
    int per_cu = occupancy(site_variant(nwords), site_lds_bytes(stack_depth));
    if (per_cu < 1) per_cu = 1;
    s.waves = per_cu * num_cus;
    // Deep trees (256 taxa: 4 parked partials = 24 KB per wave) are capped at 6 waves per CU by the LDS stack, not by
    // the registers.  The deepest slots are the least used (C5 tree: 9 of 80 pushes per evaluation reach the fourth),
    // so the streamed-words kernel has a variant that parks them in a global scratch row of the wave instead: with
    // three slots in LDS (19.7 KB) eight waves fit.  Only worth it for the persistent grid (one scratch row per wave).
    s.lds_depth = stack_depth;
    {
        const int keep = (int)((160 * 1024 / 8 - kSiteLdsHeader * sizeof(double)) / (12 * kSiteBlock * sizeof(double)));   // = 3
        bool want = nwords > 8 && stack_depth > keep && per_cu < 8;
        if (knobs.site_spill) want = (*knobs.site_spill == '1') && nwords > 8 && stack_depth > 1;
        if (want) {
            const int depth = std::max(1, std::min(keep, stack_depth - 1));
            const int per2 = occupancy(kStreamWordsSpill, site_lds_bytes(depth));
            if (per2 > per_cu && ncols / ((int64_t)per2 * num_cus) >= 1000) {   // persistent mode will be chosen below
                s.lds_depth = depth;
                s.waves = per2 * num_cus;
            }
        }
    }
    // Small batches (an equal share would be under ~1000 columns) leave the persistent grid: the mixed-loci mode below,
    // or one workgroup per locus-aligned slice (cutting a small locus in two doubles its prologue and drain: measured on C2).
    s.persistent = (ncols / s.waves >= 1000) ? 1 : 0;
    if (knobs.site_persistent) s.persistent = (*knobs.site_persistent == '1');
    if (!s.persistent && s.lds_depth < stack_depth) {   // the scratch rows are per persistent wave
        s.lds_depth = stack_depth;
        s.waves = per_cu * num_cus;
    }
    // Small batches of trees up to 64 taxa: equal shares of the work list, a wave carrying columns of several loci at
    // once (site_rate_kernel<NW, false, true>); the slice mode remains for the streamed words.
    const bool mixed_fits = nwords <= 8 && ncols < ((int64_t)1 << kMixedColBits);
    s.mixed = (!s.persistent && mixed_fits) ? 1 : 0;
    if (knobs.site_mixed) s.mixed = (*knobs.site_mixed == '1') && mixed_fits;   // set to either value, it also switches the est_rounds rule off
    if (s.mixed) {
        int per3 = 0;
        const size_t lds3 = mixed_lds_bytes(stack_depth);
        const int64_t simds = 4 * (int64_t)num_cus;
        const double est_rounds = (double)ncols * (s.start_rule == TPHIP_START_REFERENCE ? 2.2 : 1.4) / (double)(kSiteBlock * simds);
        if (lds3 > 160 * 1024 || (per3 = occupancy(kMixedVariant + site_variant(nwords), lds3)) < 1) s.mixed = 0;
        // a batch that wants two waves per SIMD on a tree whose tables leave room for six per CU (64 taxa: 23.3 KB of LDS
        // per wave) stays with the slices: 1900 loci x 1000 x 64, 3.36 ms in slices, 4.10 with 1024 mixed waves
        else if (est_rounds >= 28.0 && per3 < 8 && !knobs.site_mixed) s.mixed = 0;
        else {
            s.persistent = 0;
            // One wave per SIMD or two?  A second wave on a SIMD adds half again to its throughput (C2: 15.2 us per round of
            // evaluations alone, 19.8 us each for two) but lengthens every round of the wave that carries the slowest column
            // (22 evaluations on C2 when the average column takes 3.7), and the launch ends with that wave.  Measured, one
            // per SIMD / two: C2 (17 rounds of evaluations per SIMD) 0.348 / 0.391 ms, two C2s (34 rounds) 0.789 / 0.508,
            // 300 loci x 1000 x 64 (8 rounds) 0.757 / 0.932, the resampled 5-taxon locus of bench.py --workload R1 (18 rounds;
            // 1.5 after de-duplication) 0.150 / 0.165 and 0.099 / 0.138; 1152 waves on C2 0.422 (SIMDs shared unevenly).
            // The grid is two per SIMD where eight waves fit a CU (64-taxon trees hold six: one per SIMD, and the batches
            // that want two stay with the slices, above); the kernel uses half of it when the work list -- known on the
            // device only, after classification and de-duplication -- is shorter than ~24 rounds per SIMD at 3.7
            // evaluations per column from HyPhy's start value, 2.4 from the parsimony start.
            const int64_t want = (per3 < 8) ? std::min<int64_t>(simds, (int64_t)per3 * num_cus) : 8 * (int64_t)num_cus;
            s.mixed_few_waves = (int32_t)std::min<int64_t>(simds, want);
            s.mixed_switch_cols = (int64_t)(24.0 * (double)(kSiteBlock * simds) / (s.start_rule == TPHIP_START_REFERENCE ? 3.7 : 2.4));
            s.waves = (int32_t)std::max<int64_t>(1, std::min<int64_t>(want, (ncols + kSiteBlock - 1) / kSiteBlock));
        }
    }
    if (knobs.site_waves && *knobs.site_waves >= 1) { s.waves = (int32_t)*knobs.site_waves; s.mixed_switch_cols = 0; }  // tuning knob
    // Share sizes of the persistent grid.  Equal shares (one per resident wave) are equal column counts, not equal
    // work: loci differ in evaluations per column, and with 5-7 resident waves per CU (deep LDS stacks) a wave that
    // shares its SIMD runs slower than one that does not.  So the resident waves' first shares take 80-90 % of the
    // batch and the rest is cut into twice as many small shares that the dispatcher hands to whichever waves
    // finish first: site_rate_kernel C3 8.4 -> 7.0 ms, C4 share 9.8 -> 9.2, C5 share 20.9 -> 17.1.  Batches whose
    // shares are short anyway only gain drains (2.2 M columns in 2200 loci: +3.5 %): they keep equal shares.
    {
        const int64_t share = ncols / std::max(1, s.waves);
        const bool uneven = s.persistent && share >= 1500;
        s.grid_mult = uneven ? 3 : 1;
        // a share that spans several short loci pays a drain at every locus boundary, so its tail shares should be
        // fewer columns: 90 % up front there (C4: 9.0 vs 9.2-9.3 ms), 80 % when shares lie inside long loci (C3: 6.9 vs 7.0)
        const int64_t avg_locus = ncols / std::max<int64_t>(1, shape.nloci);
        s.first_fraction = !uneven ? 0.0 : (share >= 2 * avg_locus ? 0.9 : 0.8);
        // whole C5 with the spilled stack slot (8 waves per CU): (3, 0.8) 109.6 ms, (3, 0.9) 113.3, (4, 0.85) 109.1, (2, 0.8) 117.1
        if (uneven && s.lds_depth < stack_depth) s.first_fraction = 0.8;
        if (knobs.site_first_fraction) s.first_fraction = *knobs.site_first_fraction;
        if (knobs.site_grid_mult && *knobs.site_grid_mult >= 1 && *knobs.site_grid_mult <= 16) s.grid_mult = (int32_t)*knobs.site_grid_mult;
        // A/B and test switch: 0 = the persistent shares hand their segments out in list order, as the other modes do
        if (knobs.site_tail_order) s.tail_order = (*knobs.site_tail_order != '0');
        // Shares by predicted work (site_rate_kernel.hpp; persistent mode with one locus at a time only): the weights are the
        // mean evaluations of a marked and of an unmarked column.  TPHIP_SITE_SHARE_WORK=0 is the A/B
        // and test switch back to shares of equal column counts and a list without reserved tails.
        // On where the first-round shares lie inside long loci (C3: a locus holds ~20 of them, its reserved tail thousands
        // of columns); where a share spans several short loci the tail of a locus is a segment of a lane-fill or two with
        // a drain of its own, and the old hand-out is faster (whole C4 +6.5 %, whole C5 +2-5 %: DESIGN section 8, r10).
        double reserve = kDefaultReserve, w_slow = 2.9, w_easy = 2.04;
        s.share_work = (uneven && share < 2 * avg_locus) ? 1 : 0;
        if (knobs.site_share_work) s.share_work = (*knobs.site_share_work != '0');
        if (knobs.site_reserve) reserve = *knobs.site_reserve;
        if (knobs.site_class_weights) {
            const double a = knobs.site_class_weights->first, b = knobs.site_class_weights->second;
            if (a > 0 && b > 0 && a <= 16 && b <= 16) { w_slow = a; w_easy = b; }
        }
        // the interpolation inside a locus multiplies its predicted work by its column count in 64 bits
        if (!s.persistent || s.mixed || shape.max_locus_cols > ((int64_t)1 << 24)) s.share_work = 0;
        s.w_slow = std::max<int32_t>(1, (int32_t)lround(w_slow * (1 << kShareWeightShift)));
        s.w_easy = std::max<int32_t>(1, (int32_t)lround(w_easy * (1 << kShareWeightShift)));
        // without later shares there is nobody to take a reserved tail
        reserve = (s.share_work && s.grid_mult > 1) ? std::min(std::max(reserve, 0.0), 1.0) : 0.0;
        s.reserve_q = (int32_t)lround(reserve * (1 << kReserveShift));
        // The later shares cut the concatenated tails in whole lane-fills, long shares first (tail_shares.hpp; DESIGN section
        // 3.1): a share of n fills of easy columns issues about 2 n + 1 rounds, and a share that ends inside a fill pays for the
        // whole fill.  The tails cannot be longer than the reserved fraction of all columns; when the shares below would
        // not fit the grid for that length, all three grow by the same factor.  Batches that take later shares by the
        // knobs alone (shares under 1500 columns: the tails are a few fills altogether) keep the equal column counts, as
        // TPHIP_SITE_TAIL_SHARES=0 does everywhere; shares spelled out by the knob apply to tails of any length.
        if (s.reserve_q > 0) {
            const int64_t tails_max = (ncols * (int64_t)s.reserve_q) >> kReserveShift;
            const int64_t room = (int64_t)s.waves * (s.grid_mult - 1);
            const auto set = [&s](int big, int mid, int small, double fb, double fm) {
                TailShares& t = s.tail_shares;
                t.fills_small = std::max(1, std::min(small, 1 << 20));
                t.fills_mid = std::max(t.fills_small, std::min(mid, 1 << 20));
                t.fills_big = std::max(t.fills_mid, std::min(big, 1 << 20));
                fb = std::min(std::max(fb, 0.0), 1.0);
                fm = std::min(std::max(fm, 0.0), 1.0 - fb);
                t.frac_big_q = (int32_t)lround(fb * (1 << kReserveShift));
                t.frac_mid_q = std::min((int32_t)lround(fm * (1 << kReserveShift)), (1 << kReserveShift) - t.frac_big_q);
            };
            if (knobs.site_tail_shares) {
                const PlanKnobs::TailSharesKnob& k = *knobs.site_tail_shares;
                if (k.big > 0) set(k.big, k.mid, k.small, k.frac_big >= 0 ? k.frac_big : kTailFracBig, k.frac_mid >= 0 ? k.frac_mid : kTailFracMid);
            } else if (uneven) {
                for (int scale = 1;; ++scale) {
                    set(kTailFillsBig * scale, kTailFillsMid * scale, kTailFillsSmall * scale, kTailFracBig, kTailFracMid);
                    if (tail_share_bound(tails_max, s.tail_shares) <= room || scale >= (1 << 16)) break;
                }
                // real tails of less than a fill per later workgroup (R1: 57 site patterns per locus of 2048 columns, a tail
                // of 7 columns) stay with the equal column counts: tail_shares.hpp
                s.tail_shares.min_total = (int32_t)std::min<int64_t>(room * kSiteBlock, INT32_MAX);
            }
            if (s.tail_shares.fills_big > 0) s.tail_share_bound = tail_share_bound(tails_max, s.tail_shares);
        }
    }
    // Long loci build the work list chunk-parallel (compact_count / scan / scatter kernels); TPHIP_COMPACT_CHUNKED=0/1 is the
    // A/B and test switch that forces either path on any shape.
    s.compact_chunked = shape.max_locus_cols > 2048 ? 1 : 0;
    if (knobs.compact_chunked) s.compact_chunked = (*knobs.compact_chunked != '0');
    // Long loci take the PI partial sums in two kernels, the net-PI time tiles and the interval integrals (pi_kernels.hpp): each
    // at its own register count, for a second pass over the rates and the cull.  That pass costs short loci more than the split
    // gives them (C2 +6 us, R1 +24 us: DESIGN section 8, r12), so the switch is the chunked compaction's.  The sums are the
    // same to the bit either way; TPHIP_PI_SPLIT=0/1 is the A/B and test switch that forces either path on any shape.
    s.pi_split = shape.max_locus_cols > 2048 ? 1 : 0;
    if (knobs.pi_split) s.pi_split = (*knobs.pi_split != '0');
    s.dedup_mode = shape.pattern_dedup;
    if (knobs.dedup)   // test/tuning knob: 0 = never, 1 = always, anything else = automatic
        s.dedup_mode = (*knobs.dedup == '0') ? DEDUP_OFF : (*knobs.dedup == '1') ? DEDUP_ON : DEDUP_AUTO;
    if (s.dedup_mode == DEDUP_AUTO && ncols < kDedupAutoMinColumns) s.dedup_mode = DEDUP_OFF;   // small batch: see launch_constants.hpp
    return s;
}

// Locus groups of a host-pointer run on a big batch (host_run in tphip.hip).
// measured (C3 / C4, pinned buffers): 1 group 16.5 / 151 ms, 2: 12.8 / 127, 3: 17.3 / 154, 4: 14.9 / 140, 6: 15.2 / 135
inline int32_t host_split_groups(const PlanKnobs& knobs) {
    return knobs.host_split ? std::max(1, std::min(64, *knobs.host_split)) : 2;
}

// Chunk tables: work slices for the optimiser, 1024-column chunks for classification and PI; neither straddles a locus.
// A slice is what one wave works through with lane refill: long enough to amortise the drain at its end,
// short enough that the batch still makes >= ~8192 waves (32 per CU).
struct ChunkTables {
    std::vector<int32_t> site_chunk_locus, site_chunk_index, pi_chunk_locus, pi_chunk_index;
    std::vector<int64_t> locus_pichunk_offsets;   // [nloci + 1] first PI chunk of every locus
};

inline ChunkTables build_chunk_tables(const int64_t* locus_offsets, int64_t nloci, int32_t chunk_cols) {
    ChunkTables t;
    t.locus_pichunk_offsets.assign((size_t)nloci + 1, 0);
    for (int64_t l = 0; l < nloci; ++l) {
        const int64_t S = locus_offsets[l + 1] - locus_offsets[l];
        const int64_t ns_max = std::max<int64_t>(1, (S + chunk_cols / 2) / chunk_cols);
        for (int64_t c = 0; c < ns_max && S > 0; ++c) { t.site_chunk_locus.push_back((int32_t)l); t.site_chunk_index.push_back((int32_t)c); }
        for (int64_t c = 0; c * kPiChunk < S; ++c) { t.pi_chunk_locus.push_back((int32_t)l); t.pi_chunk_index.push_back((int32_t)c); }
        t.locus_pichunk_offsets[l + 1] = (int64_t)t.pi_chunk_locus.size();
    }
    return t;
}

// Byte offsets of the regions of the caller's workspace, each aligned to 256; a region the plan does not use keeps offset 0
// (launch_site_rates tests work_cols2 for that).  `total` is what tphip_plan_workspace_bytes promises.
struct WorkspaceLayout {
    size_t work_cols = 0, work_cols2 = 0, work_count = 0, work_prefix = 0, slice_prefix = 0;
    size_t work_class = 0, work_wprefix = 0, part_prefix = 0, part_start = 0;   // shares by predicted work
    size_t chunk_cnt = 0;                                                       // chunk-parallel compaction
    size_t partial = 0, packed = 0;
    size_t hash = 0, dup_of = 0, tab_key = 0, tab_val = 0, dedup_on = 0;        // site-pattern de-duplication
    size_t spill = 0;
    size_t total = 0;
};

inline WorkspaceLayout layout_workspace(const SiteShape& shape, const SiteLaunch& s, int64_t n_pi_chunks) {
    WorkspaceLayout w;
    size_t off = 0;
    const auto take = [&off](size_t bytes) { const size_t at = off; off = (off + bytes + 255) / 256 * 256; return at; };
    const size_t ncols = (size_t)shape.ncols, nloci = (size_t)shape.nloci;
    w.work_cols = take(sizeof(int32_t) * ncols);
    // small batches: slow-columns-first copy of the work list; reserved tails: compact_kernel's scratch
    if (!s.persistent || s.reserve_q > 0) w.work_cols2 = take(sizeof(int32_t) * ncols);
    w.work_count = take(sizeof(int32_t) * nloci);
    w.work_prefix = take(sizeof(int64_t) * (nloci + 1));
    w.slice_prefix = take(sizeof(int64_t) * (nloci + 1));
    w.work_class = take(sizeof(int32_t) * 2 * nloci);
    w.work_wprefix = take(sizeof(int64_t) * (nloci + 1));
    w.part_prefix = take(sizeof(int64_t) * 2 * (nloci + 1));
    w.part_start = take(sizeof(int64_t) * 2 * (nloci + 1));
    w.chunk_cnt = take(sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(1, n_pi_chunks));
    w.partial = take(sizeof(double) * (size_t)n_pi_chunks * (size_t)(shape.T + 2 * shape.n_i));
    w.packed = take(sizeof(uint32_t) * (size_t)shape.nwords * ncols);
    if (s.dedup_mode != DEDUP_OFF) {
        w.hash = take(sizeof(uint64_t) * ncols);
        w.dup_of = take(sizeof(int32_t) * ncols);
        w.tab_key = take(sizeof(unsigned long long) * 2 * ncols);
        w.tab_val = take(sizeof(int32_t) * 2 * ncols);
        w.dedup_on = take(sizeof(int32_t) * nloci);
    }
    if (s.lds_depth < shape.stack_depth) {
        // one row per workgroup of the persistent grid (the only mode with the spill variant)
        const size_t rows = (size_t)site_grid(s, 0) * (size_t)(shape.stack_depth - s.lds_depth);
        w.spill = take(rows * 12 * kSiteBlock * sizeof(double));
    }
    w.total = off + 256;
    return w;
}

}  // namespace tphip

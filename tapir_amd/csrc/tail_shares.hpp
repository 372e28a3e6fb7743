// tail_shares.hpp -- how site_rate_kernel's later shares cut the concatenated reserved tails (SiteParams::share_work): in whole
// lane-fills of 64 columns, the shares getting shorter in up to three steps.  Pure 64-bit integer arithmetic without a HIP
// header: the kernel calls tail_share_range, the host's launch decision (site_launch_plan.hpp) tail_share_bound, and
// tests/native/tail_shares_dump.cpp compiles both with g++ (tests/test_tail_shares.py).  tools/share_replay.py restates it.
#pragma once
#include <cstdint>

#include "launch_constants.hpp"

#if defined(__HIP__) || defined(__CUDACC__)
#define TPHIP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define TPHIP_HOST_DEVICE inline
#endif

namespace tphip {

// The tails' columns make F = ceil(ttotal / 64) lane-fills.  The first floor(F frac_big_q / 2^16) fills, rounded down to whole
// shares, go in shares of fills_big fills each; the next floor(F frac_mid_q / 2^16), rounded down likewise, in shares of
// fills_mid; the rest in shares of fills_small, the last of which takes what is left and the ragged end of the last fill.
// fills_big >= fills_mid >= fills_small >= 1 (decide_site_launch sees to it): share lengths never increase with k.  The
// later workgroups are dispatched in grid order, so the long shares (one drain round for many fills) start first and the
// short ones even out the waves' finishing times.  fills_big = 0: the cut into equal column counts over all later shares.
struct TailShares {
    int32_t fills_big = 0, fills_mid = 0, fills_small = 0;
    int32_t frac_big_q = 0, frac_mid_q = 0;   // in units of 2^-kReserveShift, frac_big_q + frac_mid_q <= 2^kReserveShift
    // Tails shorter than this keep the equal column counts.  Whole fills make fewer, longer shares; where the tails hold less
    // than one fill per later workgroup (loci whose columns repeat: after de-duplication a locus' tail is a few columns) a
    // share of several fills would walk dozens of loci, one drain each, while most later workgroups had nothing to do.
    int32_t min_total = 0;
};

// Whether tails of ttotal columns are cut in whole lane-fills (the same answer in every workgroup of a launch)
TPHIP_HOST_DEVICE bool tail_shares_apply(int64_t ttotal, const TailShares& t) { return t.fills_big > 0 && ttotal >= t.min_total; }

struct TailBands {
    int64_t fills, edge1, edge2;   // all fills; where the mid and the small shares begin (in fills)
    int64_t n1, n2, n3;            // shares of the three bands
};

TPHIP_HOST_DEVICE TailBands tail_bands(int64_t ttotal, const TailShares& t) {
    TailBands b;
    b.fills = (ttotal + kSiteBlock - 1) / kSiteBlock;
    b.n1 = ((b.fills * t.frac_big_q) >> kReserveShift) / t.fills_big;
    b.n2 = ((b.fills * t.frac_mid_q) >> kReserveShift) / t.fills_mid;
    b.edge1 = b.n1 * t.fills_big;
    b.edge2 = b.edge1 + b.n2 * t.fills_mid;
    b.n3 = (b.fills - b.edge2 + t.fills_small - 1) / t.fills_small;
    return b;
}

// Column range [*g0, *g1) of the k-th later share in the numbering of the concatenated reserved tails (ttotal columns);
// empty (0, 0) from the first k that the tails do not need.  t.fills_big >= 1.
TPHIP_HOST_DEVICE void tail_share_range(int64_t k, int64_t ttotal, const TailShares& t, int64_t* g0, int64_t* g1) {
    const TailBands b = tail_bands(ttotal, t);
    int64_t f0, f1;
    if (k < b.n1) { f0 = k * t.fills_big; f1 = f0 + t.fills_big; }
    else if (k < b.n1 + b.n2) { f0 = b.edge1 + (k - b.n1) * t.fills_mid; f1 = f0 + t.fills_mid; }
    else if (k < b.n1 + b.n2 + b.n3) { f0 = b.edge2 + (k - b.n1 - b.n2) * t.fills_small; f1 = f0 + t.fills_small; }
    else { *g0 = 0; *g1 = 0; return; }
    *g0 = f0 * kSiteBlock;
    *g1 = f1 * kSiteBlock < ttotal ? f1 * kSiteBlock : ttotal;
}

// Later shares that tails of ttotal columns need
TPHIP_HOST_DEVICE int64_t tail_share_count(int64_t ttotal, const TailShares& t) {
    const TailBands b = tail_bands(ttotal, t);
    return b.n1 + b.n2 + b.n3;
}

// An upper bound of tail_share_count over every ttotal <= ttotal_max.  (The count itself does not grow steadily with ttotal:
// a fill more can turn fills_big short shares into one long one.)  With F fills at most: n1 <= floor(F b) / big,
// n2 <= floor(F m) / mid, and the small band keeps at most F - floor(F (b + m)) + big + mid - 1 fills -- each term grows
// with F.
TPHIP_HOST_DEVICE int64_t tail_share_bound(int64_t ttotal_max, const TailShares& t) {
    const int64_t F = (ttotal_max + kSiteBlock - 1) / kSiteBlock;
    const int64_t rest = F - ((F * ((int64_t)t.frac_big_q + t.frac_mid_q)) >> kReserveShift) + t.fills_big + t.fills_mid - 1;
    return ((F * t.frac_big_q) >> kReserveShift) / t.fills_big + ((F * t.frac_mid_q) >> kReserveShift) / t.fills_mid +
           ((rest < F ? rest : F) + t.fills_small - 1) / t.fills_small;
}

}  // namespace tphip

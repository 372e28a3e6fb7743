// exact_quartet_common.hpp -- what the kernels of exact_quartet_kernels.hpp and locus_set_kernels.hpp
// (section 3.11) share: the shape of the spectrum kernels, the tile count of a window and the closed-form weights of the three
// outcome regions.  No __global__ definition.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "exact_quartet_window.hpp"
#include "wave_sum.hpp"

namespace tphip {

constexpr int kEqBlock = 128;            // spectrum kernel: two waves
constexpr int kEqFreqPerThread = 4;
constexpr int kEqTile = kEqBlock * kEqFreqPerThread;   // frequencies per workgroup
constexpr int kEqGridTiles = 17;         // workgroups of a pair at most: the tiles of a window of 128
constexpr int kEqSiteTile = 256;         // sites per LDS tile, 32 bytes each
constexpr int kEqWeights = 6;            // a1, a2, b1, e, b2, f
constexpr int kEqRow = 6;                // p_correct, p_ac, p_ad, p_polytomy, window, tail_bound
constexpr int kEqMomentBlock = 64;
constexpr int kEqFinalBlock = 256;

__host__ __device__ inline int32_t exact_tiles(int32_t m) { return (m * (m / 2 + 1) + kEqTile - 1) / kEqTile; }

// sum_{d = lo}^{hi} exp(-2 pi i k d / M) = exp(-i pi k (lo + hi) / M) sin(pi n k / M) / sin(pi k / M), n = hi - lo + 1, every
// angle reduced mod 2 pi in integers first: a window that covers all M residues gives M at k = 0 and exactly 0 elsewhere.
__device__ __forceinline__ void eq_weight(int32_t k, int32_t lo, int32_t hi, int32_t M, double& re, double& im) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)hi - lo + 1;
    if (n <= 0) {
        re = 0.0; im = 0.0;
        return;
    }
    if (k == 0) {
        re = (double)n; im = 0.0;
        return;
    }
    const int64_t two_m = 2 * (int64_t)M;
    int64_t a = ((int64_t)k * ((int64_t)lo + hi)) % two_m;
    if (a < 0) a += two_m;
    const int64_t b = ((int64_t)k * n) % two_m;
    const double inv = 1.0 / (double)M;        // a power of two: the quotients below are exact
    double s, c;
    sincospi((double)a * inv, &s, &c);
    const double r = sinpi((double)b * inv) / sinpi((double)k * inv);
    re = r * c;
    im = -(r * s);
}

// The window [c - M/2, c + M/2) cut to d > 0 (positive) or to d < 0.
__device__ __forceinline__ void eq_region(int32_t c, int32_t M, bool positive, int32_t& lo, int32_t& hi) {
    lo = c - M / 2;
    hi = c + M / 2 - 1;
    if (positive) lo = lo > 1 ? lo : 1;
    else hi = hi < -1 ? hi : -1;
}

}  // namespace tphip

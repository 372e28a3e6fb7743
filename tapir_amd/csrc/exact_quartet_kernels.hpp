// exact_quartet_kernels.hpp -- the exact law of a locus' quartet counts: the probabilities that a locus
// resolves an internode correctly, as one of the two wrong topologies or not at all, without the normal approximation of
// sections 3.6 and 3.8.  Included by exact_quartet_driver.hip only (a __global__ definition must live in one translation unit).
//
// Input: the dense per-site planes y, x1, x2 [n_q][ncols] that the *_quartet_sites_dev calls write (an equal-tip quartet passes
// its x plane twice).  Per site, independently, (D1, D2) = (S - N1, S - N2) moves by (+1, +1) with probability y, by (-1, 0)
// with x1, by (0, -1) with x2 and stays with p0 = 1 - y - x1 - x2, so on the M x M torus
//   Phi[j1, j2] = prod_sites (p0 + y z1 z2 + x1 conj(z1) + x2 conj(z2)),  z = exp(2 pi i j / M),
// and with E = D2 - D1 and F = -E the three outcome regions are rectangles:
//   p_correct = M^-2 sum Phi[j1, j2] a1[j1] a2[j2]            (D1 > 0, D2 > 0)
//   p_ac      = M^-2 sum Phi[j1, j2] b1[j1 + j2] e[j2]        (D1 < 0, E > 0: the transform of (D1, E) at (k1, kE) is Phi[k1 - kE, kE])
//   p_ad      = M^-2 sum Phi[j1, j2] b2[j1 + j2] f[j1]        (D2 < 0, F > 0)
// with w[k] = sum over the d of the count's window that lie in the region of exp(-2 pi i k d / M), windows [c - M/2, c + M/2)
// about the rounded means.  Phi and the weights are conjugate-symmetric: the rows j2 = 0 .. M/2 are computed, those strictly
// between counted twice, and the real part taken.
//
// Three kernels: moments and window (one wave per pair), spectrum (a workgroup per pair and tile of 512 frequencies), finalise
// (a thread per pair).  Every sum has a fixed shape and order and there is no atomic, so a row is a function of its locus'
// planes and the options alone.  The arithmetic is written with explicit fma() under contract(off), as the site values are.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "exact_quartet_common.hpp"   // the kernels' shape, exact_tiles, eq_weight, eq_region
#include "exact_quartet_window.hpp"
#include "wave_sum.hpp"

namespace tphip {

struct EqMoment {
    int32_t window;      // M, 0: not computed (no window up to the cap meets the tolerance)
    int32_t c1, c2, ce;  // the centres: round(E D1), round(E D2), round(E E)
    double bound;        // the tail bound at M (at the cap when not computed)
    int32_t point;       // all three variances are 0: the law is the point (c1, c2)
    int32_t pad;
};
static_assert(sizeof(EqMoment) == 32, "EqMoment is laid out in the caller's workspace");

struct EqParams {
    const double* y;               // [n_q][ncols]
    const double* x1;
    const double* x2;
    const int64_t* locus_offsets;  // the plan's
    int64_t ncols;
    int64_t pairs;                 // nloci * n_q; pair = locus * n_q + quartet
    int64_t pair0;                 // spectrum launch: its first pair
    int32_t n_q;
    int32_t cap;                   // largest window allowed
    int32_t tiles_cap;             // tiles of a pair at the cap: the pitch of partial
    double tol;
    EqMoment* mom;                 // [pairs]
    double* partial;               // [pairs][tiles_cap][3]
    double* rows;                  // [pairs][6]
};

// ---- moments and window ----------------------------------------------------------------------------------------------
// One wave per pair.  Lane l takes the locus' columns l, l + 64, ... in order; the six sums go over the wave by a butterfly
// (every lane ends with the same bits).  E D1 = sum (y - x1), Var D1 = sum [(y + x1) - (y - x1)^2], likewise D2 with x2 and
// E with (x1, x2); a site's variance term is >= 0 in exact arithmetic and is held there.
__global__ __launch_bounds__(kEqMomentBlock) void exact_moment_kernel(EqParams P) {
#pragma clang fp contract(off)
    const int64_t pair = blockIdx.x;
    const int64_t locus = pair / P.n_q;
    const int32_t q = (int32_t)(pair - locus * P.n_q);
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const size_t row = (size_t)q * (size_t)P.ncols;
    double m1 = 0.0, m2 = 0.0, me = 0.0, v1 = 0.0, v2 = 0.0, ve = 0.0;
    for (int64_t col = lo + threadIdx.x; col < hi; col += kEqMomentBlock) {
        const double y = P.y[row + col], a = P.x1[row + col], b = P.x2[row + col];
        const double d1 = y - a, d2 = y - b, de = a - b;
        m1 += d1;
        m2 += d2;
        me += de;
        v1 += fmax(0.0, fma(-d1, d1, y + a));
        v2 += fmax(0.0, fma(-d2, d2, y + b));
        ve += fmax(0.0, fma(-de, de, a + b));
    }
    m1 = wave_sum(m1);
    m2 = wave_sum(m2);
    me = wave_sum(me);
    v1 = wave_sum(v1);
    v2 = wave_sum(v2);
    ve = wave_sum(ve);
    if (threadIdx.x != 0) return;
    EqMoment r;
    r.c1 = (int32_t)rint(m1);
    r.c2 = (int32_t)rint(m2);
    r.ce = (int32_t)rint(me);
    r.point = (v1 == 0.0 && v2 == 0.0 && ve == 0.0) ? 1 : 0;
    r.pad = 0;
    r.window = exact_window(v1, v2, ve, P.cap, P.tol, &r.bound);
    if (!(isfinite(m1) && isfinite(m2) && isfinite(me) && isfinite(v1) && isfinite(v2) && isfinite(ve))) {
        r.window = 0;   // planes that are no probabilities: nothing is reported for them
        r.c1 = r.c2 = r.ce = 0;
        r.bound = __builtin_nan("");
    }
    P.mom[pair] = r;
}

// ---- spectrum --------------------------------------------------------------------------------------------------------
// (the weights of the regions: eq_weight and eq_region of exact_quartet_common.hpp)
//
// Grid (tiles at the cap but at most kEqGridTiles, pairs of this launch); a workgroup whose tile lies beyond its pair's M, or
// whose pair needs no spectrum, leaves at once, and with a cap above 128 a workgroup walks the tiles t, t + 17, ... of its
// pair one after the other (measured on 1000 loci x 500 columns x 100 quartets, all of window 64 or 128: a grid of 257 tiles
// a pair for a cap of 512 spent 360 ms on workgroups that only leave, three times the work itself).  Whichever workgroup
// computes a tile, its partial sums are the same bits.  A thread owns four frequencies f = tile * 512 + i * 128 + thread, (j1, j2) = (f mod M, f / M):
// their twiddles (sincospi on the lattice angle) and running products stay in registers.  The locus' sites stream through LDS
// in tiles of 256, in column order, as (p0, y, x1, x2); every thread reads the same site (a broadcast).  Per site and
// frequency: 6 fma/mul for the factor, 4 for the complex product.  Dynamic LDS: 8 KB of sites, 6 weight vectors of M complex
// numbers (sized for the cap), the wave sums.
__global__ __launch_bounds__(kEqBlock) void exact_spectrum_kernel(EqParams P) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double eq_lds[];
    const int64_t pair = P.pair0 + blockIdx.y;
    const EqMoment mom = P.mom[pair];
    const int32_t M = mom.window;
    const int32_t ntiles = exact_tiles(M);
    if (M == 0 || mom.point || (int32_t)blockIdx.x >= ntiles) return;   // (the same in every thread of the workgroup)
    double* site = eq_lds;                                       // [kEqSiteTile][4]
    double* wgt = eq_lds + 4 * kEqSiteTile;                      // [6][M][2]
    double* red = wgt + 2 * kEqWeights * P.cap;                  // [2][3]
    const int64_t locus = pair / P.n_q;
    const int32_t q = (int32_t)(pair - locus * P.n_q);
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const size_t row = (size_t)q * (size_t)P.ncols;
    const int tid = threadIdx.x;

    for (int idx = tid; idx < kEqWeights * M; idx += kEqBlock) {
        const int v = idx / M, k = idx - v * M;
        const int32_t c = (v == 0 || v == 2) ? mom.c1 : (v == 1 || v == 4) ? mom.c2 : (v == 3) ? mom.ce : -mom.ce;
        int32_t dlo, dhi;
        eq_region(c, M, v != 2 && v != 4, dlo, dhi);
        double re, im;
        eq_weight(k, dlo, dhi, M, re, im);
        wgt[2 * idx] = re;
        wgt[2 * idx + 1] = im;
    }

    const int32_t nfreq = M * (M / 2 + 1);
    const int shift = __ffs(M) - 1;
    const double two_inv = 2.0 / (double)M;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
    for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        double c1[kEqFreqPerThread], s1[kEqFreqPerThread], c2[kEqFreqPerThread], s2[kEqFreqPerThread], c12[kEqFreqPerThread],
            s12[kEqFreqPerThread], pr[kEqFreqPerThread], pi[kEqFreqPerThread];
#pragma unroll
        for (int i = 0; i < kEqFreqPerThread; ++i) {
            const int32_t f = tile * kEqTile + i * kEqBlock + tid;
            const int32_t j1 = f & (M - 1), j2 = f >> shift;
            if (f < nfreq) {
                sincospi((double)j1 * two_inv, &s1[i], &c1[i]);
                sincospi((double)j2 * two_inv, &s2[i], &c2[i]);
                sincospi((double)((j1 + j2) & (M - 1)) * two_inv, &s12[i], &c12[i]);
            } else {
                c1[i] = s1[i] = c2[i] = s2[i] = c12[i] = s12[i] = 0.0;
            }
            pr[i] = 1.0;
            pi[i] = 0.0;
        }

        for (int64_t base = lo; base < hi; base += kEqSiteTile) {
            __syncthreads();   // the previous tile has been read (first round: nothing to wait for but the weights' writers)
            for (int i = tid; i < kEqSiteTile; i += kEqBlock) {
                const int64_t col = base + i;
                double y = 0.0, a = 0.0, b = 0.0;
                if (col < hi) {
                    y = P.y[row + col];
                    a = P.x1[row + col];
                    b = P.x2[row + col];
                }
                site[4 * i] = ((1.0 - y) - a) - b;
                site[4 * i + 1] = y;
                site[4 * i + 2] = a;
                site[4 * i + 3] = b;
            }
            __syncthreads();
            const int n = (int)((hi - base) < kEqSiteTile ? (hi - base) : kEqSiteTile);
            for (int s = 0; s < n; ++s) {
                const double p0 = site[4 * s], y = site[4 * s + 1], a = site[4 * s + 2], b = site[4 * s + 3];
                if (y == 0.0 && a == 0.0 && b == 0.0) continue;   // the factor 1: a culled, NaN-rate or zero-rate column
#pragma unroll
                for (int i = 0; i < kEqFreqPerThread; ++i) {
                    const double fr = fma(y, c12[i], fma(a, c1[i], fma(b, c2[i], p0)));
                    const double fi = fma(y, s12[i], -fma(a, s1[i], b * s2[i]));
                    const double nr = fma(-pi[i], fi, pr[i] * fr);
                    const double ni = fma(pr[i], fi, pi[i] * fr);
                    pr[i] = nr;
                    pi[i] = ni;
                }
            }
        }
        __syncthreads();   // the weights are in LDS whether or not the locus had a site

        double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < kEqFreqPerThread; ++i) {
            const int32_t f = tile * kEqTile + i * kEqBlock + tid;
            if (f >= nfreq) continue;
            const int32_t j1 = f & (M - 1), j2 = f >> shift, j12 = (j1 + j2) & (M - 1);
            const double twice = (j2 == 0 || j2 == M / 2) ? 1.0 : 2.0;
            const double* left[3] = {wgt + 2 * (0 * M + j1), wgt + 2 * (2 * M + j12), wgt + 2 * (4 * M + j12)};
            const double* right[3] = {wgt + 2 * (1 * M + j2), wgt + 2 * (3 * M + j2), wgt + 2 * (5 * M + j1)};
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const double ar = left[w][0], ai = left[w][1], br = right[w][0], bi = right[w][1];
                const double wr = fma(-ai, bi, ar * br), wi = fma(ar, bi, ai * br);
                acc[w] = fma(twice, fma(-pi[i], wi, pr[i] * wr), acc[w]);
            }
        }
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const double v = wave_sum(acc[w]);
            if (lane == 0) red[3 * wave + w] = v;
        }
        __syncthreads();
        if (tid < 3) P.partial[((size_t)pair * P.tiles_cap + tile) * 3 + tid] = red[tid] + red[3 + tid];
    }
}

// ---- finalise --------------------------------------------------------------------------------------------------------
// A thread per pair: the pair's tiles in ascending order, 1 / M^2, the clamps.  A point law is read off its centres.
__global__ __launch_bounds__(kEqFinalBlock) void exact_finalise_kernel(EqParams P) {
#pragma clang fp contract(off)
    const int64_t pair = (int64_t)blockIdx.x * kEqFinalBlock + threadIdx.x;
    if (pair >= P.pairs) return;
    const EqMoment mom = P.mom[pair];
    double* o = P.rows + (size_t)pair * kEqRow;
    double pc, p1, p2, rest;
    if (mom.window == 0) {
        pc = p1 = p2 = rest = __builtin_nan("");
    } else if (mom.point) {
        pc = (mom.c1 > 0 && mom.c2 > 0) ? 1.0 : 0.0;
        p1 = (mom.c1 < 0 && mom.c1 < mom.c2) ? 1.0 : 0.0;
        p2 = (mom.c2 < 0 && mom.c2 < mom.c1) ? 1.0 : 0.0;
        rest = ((1.0 - pc) - p1) - p2;
    } else {
        const int32_t nt = exact_tiles(mom.window);
        const double* part = P.partial + (size_t)pair * P.tiles_cap * 3;
        double s[3] = {0.0, 0.0, 0.0};
        for (int32_t t = 0; t < nt; ++t) {
            s[0] += part[3 * t];
            s[1] += part[3 * t + 1];
            s[2] += part[3 * t + 2];
        }
        const double scale = 1.0 / ((double)mom.window * (double)mom.window);   // a power of two
        pc = fmin(1.0, fmax(0.0, s[0] * scale));
        p1 = fmin(1.0, fmax(0.0, s[1] * scale));
        p2 = fmin(1.0, fmax(0.0, s[2] * scale));
        rest = fmax(0.0, ((1.0 - pc) - p1) - p2);
    }
    o[0] = pc;
    o[1] = p1;
    o[2] = p2;
    o[3] = rest;
    o[4] = (double)mom.window;
    o[5] = mom.bound;
}

}  // namespace tphip

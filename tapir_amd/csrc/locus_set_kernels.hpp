// locus_set_kernels.hpp -- accumulation curves over an ordered list of loci: the probabilities that the
// first k loci of a quartet's order, analysed together, resolve its internode, for every k.  Sites are independent, so a set
// of loci is one long locus: the moment sums of sections 3.6 / 3.8 add, and the characteristic function of section 3.9 is the
// product of the loci's.  Included by locus_set_driver.hip only (a __global__ definition must live in one translation unit).
//
// Normal rows: locus_set_sums_kernel (a thread per quartet and moment walks the order and adds, left to right) and
// locus_set_probabilities_kernel (a thread per quartet and k: the family's own rule, quartet_probabilities.hpp /
// unequal_quartet_probabilities.hpp) -- together the "locus_set_rows_kernel" of the design.
//
// Exact rows: all prefixes of a quartet share the torus M = window_cap.
//   locus_set_moment_kernel    exact_moment_kernel's shape, but the six raw sums per (locus, quartet) are kept
//   locus_set_head_kernel      a thread per quartet: the sequential prefix of those sums over the order; per prefix the rounded
//                              centres, the Bernstein bound at the cap and whether the prefix is computed; the head's length
//   locus_set_spectrum_kernel  a workgroup per (tile of 512 frequencies, quartet) walks the head's loci in order with the running
//                              product in registers and, at every locus boundary, sums it against that prefix's weights
//   locus_set_finalise_kernel  a thread per (quartet, k): the tiles in ascending order, 1 / M^2, the clamps
// Every sum has a fixed shape and order and there is no atomic: row (q, k) is a function of the planes of the first k loci of
// the quartet's order, in that order, of the cap and of the tolerance alone.  The arithmetic is written with explicit fma()
// under contract(off), as section 3.9's is.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "exact_quartet_common.hpp"
#include "exact_quartet_window.hpp"
#include "quartet_probabilities.hpp"
#include "unequal_quartet_probabilities.hpp"

namespace tphip {

constexpr int kLsBlock = 256;            // the rows, head and finalise kernels
constexpr int kLsEqualSums = 5, kLsEqualRow = 8;       // quartet_kernels.hpp: kQtSums, kQtRow
constexpr int kLsUnequalSums = 9, kLsUnequalRow = 13;  // unequal_quartet_kernels.hpp: kUqSums, kUqRow

// ---- normal rows -------------------------------------------------------------------------------------------------------
struct LsRowsParams {
    const double* locus_rows;   // [nloci][n_q][row]
    const int32_t* order;       // [n_q][n_k]
    int32_t n_q, n_k;
    int32_t sums, row;          // 5, 8 or 9, 13
    double* rows;               // [n_q][n_k][row]
};

// The cost grows with n_k: the sums of a (quartet, moment) are one thread's sequential additions.
__global__ __launch_bounds__(kLsBlock) void locus_set_sums_kernel(LsRowsParams P) {
    const int64_t idx = (int64_t)blockIdx.x * kLsBlock + threadIdx.x;
    if (idx >= (int64_t)P.n_q * P.sums) return;
    const int32_t q = (int32_t)(idx / P.sums), m = (int32_t)(idx - (int64_t)q * P.sums);
    const int32_t* ord = P.order + (size_t)q * P.n_k;
    double* out = P.rows + (size_t)q * P.n_k * P.row + m;
    double s = 0.0;
    for (int32_t k = 0; k < P.n_k; ++k) {
        s += P.locus_rows[((size_t)ord[k] * P.n_q + q) * P.row + m];
        out[(size_t)k * P.row] = s;
    }
}

__global__ __launch_bounds__(kLsBlock) void locus_set_probabilities_kernel(LsRowsParams P) {
    const int64_t idx = (int64_t)blockIdx.x * kLsBlock + threadIdx.x;
    if (idx >= (int64_t)P.n_q * P.n_k) return;
    double* o = P.rows + (size_t)idx * P.row;
    if (P.sums == kLsEqualSums) quartet_probabilities(o);
    else uquartet_probabilities(o);
}

// ---- exact rows ----------------------------------------------------------------------------------------------------------
struct LsSums {
    double m1, m2, me, v1, v2, ve;   // sum (y - x1), (y - x2), (x1 - x2) and the three variance sums of one locus
};
static_assert(sizeof(LsSums) == 48, "LsSums is laid out in the caller's workspace");

struct LsPrefix {
    int32_t c1, c2, ce;   // the centres: round(E D1), round(E D2), round(E E) of the first k loci
    int32_t state;        // 0: not computed, 1: computed, 2: computed and a point law
    double bound;         // the tail bound at the cap
    double pad;
};
static_assert(sizeof(LsPrefix) == 32, "LsPrefix is laid out in the caller's workspace");

struct LsParams {
    const double* y;               // [n_q][ncols]
    const double* x1;
    const double* x2;
    const int64_t* locus_offsets;  // the plan's
    int64_t ncols;
    int64_t pairs;                 // nloci * n_q; pair = locus * n_q + quartet
    int32_t n_q, n_k, n_head;
    int32_t cap;                   // M of every prefix
    int32_t tiles_cap;             // exact_tiles(cap)
    double tol;
    const int32_t* order;          // [n_q][n_k]
    LsSums* sums;                  // [pairs]
    LsPrefix* prefix;              // [n_q][n_k]
    int32_t* head;                 // [n_q]: K_q, the prefixes 1 .. K_q are computed
    double* partial;               // [n_q][n_head][tiles_cap][3]
    double* rows;                  // [n_q][n_k][6]
};

// The order reaches the workspace as kernel arguments: a launch writes the n <= kLsOrderBatch indices it carries to
// dst[at .. at + n).
constexpr int kLsOrderBatch = 960;   // 3840 bytes of the 4 KB a launch's arguments may take
struct LsOrderBatch {
    int32_t v[kLsOrderBatch];
};

__global__ __launch_bounds__(kLsBlock) void locus_set_order_kernel(int32_t* __restrict__ dst, int64_t at, int32_t n, LsOrderBatch B) {
    const int32_t i = (int32_t)(blockIdx.x * kLsBlock + threadIdx.x);
    if (i < n) dst[at + i] = B.v[i];
}

// One wave per pair.  Lane l takes the locus' columns l, l + 64, ... in order; the six sums go over the wave by a butterfly.
__global__ __launch_bounds__(kEqMomentBlock) void locus_set_moment_kernel(LsParams P) {
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
    LsSums s;
    s.m1 = wave_sum(m1);
    s.m2 = wave_sum(m2);
    s.me = wave_sum(me);
    s.v1 = wave_sum(v1);
    s.v2 = wave_sum(v2);
    s.ve = wave_sum(ve);
    if (threadIdx.x == 0) P.sums[pair] = s;
}

// A thread per quartet.  A site's variance term is >= 0, so the bound grows with k and the computed prefixes form a head; the
// latch `open` holds that against the rounding of exp().  A prefix beyond n_head is reported as not computed.
__global__ __launch_bounds__(kLsBlock) void locus_set_head_kernel(LsParams P) {
#pragma clang fp contract(off)
    const int32_t q = (int32_t)(blockIdx.x * kLsBlock + threadIdx.x);
    if (q >= P.n_q) return;
    const int32_t* ord = P.order + (size_t)q * P.n_k;
    double m1 = 0.0, m2 = 0.0, me = 0.0, v1 = 0.0, v2 = 0.0, ve = 0.0;
    bool open = true;
    int32_t head = 0;
    for (int32_t k = 0; k < P.n_k; ++k) {
        const LsSums s = P.sums[(size_t)ord[k] * P.n_q + q];
        m1 += s.m1;
        m2 += s.m2;
        me += s.me;
        v1 += s.v1;
        v2 += s.v2;
        ve += s.ve;
        LsPrefix r;
        r.pad = 0.0;
        const bool finite = isfinite(m1) && isfinite(m2) && isfinite(me) && isfinite(v1) && isfinite(v2) && isfinite(ve);
        if (finite) {
            r.c1 = (int32_t)rint(m1);
            r.c2 = (int32_t)rint(m2);
            r.ce = (int32_t)rint(me);
            r.bound = exact_tail_bound(v1, v2, ve, P.cap);
        } else {   // planes that are no probabilities: nothing is reported for them
            r.c1 = r.c2 = r.ce = 0;
            r.bound = __builtin_nan("");
        }
        open = open && finite && r.bound <= P.tol && k < P.n_head;
        r.state = !open ? 0 : (v1 == 0.0 && v2 == 0.0 && ve == 0.0) ? 2 : 1;
        if (open) head = k + 1;
        P.prefix[(size_t)q * P.n_k + k] = r;
    }
    P.head[q] = head;
}

// Grid (tiles at the cap but at most kEqGridTiles, quartets); with a cap above 128 a workgroup walks the tiles t, t + 17, ...
// one after the other, as exact_spectrum_kernel does, and whichever workgroup computes a tile, its partial sums are the same
// bits.  A thread owns four frequencies f = tile * 512 + i * 128 + thread, (j1, j2) = (f mod M, f / M): their twiddles and the
// running product stay in registers across the loci of the head.  Each locus' columns stream through LDS in tiles of 256, in
// column order, as (p0, y, x1, x2) broadcasts; a dead site (the factor 1) is skipped.  At a locus boundary the six weight
// vectors of that prefix's centres are filled into LDS, the three weighted sums formed, added over the wave by a butterfly
// and over the two waves in order, and written to partial[q][k][tile][3]; the product carries on into the next locus.  An
// empty locus changes neither product nor weights, but its row is written all the same.  A point law needs no sum (the
// finalise kernel reads it off the centres), only the product.  Dynamic LDS: that of exact_spectrum_kernel at the cap.
__global__ __launch_bounds__(kEqBlock) void locus_set_spectrum_kernel(LsParams P) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double ls_lds[];
    const int32_t q = blockIdx.y;
    const int32_t head = P.head[q];
    if (head == 0) return;   // (the same in every thread of the workgroup)
    const int32_t M = P.cap;
    double* site = ls_lds;                                       // [kEqSiteTile][4]
    double* wgt = ls_lds + 4 * kEqSiteTile;                      // [6][M][2]
    double* red = wgt + 2 * kEqWeights * M;                      // [2][3]
    const int32_t* ord = P.order + (size_t)q * P.n_k;
    const LsPrefix* pre = P.prefix + (size_t)q * P.n_k;
    const size_t row = (size_t)q * (size_t)P.ncols;
    const int tid = threadIdx.x;
    const int32_t nfreq = M * (M / 2 + 1);
    const int shift = __ffs(M) - 1;
    const double two_inv = 2.0 / (double)M;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
    for (int32_t tile = blockIdx.x; tile < P.tiles_cap; tile += gridDim.x) {
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

#pragma unroll 1
        for (int32_t k = 0; k < head; ++k) {
            const int64_t locus = ord[k];
            const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
            for (int64_t base = lo; base < hi; base += kEqSiteTile) {
                __syncthreads();   // the previous tile of sites has been read
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

            // the boundary after locus k: the row of the set of size k + 1
            const LsPrefix mom = pre[k];
            if (mom.state != 1) continue;   // a point law (the same in every thread of the workgroup)
            __syncthreads();   // the weights and sums of the previous boundary have been read
            for (int idx = tid; idx < kEqWeights * M; idx += kEqBlock) {
                const int v = idx >> shift, j = idx & (M - 1);
                const int32_t c = (v == 0 || v == 2) ? mom.c1 : (v == 1 || v == 4) ? mom.c2 : (v == 3) ? mom.ce : -mom.ce;
                int32_t dlo, dhi;
                eq_region(c, M, v != 2 && v != 4, dlo, dhi);
                double re, im;
                eq_weight(j, dlo, dhi, M, re, im);
                wgt[2 * idx] = re;
                wgt[2 * idx + 1] = im;
            }
            __syncthreads();
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
            if (tid < 3) P.partial[(((size_t)q * P.n_head + k) * P.tiles_cap + tile) * 3 + tid] = red[tid] + red[3 + tid];
        }
        __syncthreads();   // the next tile's sites and weights overwrite what this one may still be reading
    }
}

// A thread per (quartet, k): the tiles in ascending order, 1 / M^2, the clamps.  A point law is read off its centres; a prefix
// that is not computed gets NaN probabilities, window 0 and the bound at the cap.
__global__ __launch_bounds__(kLsBlock) void locus_set_finalise_kernel(LsParams P) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * kLsBlock + threadIdx.x;
    if (idx >= (int64_t)P.n_q * P.n_k) return;
    const int32_t q = (int32_t)(idx / P.n_k), k = (int32_t)(idx - (int64_t)q * P.n_k);
    const LsPrefix mom = P.prefix[idx];
    double* o = P.rows + (size_t)idx * kEqRow;
    double pc, p1, p2, rest;
    if (mom.state == 0) {
        pc = p1 = p2 = rest = __builtin_nan("");
    } else if (mom.state == 2) {
        pc = (mom.c1 > 0 && mom.c2 > 0) ? 1.0 : 0.0;
        p1 = (mom.c1 < 0 && mom.c1 < mom.c2) ? 1.0 : 0.0;
        p2 = (mom.c2 < 0 && mom.c2 < mom.c1) ? 1.0 : 0.0;
        rest = ((1.0 - pc) - p1) - p2;
    } else {
        const double* part = P.partial + ((size_t)q * P.n_head + k) * P.tiles_cap * 3;
        double s[3] = {0.0, 0.0, 0.0};
        for (int32_t t = 0; t < P.tiles_cap; ++t) {
            s[0] += part[3 * t];
            s[1] += part[3 * t + 1];
            s[2] += part[3 * t + 2];
        }
        const double scale = 1.0 / ((double)P.cap * (double)P.cap);   // a power of two
        pc = fmin(1.0, fmax(0.0, s[0] * scale));
        p1 = fmin(1.0, fmax(0.0, s[1] * scale));
        p2 = fmin(1.0, fmax(0.0, s[2] * scale));
        rest = fmax(0.0, ((1.0 - pc) - p1) - p2);
    }
    o[0] = pc;
    o[1] = p1;
    o[2] = p2;
    o[3] = rest;
    o[4] = mom.state == 0 ? 0.0 : (double)P.cap;
    o[5] = mom.bound;
}

}  // namespace tphip

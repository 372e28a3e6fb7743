// quartet_kernels.hpp -- signal and noise probabilities of a four-taxon tree per site, their per-locus sums and the
// probabilities that the locus resolves the internode (Townsend, Su & Tekle 2012; Su et al. 2014).
// Included by quartet_driver.hip only (a __global__ definition must live in one translation unit).
//
// The quartet is ((a:T, b:T)u, (c:T, d:T)v) with u-v of length t_o.  For a site of final rate r (finalize_rate) under the
// locus' generator normalised to one substitution, M = exp(Q r T / kappa) and N = exp(Q r t_o / kappa), and with
// w_xy = pi_x N_xy
//   signal y = sum_xy w_xy sum_{i != j} M_xi^2 M_yj^2                (pattern iijj)
//   noise  x = sum_xy w_xy 2 sum_{i < j} (M_xi M_yi)(M_xj M_yj)      (pattern ijij; ijji has the same probability)
// Every sum is a sum of non-negative terms: nothing of the form S^2 - sum m^2, which cancels to nothing at small r T.
//
// The arithmetic of a site is written with explicit fma() under contract(off): the value of (y, x) is then a function of
// (model, r, T, t_o) alone -- not of the kernel it is inlined into, of the quartet's position in the list or of which
// matrix came out of the cache -- which is what the bit-identity contract of the rows rests on.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gtr_model.hpp"
#include "pi_rate.hpp"
#include "quartet_common.hpp"
#include "quartet_probabilities.hpp"
#include "transition_row.hpp"

namespace tphip {

constexpr int kQtBlock = 256;
constexpr int kQtColsPerThread = 4;
constexpr int kQtChunk = kQtBlock * kQtColsPerThread;   // the plan's PI chunks (pi_kernels.hpp: kPiChunk)
static_assert(kQtChunk == 1024, "the plan's chunk_locus / chunk_index are cut for 1024 columns");
constexpr int kQtBatch = 64;     // quartets per launch: their lengths travel as kernel arguments (no copy, no synchronisation)
constexpr int kQtTile = 4;       // quartets whose five sums a thread keeps (in LDS) while it walks its columns
constexpr int kQtSums = 5;       // Y, X, Yy, Xx, XY
constexpr int kQtRow = 8;        // + p_correct, p_incorrect, p_polytomy
constexpr int kQtReduceBlock = 64;

struct QuartetBatch {
    double tip[kQtBatch];
    double internode[kQtBatch];
};

struct QuartetParams {
    PiParams pi;                 // rates, cull and the chunk map; pi.partial is not used
    const LocusModel* models;
    int32_t f81;                 // the plan's models are F81: the closed form e I + (1 - e) Pi
    int32_t n_q;                 // quartets of the whole call (row pitch of partial / sites)
    int32_t q0, nq;              // this launch: quartets q0 .. q0 + nq - 1 = the entries 0 .. nq - 1 of the batch
    double* partial;             // [nchunks][n_q][5]
    double* sites;               // [2][n_q][ncols]
    int64_t ncols;
};

// P(tau) = exp(Q r tau / kappa), row-major: the four rows of transition_row.hpp (the expm1 form; F81 in closed form).
__device__ __forceinline__ void quartet_transition(const LocusModel& m, bool f81, double r, double tau, double* __restrict__ P) {
    double e[3];
    transition_exps(m, f81, transition_scale(m, r, tau), e);
#pragma unroll
    for (int i = 0; i < 4; ++i) transition_row(m, f81, e, i, P + 4 * i);
}

// (y, x) of one site from its two matrices.  With a_x[i] = M_xi^2 and R_y[i] = sum_{j != i} a_y[j] (three additions each),
// the signal's inner sum is sum_i a_x[i] R_y[i]; with c[i] = M_xi M_yi the noise's is
// 2 (c0 (c1 + c2 + c3) + c1 (c2 + c3) + c2 c3), symmetric in (x, y), so the pairs x < y carry the weight w_xy + w_yx.
__device__ __forceinline__ void quartet_signal_noise(const LocusModel& m, const double* __restrict__ M, const double* __restrict__ N,
                                                     double& y, double& x) {
#pragma clang fp contract(off)
    double a[16], R[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = M[k] * M[k];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        R[4 * s + 0] = (a[4 * s + 1] + a[4 * s + 2]) + a[4 * s + 3];
        R[4 * s + 1] = (a[4 * s + 0] + a[4 * s + 2]) + a[4 * s + 3];
        R[4 * s + 2] = (a[4 * s + 0] + a[4 * s + 1]) + a[4 * s + 3];
        R[4 * s + 3] = (a[4 * s + 0] + a[4 * s + 1]) + a[4 * s + 2];
    }
    double sy = 0.0, sx = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double w = m.pi[s] * N[4 * s + t];
            double in = a[4 * s] * R[4 * t];
            in = fma(a[4 * s + 1], R[4 * t + 1], in);
            in = fma(a[4 * s + 2], R[4 * t + 2], in);
            in = fma(a[4 * s + 3], R[4 * t + 3], in);
            sy = fma(w, in, sy);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int t = s; t < 4; ++t) {
            const double w = (s == t) ? m.pi[s] * N[4 * s + s] : m.pi[s] * N[4 * s + t] + m.pi[t] * N[4 * t + s];
            const double c0 = M[4 * s] * M[4 * t], c1 = M[4 * s + 1] * M[4 * t + 1], c2 = M[4 * s + 2] * M[4 * t + 2],
                         c3 = M[4 * s + 3] * M[4 * t + 3];
            double in = c2 * c3;
            in = fma(c1, c2 + c3, in);
            in = fma(c0, (c1 + c2) + c3, in);
            sx = fma(w, 2.0 * in, sx);
        }
    }
    y = sy;
    x = sx;
}

// One workgroup per 1024-column chunk of a locus, a thread four columns (column = base + j * 256 + thread, as
// pi_partial_kernel).  The locus' model is wave-uniform: it is read through the scalar cache into SGPRs, once per wave.
// Quartets go through in tiles of kQtTile: per tile a thread walks its columns and, per column, the tile's quartets in
// order, keeping the last M and the last N so that a quartet whose T or t_o equals its predecessor's in the tile reuses the
// matrix.  The thread's 20 running sums of the tile live in LDS (its own slots, [sum][thread]: no bank conflict, no
// barrier), which keeps the quartet loop a loop -- one copy of the site arithmetic -- instead of four unrolled ones.  The
// tile's sums are then added over the wave by a butterfly and over the four waves in order: a fixed shape, no atomics.
// Two waves per SIMD: 206 VGPRs without a spill; asked for three (168) the compiler spills 50 of them to scratch.
constexpr int kQtWavesPerSimd = 2;
__global__ __launch_bounds__(kQtBlock, kQtWavesPerSimd) void quartet_partial_kernel(QuartetParams P, QuartetBatch B) {
    __shared__ double acc[kQtTile * kQtSums][kQtBlock];
    __shared__ double red[kQtBatch * kQtSums][kQtBlock / 64];
    const int chunk = blockIdx.x;
    const QuartetChunk ch = quartet_chunk<kQtChunk>(P.pi);
    const int locus = ch.locus;
    const int64_t hi = ch.hi, base = ch.base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LocusModel& model = P.models[locus];
    double r[kQtColsPerThread];
#pragma unroll
    for (int j = 0; j < kQtColsPerThread; ++j) {
        const int64_t col = base + j * kQtBlock + threadIdx.x;
        r[j] = (col < hi) ? finalize_rate(P.pi, col) : 0.0;
    }
    const bool f81 = P.f81 != 0;
    for (int t0 = 0; t0 < P.nq; t0 += kQtTile) {
        const int nk = min(kQtTile, P.nq - t0);
#pragma unroll
        for (int w = 0; w < kQtTile * kQtSums; ++w) acc[w][threadIdx.x] = 0.0;
#pragma unroll 1
        for (int j = 0; j < kQtColsPerThread; ++j) {
            if (!quartet_live(r[j])) continue;
            double M[16], N[16];
#pragma unroll 1
            for (int k = 0; k < nk; ++k) {
                const int q = t0 + k;
                if (k == 0 || B.tip[q] != B.tip[q - 1]) quartet_transition(model, f81, r[j], B.tip[q], M);
                if (k == 0 || B.internode[q] != B.internode[q - 1]) quartet_transition(model, f81, r[j], B.internode[q], N);
                double y, x;
                quartet_signal_noise(model, M, N, y, x);
                double* a = &acc[k * kQtSums][threadIdx.x];
                a[0] += y;
                a[kQtBlock] += x;
                a[2 * kQtBlock] = fma(y, y, a[2 * kQtBlock]);
                a[3 * kQtBlock] = fma(x, x, a[3 * kQtBlock]);
                a[4 * kQtBlock] = fma(x, y, a[4 * kQtBlock]);
            }
        }
        for (int w = 0; w < nk * kQtSums; ++w) {
            const double v = wave_sum(acc[w][threadIdx.x]);
            if (lane == 0) red[t0 * kQtSums + w][wave] = v;
        }
    }
    __syncthreads();
    double* out = P.partial + ((size_t)chunk * P.n_q + P.q0) * kQtSums;
    for (int w = threadIdx.x; w < P.nq * kQtSums; w += kQtBlock) out[w] = ((red[w][0] + red[w][1]) + red[w][2]) + red[w][3];
}

// Dense per-site values: sites[0][q][col] = y, sites[1][q][col] = x; a thread is one column at a time and walks the batch's
// quartets with the same matrix reuse.  Culled and zero-rate columns get exactly 0.
__global__ __launch_bounds__(kQtBlock, kQtWavesPerSimd) void quartet_sites_kernel(QuartetParams P, QuartetBatch B) {
    const QuartetChunk ch = quartet_chunk<kQtChunk>(P.pi);
    const int locus = ch.locus;
    const int64_t hi = ch.hi, base = ch.base;
    const LocusModel& model = P.models[locus];
    const bool f81 = P.f81 != 0;
#pragma unroll 1
    for (int j = 0; j < kQtColsPerThread; ++j) {
        const int64_t col = base + j * kQtBlock + threadIdx.x;
        if (col >= hi) continue;
        const double r = finalize_rate(P.pi, col);
        const bool live = quartet_live(r);
        double M[16], N[16];
#pragma unroll 1
        for (int q = 0; q < P.nq; ++q) {
            double y = 0.0, x = 0.0;
            if (live) {
                if (q == 0 || B.tip[q] != B.tip[q - 1]) quartet_transition(model, f81, r, B.tip[q], M);
                if (q == 0 || B.internode[q] != B.internode[q - 1]) quartet_transition(model, f81, r, B.internode[q], N);
                quartet_signal_noise(model, M, N, y, x);
            }
            P.sites[(size_t)(P.q0 + q) * P.ncols + col] = y;
            P.sites[((size_t)P.n_q + P.q0 + q) * P.ncols + col] = x;
        }
    }
}

// ---- resolution probabilities: quartet_probabilities() of quartet_probabilities.hpp ---------------------------------

// One workgroup per locus: the five sums of every quartet over the locus' chunks in ascending order, then the three
// probabilities.  rows [L][n_q][8] = Y, X, Yy, Xx, XY, p_correct, p_incorrect, p_polytomy.
__global__ __launch_bounds__(kQtReduceBlock) void quartet_reduce_kernel(const double* __restrict__ partial,
                                                                      const int64_t* __restrict__ locus_chunk_offsets, int32_t n_q,
                                                                      double* __restrict__ rows) {
    const int locus = blockIdx.x;
    const int64_t c0 = locus_chunk_offsets[locus], c1 = locus_chunk_offsets[locus + 1];
    const int Wp = n_q * kQtSums;
    double* row = rows + (size_t)locus * n_q * kQtRow;
    for (int w = threadIdx.x; w < Wp; w += kQtReduceBlock) {
        double s = 0.0;
        for (int64_t c = c0; c < c1; ++c) s += partial[(size_t)c * Wp + w];
        row[(w / kQtSums) * kQtRow + (w % kQtSums)] = s;
    }
    __syncthreads();   // a quartet's five sums were written by up to five threads of this workgroup
    for (int q = threadIdx.x; q < n_q; q += kQtReduceBlock) {
        double* o = row + q * kQtRow;
        quartet_probabilities(o);
    }
}

}  // namespace tphip

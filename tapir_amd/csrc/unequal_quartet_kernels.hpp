// unequal_quartet_kernels.hpp -- signal and noise of a four-taxon tree whose four tip branches differ, per site, their
// per-locus sums and the probabilities that the locus resolves the internode, or one of the two wrong topologies
// (Townsend, Su & Tekle 2012; Su & Townsend 2015).  Included by unequal_quartet_driver.hip only (a
// __global__ definition must live in one translation unit).
//
// The quartet is ((a:Ta, b:Tb)u, (c:Tc, d:Td)v) with u-v of length t_o.  For a site of final rate r (finalize_rate) under
// the locus' generator normalised to one substitution, A = P(r Ta), B = P(r Tb), C = P(r Tc), D = P(r Td), N = P(r t_o) with
// P of transition_row.hpp.  Rooted at u (the model is reversible), with R_u[i][j] = sum_v N_uv C_vi D_vj and i != j:
//   signal y  = sum_u pi_u sum_i A_ui B_ui sum_{j != i} R_u[j][j]      (pattern iijj, supports ab|cd)
//   noise  x1 = sum_u pi_u sum_{i != j} A_ui B_uj R_u[i][j]            (pattern ijij, supports ac|bd)
//   noise  x2 = sum_u pi_u sum_{i != j} A_ui B_uj R_u[j][i]            (pattern ijji, supports ad|bc)
// Every sum is a sum of products of matrix entries: nothing of the form "total minus the rest".
//
// The arithmetic of a site is written with explicit fma() under contract(off): (y, x1, x2) is then a function of (model, r,
// the five lengths) alone -- not of the kernel it is inlined into, nor of the quartet's position in the list -- which is
// what the bit-identity contract of the rows rests on.  x2 walks the pairs (i, j) in x1's order and takes the term
// (A_uj B_ui) R_u[i][j]: with Ta = Tb the two are then the same number, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gtr_model.hpp"
#include "pi_rate.hpp"
#include "quartet_common.hpp"
#include "transition_row.hpp"
#include "unequal_quartet_probabilities.hpp"

namespace tphip {

constexpr int kUqBlock = 256;
constexpr int kUqColsPerThread = 4;
constexpr int kUqChunk = kUqBlock * kUqColsPerThread;   // the plan's PI chunks (pi_kernels.hpp: kPiChunk)
static_assert(kUqChunk == 1024, "the plan's chunk_locus / chunk_index are cut for 1024 columns");
constexpr int kUqBatch = 64;     // quartets per launch: their lengths travel as kernel arguments (no copy, no synchronisation)
constexpr int kUqSums = 9;       // Y, X1, X2, Yy, X1x1, X2x2, YX1, YX2, X1X2
constexpr int kUqRow = 13;       // + p_correct, p_ac, p_ad, p_polytomy
constexpr int kUqReduceBlock = 64;

struct UnequalQuartetBatch {
    double tip[4][kUqBatch];     // Ta, Tb, Tc, Td
    double internode[kUqBatch];
};

struct UnequalQuartetParams {
    PiParams pi;                 // rates, cull and the chunk map; pi.partial is not used
    const LocusModel* models;
    int32_t f81;                 // the plan's models are F81: the closed form e I + (1 - e) Pi
    int32_t n_q;                 // quartets of the whole call (row pitch of partial / sites)
    int32_t q0, nq;              // this launch: quartets q0 .. q0 + nq - 1 = the entries 0 .. nq - 1 of the batch
    double* partial;             // [nchunks][n_q][9]
    double* sites;               // [3][n_q][ncols]
    int64_t ncols;
};

// (y, x1, x2) of one live site.  C and D are held whole (32 doubles); of A, B and N only what all rows of a matrix share
// (transition_exps: three numbers each), and row u of each is made where u needs it.  Per u: n C (16 products), R_u (16
// products + 48 fma), the three contributions.
__device__ __forceinline__ void uquartet_signal_noise(const LocusModel& m, bool f81, double r, double ta, double tb, double tc,
                                                      double td, double to, double& y, double& x1, double& x2) {
#pragma clang fp contract(off)
    double eA[3], eB[3], eN[3], e[3], C[16], D[16];
    transition_exps(m, f81, transition_scale(m, r, ta), eA);
    if (tb == ta) {                  // (wave-uniform; the rule on an ultrametric tree) the same three numbers, not made twice
        eB[0] = eA[0]; eB[1] = eA[1]; eB[2] = eA[2];
    } else {
        transition_exps(m, f81, transition_scale(m, r, tb), eB);
    }
    transition_exps(m, f81, transition_scale(m, r, to), eN);
    transition_exps(m, f81, transition_scale(m, r, tc), e);
#pragma unroll
    for (int i = 0; i < 4; ++i) transition_row(m, f81, e, i, C + 4 * i);
    transition_exps(m, f81, transition_scale(m, r, td), e);
#pragma unroll
    for (int i = 0; i < 4; ++i) transition_row(m, f81, e, i, D + 4 * i);
    double sy = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        double a[4], b[4], n[4], nC[16], R[16];
        transition_row(m, f81, eA, u, a);
        transition_row(m, f81, eB, u, b);
        transition_row(m, f81, eN, u, n);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int i = 0; i < 4; ++i) nC[4 * v + i] = n[v] * C[4 * v + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = nC[i] * D[j];
                s = fma(nC[4 + i], D[4 + j], s);
                s = fma(nC[8 + i], D[8 + j], s);
                s = fma(nC[12 + i], D[12 + j], s);
                R[4 * i + j] = s;
            }
        }
        // signal: sum_i (a_i b_i) (sum_{j != i} R_jj), the inner sums by three additions each
        const double d0 = R[0], d1 = R[5], d2 = R[10], d3 = R[15];
        double in = (a[0] * b[0]) * ((d1 + d2) + d3);
        in = fma(a[1] * b[1], (d0 + d2) + d3, in);
        in = fma(a[2] * b[2], (d0 + d1) + d3, in);
        in = fma(a[3] * b[3], (d0 + d1) + d2, in);
        sy = fma(m.pi[u], in, sy);
        // noise: the twelve pairs i != j in row order; x2 takes the transposed tip product on the same entry of R
        double i1 = 0.0, i2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i == j) continue;
                i1 = fma(a[i] * b[j], R[4 * i + j], i1);
                i2 = fma(a[j] * b[i], R[4 * i + j], i2);
            }
        }
        s1 = fma(m.pi[u], i1, s1);
        s2 = fma(m.pi[u], i2, s2);
    }
    y = sy;
    x1 = s1;
    x2 = s2;
}

// One workgroup per 1024-column chunk of a locus, a thread four columns (column = base + j * 256 + thread, as
// pi_partial_kernel).  The locus' model is wave-uniform: it is read through the scalar cache into SGPRs, once per wave.
// Quartets go through one at a time; a thread's nine running sums of the quartet live in registers while it walks its four
// columns (their rates wait in LDS, so that the walk is a loop -- one copy of the site arithmetic -- not four unrolled
// ones).  The nine sums are then added over the wave by a butterfly and over the four waves in order: a fixed shape, no
// atomics.  Static LDS: 8 KB of rates + 18 KB of wave sums.
constexpr int kUqWavesPerSimd = 2;
__global__ __launch_bounds__(kUqBlock, kUqWavesPerSimd) void uquartet_partial_kernel(UnequalQuartetParams P, UnequalQuartetBatch B) {
    __shared__ double rate[kUqColsPerThread][kUqBlock];
    __shared__ double red[kUqBatch * kUqSums][kUqBlock / 64];
    const int chunk = blockIdx.x;
    const QuartetChunk ch = quartet_chunk<kUqChunk>(P.pi);
    const int locus = ch.locus;
    const int64_t hi = ch.hi, base = ch.base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LocusModel& model = P.models[locus];
#pragma unroll
    for (int j = 0; j < kUqColsPerThread; ++j) {
        const int64_t col = base + j * kUqBlock + threadIdx.x;
        rate[j][threadIdx.x] = (col < hi) ? finalize_rate(P.pi, col) : 0.0;   // a thread reads back its own slots only
    }
    const bool f81 = P.f81 != 0;
#pragma unroll 1
    for (int q = 0; q < P.nq; ++q) {
        const double ta = B.tip[0][q], tb = B.tip[1][q], tc = B.tip[2][q], td = B.tip[3][q], to = B.internode[q];
        double s[kUqSums];
#pragma unroll
        for (int w = 0; w < kUqSums; ++w) s[w] = 0.0;
#pragma unroll 1
        for (int j = 0; j < kUqColsPerThread; ++j) {
            const double r = rate[j][threadIdx.x];
            if (!quartet_live(r)) continue;
            double y, x1, x2;
            uquartet_signal_noise(model, f81, r, ta, tb, tc, td, to, y, x1, x2);
            s[0] += y;
            s[1] += x1;
            s[2] += x2;
            s[3] = fma(y, y, s[3]);
            s[4] = fma(x1, x1, s[4]);
            s[5] = fma(x2, x2, s[5]);
            s[6] = fma(y, x1, s[6]);
            s[7] = fma(y, x2, s[7]);
            s[8] = fma(x1, x2, s[8]);
        }
#pragma unroll
        for (int w = 0; w < kUqSums; ++w) {
            const double v = wave_sum(s[w]);
            if (lane == 0) red[q * kUqSums + w][wave] = v;
        }
    }
    __syncthreads();
    double* out = P.partial + ((size_t)chunk * P.n_q + P.q0) * kUqSums;
    for (int w = threadIdx.x; w < P.nq * kUqSums; w += kUqBlock) out[w] = ((red[w][0] + red[w][1]) + red[w][2]) + red[w][3];
}

// Dense per-site values: sites[0][q][col] = y, sites[1][q][col] = x1, sites[2][q][col] = x2; a thread is one column at a
// time and walks the batch's quartets.  Culled and zero-rate columns get exactly 0.
__global__ __launch_bounds__(kUqBlock, kUqWavesPerSimd) void uquartet_sites_kernel(UnequalQuartetParams P, UnequalQuartetBatch B) {
    const QuartetChunk ch = quartet_chunk<kUqChunk>(P.pi);
    const int locus = ch.locus;
    const int64_t hi = ch.hi, base = ch.base;
    const LocusModel& model = P.models[locus];
    const bool f81 = P.f81 != 0;
    const size_t plane = (size_t)P.n_q * (size_t)P.ncols;
#pragma unroll 1
    for (int j = 0; j < kUqColsPerThread; ++j) {
        const int64_t col = base + j * kUqBlock + threadIdx.x;
        if (col >= hi) continue;
        const double r = finalize_rate(P.pi, col);
        const bool live = quartet_live(r);
#pragma unroll 1
        for (int q = 0; q < P.nq; ++q) {
            double y = 0.0, x1 = 0.0, x2 = 0.0;
            if (live) uquartet_signal_noise(model, f81, r, B.tip[0][q], B.tip[1][q], B.tip[2][q], B.tip[3][q], B.internode[q], y, x1, x2);
            double* o = P.sites + (size_t)(P.q0 + q) * P.ncols + col;
            o[0] = y;
            o[plane] = x1;
            o[2 * plane] = x2;
        }
    }
}

// ---- resolution probabilities: uquartet_probabilities() of unequal_quartet_probabilities.hpp ------------------------

// One workgroup per locus: the nine sums of every quartet over the locus' chunks in ascending order, then the four
// probabilities, a thread per quartet.  rows [L][n_q][13].
__global__ __launch_bounds__(kUqReduceBlock) void uquartet_reduce_kernel(const double* __restrict__ partial,
                                                                        const int64_t* __restrict__ locus_chunk_offsets, int32_t n_q,
                                                                        double* __restrict__ rows) {
    const int locus = blockIdx.x;
    const int64_t c0 = locus_chunk_offsets[locus], c1 = locus_chunk_offsets[locus + 1];
    const int Wp = n_q * kUqSums;
    double* row = rows + (size_t)locus * n_q * kUqRow;
    for (int w = threadIdx.x; w < Wp; w += kUqReduceBlock) {
        double s = 0.0;
        for (int64_t c = c0; c < c1; ++c) s += partial[(size_t)c * Wp + w];
        row[(w / kUqSums) * kUqRow + (w % kUqSums)] = s;
    }
    __syncthreads();   // a quartet's nine sums were written by up to nine threads of this workgroup
    for (int q = threadIdx.x; q < n_q; q += kUqReduceBlock) {
        double* o = row + q * kUqRow;
        uquartet_probabilities(o);
    }
}

}  // namespace tphip

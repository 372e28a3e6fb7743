// bootstrap_kernels.hpp -- site bootstrap of the per-locus PI rows.
//
// A column's final rate depends on the column and the locus' model only, so an alignment resampled with replacement has
// the same per-site rates with multiplicities: replicate b of a locus' PI row is X_b[w] = sum_i c[b][i] p_i[w], c the
// multinomial counts and p_i site i's row of PI values (net PI at t = 0..T-1, then one integral per interval).  All
// replicates of a locus are one [B x n] . [n x (T + n_i)] FP64 matrix product.
//
// bootstrap_draw_kernel       counts from a counter-based generator (Philox4x32-10): every draw is addressed by
//                             (seed, locus id, replicate, draw index) and nothing depends on the launch geometry
// bootstrap_integrals_kernel  per-site interval integrals, once per block of loci (never per replicate)
// bootstrap_matrix_kernel     the product, v_mfma_f64_16x16x4_f64: A = counts as f64 (exact integers), B = site values
//                             generated per 32-column chunk into LDS with the time-tile recurrence of pi_partial_kernel
// bootstrap_summary_kernel    mean, sd, and two quantiles per (locus, entry) from the B replicate values, sorted in LDS
//
// Determinism: a replicate row is accumulated over the locus' columns in ascending order, in k-steps of four counted
// from the locus' first column with a zero-padded tail, by one wave, without atomics on FP64.  It therefore depends on the
// seed, the locus id, the replicate, the locus' final rates and the schedule -- not on the other loci, on B, on how the
// host blocks loci and replicate ranges to fit its workspace, or on the GPU count.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "band_blocks.hpp"
#include "philox4x32.hpp"
#include "pi_rate.hpp"
#include "quadpack_device.hpp"
#include "tphip.h"

namespace tphip {

constexpr int kBsBlock = 256;                 // threads of the matrix kernel: four waves
constexpr int kBsChunk = 32;                  // columns staged per pass through LDS (eight k-steps of four)
constexpr int kBsSub = 8;                     // 16-entry output sub-tiles per workgroup
constexpr int kBsOutTile = 16 * kBsSub;       // 128 output entries per workgroup
constexpr int kBsWaveReps = 32;               // replicates per wave: two 16-row MFMA tiles that share every B operand
constexpr int kBsRepTile = 4 * kBsWaveReps;   // 128 replicates per workgroup
constexpr int kBsPitch = 129;                 // doubles per staged column: odd, so that the 32 columns a wave writes at one
                                              // entry index fall into 32 different bank pairs
constexpr int kBsDrawBlock = 256;

// ---- generator: philox4x32.hpp (plain C++, so that a host program can pin it to the known answers) ----------------
struct DrawParams {
    const int64_t* locus_offsets;  // plan's [L+1] column offsets, or null: one locus of `single_n` columns
    const int64_t* locus_ids;      // [L] (device), or null: the locus index (or `single_id`)
    int64_t single_n, single_id;
    int32_t locus0;                // first locus of the block
    int32_t nrep;                  // replicates of the block
    int64_t rep0;                  // global index of the block's first replicate
    uint64_t seed;
    uint32_t* words;               // counts of the block as packed pairs of 16-bit counters, zeroed by the caller
    int64_t pitch;                 // 16-bit counters per replicate row (even)
    int64_t col_base;              // plan column that sits at index 0 of a row
};

// One thread per Philox call = two draws.  grid.x = block loci x block replicates, grid.y covers the draw index.
// The counts are scattered with 32-bit integer atomics on the packed words: exact whatever the order.
// (These atomics are the larger part of the call on long loci -- profiles/r07_bootstrap_timing.txt; counting per row tile
// in LDS is the next step)
__global__ __launch_bounds__(kBsDrawBlock) void bootstrap_draw_kernel(DrawParams P) {
    const int64_t li = blockIdx.x / (unsigned)P.nrep, rb = blockIdx.x % (unsigned)P.nrep;
    const int64_t locus = P.locus0 + li;
    const int64_t lo = P.locus_offsets ? P.locus_offsets[locus] : 0;
    const uint64_t n = P.locus_offsets ? (uint64_t)(P.locus_offsets[locus + 1] - lo) : (uint64_t)P.single_n;
    const uint64_t j = (uint64_t)blockIdx.y * kBsDrawBlock + threadIdx.x;
    if (2 * j >= n) return;
    const uint64_t id = P.locus_offsets ? (P.locus_ids ? (uint64_t)P.locus_ids[locus] : (uint64_t)locus) : (uint64_t)P.single_id;
    uint64_t d0, d1;
    bootstrap_draw_pair(P.seed, id, (uint32_t)(P.rep0 + rb), (uint32_t)j, n, &d0, &d1);
    const int64_t row = rb * P.pitch + (lo - P.col_base);
    int64_t e = row + (int64_t)d0;
    atomicAdd(P.words + (e >> 1), 1u << (16 * (int)(e & 1)));
    if (2 * j + 1 < n) {   // an odd locus discards its last draw
        e = row + (int64_t)d1;
        atomicAdd(P.words + (e >> 1), 1u << (16 * (int)(e & 1)));
    }
}

// ---- per-site integrals ------------------------------------------------------------------------------------------
// integ[(col - col0) * n_i + k] = the integral of site `col` over interval k, 0 for a culled or constant column: the
// device functions and the fast-path choice of pi_partial_kernel (pi_kernels.hpp) under the plan's integ_mode.
__global__ __launch_bounds__(128) void bootstrap_integrals_kernel(PiParams P, int64_t col0, int64_t ncols, double* __restrict__ integ) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncols) return;
    const double r = finalize_rate(P, col0 + i);
    const bool ok = isfinite(r) && r != 0.0;
    double* out = integ + (size_t)i * P.n_i;
    GkFactors F;
    double have_h = -1.0;
    for (int k = 0; k < P.n_i; ++k) {
        double res = 0.0, err = 0.0;
        if (ok) {
            const double a = (double)P.intervals[2 * k], b = (double)P.intervals[2 * k + 1];
            if (P.integ_mode == TPHIP_INTEG_QUADPACK) {
                const double hl = 0.5 * (b - a);
                if (4.0 * r * hl < 30.0) {
                    if (hl != have_h) { gk_factors(r, hl, F); have_h = hl; }
                    quad_townsend_factored(a, b, r, F, res, err);
                } else {
                    quad_townsend<false>(a, b, r, nullptr, res, err);
                }
            } else {
                res = integral_closed(a, b, r);
            }
        }
        out[k] = res;
    }
}

// ---- the matrix product ------------------------------------------------------------------------------------------
struct BootMatParams {
    PiParams pi;             // rates, nres, offsets, schedule (chunk tables and `partial` unused)
    const uint16_t* counts;  // [nrep][count_pitch]
    int64_t count_pitch;
    int64_t col_base;        // plan column at index 0 of a counts row
    const double* integ;     // [columns from integ_col_base on][n_i] (bootstrap_integrals_kernel)
    int64_t integ_col_base;
    double* rows;            // [block loci][rows_reps][Wb]
    int64_t rows_reps;       // replicates per locus in `rows`
    int64_t rows_rep0;       // where this launch's first replicate sits among them
    int32_t locus0;          // first locus of the block
    int32_t nrep;            // replicates of this launch
    int32_t Tp;              // T rounded up to 16: internal entry index wi < Tp is the time wi, wi >= Tp interval wi - Tp
};

typedef double bs_f64x4 __attribute__((ext_vector_type(4)));

// A workgroup owns (locus, 128 replicates, 128 entries).  Operand layout of v_mfma_f64_16x16x4_f64, lane l:
// A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15], four results D[row = (l >> 4) + 4 v][col = l & 15], v = 0..3
// (confirmed with one-hot counts by tests/test_gpu_bootstrap.py).  Rows are replicates, k the locus' columns, D's columns
// entries.  Per 32-column chunk: every lane fetches its 2 x 8 counts, thread (column c, sub-tile j) writes the 16 values of
// column c in sub-tile j to LDS -- 32 x 8 = 256 tasks, one per thread -- and every wave then issues 8 k-steps x 8 sub-tiles x
// 2 replicate tiles of MFMA on operands that the four waves (eight replicate tiles) share.
__global__ __launch_bounds__(kBsBlock) void bootstrap_matrix_kernel(BootMatParams P) {
    __shared__ double vals[kBsChunk * kBsPitch];
    const int locus = P.locus0 + (int)blockIdx.x;
    const int64_t lo = P.pi.locus_offsets[locus], hi = P.pi.locus_offsets[locus + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, m = lane & 15;
    const int rep_base = (int)blockIdx.y * kBsRepTile + wave * kBsWaveReps;
    const int o0 = (int)blockIdx.z * kBsOutTile;
    const int Wi = P.Tp + P.pi.n_i;
    const int nsub = min(kBsSub, (Wi - o0 + 15) >> 4);
    const bool tile_on[2] = {rep_base < P.nrep, rep_base + 16 < P.nrep};   // wave-uniform
    bs_f64x4 acc[2][kBsSub];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int j = 0; j < kBsSub; ++j) acc[rt][j] = (bs_f64x4){0.0, 0.0, 0.0, 0.0};
    const int gc = threadIdx.x & 31, gj = threadIdx.x >> 5;   // this thread's part of the chunk's values
    for (int64_t base = lo; base < hi; base += kBsChunk) {
        // A operands: the counts of replicate (rep_base + 16 rt + m) at columns base + 4 s + q; 0 beyond the locus
        // and beyond the last replicate (nothing is read there)
        uint16_t cnt[2][8];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const int rep = rep_base + 16 * rt + m;
            const uint16_t* crow = P.counts + (int64_t)rep * P.count_pitch + (base - P.col_base);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int64_t col = base + 4 * s + q;
                cnt[rt][s] = (rep < P.nrep && col < hi) ? crow[4 * s + q] : (uint16_t)0;
            }
        }
        if (gj < nsub) {
            const int64_t col = base + gc;
            double* dst = vals + gc * kBsPitch + 16 * gj;
            const double r = (col < hi) ? finalize_rate(P.pi, col) : 0.0;
            const bool ok = isfinite(r) && r != 0.0;   // a NaN or zero rate has an all-zero row, as in nansum
            const int wi0 = o0 + 16 * gj;
            if (!ok) {
#pragma unroll
                for (int i = 0; i < 16; ++i) dst[i] = 0.0;
            } else if (wi0 < P.Tp) {
                // 16 r^2 t e^{-4rt} at t = wi0 .. wi0 + 15 by the time-tile recurrence of pi_partial_kernel
                const double c = 16.0 * (r * r);
                const double e1 = exp(-(4.0 * r));
                double p = exp(-(4.0 * r * (double)wi0));
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    dst[i] = (c * (double)(wi0 + i)) * p;
                    p *= e1;
                }
            } else {
                const double* src = P.integ + (size_t)(col - P.integ_col_base) * P.pi.n_i;
                const int k0 = wi0 - P.Tp;
#pragma unroll
                for (int i = 0; i < 16; ++i) dst[i] = (k0 + i < P.pi.n_i) ? src[k0 + i] : 0.0;
            }
        }
        __syncthreads();
        if (tile_on[0]) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const double a0 = (double)cnt[0][s], a1 = (double)cnt[1][s];
                const double* brow = vals + (4 * s + q) * kBsPitch + m;
#pragma unroll
                for (int j = 0; j < kBsSub; ++j) {
                    if (j < nsub) {
                        const double b = brow[16 * j];
                        acc[0][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][j], 0, 0, 0);
                        if (tile_on[1]) acc[1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][j], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    const int Wb = P.pi.T + P.pi.n_i;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
        for (int j = 0; j < kBsSub; ++j) {
            if (j >= nsub) continue;
            const int wi = o0 + 16 * j + m;
            int w = -1;
            if (wi < P.Tp) { if (wi < P.pi.T) w = wi; }
            else if (wi - P.Tp < P.pi.n_i) w = P.pi.T + (wi - P.Tp);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rep = rep_base + 16 * rt + q + 4 * v;
                if (w >= 0 && rep < P.nrep)
                    P.rows[((size_t)blockIdx.x * P.rows_reps + P.rows_rep0 + rep) * Wb + w] = acc[rt][j][v];
            }
        }
    }
}

// ---- summary -----------------------------------------------------------------------------------------------------
struct SummaryParams {
    const double* rows;    // [block loci][B][Wb]
    double* summary;       // [block loci][4][Wb]: mean, sd, lo, hi
    int32_t B, Wb, npow2;  // npow2: B rounded up to a power of two (the sort's length)
    // numpy's default (linear) quantile rule, prepared on the host: index of the lower neighbour and the weight of the upper
    int32_t idx_lo, idx_hi;
    double frac_lo, frac_hi;
};

// numpy's _lerp: a + (b - a) t, from the other end for t >= 0.5
__device__ __forceinline__ double numpy_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double d = b - a;
    return (t >= 0.5) ? b - d * (1.0 - t) : a + d * t;
}

// One workgroup per (locus, entry): the B values go to LDS, are sorted (bitonic, padded with +inf), and are summed in a
// fixed order -- thread t adds the sorted values t, t + 256, ... and a fixed tree adds the 256 partial sums -- so the
// result depends on the multiset of values only.  sd is two-pass with B - 1 in the denominator.
__global__ __launch_bounds__(256) void bootstrap_summary_kernel(SummaryParams P) {
    __shared__ double v[kBandMaxReplicates];
    __shared__ double red[256];
    const int li = blockIdx.x / (unsigned)P.Wb, w = blockIdx.x % (unsigned)P.Wb;
    const double* src = P.rows + (size_t)li * P.B * P.Wb + w;
    for (int b = threadIdx.x; b < P.npow2; b += 256)
        v[b] = (b < P.B) ? src[(size_t)b * P.Wb] : __longlong_as_double(0x7ff0000000000000ll);
    __syncthreads();
    for (int k = 2; k <= P.npow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P.npow2; i += 256) {
                const int o = i ^ j;
                if (o > i) {
                    const double a = v[i], b = v[o];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { v[i] = b; v[o] = a; }
                }
            }
            __syncthreads();
        }
    }
    auto block_sum = [&](double mine) {
        red[threadIdx.x] = mine;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        const double tot = red[0];
        __syncthreads();
        return tot;
    };
    double s = 0.0;
    for (int b = threadIdx.x; b < P.B; b += 256) s += v[b];
    const double mean = block_sum(s) / (double)P.B;
    double d2 = 0.0;
    for (int b = threadIdx.x; b < P.B; b += 256) { const double d = v[b] - mean; d2 += d * d; }
    const double var = block_sum(d2) / (double)(P.B - 1);
    if (threadIdx.x == 0) {
        double* out = P.summary + (size_t)li * 4 * P.Wb + w;
        out[0] = mean;
        out[(size_t)P.Wb] = sqrt(var);
        out[(size_t)2 * P.Wb] = numpy_lerp(v[P.idx_lo], v[min(P.idx_lo + 1, P.B - 1)], P.frac_lo);
        out[(size_t)3 * P.Wb] = numpy_lerp(v[P.idx_hi], v[min(P.idx_hi + 1, P.B - 1)], P.frac_hi);
    }
}

}  // namespace tphip

// posterior_pi_kernels.hpp -- the empirical-Bayes rate posterior carried into the per-locus PI rows.
//
// Given the fitted (mu_l, alpha_l) a site of locus l has one of K rates r_lk only, so the locus has K distinct per-site PI
// rows P_l[k][.] and a posterior draw of its row is sum_k N_k P_l[k][.], N_k = the live sites drawn into category k: the
// image of a Poisson-multinomial count vector.  No per-site x per-time table is formed anywhere.
//
// posterior_normalize_kernel      p_ck from the f_k + log w_k the table variant of the mixture kernel left (in place)
// posterior_category_rows_kernel  r_lk and P_l[k][w], w < Wb = T + n_i, by the device functions of the PI tables
// posterior_moments_kernel        n_lk = sum_c p_ck, mean[w] = sum_k n_lk P[k][w], var[w] = sum_c Var_k(P[k][w] | c)
// posterior_draw_kernel           the hot path: B x ncols categorical draws (Philox4x32-10) counted per category
// posterior_rows_kernel           X_b = N_b . P_l
//
// Determinism: every floating-point sum runs over the locus' own columns (or categories) in a fixed order, without
// floating-point atomics; the draw of (column, replicate) is addressed by (seed, locus id, replicate, column index within
// the locus) and the counts are integers.  A locus' outputs therefore do not depend on the other loci, on B, on the
// workspace, on how the host blocks loci or cuts a locus into column segments, or on the GPU count.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gtr_model.hpp"
#include "philox4x32.hpp"
#include "pi_rate.hpp"
#include "quadpack_device.hpp"
#include "tphip.h"

namespace tphip {

constexpr int kPpMaxCat = 16;       // K's limit (that of the mixture kernel)
constexpr int kPpBlock = 256;       // threads of the moments and rows kernels; the draw kernel's at most
constexpr int kPpTile = 256;        // columns whose thresholds one pass of the draw kernel stages in LDS: a multiple of 4
                                    // (a Philox block serves four columns), 30 KB at K = 16
constexpr int kPpWTile = 64;        // entries of the row a workgroup of the moments kernel owns: one per lane
constexpr int kPpColWaves = kPpBlock / kPpWTile;   // its waves take the locus' columns in turn: part of the summation order

// ---- category posterior ------------------------------------------------------------------------------------------
// post holds logp[k][c] = f_k + log w_k of the representatives (the table variant of site_posterior_body).  Pass 0 turns a
// representative's column into e_k = exp(logp_k - f_c), p_k = e_k / sum_k e_k (the division makes the column sum to 1
// within rounding whatever |f_c| is); pass 1, a launch of its own, copies representatives to their repeats, as
// eb_finish_kernel does for the moments.  Chunks of 1024 columns of one locus: the PI chunk tables.
__global__ __launch_bounds__(256) void posterior_normalize_kernel(const int64_t* __restrict__ locus_offsets,
                                                                  const int32_t* __restrict__ chunk_locus,
                                                                  const int32_t* __restrict__ chunk_index,
                                                                  const int32_t* __restrict__ dup_of, const double* __restrict__ f,
                                                                  double* post, int32_t K, int64_t ncols_total, int32_t pass) {
    const int locus = chunk_locus[blockIdx.x];
    const int64_t hi = locus_offsets[locus + 1];
    const int64_t base = locus_offsets[locus] + (int64_t)chunk_index[blockIdx.x] * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t c = base + j * 256 + threadIdx.x;
        if (c >= hi) continue;
        const int32_t r = dup_of[c];
        if (pass == 0) {
            if (r >= 0) continue;
            const double fc = f[c];
            double s = 0.0;
            for (int k = 0; k < K; ++k) {
                const double e = exp(post[(int64_t)k * ncols_total + c] - fc);
                post[(int64_t)k * ncols_total + c] = e;
                s += e;
            }
            for (int k = 0; k < K; ++k) post[(int64_t)k * ncols_total + c] = post[(int64_t)k * ncols_total + c] / s;
        } else {
            if (r < 0) continue;
            for (int k = 0; k < K; ++k) post[(int64_t)k * ncols_total + c] = post[(int64_t)k * ncols_total + (int64_t)r];
        }
    }
}

// ---- what the kernels below share --------------------------------------------------------------------------------
struct PostPiParams {
    PiParams pi;                  // nres (may be null: no cull), offsets, schedule, rounding and correction; `rates` unused
    const LocusModel* models;     // kappa
    const double* scale;          // [nloci] mu
    const double* cat_rate;       // [nloci][K] rho
    const double* post;           // [K][ncols_total] p_ck
    int64_t ncols_total;
    int32_t K;
    int32_t locus0;               // first locus of the block
    int32_t B;
    double* ptab;                 // [block loci][K][Wb]
    double* analytic;             // [nloci][2][Wb] mean, sd
    double* expected;             // [nloci][K]
    const int32_t* counts;        // [block loci][B][K]
    double* rows;                 // [block loci][B][Wb]
};

__device__ __forceinline__ bool pp_live(const PiParams& P, int64_t col) { return !P.nres || P.nres[col] >= P.threshold; }

// r_lk: the plan's finalisation of the raw rate (kappa mu) rho_k -- finalize_rate's round trip and /correction
__device__ __forceinline__ double pp_category_rate(const PostPiParams& P, int locus, int k) {
#pragma clang fp contract(off)
    double r = (P.models[locus].kappa * P.scale[locus]) * P.cat_rate[(int64_t)locus * P.K + k];
    if (P.pi.round_scale > 0.0) r = round_like_printf(r, P.pi.round_scale);
    return r / P.pi.correction;
}

// ---- category rows -----------------------------------------------------------------------------------------------
// One workgroup per locus.  P[k][t] = 16 r^2 t e^(-4rt), t < T; P[k][T + i] = the integral over interval i with the
// fast-path choice of bootstrap_integrals_kernel under the plan's integ_mode.  A non-finite or zero rate has an all-zero row.
__global__ __launch_bounds__(kPpBlock) void posterior_category_rows_kernel(PostPiParams P) {
    __shared__ double rk[kPpMaxCat];
    const int li = blockIdx.x, locus = P.locus0 + li;
    const int K = P.K, T = P.pi.T, n_i = P.pi.n_i, Wb = T + n_i;
    if ((int)threadIdx.x < K) rk[threadIdx.x] = pp_category_rate(P, locus, threadIdx.x);
    __syncthreads();
    double* out = P.ptab + (size_t)li * K * Wb;
    for (int i = threadIdx.x; i < K * T; i += kPpBlock) {
        const int k = i / T, t = i % T;
        const double r = rk[k];
        const bool ok = isfinite(r) && r != 0.0;
        out[(size_t)k * Wb + t] = ok ? (16.0 * (r * r) * (double)t) * exp(-(4.0 * r * (double)t)) : 0.0;
    }
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        const double r = rk[k];
        const bool ok = isfinite(r) && r != 0.0;
        GkFactors F;
        double have_h = -1.0;
        for (int i = 0; i < n_i; ++i) {
            double res = 0.0, err = 0.0;
            if (ok) {
                const double a = (double)P.pi.intervals[2 * i], b = (double)P.pi.intervals[2 * i + 1];
                if (P.pi.integ_mode == TPHIP_INTEG_QUADPACK) {
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
            out[(size_t)k * Wb + T + i] = res;
        }
    }
}

// ---- expected counts and analytic moments ------------------------------------------------------------------------
// Workgroup (locus, tile of 64 entries).  n_lk: thread t adds the live columns t, t + 256, ... of the locus in sequence,
// then a binary tree over the 256 partial sums (the order of locus_marginal_reduce_kernel).  Variance: wave g takes the live
// columns g, g + 4, ... in sequence, lane = entry w; a column's term is sum_k p_k (P[k][w] - a)^2 with a = sum_k p_k P[k][w]
// -- the centred form of sum_k p_k P^2 - a^2, which cannot go negative and loses nothing where the posterior is narrow --
// and the four waves' sums are added in ascending g.  Every multiply-add is an explicit fma.
__global__ __launch_bounds__(kPpBlock) void posterior_moments_kernel(PostPiParams P) {
#pragma clang fp contract(off)
    __shared__ double ptile[kPpMaxCat][kPpWTile];
    __shared__ double red[kPpBlock];
    __shared__ double nk[kPpMaxCat];
    const int li = blockIdx.x, locus = P.locus0 + li;
    const int K = P.K, Wb = P.pi.T + P.pi.n_i;
    const int w0 = (int)blockIdx.y * kPpWTile;
    const int64_t lo = P.pi.locus_offsets[locus], hi = P.pi.locus_offsets[locus + 1];
    const double* tab = P.ptab + (size_t)li * K * Wb;
    for (int i = threadIdx.x; i < K * kPpWTile; i += kPpBlock) {
        const int k = i / kPpWTile, j = i % kPpWTile;
        ptile[k][j] = (w0 + j < Wb) ? tab[(size_t)k * Wb + w0 + j] : 0.0;
    }
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int64_t c = lo + threadIdx.x; c < hi; c += kPpBlock)
            if (pp_live(P.pi, c)) s += P.post[(int64_t)k * P.ncols_total + c];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = kPpBlock / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) nk[k] = red[0];
        __syncthreads();
    }
    if (blockIdx.y == 0 && (int)threadIdx.x < K) P.expected[(size_t)locus * K + threadIdx.x] = nk[threadIdx.x];
    const int j = threadIdx.x % kPpWTile, g = threadIdx.x / kPpWTile;
    double v = 0.0;
    for (int64_t c = lo + g; c < hi; c += kPpColWaves) {   // wave-uniform
        if (!pp_live(P.pi, c)) continue;
        double a = 0.0;
        for (int k = 0; k < K; ++k) a = fma(P.post[(int64_t)k * P.ncols_total + c], ptile[k][j], a);
        double t = 0.0;
        for (int k = 0; k < K; ++k) {
            const double d = ptile[k][j] - a;
            t = fma(P.post[(int64_t)k * P.ncols_total + c], d * d, t);
        }
        v += t;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    if (g == 0 && w0 + j < Wb) {
        double var = red[j];
        for (int q = 1; q < kPpColWaves; ++q) var += red[q * kPpWTile + j];
        double m = 0.0;
        for (int k = 0; k < K; ++k) m = fma(nk[k], ptile[k][j], m);
        double* out = P.analytic + (size_t)locus * 2 * Wb + w0 + j;
        out[0] = m;
        out[Wb] = sqrt(var);
    }
}

// ---- draw and count ----------------------------------------------------------------------------------------------
struct PostDrawParams {
    const int64_t* locus_offsets;
    const int64_t* locus_ids;     // [nloci] (device) or null: the locus index
    const int32_t* nres;          // may be null: no cull
    int32_t threshold;
    const double* post;           // [K][ncols_total]
    int64_t ncols_total;
    int32_t K;
    int32_t locus0;               // first locus of the block
    int32_t B;
    int32_t seg_cols;             // columns per segment (grid.z): a multiple of kPpTile
    uint64_t seed;
    int32_t* counts;              // [block loci][B][K], zeroed by the caller
};

// Workgroup (replicate tile, locus, column segment); thread = replicate.  The segment's columns stream through LDS in tiles
// of kPpTile as their K - 1 thresholds d_k = c_k 2^32 - 0.5, c_k the fp64 running sum p_0 + ... + p_k added in that order
// while staging: for a 32-bit word x, (x + 0.5) 2^-32 >= c_k exactly when (double)x >= d_k (both sides of the first are
// exact in fp64; c_k 2^32 - 0.5 is exact from c_k 2^32 >= 1 on, and below that its rounding keeps the sign, which is all an
// integer x >= 0 asks of it).  A culled column, a column beyond the segment and the thresholds from K - 1 up to KM - 1 are
// +inf: their words are consumed and nothing is counted.  Every thread reads the same column at a time (a broadcast read),
// runs one Philox block per four columns -- counter (j, b, id lo, id hi), word i for the column 4j + i of the locus -- and
// keeps the KM - 1 counters G_k = #{live columns: x >= d_k} in registers; N_k = G_(k-1) - G_k with G_(-1) the live columns of
// the segment, so no register array is indexed dynamically.  Segments add their integer counts with atomics: exact in any
// order.  KM = 2, 4, 8, 16: the smallest that holds K.
template <int KM>
__global__ __launch_bounds__(kPpBlock) void posterior_draw_kernel(PostDrawParams P) {
    __shared__ double thr[kPpTile * (KM - 1)];
    __shared__ int s_live;
    const int li = blockIdx.y, locus = P.locus0 + li;
    const int64_t lo = P.locus_offsets[locus];
    const int64_t n = P.locus_offsets[locus + 1] - lo;
    const int64_t seg0 = (int64_t)blockIdx.z * P.seg_cols;
    if (seg0 >= n) return;   // workgroup-uniform
    const int64_t seg1 = (seg0 + P.seg_cols < n) ? seg0 + P.seg_cols : n;
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool active = b < P.B;
    const uint64_t id = P.locus_ids ? (uint64_t)P.locus_ids[locus] : (uint64_t)locus;
    const int K = P.K;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    if (threadIdx.x == 0) s_live = 0;
    int G[KM - 1];
#pragma unroll
    for (int k = 0; k < KM - 1; ++k) G[k] = 0;
    for (int64_t t0 = seg0; t0 < seg1; t0 += kPpTile) {
        __syncthreads();   // the tile before is consumed (and s_live is zero before the first)
        for (int i = threadIdx.x; i < kPpTile; i += blockDim.x) {
            const int64_t c = t0 + i;
            const bool live = c < seg1 && (!P.nres || P.nres[lo + c] >= P.threshold);
            double run = 0.0;
#pragma unroll
            for (int k = 0; k < KM - 1; ++k) {
                double d = inf;
                if (live && k < K - 1) {
                    run += P.post[(int64_t)k * P.ncols_total + lo + c];
                    d = run * 4294967296.0 - 0.5;
                }
                thr[i * (KM - 1) + k] = d;
            }
            if (live) atomicAdd(&s_live, 1);
        }
        __syncthreads();
        if (active) {
            const int ncol = (int)((seg1 - t0 < kPpTile) ? seg1 - t0 : kPpTile);
            for (int q = 0; q < ncol; q += 4) {
                uint32_t x[4] = {(uint32_t)((t0 + q) >> 2), (uint32_t)b, (uint32_t)id, (uint32_t)(id >> 32)};
                philox4x32_10(x, (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double xd = (double)x[i];
                    const double* d = thr + (q + i) * (KM - 1);
#pragma unroll
                    for (int k = 0; k < KM - 1; ++k) G[k] += (xd >= d[k]) ? 1 : 0;
                }
            }
        }
    }
    if (!active) return;
    const int nlive = s_live;   // complete: every thread passed the barrier after the last tile's staging
    int32_t* out = P.counts + ((size_t)li * P.B + b) * K;
    int prev = nlive;
#pragma unroll
    for (int k = 0; k < KM - 1; ++k) {   // G_k = 0 from k = K - 1 on
        if (k < K && prev - G[k] != 0) atomicAdd(out + k, prev - G[k]);
        prev = G[k];
    }
    if (KM - 1 < K && prev != 0) atomicAdd(out + (KM - 1), prev);
}

// ---- rows --------------------------------------------------------------------------------------------------------
// X_b[w] = sum_k N_b[k] P[k][w], explicit fma in ascending k; one thread per (replicate, entry) of a locus
__global__ __launch_bounds__(kPpBlock) void posterior_rows_kernel(PostPiParams P) {
#pragma clang fp contract(off)
    const int li = blockIdx.x;
    const int K = P.K, Wb = P.pi.T + P.pi.n_i;
    const int64_t e = (int64_t)blockIdx.y * kPpBlock + threadIdx.x;
    if (e >= (int64_t)P.B * Wb) return;
    const int b = (int)(e / Wb), w = (int)(e % Wb);
    const int32_t* cnt = P.counts + ((size_t)li * P.B + b) * K;
    const double* tab = P.ptab + (size_t)li * K * Wb + w;
    double x = 0.0;
    for (int k = 0; k < K; ++k) x = fma((double)cnt[k], tab[(size_t)k * Wb], x);
    P.rows[((size_t)li * P.B + b) * Wb + w] = x;
}

}  // namespace tphip

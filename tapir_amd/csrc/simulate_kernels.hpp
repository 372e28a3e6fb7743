// simulate_kernels.hpp -- parametric bootstrap of the site rates: alignment columns simulated down
// the plan's tree under the locus' fitted model at the site's fitted rate, and the running moments of the re-estimated
// rates.  Included by simulate_driver.hip only (a __global__ definition must live in one translation unit).
//
// simulate_columns_kernel  one thread per column: root state from pi, then every node from nnodes - 1 down to 0 (post-order
//                          numbering: parents before children) draws its state from the row of exp(Q r t / kappa) that
//                          its parent's state selects (transition_row.hpp, the quartet kernels' expm1 form)
// rate_moments_kernel      Welford update of mean and sum of squared deviations of a column's final rate, one replicate
//                          per launch in replicate order
//
// Random numbers: Philox4x32-10 (philox4x32.hpp), key ((seed & 0xffffffff) ^ 0x73696D75, seed >> 32), counter
// (i, b | ((d >> 1) << 16), id & 0xffffffff, id >> 32) for column i of the locus with stream id `id`, replicate b and node d;
// u = (((x1 << 32) | x0) >> 11) 2^-53 for an even d, the same from (x3, x2) for an odd one: a call serves two nodes.  Every
// node has its draw whether its cell is masked or not, so a column's bytes depend on (seed, id, i, b, r, model, tree, the
// column's mask) alone -- not on the loci beside it or on the launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gtr_model.hpp"
#include "philox4x32.hpp"
#include "pi_rate.hpp"
#include "simulate_launch_shape.hpp"
#include "transition_row.hpp"

namespace tphip {

constexpr int kSimChunk = 1024;          // the plan's PI chunks (pi_kernels.hpp: kPiChunk): a workgroup never straddles a locus
// kSimMaxBlock, kSimMinBlock, kSimLdsBytes: simulate_launch_shape.hpp
constexpr uint32_t kSimKeyTag = 0x73696D75u;   // "simu": the stream is not the site bootstrap's
constexpr int32_t kSimMaxNodes = 1 << 17;      // (d >> 1) has 16 bits of the counter
constexpr int32_t kSimMaxReplicate = 1 << 16;  // b has the other 16

// A node as the kernel reads it, one 16-byte scalar load: pslot = the parent's slot among the internal nodes (-1: the
// root); self >= 0: a leaf, the alignment row; self < 0: an internal node with slot ~self.  Slots count the internal nodes
// in the order the kernel visits them (root = 0), so the packed words fill up front to back.
struct SimNode {
    int32_t pslot;
    int32_t self;
    double t;      // branch length above the node, as the plan has it (already / correction); the root's is not read
};
static_assert(sizeof(SimNode) == 16, "SimNode is read with one s_load_dwordx4");

struct SimParams {
    const double* rates;            // [ncols] raw rates, kappa * s: the unit of tphip_site_rates' rate
    const uint8_t* mask;            // [ntaxa][ncols] observed alignment, or null
    uint8_t* out;                   // [ntaxa][ncols]
    int64_t ncols;
    const LocusModel* models;
    const int64_t* locus_offsets;
    const int32_t* chunk_locus;
    const int32_t* chunk_index;
    const int64_t* locus_ids;       // [L] (device), or null: the locus index
    const SimNode* nodes;
    int32_t nnodes;
    int32_t f81;
    uint32_t replicate;
    uint32_t key0, key1;
};

// state by inversion: c_k the running sums of the probabilities clamped at >= 0, v = u c3, state = #{k < 3: v >= c_k}.
// A state of probability exactly 0 has c_k == c_{k-1} and is never drawn.
__device__ __forceinline__ int sim_select(const double* __restrict__ p, double u) {
#pragma clang fp contract(off)
    const double c0 = fmax(p[0], 0.0);
    const double c1 = c0 + fmax(p[1], 0.0);
    const double c2 = c1 + fmax(p[2], 0.0);
    const double c3 = c2 + fmax(p[3], 0.0);
    const double v = u * c3;
    return (int)(v >= c0) + (int)(v >= c1) + (int)(v >= c2);
}

// grid (PI chunks of the plan, 1024 / blockDim.x), blockDim.x in {64, 128, 256}: consecutive lanes take consecutive columns
// of one locus, so a leaf's row is one coalesced byte store per wave and the model, the node and the branch length are
// wave-uniform (scalar loads).  The states of the internal nodes are kept 2-bit packed in LDS, words[slot >> 4][thread]:
// a thread reads and writes its own column only -- no barrier, no bank conflict.  The word being filled is kept in a
// register and stored whole after every internal node, so no word is ever read before it was written.
// Dynamic LDS: ceil(internal nodes / 16) * blockDim.x * 4 bytes.
__global__ __launch_bounds__(kSimMaxBlock) void simulate_columns_kernel(SimParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sim_words[];
    const int chunk = blockIdx.x;
    const int locus = P.chunk_locus[chunk];
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const int64_t col = lo + (int64_t)P.chunk_index[chunk] * kSimChunk + (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (col >= hi) return;
    const LocusModel& model = P.models[locus];
    const bool f81 = P.f81 != 0;
    const uint64_t id = P.locus_ids ? (uint64_t)P.locus_ids[locus] : (uint64_t)locus;
    const uint32_t i = (uint32_t)(col - lo);
    const double r_in = P.rates[col];
    const bool bad = !(r_in >= 0.0) || isinf(r_in);   // NaN, negative, infinite: the column comes out all missing
    const double r = bad ? 0.0 : r_in;
    const unsigned bs = blockDim.x;
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    uint32_t cur = 0u;
    for (int d = P.nnodes - 1; d >= 0; --d) {
        const SimNode nd = P.nodes[d];
        if ((d & 1) || d == P.nnodes - 1) {
            x[0] = i; x[1] = P.replicate | ((uint32_t)(d >> 1) << 16); x[2] = (uint32_t)id; x[3] = (uint32_t)(id >> 32);
            philox4x32_10(x, P.key0, P.key1);
        }
        const uint64_t bits = (d & 1) ? (((uint64_t)x[3] << 32) | x[2]) : (((uint64_t)x[1] << 32) | x[0]);
        const double u = (double)(bits >> 11) * 0x1.0p-53;
        double p[4];
        if (nd.pslot < 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = model.pi[j];
        } else {
            const int px = (int)((sim_words[(unsigned)(nd.pslot >> 4) * bs + threadIdx.x] >> (2 * (nd.pslot & 15))) & 3u);
            double e[3];
            transition_exps(model, f81, transition_scale(model, r, nd.t), e);
            transition_row(model, f81, e, px, p);
        }
        const int state = sim_select(p, u);
        if (nd.self < 0) {
            const int slot = ~nd.self;
            if ((slot & 15) == 0) cur = 0u;
            cur |= (uint32_t)state << (2 * (slot & 15));
            sim_words[(unsigned)(slot >> 4) * bs + threadIdx.x] = cur;
        } else {
            const size_t cell = (size_t)nd.self * (size_t)P.ncols + (size_t)col;
            uint8_t o = (uint8_t)(1u << state);
            if (P.mask) {
                uint8_t m = P.mask[cell];
                if (m == 0) m = 15;
                if (!(m == 1 || m == 2 || m == 4 || m == 8)) o = m;   // not a single base: copied through
            }
            P.out[cell] = bad ? (uint8_t)15 : o;
        }
    }
}

struct MomentParams {
    PiParams pi;          // rates = the replicate's raw rates, nres = its informative-cell counts: finalize_rate's inputs
    int64_t ncols;
    int32_t b, B;         // this replicate, and how many there are
    double* mean;         // [ncols] running mean (in/out)
    double* m2;           // [ncols] running sum of squared deviations (in/out)
    double* out_mean;     // written after the last replicate; may be null
    double* out_sd;       // sqrt(m2 / (B - 1)); may be null
};

// Welford in replicate order, one column per thread: the result does not depend on the launch shape.  A NaN final rate (a
// culled column) makes mean and m2 NaN for good.
__global__ __launch_bounds__(256) void rate_moments_kernel(MomentParams P) {
#pragma clang fp contract(off)
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= P.ncols) return;
    const double x = finalize_rate(P.pi, col);
    double mean = P.b ? P.mean[col] : 0.0, m2 = P.b ? P.m2[col] : 0.0;
    const double d = x - mean;
    mean = mean + d / (double)(P.b + 1);
    m2 = m2 + d * (x - mean);
    P.mean[col] = mean;
    P.m2[col] = m2;
    if (P.b == P.B - 1) {
        if (P.out_mean) P.out_mean[col] = mean;
        if (P.out_sd) P.out_sd[col] = sqrt(m2 / (double)(P.B - 1));
    }
}

// rows[l][b][0..T) = the table's net PI, rows[l][b][T..T + n_i) = its interval integrals (the table row is
// [net T | times n_t | integrals n_i | errors n_i]): the layout of tphip_pi_bootstrap's replicate rows
__global__ __launch_bounds__(256) void parboot_rows_kernel(const double* __restrict__ tables, int32_t W, int32_t T, int32_t n_t, int32_t n_i,
                                                          int32_t b, int32_t B, double* __restrict__ rows) {
    const int locus = blockIdx.x, Wb = T + n_i;
    const double* src = tables + (size_t)locus * W;
    double* dst = rows + ((size_t)locus * B + b) * Wb;
    for (int w = threadIdx.x; w < Wb; w += 256) dst[w] = src[w < T ? w : w + n_t];
}

}  // namespace tphip

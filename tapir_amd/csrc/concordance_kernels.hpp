// concordance_kernels.hpp -- site concordance factors: what the alignment shows at an internode.
//
// concordance_counts_kernel: for every locus and every set of four taxon groups A, B | C, D the number of quartets
// (a, b, c, d) in A x B x C x D that the locus' columns support as ab|cd, ac|bd and ad|bc, summed over its columns.  Only cells
// that are exactly one base (mask 1, 2, 4 or 8) count; a quartet with any other cell at a column is not decisive there.  Per
// column the three numbers come from the groups' base counts in closed form,
//     conc  = (sum_x a_x b_x)(sum_y c_y d_y) - sum_x a_x b_x c_x d_x      (and the two other pairings likewise),
// in 64-bit integers; everything is integer addition, so any order gives the same bits.
//
// Lane = column.  A workgroup owns kCcChunk consecutive columns of the batch and a tile of kCcTile sets; it walks the loci that
// meet its columns, and per locus sums into an LDS table [tile][3] (one LDS atomic per wave, set and number), which it then adds
// to the output with one global 64-bit atomic per non-zero entry.  The set tables are read at wave-uniform addresses.  A set of
// four single taxa takes four cells, three comparisons and a wave ballot with a population count; any other set counts its
// groups' bases in four 16-bit fields of a 64-bit word (unpacked every 65535 taxa, so a group may be of any size).
//
// concordance_rows_kernel: the per-(locus, internode) row of 12 doubles from the counts of the internode's sets, the sums taken
// in set order by one thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tphip {

constexpr int kCcBlock = 256;       // threads of a workgroup: one strip of columns
constexpr int kCcChunk = 2048;      // columns of the batch a workgroup walks (kCcChunk / kCcBlock strips)
constexpr int kCcTile = 1024;       // sets a workgroup holds sums for: 24 KiB of LDS
constexpr int kCcPackRun = 65535;   // taxa whose base counts fit the 16-bit fields
constexpr int kCcRow = 12;          // doubles of a row

struct CcParams {
    const uint8_t* states;          // [ntaxa][row_pitch]
    int64_t ncols_total, row_pitch;
    const int64_t* locus_offsets;   // [nloci + 1]
    int64_t nloci;
    const int32_t* goff;            // [4 * n_sets + 1] into taxa
    const int32_t* taxa;            // taxon rows, validated on the host: 0..ntaxa-1
    int64_t n_sets;
    unsigned long long* counts;     // [nloci][n_sets][3], zero on entry
};

__device__ __forceinline__ bool cc_one_base(unsigned m) { return m == 1u || m == 2u || m == 4u || m == 8u; }

// 1 in the 16-bit field of the cell's base, 0 for a cell that is not exactly one base
__device__ __forceinline__ unsigned long long cc_field(unsigned m) {
    return cc_one_base(m) ? (1ull << (16 * (__ffs((int)m) - 1))) : 0ull;
}

// base counts n[0..3] of the taxa goff[g] .. goff[g + 1] at this lane's column (row = states + column)
__device__ __forceinline__ void cc_group_counts(const CcParams& P, const uint8_t* row, int32_t lo, int32_t hi, bool live, uint32_t n[4]) {
    n[0] = n[1] = n[2] = n[3] = 0;
    for (int32_t t0 = lo; t0 < hi; t0 += kCcPackRun) {
        const int32_t t1 = (hi - t0 > kCcPackRun) ? t0 + kCcPackRun : hi;
        unsigned long long w = 0;
        for (int32_t t = t0; t < t1; ++t) {
            const int64_t at = (int64_t)P.taxa[t] * P.row_pitch;
            w += live ? cc_field(row[at]) : 0ull;
        }
        n[0] += (uint32_t)(w & 0xffffu);
        n[1] += (uint32_t)((w >> 16) & 0xffffu);
        n[2] += (uint32_t)((w >> 32) & 0xffffu);
        n[3] += (uint32_t)(w >> 48);
    }
}

__device__ __forceinline__ unsigned long long cc_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kCcBlock) void concordance_counts_kernel(CcParams P) {
    __shared__ unsigned long long acc[kCcTile * 3];
    const int64_t c_lo = (int64_t)blockIdx.x * kCcChunk;
    const int64_t c_hi = (c_lo + kCcChunk < P.ncols_total) ? c_lo + kCcChunk : P.ncols_total;
    const int64_t s_lo = (int64_t)blockIdx.y * kCcTile;
    const int n_tile = (int)((P.n_sets - s_lo < kCcTile) ? P.n_sets - s_lo : kCcTile);
    if (c_lo >= c_hi || n_tile <= 0) return;
    const bool lane0 = (threadIdx.x & 63) == 0;
    // the first locus that ends beyond c_lo
    int64_t l = 0, r = P.nloci;
    while (l < r) {
        const int64_t m = (l + r) >> 1;
        if (P.locus_offsets[m + 1] > c_lo) r = m; else l = m + 1;
    }
    for (; l < P.nloci; ++l) {
        int64_t lo = P.locus_offsets[l], hi = P.locus_offsets[l + 1];
        if (lo >= c_hi) break;
        lo = lo > c_lo ? lo : c_lo;
        hi = hi < c_hi ? hi : c_hi;
        if (lo >= hi) continue;   // (wave-uniform: every thread of the workgroup takes the same way)
        for (int i = threadIdx.x; i < n_tile * 3; i += kCcBlock) acc[i] = 0;
        __syncthreads();
        for (int64_t c0 = lo; c0 < hi; c0 += kCcBlock) {
            const int64_t col = c0 + threadIdx.x;
            const bool live = col < hi;
            const uint8_t* row = P.states + (live ? col : lo);   // a dead lane points at a column of the batch and reads nothing
            for (int s = 0; s < n_tile; ++s) {
                const int32_t* g = P.goff + 4 * (s_lo + s);
                const int32_t g0 = g[0], g4 = g[4];
                if (g4 - g0 == 4) {   // four single taxa
                    unsigned a = 0, b = 0, c = 0, d = 0;
                    if (live) {
                        a = row[(int64_t)P.taxa[g0] * P.row_pitch];
                        b = row[(int64_t)P.taxa[g0 + 1] * P.row_pitch];
                        c = row[(int64_t)P.taxa[g0 + 2] * P.row_pitch];
                        d = row[(int64_t)P.taxa[g0 + 3] * P.row_pitch];
                    }
                    const bool ab = cc_one_base(a) && cc_one_base(b), ac = cc_one_base(a) && cc_one_base(c);
                    const unsigned long long k0 = __ballot(ac && a == b && c == d && a != c);
                    const unsigned long long k1 = __ballot(ab && a == c && b == d && a != b);
                    const unsigned long long k2 = __ballot(ab && a == d && b == c && a != b);
                    if (lane0) {
                        if (k0) atomicAdd(&acc[3 * s], (unsigned long long)__popcll(k0));
                        if (k1) atomicAdd(&acc[3 * s + 1], (unsigned long long)__popcll(k1));
                        if (k2) atomicAdd(&acc[3 * s + 2], (unsigned long long)__popcll(k2));
                    }
                } else {
                    uint32_t na[4], nb[4], nc[4], nd[4];
                    cc_group_counts(P, row, g0, g[1], live, na);
                    cc_group_counts(P, row, g[1], g[2], live, nb);
                    cc_group_counts(P, row, g[2], g[3], live, nc);
                    cc_group_counts(P, row, g[3], g4, live, nd);
                    unsigned long long ab = 0, cd = 0, ac = 0, bd = 0, ad = 0, bc = 0, all = 0;
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const unsigned long long A = na[x], B = nb[x], C = nc[x], D = nd[x];
                        ab += A * B; cd += C * D; ac += A * C; bd += B * D; ad += A * D; bc += B * C;
                        all += A * B * C * D;
                    }
                    const unsigned long long k0 = cc_wave_sum(ab * cd - all);
                    const unsigned long long k1 = cc_wave_sum(ac * bd - all);
                    const unsigned long long k2 = cc_wave_sum(ad * bc - all);
                    if (lane0) {
                        if (k0) atomicAdd(&acc[3 * s], k0);
                        if (k1) atomicAdd(&acc[3 * s + 1], k1);
                        if (k2) atomicAdd(&acc[3 * s + 2], k2);
                    }
                }
            }
        }
        __syncthreads();
        unsigned long long* out = P.counts + ((size_t)l * (size_t)P.n_sets + (size_t)s_lo) * 3;
        for (int i = threadIdx.x; i < n_tile * 3; i += kCcBlock) {
            const unsigned long long v = acc[i];
            if (v) atomicAdd(&out[i], v);
        }
        __syncthreads();   // acc is zeroed again for the next locus
    }
}

struct CcRowsParams {
    const unsigned long long* counts;   // [nloci][n_sets][3]
    int64_t nloci, n_sets, n_nodes;
    const int64_t* node_sets;           // [n_nodes + 1], validated on the host: at least two sets per internode, within n_sets
    double* rows;                       // [nloci][n_nodes][12]
};

__global__ __launch_bounds__(256) void concordance_rows_kernel(CcRowsParams P) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= P.nloci * P.n_nodes) return;
    const int64_t l = id / P.n_nodes, i = id - l * P.n_nodes;
    const unsigned long long* c = P.counts + (size_t)l * (size_t)P.n_sets * 3;
    const int64_t s0 = P.node_sets[i], s1 = P.node_sets[i + 1];
    double* row = P.rows + (size_t)id * kCcRow;
    for (int k = 0; k < 6; ++k) row[k] = (double)c[3 * s0 + k];   // the pooled set, then the nearest-tip quartet
    double f0 = 0.0, f1 = 0.0, f2 = 0.0, n = 0.0;
    int64_t decisive = 0;
    for (int64_t s = s0 + 2; s < s1; ++s) {
        const double k0 = (double)c[3 * s], k1 = (double)c[3 * s + 1], k2 = (double)c[3 * s + 2];
        const double dec = k0 + k1 + k2;
        if (dec > 0.0) {
            f0 += k0 / dec; f1 += k1 / dec; f2 += k2 / dec; n += dec;
            ++decisive;
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double m = (double)decisive;
    row[6] = decisive ? f0 / m : nan;
    row[7] = decisive ? f1 / m : nan;
    row[8] = decisive ? f2 / m : nan;
    row[9] = decisive ? n / m : nan;
    row[10] = m;
    row[11] = (double)(s1 - s0 - 2);
}

}  // namespace tphip

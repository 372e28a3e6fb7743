// pi_kernels.hpp -- column classification / compaction and the PI-table kernels.
//
// classify_kernel + compact_kernel   (HBM-bound byte work: ntaxa bytes read per column)
//     replace HyPhy's unique-pattern bookkeeping (bf:1033-1044) and tapir's informative-site count
//     (tapir/compute.py:96-106): per column the number of plain A/C/G/T cells, and whether the likelihood
//     has a closed-form maximiser (all resolved taxa identical -> s = 0; <= 1 resolved taxon -> flat).
// pi_partial_kernel + pi_reduce_kernel
//     replace bin/tapir_compute.py:114-122: pi = get_townsend_pi(time_vector, rates) is never materialised;
//     the (T x S) matrix is reduced over S on the fly into per-locus rows
//     [net PI(t=0..T-1) | PI at --times | sum(integral) per interval | sum(error) per interval].
//     Summation order is fixed (1024-column blocks, lane-strided, then block order) so a locus gives the
//     same bits no matter how many GPUs the batch is sharded over.
// pi_net_kernel + pi_interval_kernel
//     pi_partial_kernel's two jobs as two kernels, for plans with long loci (SiteLaunch::pi_split); the same sums, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gtr_model.hpp"
#include "tree_program.hpp"
#include "quadpack_device.hpp"
#include "site_rate_params.hpp"
#include "pi_rate.hpp"
#include "tphip.h"
#include "wave_sum.hpp"

namespace tphip {

// (kPiBlock, kPiColsPerThread, kPiChunk: launch_constants.hpp)
constexpr int kTimeTile = 16;
constexpr int kIvTile = 8;      // intervals per register tile of pi_partial_kernel (2 * kIvTile <= kTimeTile rows of `red`)

struct ClassifyParams {
    const uint8_t* states;
    int64_t ncols_total;
    int32_t ntaxa;
    const LocusModel* models;
    const int64_t* locus_offsets;
    const int32_t* chunk_locus;   // PI chunks (1024 columns, one locus each)
    const int32_t* chunk_index;
    double* rate;
    double* subst;
    double* lnl;
    uint8_t* flag;
    int32_t* nres;
    double chrono_length;
    // the tree program as the parsimony pass sees it (TreeProgram::cls_steps, built once per plan): per tip k in program
    // order {alignment row, ctl}, ctl = (stack pops before the tip << 1) | (push before the tip); padded to a multiple of 8
    const int2* steps;
    int32_t tail_pops;            // pops after the last tip
    int32_t max_pops;             // most pops before one tip
    uint32_t* packed;             // [ceil(ntaxa/8)][ncols_total] out: 8 four-bit masks per word, program tip order
    double start_scale;           // 1: start at the parsimony rate; 0: at HyPhy's siteRate = 1 (bf:1050), TPHIP_START_*
    uint64_t* hash;               // [ncols_total] out (may be null): hash of the column's packed words, for the
                                  // per-pattern de-duplication of the site-rate stage (dedup_kernels.hpp)
};

// The step table through the constant address space: classify_kernel also stores, so through a plain pointer the
// compiler cannot prove the table invariant and fetches it with vector loads.  As constant memory its wave-uniform
// entries come in with scalar loads that the compiler is free to issue early and batch (no wait per entry).
typedef const __attribute__((address_space(4))) int2 ConstInt2;
__device__ __forceinline__ ConstInt2* as_constant(const int2* p) { return (ConstInt2*)(uintptr_t)p; }

// Per-column bookkeeping of classify_kernel, as its finishing code reads it.
struct ColumnScan {
    unsigned uni = 0;
    int resolved = 0, informative = 0;
    unsigned changes = 0;   // Fitch parsimony: minimum number of substitutions on the tree
    int base[3] = {0, 0, 0};   // plain A, C, G cells (T = informative - the three): the column's own exit rate, start_log_rate
};

// Four consecutive columns at once: a thread's four state bytes of one taxon arrive as one dword, and every quantity
// classify_kernel needs per tip is a per-byte operation on 4-bit masks (SWAR): 10 integer instructions per column and
// tip instead of 30 with one ColumnScan per column, which made this byte kernel VALU-bound at 0.48 ms on C3 (its
// 575 MB move in ~0.15 ms).
//   * `set4` / `stk`: Fitch parsimony along the tree program -- the state set of the subtree in the accumulator (one
//     byte per column) and the sets of the parked siblings (4 bits per level and column);
//   * counters (resolved taxa, plain A/C/G/T cells, Fitch changes) accumulate one byte per column and are flushed
//     into 32-bit totals every 64 tips.
struct ColumnScan4 {
    static constexpr uint32_t k01 = 0x01010101u, k0f = 0x0f0f0f0fu;
    uint32_t uni4 = 0, set4 = k0f;
    uint32_t res8 = 0, inf8 = 0, chg8 = 0;            // byte counters since the last flush
    uint32_t a8 = 0, c8 = 0, g8 = 0;                  // ... of the plain A / C / G cells
    int base[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    uint64_t hsh[4] = {0x243F6A8885A308D3ull, 0x243F6A8885A308D3ull, 0x243F6A8885A308D3ull, 0x243F6A8885A308D3ull};
    int resolved[4] = {0, 0, 0, 0}, informative[4] = {0, 0, 0, 0};
    unsigned changes[4] = {0, 0, 0, 0};
    unsigned long long stk[4] = {0, 0, 0, 0};
    // 0x01 in every byte whose low nibble (the only bits set) is nonzero / equals 15
    static __device__ __forceinline__ uint32_t nonzero(uint32_t x) { return ((x + k0f) >> 4) & k01; }
    static __device__ __forceinline__ uint32_t is15(uint32_t x) { return ((x + k01) >> 4) & k01; }
    // 0x01 -> 0x0f per byte.  The empty asm keeps the shift opaque: folded, (b << 4) - b becomes b * 15, a quarter-rate
    // v_mul_lo_u32 (three per tip)
    static __device__ __forceinline__ uint32_t spread(uint32_t b) {
        uint32_t s = b << 4;
        asm("" : "+v"(s));
        return s - b;
    }
    __device__ __forceinline__ void flush() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            resolved[j] += (int)((res8 >> (8 * j)) & 0xffu);
            informative[j] += (int)((inf8 >> (8 * j)) & 0xffu);
            changes[j] += (chg8 >> (8 * j)) & 0xffu;
            base[0][j] += (int)((a8 >> (8 * j)) & 0xffu);
            base[1][j] += (int)((c8 >> (8 * j)) & 0xffu);
            base[2][j] += (int)((g8 >> (8 * j)) & 0xffu);
        }
        res8 = inf8 = chg8 = 0;
        a8 = c8 = g8 = 0;
    }
    __device__ __forceinline__ void fitch_join(uint32_t x4) {
        const uint32_t both = set4 & x4;
        const uint32_t empty = nonzero(both) ^ k01;
        chg8 += empty;
        set4 = both | ((set4 | x4) & spread(empty));
    }
    __device__ __forceinline__ void fitch_push() {
#pragma unroll
        for (int j = 0; j < 4; ++j) stk[j] = (stk[j] << 4) | ((set4 >> (8 * j)) & 15u);
        set4 = k0f;
    }
    __device__ __forceinline__ void fitch_pop() {
        uint32_t x4 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { x4 |= (uint32_t)(stk[j] & 15ull) << (8 * j); stk[j] >>= 4; }
        fitch_join(x4);
    }
    // v: the state bytes of the next tip (program order) for the four columns; returns its four masks (one per byte)
    __device__ __forceinline__ uint32_t tip(uint32_t v) {
        uint32_t m4 = v & k0f;
        m4 |= spread(nonzero(m4) ^ k01);              // code 0 (nothing allowed) reads as "anything": 15
        const uint32_t res = is15(m4) ^ k01;          // resolved: not a gap / ? / N
        uni4 |= m4 & spread(res);
        res8 += res;
        const uint32_t single = nonzero(m4 & (m4 - k01)) ^ k01;   // exactly one bit set (m4 >= 1 in every byte: no borrow)
        inf8 += single;
        a8 += single & m4;                            // ... and it is bit 0 / 1 / 2 (the neighbour byte's bit that a shift
        c8 += single & (m4 >> 1);                     // brings into bit 7 is masked away by `single`)
        g8 += single & (m4 >> 2);
        fitch_join(m4);
        return m4;
    }
    // The packed tip words of eight tips: word[j] nibble i = byte j of m[i].  Pairs of tips first share a byte
    // (a01 byte j = m[0] nibble | m[1] nibble << 4), then a 4 x 4 byte transpose in eight byte permutes.
    static __device__ __forceinline__ void pack8(const uint32_t* m, uint32_t* word) {
        const uint32_t a01 = m[0] | (m[1] << 4), a23 = m[2] | (m[3] << 4), a45 = m[4] | (m[5] << 4), a67 = m[6] | (m[7] << 4);
        // __builtin_amdgcn_perm(hi, lo, sel): byte n of the result = byte sel_n of the 8-byte value hi:lo
        const uint32_t t_lo = __builtin_amdgcn_perm(a23, a01, 0x05010400u);   // a01.b0 a23.b0 a01.b1 a23.b1
        const uint32_t t_hi = __builtin_amdgcn_perm(a23, a01, 0x07030602u);   // a01.b2 a23.b2 a01.b3 a23.b3
        const uint32_t u_lo = __builtin_amdgcn_perm(a67, a45, 0x05010400u);
        const uint32_t u_hi = __builtin_amdgcn_perm(a67, a45, 0x07030602u);
        word[0] = __builtin_amdgcn_perm(u_lo, t_lo, 0x05040100u);   // a01.b0 a23.b0 a45.b0 a67.b0
        word[1] = __builtin_amdgcn_perm(u_lo, t_lo, 0x07060302u);
        word[2] = __builtin_amdgcn_perm(u_hi, t_hi, 0x05040100u);
        word[3] = __builtin_amdgcn_perm(u_hi, t_hi, 0x07060302u);
    }
    __device__ __forceinline__ ColumnScan column(int j) const {   // after flush()
        ColumnScan c;
        c.uni = (uni4 >> (8 * j)) & 15u;
        c.resolved = resolved[j];
        c.informative = informative[j];
        c.changes = changes[j];
        c.base[0] = base[0][j]; c.base[1] = base[1][j]; c.base[2] = base[2][j];
        return c;
    }
};

constexpr double kStartA = 0.25, kStartDensityCap = 0.235;   // (0.30 / 0.28 before the column's own exit rate went into the start)

// Where the optimiser starts for a column that needs it: the rate at which the tree would carry the column's
// parsimony count, s0 = changes / (kappa * tree length * fraction of taxa present).  HyPhy starts every column at
// siteRate = 1 (bf:1050), typically e^3 away from the optimum; from s0 (median error 10 %) the same maximum is reached in
// 2.8 instead of 4.4 evaluations on the C3 shape.  Passed to site_rate_kernel through the column's `rate` slot.
// -Q_xx of the locus' model for x = A, C, G, T: -sum_k U[x][k] lam_k U^-1[k][x] (lam_0 = 0); once per thread, the four columns
// of a thread belong to one locus
__device__ __forceinline__ void exit_rates(const LocusModel* __restrict__ M, double* ex) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        double qxx = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) qxx = fma(M->U[x * 3 + k] * M->lam[k], M->Ui[k * 4 + x], qxx);
        ex[x] = -qxx;
    }
}

__device__ __forceinline__ double start_log_rate(const ClassifyParams& P, const LocusModel* __restrict__ M, const ColumnScan& c,
                                                 const double* ex) {
    // Rate at which THIS column's states are left: sum_x p_x (-Q_xx) over its plain cells instead of the stationary mean
    // kappa = sum_x pi_x (-Q_xx).  A column of mostly fast-leaving bases reaches its parsimony count at a lower site rate; with
    // the column's own exit rate the start lands 2-3 x closer (64 taxa: rms miss 0.20 -> 0.105 log-units, 256 taxa: 0.36 ->
    // 0.13; same rule as the oracle).  ex[x] = -Q_xx (exit_rates).
    double exit_rate = M->kappa;
    if (c.informative > 0) {
        const int cnt[4] = {c.base[0], c.base[1], c.base[2], c.informative - c.base[0] - c.base[1] - c.base[2]};
        double acc = 0.0;
#pragma unroll
        for (int x = 0; x < 4; ++x) acc = fma((double)cnt[x], ex[x], acc);
        if (acc > 0.0) exit_rate = acc / (double)c.informative;
    }
    const double len = exit_rate * P.chrono_length * ((double)(c.resolved > 0 ? c.resolved : 1) / (double)P.ntaxa);
    double m = (double)(c.changes > 0u ? c.changes : 1u);
    // parsimony undercounts where changes are dense: with p = changes per branch among the taxa present, the count is
    // stretched to B * (-a ln(1 - p/a)), a = kStartA (the shape of a multiple-hit correction; a calibrated on the
    // synthetic shapes, where it centres the start on the optimum for p up to kStartDensityCap and saves another 6-12 %
    // of the evaluations; only the starting point depends on it)
    const double B = (double)(2 * c.resolved - 3 > 1 ? 2 * c.resolved - 3 : 1);
    const double pden = fmin(m / B, kStartDensityCap);
    m = B * (-kStartA * log(1.0 - pden / kStartA));
    double u0 = (len > 0.0) ? log(m / len) : 0.0;
    u0 = (u0 == u0) ? u0 : 0.0;
    return fmin(fmax(u0, -20.0), 8.0);
}

__device__ __forceinline__ void classify_finish(const ClassifyParams& P, const LocusModel* __restrict__ M, int64_t col,
                                                const ColumnScan& c, const double* ex, uint8_t& flg_out) {
    uint8_t flg = TPHIP_FLAG_OK;  // provisional: site_rate_kernel will overwrite
    if (c.resolved <= 1) flg = TPHIP_FLAG_FLAT;
    else if (__popc(c.uni) == 1) flg = TPHIP_FLAG_ZERO;
    flg_out = flg;
    if (flg != TPHIP_FLAG_OK) {
        // L = sum over the states allowed by the one informative mask of pi_x (1 if nothing is resolved)
        double L = 0;
        if (c.uni == 0) L = 1.0;
        else {
#pragma unroll
            for (int x = 0; x < 4; ++x) L += ((c.uni >> x) & 1u) ? M->pi[x] : 0.0;
        }
        const double s = (flg == TPHIP_FLAG_FLAT) ? 1.0 : 0.0;  // flat: siteRate keeps its start value (bf:1050)
        const double r = s * M->kappa;
        P.rate[col] = r;
        P.subst[col] = r * P.chrono_length;
        P.lnl[col] = log(L);
    } else {
        // u0 for site_rate_kernel, which overwrites it with the answer: the parsimony start, or u = log 1 = 0 when the
        // plan asks for HyPhy's start value (start_scale = 0; a multiplication, not a branch: + 0.0 turns -0.0 into 0.0)
        P.rate[col] = start_log_rate(P, M, c, ex) * P.start_scale + 0.0;
        // the column's parsimony length for the optimiser's first step (site_rate_kernel overwrites the slot with the answer);
        // 0 = none: HyPhy's start value asks for the plain step from there, and on small trees an evaluation is so cheap that
        // the extra logarithm costs more than the saved evaluations (C2, 16 taxa: +4 % time with it; C3 -2 %, C5 -4 %)
        P.subst[col] = (P.ntaxa >= kFirstStepMinTaxa) ? (double)c.changes * P.start_scale : 0.0;
        // ... and in the `lnl` slot (also overwritten with the answer) whether the column is likely to need many evaluations:
        // a parsimony count of 30 % or more of the resolved taxa.  Small batches (slice and mixed-loci modes of site_rate_kernel) last as
        // long as their slowest wave; a slow column (one in a hundred needs 9-17 evaluations from siteRate = 1, all of them
        // in this class: tools/debug note in DESIGN section 8 r3) taken late keeps its wave alive alone, so those waves
        // take the marked columns first (site_rate_kernel, small-batch mode).  The order changes no column's result.
        P.lnl[col] = (10u * c.changes >= 3u * (c.resolved > 1u ? c.resolved - 1u : 1u)) ? 1.0 : 0.0;
    }
}

// The tip loop of classify_kernel, one instance per access kind (kFast: aligned dword loads and 16-byte stores; the
// byte path's per-column conditions would otherwise sit between every load and its use) and, for the trees that allow
// it, with the pops before a tip written out (kPopsUnrolled: no inner loop).
constexpr int kMaxUnrolledPops = 6;
template <bool kFast, bool kPopsUnrolled>
__device__ __forceinline__ void classify_scan(const ClassifyParams& P, int64_t c0, int n, ColumnScan4& c) {
    ConstInt2* steps = as_constant(P.steps);
    // the state dwords of the eight tips of group g (missing columns of a ragged thread read as gaps)
    auto load_group = [&](int g, uint32_t* buf) {
        const uint8_t* row[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = P.states + (int64_t)steps[8 * g + i].x * P.ncols_total + c0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (kFast) {
                buf[i] = *reinterpret_cast<const uint32_t*>(row[i]);
            } else {
                uint32_t w = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < n) w |= (uint32_t)row[i][j] << (8 * j);
                buf[i] = w;
            }
        }
    };
    // Tips go in groups of eight, written out in full so that a tip's state dword is a fixed register (no select chain
    // on the tip index).  The next group's dwords are requested before this group is worked on.  (steps is padded to
    // a multiple of 8.)
    auto group = [&](int g, const uint32_t* cur) {
        uint32_t m[8];
        int ctl[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ctl[i] = steps[8 * g + i].y;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            m[i] = 0;
            if (8 * g + i < P.ntaxa) {   // wave-uniform: only the last group can be partial
                const int np = ctl[i] >> 1;
                if (kPopsUnrolled) {   // the plan saw at most kMaxUnrolledPops between two tips: no inner loop
#pragma unroll
                    for (int q = 0; q < kMaxUnrolledPops; ++q) if (q < np) c.fitch_pop();
                } else {
                    for (int q = np; q > 0; --q) c.fitch_pop();
                }
                if (ctl[i] & 1) c.fitch_push();
                m[i] = c.tip(cur[i]);
            }
        }
        if ((g & 7) == 7) c.flush();   // after every 64th tip: <= 64 tip joins + <= 64 + 16 sibling joins per window, no byte overflows
        uint32_t word[4];
        ColumnScan4::pack8(m, word);
        if (kFast) {
            *reinterpret_cast<uint4*>(P.packed + (int64_t)g * P.ncols_total + c0) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) P.packed[(int64_t)g * P.ncols_total + c0 + j] = word[j];
        }
        if (P.hash) {   // wave-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint64_t h = (c.hsh[j] ^ word[j]) * 0x9E3779B97F4A7C15ull;
                c.hsh[j] = h ^ (h >> 29);
            }
        }
    };
    // two buffers, two groups per trip: no register copies between a load and its use
    const int ngroups = (P.ntaxa + 7) >> 3;
    uint32_t b0[8], b1[8];
    load_group(0, b0);
    // (the empty asm statements pin the loads ahead of the group they overlap: the scheduler would otherwise sink them
    // down to their first use)
    int g = 0;
    for (; g + 1 < ngroups; g += 2) {
        load_group(g + 1, b1);
        asm volatile("" ::: "memory");
        group(g, b0);
        if (g + 2 < ngroups) load_group(g + 2, b0);
        asm volatile("" ::: "memory");
        group(g + 1, b1);
    }
    if (g < ngroups) group(g, b0);
    for (int q = P.tail_pops; q > 0; --q) c.fitch_pop();
}

// HBM-bound byte kernel.  Each thread owns 4 CONSECUTIVE columns: when the row addresses are 4-byte aligned
// (alignment of the states pointer, of ncols_total and of the locus offset: true for every BASELINE shape) a taxon
// row is read as one dword per lane (256 B per wave instruction instead of 64), the packed tip words and the
// counts go out as one 16-byte store per lane and the four flags as one dword.  Unaligned batches fall back to
// byte accesses with the same thread-to-column map.  Tips are visited in tree-program order so that the same
// pass emits the packed words site_rate_kernel keeps in registers.
__global__ __launch_bounds__(kPiBlock) void classify_kernel(ClassifyParams P) {
    const int locus = P.chunk_locus[blockIdx.x];
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const LocusModel* __restrict__ M = P.models + locus;
    const int64_t c0 = lo + (int64_t)P.chunk_index[blockIdx.x] * kPiChunk + 4 * (int64_t)threadIdx.x;
    if (c0 >= hi) return;
    const bool full = (c0 + 4 <= hi);
    // (the three output pointers are the caller's or a workspace region: legal at their element type's alignment, while the
    //  fast path stores 16 bytes through nres and packed and 4 through flag; with ncols_total and c0 multiples of 4 the bases
    //  decide for every row and column.  Kernel arguments: the test is a few scalar ANDs)
    const bool wide_ok = ((reinterpret_cast<uintptr_t>(P.states) & 3u) | (reinterpret_cast<uintptr_t>(P.flag) & 3u) |
                          (reinterpret_cast<uintptr_t>(P.nres) & 15u) | (reinterpret_cast<uintptr_t>(P.packed) & 15u)) == 0;
    const bool aligned = full && wide_ok && ((P.ncols_total & 3) == 0) && ((c0 & 3) == 0);
    const int n = full ? 4 : (int)(hi - c0);
    const bool fast = __all(aligned);   // wave-uniform: only the last wave of a locus can have a ragged thread
    ColumnScan4 c;
    if (fast) {
        if (P.max_pops <= kMaxUnrolledPops) classify_scan<true, true>(P, c0, n, c);
        else classify_scan<true, false>(P, c0, n, c);
    } else {
        classify_scan<false, false>(P, c0, n, c);
    }
    c.flush();
    uint8_t f[4] = {0, 0, 0, 0};
    double ex[4];
    exit_rates(M, ex);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j < n) classify_finish(P, M, c0 + j, c.column(j), ex, f[j]);
    if (P.hash) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < n) P.hash[c0 + j] = c.hsh[j] ^ (c.hsh[j] >> 32);
    }
    if (fast) {
        *reinterpret_cast<int4*>(P.nres + c0) = make_int4(c.informative[0], c.informative[1], c.informative[2], c.informative[3]);
        *reinterpret_cast<uint32_t*>(P.flag + c0) = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) { P.nres[c0 + j] = c.informative[j]; P.flag[c0 + j] = f[j]; }
        }
    }
}

// One workgroup per locus: stable compaction of the columns that still need the optimiser.  The loop is a chain of
// barriers, so its time is the number of rounds: long loci get 1024 threads (C3: 49 rounds per locus instead of 196),
// short ones 256.
template <int kCompactBlock>
__global__ __launch_bounds__(kCompactBlock) void compact_kernel(const uint8_t* __restrict__ flag, const int64_t* __restrict__ locus_offsets,
                                                                int32_t* __restrict__ work_cols, int32_t* __restrict__ work_count) {
    constexpr int kWaves = kCompactBlock / 64;
    __shared__ int wave_tot[kWaves];
    __shared__ int running;
    const int locus = blockIdx.x;
    const int64_t lo = locus_offsets[locus], hi = locus_offsets[locus + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    for (int64_t base = lo; base < hi; base += kCompactBlock) {
        const int64_t col = base + threadIdx.x;
        const bool want = (col < hi) && (flag[col] == TPHIP_FLAG_OK);
        const unsigned long long bal = __ballot(want);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int off = running, tot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { off += (w < wave) ? wave_tot[w] : 0; tot += wave_tot[w]; }
        if (want) work_cols[lo + off + before] = (int32_t)col;
        __syncthreads();
        if (threadIdx.x == 0) running += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) work_count[locus] = running;
}

// compact_kernel for the hand-out by predicted work (site_rate_kernel.hpp): the columns are also counted by class -- slow (classify_kernel's mark, a non-zero lnl slot) and easy (the
// others) -- into work_class[locus][2], and reserve_q / 2^16 of the locus' easy columns (reserved_before: by their rank among
// the locus' easy columns, so the choice sees this locus alone) leave the main part for a reserved tail at the end of the
// locus' part of the list: [main part, stable][reserved tail, stable].  The tail's place is known only when the locus has
// been counted, so its entries are collected in `scratch` (same shape as work_cols) and appended after the loop.
// reserve_q = 0 gives the plain stable list.
template <int kCompactBlock>
__global__ __launch_bounds__(kCompactBlock) void compact_classes_kernel(const uint8_t* __restrict__ flag, const int64_t* __restrict__ locus_offsets,
                                                                int32_t* __restrict__ work_cols, int32_t* __restrict__ work_count,
                                                                const double* __restrict__ lnl, int32_t reserve_q,
                                                                int32_t* __restrict__ scratch,
                                                                int32_t* __restrict__ work_class) {
    constexpr int kWaves = kCompactBlock / 64;
    __shared__ int wave_tot[kWaves], wave_easy[kWaves];
    __shared__ int running, running_easy;
    const int locus = blockIdx.x;
    const int64_t lo = locus_offsets[locus], hi = locus_offsets[locus + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { running = 0; running_easy = 0; }
    __syncthreads();
    for (int64_t base = lo; base < hi; base += kCompactBlock) {
        const int64_t col = base + threadIdx.x;
        const bool want = (col < hi) && (flag[col] == TPHIP_FLAG_OK);
        const bool easy = want && lnl[col] == 0.0;
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long bal = __ballot(want), bal_easy = __ballot(easy);
        const int before = __popcll(bal & below);
        if (lane == 0) { wave_tot[wave] = __popcll(bal); wave_easy[wave] = __popcll(bal_easy); }
        __syncthreads();
        int off = running, tot = 0, eoff = running_easy, etot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            off += (w < wave) ? wave_tot[w] : 0; tot += wave_tot[w];
            eoff += (w < wave) ? wave_easy[w] : 0; etot += wave_easy[w];
        }
        if (want) {
            // eoff: the easy columns of the locus before this one; that many of them were reserved, the others are ahead
            // of this column in the main part
            eoff += __popcll(bal_easy & below);
            const int res = reserved_before(eoff, reserve_q);
            if (easy && reserved_before((int64_t)eoff + 1, reserve_q) != res) scratch[lo + res] = (int32_t)col;
            else work_cols[lo + off + before - res] = (int32_t)col;
        }
        __syncthreads();
        if (threadIdx.x == 0) { running += tot; running_easy += etot; }
        __syncthreads();
    }
    const int n_res = reserved_before(running_easy, reserve_q), n_main = running - n_res;
    if (n_res > 0) {
        __threadfence_block();
        __syncthreads();
        for (int i = threadIdx.x; i < n_res; i += kCompactBlock) work_cols[lo + n_main + i] = scratch[lo + i];
    }
    if (threadIdx.x == 0) {
        work_count[locus] = running;
        work_class[2 * locus] = running - running_easy; work_class[2 * locus + 1] = running_easy;
    }
}

// ---- The same lists for long loci, chunk-parallel.  One workgroup per locus is a chain of barriers as long as the locus
// (C3: 100 workgroups on 256 CUs, 49 rounds of three barriers each, then the append pass).  Three steps instead, ordered
// by the stream alone (no workgroup waits for another):
//   compact_count_kernel    per 1024-column chunk: its wanted columns and its easy ones            -> chunk_cnt[chunk]
//   compact_scan_kernel     per locus: exclusive scan of its chunks' counts (in place); work_count, work_class
//   compact_scatter_kernel  per chunk: every entry of work_cols straight to its final place -- main part
//                           lo + before - reserved_before(easy rank), reserved tail lo + n_main + reserved_before(easy rank),
//                           n_main from the locus totals: no scratch list, no append pass.
// kClasses = false is compact_kernel's plain list (no marks read, reserve 0).  The lists, counts and class counts are the
// one-workgroup kernels' entry for entry.
constexpr int kCompactChunkBlock = 256;

// A chunk's columns in kPiColsPerThread rounds of 256: which of them are wanted / easy, as one ballot per round and wave.
template <bool kClasses>
__device__ __forceinline__ void compact_chunk_ballots(const uint8_t* __restrict__ flag, const double* __restrict__ lnl,
                                                      int64_t base, int64_t hi, unsigned long long* bal,
                                                      unsigned long long* bal_easy) {
#pragma unroll
    for (int it = 0; it < kPiColsPerThread; ++it) {
        const int64_t col = base + it * kCompactChunkBlock + threadIdx.x;
        const bool want = (col < hi) && (flag[col] == TPHIP_FLAG_OK);
        bool easy = false;
        if (kClasses) easy = want && lnl[col] == 0.0;
        bal[it] = __ballot(want);
        bal_easy[it] = kClasses ? __ballot(easy) : 0ull;
    }
}

template <bool kClasses>
__global__ __launch_bounds__(kCompactChunkBlock) void compact_count_kernel(const uint8_t* __restrict__ flag, const double* __restrict__ lnl,
                                                                          const int64_t* __restrict__ locus_offsets,
                                                                          const int32_t* __restrict__ chunk_locus,
                                                                          const int32_t* __restrict__ chunk_index,
                                                                          int2* __restrict__ chunk_cnt) {
    constexpr int kWaves = kCompactChunkBlock / 64;
    __shared__ int wave_tot[kWaves], wave_easy[kWaves];
    const int chunk = blockIdx.x, locus = chunk_locus[chunk];
    const int64_t base = locus_offsets[locus] + (int64_t)chunk_index[chunk] * kPiChunk, hi = locus_offsets[locus + 1];
    unsigned long long bal[kPiColsPerThread], bal_easy[kPiColsPerThread];
    compact_chunk_ballots<kClasses>(flag, lnl, base, hi, bal, bal_easy);
    int tot = 0, etot = 0;
#pragma unroll
    for (int it = 0; it < kPiColsPerThread; ++it) { tot += __popcll(bal[it]); etot += __popcll(bal_easy[it]); }
    if ((threadIdx.x & 63) == 0) { wave_tot[threadIdx.x >> 6] = tot; wave_easy[threadIdx.x >> 6] = etot; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { a += wave_tot[w]; b += wave_easy[w]; }
        chunk_cnt[chunk] = make_int2(a, b);
    }
}

template <bool kClasses>
__global__ __launch_bounds__(kCompactChunkBlock) void compact_scan_kernel(const int64_t* __restrict__ locus_chunk_offsets, int2* __restrict__ chunk_cnt,
                                                                         int32_t* __restrict__ work_count, int32_t* __restrict__ work_class) {
    constexpr int kWaves = kCompactChunkBlock / 64;
    __shared__ int wave_tot[kWaves], wave_easy[kWaves];
    const int locus = blockIdx.x;
    const int64_t c0 = locus_chunk_offsets[locus], c1 = locus_chunk_offsets[locus + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int running = 0, running_easy = 0;   // the same in every thread
    for (int64_t cb = c0; cb < c1; cb += kCompactChunkBlock) {
        const int64_t c = cb + threadIdx.x;
        const int2 mine = (c < c1) ? chunk_cnt[c] : make_int2(0, 0);
        int inc = mine.x, einc = mine.y;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o), eup = __shfl_up(einc, o);
            if (lane >= o) { inc += up; einc += eup; }
        }
        if (lane == 63) { wave_tot[wave] = inc; wave_easy[wave] = einc; }
        __syncthreads();
        int off = running, eoff = running_easy;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            off += (w < wave) ? wave_tot[w] : 0; running += wave_tot[w];
            eoff += (w < wave) ? wave_easy[w] : 0; running_easy += wave_easy[w];
        }
        if (c < c1) chunk_cnt[c] = make_int2(off + inc - mine.x, eoff + einc - mine.y);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        work_count[locus] = running;
        if (kClasses) { work_class[2 * locus] = running - running_easy; work_class[2 * locus + 1] = running_easy; }
    }
}

template <bool kClasses>
__global__ __launch_bounds__(kCompactChunkBlock) void compact_scatter_kernel(const uint8_t* __restrict__ flag, const double* __restrict__ lnl,
                                                                            const int64_t* __restrict__ locus_offsets,
                                                                            const int32_t* __restrict__ chunk_locus,
                                                                            const int32_t* __restrict__ chunk_index,
                                                                            const int2* __restrict__ chunk_off,
                                                                            const int32_t* __restrict__ work_count,
                                                                            const int32_t* __restrict__ work_class, int32_t reserve_q,
                                                                            int32_t* __restrict__ work_cols) {
    constexpr int kWaves = kCompactChunkBlock / 64;
    __shared__ int wave_tot[kPiColsPerThread][kWaves], wave_easy[kPiColsPerThread][kWaves];
    const int chunk = blockIdx.x, locus = chunk_locus[chunk];
    const int64_t lo = locus_offsets[locus], hi = locus_offsets[locus + 1];
    const int64_t base = lo + (int64_t)chunk_index[chunk] * kPiChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long bal[kPiColsPerThread], bal_easy[kPiColsPerThread];
    compact_chunk_ballots<kClasses>(flag, lnl, base, hi, bal, bal_easy);
    if (lane == 0) {
#pragma unroll
        for (int it = 0; it < kPiColsPerThread; ++it) { wave_tot[it][wave] = __popcll(bal[it]); wave_easy[it][wave] = __popcll(bal_easy[it]); }
    }
    __syncthreads();
    const int2 start = chunk_off[chunk];   // the locus' wanted / easy columns before this chunk
    int n_main = 0;
    if (kClasses) n_main = work_count[locus] - reserved_before(work_class[2 * locus + 1], reserve_q);
    const unsigned long long below = (1ull << lane) - 1ull;
    int off = start.x, eoff = start.y;     // ... before this round's first column
#pragma unroll
    for (int it = 0; it < kPiColsPerThread; ++it) {
        int woff = off, weoff = eoff;      // ... before this wave's first column of the round
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            woff += (w < wave) ? wave_tot[it][w] : 0; off += wave_tot[it][w];
            weoff += (w < wave) ? wave_easy[it][w] : 0; eoff += wave_easy[it][w];
        }
        if ((bal[it] >> lane) & 1ull) {
            const int32_t col = (int32_t)(base + it * kCompactChunkBlock + threadIdx.x);
            const int before = woff + __popcll(bal[it] & below);
            if (kClasses) {
                // erank: the easy columns of the locus before this one; that many of them were reserved, the others are
                // ahead of this column in the main part
                const int erank = weoff + __popcll(bal_easy[it] & below);
                const int res = reserved_before(erank, reserve_q);
                const bool easy = (bal_easy[it] >> lane) & 1ull;
                if (easy && reserved_before((int64_t)erank + 1, reserve_q) != res) work_cols[lo + n_main + res] = col;
                else work_cols[lo + before - res] = col;
            } else {
                work_cols[lo + before] = col;
            }
        }
    }
}

__global__ __launch_bounds__(kPiBlock) void pi_partial_kernel(PiParams P) {
    __shared__ double red[kTimeTile][4];
    // per-tile transpose buffer: [time][16 segments of 16 threads, each padded to 17 doubles]
    __shared__ double tile[kTimeTile][16 * 17];
    const int chunk = blockIdx.x;
    const int locus = P.chunk_locus[chunk];
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const int64_t base = lo + (int64_t)P.chunk_index[chunk] * kPiChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double r[kPiColsPerThread];
    bool ok[kPiColsPerThread];
#pragma unroll
    for (int j = 0; j < kPiColsPerThread; ++j) {
        const int64_t col = base + j * kPiBlock + threadIdx.x;
        r[j] = (col < hi) ? finalize_rate(P, col) : __longlong_as_double(0x7ff8000000000000ll);
        // nansum skips NaN (bin/tapir_compute.py:119); quad only sees finite rates (:122); and a rate of exactly 0
        // (constant columns: 22-41 % of the synthetic shapes) contributes exactly 0 to every sum, error estimates included
        ok[j] = isfinite(r[j]) && r[j] != 0.0;
    }
    // Pack the chunk's contributing rates to the front (thread-major order, fixed for a given chunk): the slots the
    // culled and constant columns would have occupied are whole waves that skip the body below instead of lanes idling
    // inside it (C2: 290 of a locus' 500 columns contribute -- 5 wave-slots instead of 8).
    {
        __shared__ double packed_rate[kPiChunk];
        __shared__ int wave_count[kPiBlock / 64];
        int c = 0;
#pragma unroll
        for (int j = 0; j < kPiColsPerThread; ++j) c += ok[j] ? 1 : 0;
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wave_count[wave] = inc;
        __syncthreads();
        int pos = inc - c, total = 0;
#pragma unroll
        for (int w = 0; w < kPiBlock / 64; ++w) { pos += (w < wave) ? wave_count[w] : 0; total += wave_count[w]; }
#pragma unroll
        for (int j = 0; j < kPiColsPerThread; ++j) if (ok[j]) packed_rate[pos++] = r[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPiColsPerThread; ++j) {
            const int idx = j * kPiBlock + (int)threadIdx.x;
            ok[j] = idx < total;
            r[j] = ok[j] ? packed_rate[idx] : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    const int Wp = P.T + 2 * P.n_i;
    double* out = P.partial + (size_t)chunk * Wp;
    // ---- net PI(t), t = 0..T-1, in tiles of kTimeTile time points
    for (int t0 = 0; t0 < P.T; t0 += kTimeTile) {
        double acc[kTimeTile];
#pragma unroll
        for (int i = 0; i < kTimeTile; ++i) acc[i] = 0.0;
#pragma unroll
        for (int j = 0; j < kPiColsPerThread; ++j) {
            if (!ok[j]) continue;
            const double c = 16.0 * (r[j] * r[j]);
            const double q = exp(-(4.0 * r[j]));
            double p = exp(-(4.0 * r[j] * (double)t0));
#pragma unroll
            for (int i = 0; i < kTimeTile; ++i) {
                acc[i] = fma(c * (double)(t0 + i), p, acc[i]);
                p *= q;
            }
        }
        // Sum over the 256 threads WITHOUT 16 butterfly reductions (96 cross-lane FP64 exchanges per wave cost ten
        // times the arithmetic above): transpose through LDS, each thread then adds one 16-value segment of one
        // time point in a fixed order, and a 4-step exchange inside 16-lane groups finishes the sum.
        {
            const int slot = (threadIdx.x >> 4) * 17 + (threadIdx.x & 15);
#pragma unroll
            for (int i = 0; i < kTimeTile; ++i) tile[i][slot] = acc[i];
        }
        __syncthreads();
        {
            const int i = threadIdx.x >> 4, seg = threadIdx.x & 15;
            const double* src = &tile[i][seg * 17];
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) sum += src[k];
            sum += __shfl_xor(sum, 8);
            sum += __shfl_xor(sum, 4);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 1);
            if (seg == 0 && t0 + i < P.T) out[t0 + i] = sum;
        }
        __syncthreads();
    }
    // ---- interval integrals, in tiles of kIvTile intervals: per column the first-panel exponentials of consecutive
    // intervals of equal length are computed once (quadpack_device.hpp: GkFactors).  Per (thread, interval) the columns
    // are still added in the order j = 0..3, then lanes, then waves: the sums keep their fixed order.
    for (int k0 = 0; k0 < P.n_i; k0 += kIvTile) {
        double si[kIvTile], se[kIvTile];
#pragma unroll
        for (int kk = 0; kk < kIvTile; ++kk) { si[kk] = 0.0; se[kk] = 0.0; }
#pragma unroll 1
        for (int j = 0; j < kPiColsPerThread; ++j) {
            if (!ok[j]) continue;
            GkFactors F;
            double have_h = -1.0;        // half-length the factors in F were built for (intervals are wave-uniform)
#pragma unroll
            for (int kk = 0; kk < kIvTile; ++kk) {
                const int k = k0 + kk;
                if (k < P.n_i) {         // wave-uniform
                    const double a = (double)P.intervals[2 * k], b = (double)P.intervals[2 * k + 1];
                    double res, err = 0.0;
                    // (measured: the table-driven exp of fast_exp.hpp makes this kernel 1.65x SLOWER -- scattered LDS reads
                    //  from one table shared by 256 threads -- and its degree-13 polynomial 1.3x: the library exp stays)
                    if (P.integ_mode == TPHIP_INTEG_QUADPACK) {
                        const double hl = 0.5 * (b - a);
                        if (4.0 * r[j] * hl < 30.0) {        // per lane: a huge rate takes the generic panel
                            if (hl != have_h) { gk_factors(r[j], hl, F); have_h = hl; }
                            quad_townsend_factored(a, b, r[j], F, res, err);
                        } else {
                            quad_townsend<false>(a, b, r[j], nullptr, res, err);
                        }
                    } else {
                        res = integral_closed(a, b, r[j]);
                    }
                    si[kk] += res;
                    se[kk] += err;
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < kIvTile; ++kk) {
            const int k = k0 + kk;
            if (k < P.n_i) {
                const double s1 = wave_sum(si[kk]), s2 = wave_sum(se[kk]);
                if (lane == 0) { red[2 * kk][wave] = s1; red[2 * kk + 1][wave] = s2; }
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 * kIvTile && k0 + (int)(threadIdx.x >> 1) < P.n_i) {
            const int kk = threadIdx.x >> 1, which = threadIdx.x & 1;
            out[P.T + which * P.n_i + k0 + kk] =
                ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
        }
        __syncthreads();
    }
}

// ---- pi_partial_kernel as two kernels, for long loci (SiteLaunch::pi_split).  Its two jobs want opposite things: the time
// tiles ~100 VGPRs and many waves, the interval integrals every register they can get.  Fused, the integrals pin the whole
// kernel at 255 VGPRs and 2 waves per SIMD.  pi_net_kernel writes out[0 .. T), pi_interval_kernel out[T .. T + 2 n_i); each
// packs the chunk as pi_partial_kernel does and adds in pi_partial_kernel's order, so `partial` holds the same bits.

// The chunk's rates as the PI sums see them, the contributing ones packed to the front in thread-major order (see
// pi_partial_kernel): r[j] / ok[j] is the thread's packed slot j * kPiBlock + threadIdx.x.  `packed_rate`: kPiChunk doubles
// of LDS, the caller's, read here after the last barrier: a caller that writes them again puts a barrier in front.
__device__ __forceinline__ void pi_pack_chunk(const PiParams& P, int64_t base, int64_t hi, double* packed_rate, double* r, bool* ok) {
    __shared__ int wave_count[kPiBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kPiColsPerThread; ++j) {
        const int64_t col = base + j * kPiBlock + threadIdx.x;
        r[j] = (col < hi) ? finalize_rate(P, col) : __longlong_as_double(0x7ff8000000000000ll);
        ok[j] = isfinite(r[j]) && r[j] != 0.0;
    }
    int c = 0;
#pragma unroll
    for (int j = 0; j < kPiColsPerThread; ++j) c += ok[j] ? 1 : 0;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_count[wave] = inc;
    __syncthreads();
    int pos = inc - c, total = 0;
#pragma unroll
    for (int w = 0; w < kPiBlock / 64; ++w) { pos += (w < wave) ? wave_count[w] : 0; total += wave_count[w]; }
#pragma unroll
    for (int j = 0; j < kPiColsPerThread; ++j) if (ok[j]) packed_rate[pos++] = r[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPiColsPerThread; ++j) {
        const int idx = j * kPiBlock + (int)threadIdx.x;
        ok[j] = idx < total;
        r[j] = ok[j] ? packed_rate[idx] : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// The net-PI time tiles of pi_partial_kernel.  The tile's sixteen times are converted to double once per tile, not once per
// column (the same conversion: the same bits).  The rates are packed through the transpose buffer: 34 KB of LDS and 128
// VGPRs, four workgroups per CU, one wave of each per SIMD.
__global__ __launch_bounds__(kPiBlock, 4) void pi_net_kernel(PiParams P) {
    __shared__ double tile[kTimeTile][16 * 17];
    static_assert(kTimeTile * 16 * 17 >= kPiChunk, "the transpose buffer holds a chunk's packed rates");
    const int chunk = blockIdx.x;
    const int locus = P.chunk_locus[chunk];
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const int64_t base = lo + (int64_t)P.chunk_index[chunk] * kPiChunk;
    double r[kPiColsPerThread];
    bool ok[kPiColsPerThread];
    pi_pack_chunk(P, base, hi, &tile[0][0], r, ok);
    __syncthreads();
    double* out = P.partial + (size_t)chunk * (P.T + 2 * P.n_i);
    for (int t0 = 0; t0 < P.T; t0 += kTimeTile) {
        double acc[kTimeTile], t[kTimeTile];
#pragma unroll
        for (int i = 0; i < kTimeTile; ++i) { acc[i] = 0.0; t[i] = (double)(t0 + i); }
#pragma unroll
        for (int j = 0; j < kPiColsPerThread; ++j) {
            if (!ok[j]) continue;
            const double c = 16.0 * (r[j] * r[j]);
            const double q = exp(-(4.0 * r[j]));
            double p = exp(-(4.0 * r[j] * (double)t0));
#pragma unroll
            for (int i = 0; i < kTimeTile; ++i) {
                acc[i] = fma(c * t[i], p, acc[i]);
                p *= q;
            }
        }
        // (the transpose-and-add of pi_partial_kernel)
        {
            const int slot = (threadIdx.x >> 4) * 17 + (threadIdx.x & 15);
#pragma unroll
            for (int i = 0; i < kTimeTile; ++i) tile[i][slot] = acc[i];
        }
        __syncthreads();
        {
            const int i = threadIdx.x >> 4, seg = threadIdx.x & 15;
            const double* src = &tile[i][seg * 17];
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) sum += src[k];
            sum += __shfl_xor(sum, 8);
            sum += __shfl_xor(sum, 4);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 1);
            if (seg == 0 && t0 + i < P.T) out[t0 + i] = sum;
        }
        __syncthreads();
    }
}

// The generic first panel (4 r hl >= 30: a few hundred columns in millions) out of line, so that its 21 exponentials and
// the call into dqagse_adaptive cost the factored path no registers.
struct QuadResult { double result, abserr; };
__device__ __noinline__ QuadResult quad_townsend_generic(double a, double b, double rate) {
    QuadResult o;
    o.abserr = 0.0;
    quad_townsend<false>(a, b, rate, nullptr, o.result, o.abserr);
    return o;
}

// The interval integrals of pi_partial_kernel in register tiles of kIvSplitTile intervals:
//   * only the factored panel is inline: the generic panel and the adaptive bisection are calls behind branches that almost
//     no wave takes;
//   * a column's rate is read from the packed list when its turn comes, its slots are the thread's first n_ok;
//   * what a panel derives from the interval's bounds alone is derived per column, where it is used (below).
// 234 VGPRs, two waves per SIMD.  A build for three (168 VGPRs: the twenty factors of a column in LDS instead of registers) was
// measured and is slower by what the LDS traffic costs: the kernel's time is its vector instructions.
// Per (thread, interval) the columns are added in the order j = 0..3, then lanes, then waves, as in pi_partial_kernel.
constexpr int kIvSplitTile = 4;
__global__ __launch_bounds__(kPiBlock, 2) void pi_interval_kernel(PiParams P) {
    __shared__ double red[2 * kIvSplitTile][4];
    __shared__ double packed_rate[kPiChunk];
    const int chunk = blockIdx.x;
    const int locus = P.chunk_locus[chunk];
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const int64_t base = lo + (int64_t)P.chunk_index[chunk] * kPiChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n_ok = 0;   // the thread's contributing slots are its first n_ok: slot j is the packed index j * kPiBlock + threadIdx.x
    {
        double r[kPiColsPerThread];
        bool ok[kPiColsPerThread];
        pi_pack_chunk(P, base, hi, packed_rate, r, ok);
#pragma unroll
        for (int j = 0; j < kPiColsPerThread; ++j) n_ok += ok[j] ? 1 : 0;
    }
    double* out = P.partial + (size_t)chunk * (P.T + 2 * P.n_i);
    for (int k0 = 0; k0 < P.n_i; k0 += kIvSplitTile) {
        int a[kIvSplitTile], b[kIvSplitTile];   // wave-uniform; entries past n_i repeat the last interval and are not used
#pragma unroll
        for (int kk = 0; kk < kIvSplitTile; ++kk) {
            const int k = (k0 + kk < P.n_i) ? k0 + kk : P.n_i - 1;
            a[kk] = __builtin_amdgcn_readfirstlane(P.intervals[2 * k]);
            b[kk] = __builtin_amdgcn_readfirstlane(P.intervals[2 * k + 1]);
        }
        double si[kIvSplitTile], se[kIvSplitTile];
#pragma unroll
        for (int kk = 0; kk < kIvSplitTile; ++kk) { si[kk] = 0.0; se[kk] = 0.0; }
#pragma unroll 1
        for (int j = 0; j < n_ok; ++j) {
            const double rj = packed_rate[j * kPiBlock + (int)threadIdx.x];
            GkFactors F;
            double have_h = -1.0;        // half-length the factors in F were built for
#pragma unroll
            for (int kk = 0; kk < kIvSplitTile; ++kk) {
                if (k0 + kk < P.n_i) {   // wave-uniform
                    // The bounds are the same for every column, and so is all that a panel derives from them alone: the
                    // bounds as doubles, centre, half-length, the 21 abscissae.  Hoisted out of the column loop those are
                    // 44 live doubles per interval of the tile, next to the column's own values.  The empty asm makes the
                    // bounds (two SGPRs) this column's own, so that all of it is derived again where it is used (the
                    // arithmetic the panel is written with).
                    int ai = a[kk], bi = b[kk];
                    asm volatile("" : "+s"(ai), "+s"(bi));
                    const double aj = (double)ai, bj = (double)bi;
                    double res, err = 0.0;
                    if (P.integ_mode == TPHIP_INTEG_QUADPACK) {
                        const double hl = 0.5 * (bj - aj);
                        if (4.0 * rj * hl < 30.0) {          // per lane: a huge rate takes the generic panel
                            if (hl != have_h) { gk_factors(rj, hl, F); have_h = hl; }
                            quad_townsend_factored(aj, bj, rj, F, res, err);
                        } else {
                            const QuadResult g = quad_townsend_generic(aj, bj, rj);
                            res = g.result;
                            err = g.abserr;
                        }
                    } else {
                        res = integral_closed(aj, bj, rj);
                    }
                    si[kk] += res;
                    se[kk] += err;
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < kIvSplitTile; ++kk) {
            if (k0 + kk < P.n_i) {
                const double s1 = wave_sum(si[kk]), s2 = wave_sum(se[kk]);
                if (lane == 0) { red[2 * kk][wave] = s1; red[2 * kk + 1][wave] = s2; }
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 * kIvSplitTile && k0 + (int)(threadIdx.x >> 1) < P.n_i) {
            const int kk = threadIdx.x >> 1, which = threadIdx.x & 1;
            out[P.T + which * P.n_i + k0 + kk] =
                ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
        }
        __syncthreads();
    }
}

// tables[l] = [net(T) | disc(n_t) | integral(n_i) | error(n_i)], summing the locus' chunks in order.  A thread's sum
// is a chain of dependent adds whose operands are independent loads: they are requested eight at a time, so the chain
// waits for one memory round trip per eight chunks instead of one per chunk (the order of the adds is unchanged).
// 64 threads: with 128 (one thread per entry on the C2-C5 rows) site_rate_kernel of the next pass ran 22 % slower on C2
// (0.36 -> 0.45 ms at the same evaluation count), the front-of-kernel effect noted at dedup_estimate_kernel
constexpr int kPiReduceBlock = 64;
__global__ __launch_bounds__(kPiReduceBlock) void pi_reduce_kernel(const double* __restrict__ partial, const int64_t* __restrict__ locus_chunk_offsets,
                                 int32_t T, const int32_t* __restrict__ times, int32_t n_t, int32_t n_i,
                                 double* __restrict__ tables) {
    const int locus = blockIdx.x;
    const int64_t c0 = locus_chunk_offsets[locus], c1 = locus_chunk_offsets[locus + 1];
    const int Wp = T + 2 * n_i, W = T + n_t + 2 * n_i;
    double* row = tables + (size_t)locus * W;
    for (int w = threadIdx.x; w < Wp + n_t; w += blockDim.x) {
        // w < Wp: a partial column; else a --times entry, which is net[times[k]] (tapir/compute.py:76-79)
        const int src = (w < Wp) ? w : times[w - Wp];
        double s = 0.0;
        int64_t c = c0;
        for (; c + 8 <= c1; c += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(c + u) * Wp + src];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; c < c1; ++c) s += partial[(size_t)c * Wp + src];
        const int dst = (w < T) ? w : (w < Wp ? w + n_t : T + (w - Wp));
        row[dst] = s;
    }
}

// parse_site_rates + cull_uninformative_rates as the PI kernels see a rate (tapir/compute.py:38-39, 108-110):
// out[c] = round4(rate[c]) / correction, NaN where nres[c] < threshold (nres may be null: no cull).
__global__ void corrected_rates_kernel(PiParams P, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = finalize_rate(P, i);
}

// tapir/compute.py:46-48 as a dense (n_times, n) matrix: out[k*n + i] = 16 r_i^2 t_k exp(-4 r_i t_k).
// Pure streaming: 8 B read per site, 8*n_times B written; consecutive lanes write consecutive doubles.
__global__ void townsend_dense_kernel(const double* __restrict__ rates, int64_t n, const double* __restrict__ times,
                                      int32_t n_times, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double r = rates[i];
    for (int k = 0; k < n_times; ++k) out[(size_t)k * n + i] = townsend_pi<false>(times[k], r, nullptr);
}

// tapir/compute.py:50-52 vectorised over sites (what numpy.vectorize(get_integral_over_times) returns)
__global__ void quad_sites_kernel(const double* __restrict__ rates, int64_t n, double a, double b, int32_t integ_mode,
                                  double* __restrict__ integral, double* __restrict__ abserr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double r = rates[i];
    double res = __longlong_as_double(0x7ff8000000000000ll), err = res;
    if (isfinite(r)) {
        err = 0.0;
        if (integ_mode == TPHIP_INTEG_QUADPACK) quad_townsend<false>(a, b, r, nullptr, res, err);
        else res = integral_closed(a, b, r);
    }
    integral[i] = res;
    abserr[i] = err;
}

// per-locus histogram of the 16 state masks (HarvestFrequencies, bf:968)
__global__ __launch_bounds__(256) void state_histogram_kernel(const uint8_t* __restrict__ states, int64_t ncols_total,
                                                              int32_t ntaxa, const int64_t* __restrict__ locus_offsets,
                                                              unsigned long long* __restrict__ hist) {
    __shared__ unsigned int h[16];
    const int locus = blockIdx.x;
    const int64_t lo = locus_offsets[locus], hi = locus_offsets[locus + 1];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    unsigned int mine[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) mine[m] = 0;
    for (int t = 0; t < ntaxa; ++t) {
        const uint8_t* row = states + (int64_t)t * ncols_total;
        for (int64_t c = lo + threadIdx.x; c < hi; c += blockDim.x) {
            unsigned m = row[c] & 15u;
            m = m ? m : 15u;
#pragma unroll
            for (int k = 0; k < 16; ++k) mine[k] += (m == (unsigned)k);
        }
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        unsigned v = mine[m];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(&h[m], v);
    }
    __syncthreads();
    if (threadIdx.x < 16) hist[(size_t)locus * 16 + threadIdx.x] = h[threadIdx.x];
}

}  // namespace tphip

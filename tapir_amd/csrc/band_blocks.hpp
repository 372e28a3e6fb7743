// band_blocks.hpp -- how the replicate-band stages (site bootstrap; parametric bootstrap, 3.7; posterior
// PI, 3.10) cut their work to the caller's workspace: exact byte arithmetic on plain integers, decided on the host alone.  No
// HIP header and nothing else of the project: tests/native/band_blocks_dump.cpp compiles it with g++ (tests/test_band_blocks.py).
// A block is a run of consecutive loci whose regions fit the usable bytes together.  No kernel's arithmetic looks beyond its
// own locus and a replicate row is computed from the locus' own columns in a fixed order, so the blocking changes no bit.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace tphip {

constexpr size_t kBandAlign = 256;                     // every region of a workspace starts on a multiple of it
constexpr size_t kBandPreferredCap = (size_t)1 << 30;  // like stage 1's chunks: about 1 GiB of workspace at most
constexpr int kBandMaxReplicates = 4096;               // the summary kernel sorts one entry's replicates in 32 KB of LDS
constexpr int64_t kBandMaxBlockLoci = 65535;           // loci of a block: a grid dimension of the kernels

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// the first aligned address in (address, bytes) and what is left from there on (0 when the padding eats it all)
struct BandBase { uintptr_t base; size_t usable; };
inline BandBase band_base(uintptr_t address, size_t bytes) {
    const uintptr_t b = (address + kBandAlign - 1) / kBandAlign * kBandAlign;
    return {b, bytes > (size_t)(b - address) ? bytes - (size_t)(b - address) : 0};
}

// fixed = what every call needs, one = the largest single block's regions, all = every locus at once
struct BandBytes { size_t min, preferred; };
inline BandBytes band_bytes(size_t fixed, size_t one, size_t all) {
    return {fixed + one, fixed + std::max(one, std::min(all, kBandPreferredCap))};
}

inline size_t band_ids_bytes(int64_t nloci) { return align_up(sizeof(int64_t) * (size_t)nloci, kBandAlign); }
inline size_t band_rows_bytes(size_t loci, size_t reps, size_t Wb) { return align_up(sizeof(double) * loci * reps * Wb, kBandAlign); }

// ---- site bootstrap: per-site integrals [columns][n_i], counts [replicates][pitch] of 16-bit counters, rows [loci][B][Wb] ----
inline size_t bs_pitch(int64_t cols) { return (size_t)((cols + 1) & ~(int64_t)1); }   // whole 32-bit words per row
inline size_t bs_integ_bytes(int64_t cols, int32_t n_i) { return align_up(sizeof(double) * (size_t)cols * (size_t)n_i, kBandAlign); }
inline size_t bs_counts_bytes(int64_t cols, int64_t reps) { return align_up(sizeof(uint16_t) * bs_pitch(cols) * (size_t)reps, kBandAlign); }
inline size_t bs_block_bytes(int64_t cols, int64_t loci, int64_t reps, int64_t B, int32_t n_i, int32_t Wb) {
    return bs_integ_bytes(cols, n_i) + bs_counts_bytes(cols, reps) + band_rows_bytes((size_t)loci, (size_t)B, (size_t)Wb);
}

// offsets[nloci + 1]; tile = replicates drawn together when a locus goes through the workspace in ranges (whole replicate
// tiles of the matrix kernel)
inline BandBytes bootstrap_bytes(const int64_t* offsets, int64_t nloci, int32_t n_i, int32_t Wb, int64_t B, int64_t tile) {
    size_t one = 0;
    for (int64_t l = 0; l < nloci; ++l)
        one = std::max(one, bs_block_bytes(offsets[l + 1] - offsets[l], 1, std::min(B, tile), B, n_i, Wb));
    return band_bytes(kBandAlign + band_ids_bytes(nloci), one, bs_block_bytes(offsets[nloci] - offsets[0], nloci, B, B, n_i, Wb));
}

// The block that starts at locus l0, as [l0, l1) and the replicates drawn at a time: as many consecutive loci as fit with all
// B replicates' counts (65535 at most); a locus that does not fit alone goes in ranges of whole tiles, as large as fit.
// `usable` holds at least the minimum of bootstrap_bytes less its fixed part.
struct BsBlock { int64_t l1, range; };
inline BsBlock bootstrap_next_block(const int64_t* offsets, int64_t nloci, int64_t l0, int32_t n_i, int32_t Wb, int64_t B, int64_t tile,
                                    size_t usable) {
    int64_t l1 = l0;
    while (l1 < nloci && l1 - l0 < kBandMaxBlockLoci && bs_block_bytes(offsets[l1 + 1] - offsets[l0], l1 + 1 - l0, B, B, n_i, Wb) <= usable)
        ++l1;
    if (l1 > l0) return {l1, B};
    const int64_t n = offsets[l0 + 1] - offsets[l0];
    const size_t left = usable - bs_block_bytes(n, 1, 0, B, n_i, Wb);   // what the integrals and the rows leave for counts
    int64_t range = std::min(B, tile);
    while (range + tile <= B && bs_counts_bytes(n, range + tile) <= left) range += tile;
    return {l0 + 1, range};
}

// resampling on the caller's counts keeps the integrals only: consecutive loci as far as the bytes reach, one at least
inline BandBytes resample_bytes(int64_t max_locus_cols, int64_t ncols, int32_t n_i) {
    return band_bytes(kBandAlign, bs_integ_bytes(max_locus_cols, n_i), bs_integ_bytes(ncols, n_i));
}
inline int64_t resample_next_block(const int64_t* offsets, int64_t nloci, int64_t l0, int32_t n_i, size_t usable) {
    int64_t l1 = l0;
    while (l1 < nloci && (l1 == l0 || bs_integ_bytes(offsets[l1 + 1] - offsets[l0], n_i) <= usable)) ++l1;
    return l1;
}

// ---- posterior PI: category rows [loci][K][Wb], counts [loci][B][K] of int32, rows [loci][B][Wb]; every locus needs the same ----
inline size_t pp_ptab_bytes(size_t loci, size_t K, size_t Wb) { return align_up(sizeof(double) * loci * K * Wb, kBandAlign); }
inline size_t pp_counts_bytes(size_t loci, size_t B, size_t K) { return align_up(sizeof(int32_t) * loci * B * K, kBandAlign); }
inline size_t pp_block_bytes(size_t loci, size_t K, size_t B, size_t Wb) {
    return pp_ptab_bytes(loci, K, Wb) + pp_counts_bytes(loci, B, K) + band_rows_bytes(loci, B, Wb);
}
inline BandBytes posterior_bytes(int64_t nloci, size_t K, size_t B, size_t Wb) {
    const int64_t L = nloci ? nloci : 1;
    return band_bytes(kBandAlign + band_ids_bytes(L), pp_block_bytes(1, K, B, Wb), pp_block_bytes((size_t)L, K, B, Wb));
}
// loci per block: the most whose three regions fit, one at least and 65535 at most
inline size_t posterior_block_loci(size_t nloci, size_t K, size_t B, size_t Wb, size_t usable) {
    size_t lo = 1, hi = std::min<size_t>(nloci, (size_t)kBandMaxBlockLoci);
    while (lo < hi) {
        const size_t mid = (lo + hi + 1) / 2;
        if (pp_block_bytes(mid, K, B, Wb) <= usable) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- parametric bootstrap: one replicate of states, the per-column outputs of the site-rate stage, one table [loci][W], the
// rows, the moments and the plan's own workspace; total allows for aligning the caller's pointer up ----
struct ParbootLayout { size_t states, rate, subst, lnl, flag, nres, tables, rows, mean, m2, plan_ws, total; };
inline ParbootLayout parboot_layout(size_t ntaxa, size_t ncols, size_t nloci, size_t W, size_t Wb, size_t B, size_t plan_ws_bytes) {
    ParbootLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = align_up(off + bytes, kBandAlign); return at; };
    L.states = take(ntaxa * ncols);
    L.rate = take(sizeof(double) * ncols);
    L.subst = take(sizeof(double) * ncols);
    L.lnl = take(sizeof(double) * ncols);
    L.flag = take(ncols);
    L.nres = take(sizeof(int32_t) * ncols);
    L.tables = take(sizeof(double) * nloci * W);
    L.rows = take(sizeof(double) * nloci * B * Wb);
    L.mean = take(sizeof(double) * ncols);
    L.m2 = take(sizeof(double) * ncols);
    L.plan_ws = take(plan_ws_bytes);
    L.total = off + kBandAlign;
    return L;
}

}  // namespace tphip

// launch_constants.hpp -- the constants that the kernels and the host's launch decisions (site_launch_plan.hpp,
// locus_launch_plan.hpp) share.
// No HIP header: the two decision headers and their test programs compile with a plain C++ compiler.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tphip {

// ---- site-rate kernels (site_rate_params.hpp, site_rate_kernel.hpp) ----
constexpr int kFirstStepMinTaxa = 32;   // trees from this size on use the parsimony length in the optimiser's first step (pi_kernels.hpp)
constexpr int kSiteBlock = 64;      // one wavefront per workgroup
constexpr int kReserveShift = 16;     // the reserved fraction of a locus' easy columns is reserve_q / 2^16 (reserved_before)
constexpr int kShareWeightShift = 10; // predicted evaluations per column of a class, in units of 2^-10 (the weighted scan stays exact)
constexpr double kDefaultReserve = 0.15;  // shares by predicted work (SiteParams::share_work): this fraction of every locus' easy columns
                                          //   forms its reserved tail; TPHIP_SITE_RESERVE
// the later shares' cut of the reserved tails (tail_shares.hpp): lane-fills per share in the three bands, and the fractions of
// the tails that the first two take; TPHIP_SITE_TAIL_SHARES (chosen with tools/share_replay.py: profiles/r17_tail_share_sweep.txt)
constexpr int kTailFillsBig = 5, kTailFillsMid = 3, kTailFillsSmall = 2;
constexpr double kTailFracBig = 0.4, kTailFracMid = 0.3;
constexpr int kMixedLoci = 8;       // loci whose columns a wave of the mixed-loci mode carries at a time (site_rate_kernel.hpp)
constexpr int kMixedLdsHeader = kMixedLoci * 64 + 64 + 32;   // doubles: tip tables, 2^(j/64), segment table
constexpr int kMixedColBits = 28;    // a work entry of that mode = column | locus-in-group << 28: batches below 2^28 columns
constexpr int kSiteLdsHeader = 160;  // doubles of LDS before the stack: tip table [16][4] + model [32] + 2^(j/64) [64]
constexpr int kStreamWords = -1;   // NW value of the streamed-words path
constexpr int kStreamWordsSpill = -2;   // launcher variant: streamed words + SPILL
constexpr int kMixedVariant = 100;   // launcher variants 102 / 108: packed words in registers, mixed-loci mode

// ---- stage-1 likelihood and gradient kernels (locus_*_kernel.hpp; launch decisions: locus_launch_plan.hpp) ----
#ifndef TPHIP_LIK_BLOCK
#define TPHIP_LIK_BLOCK 128   // threads per workgroup of the locus likelihood kernels (a build-time knob for A/B runs)
#endif
constexpr int kLikBlock = TPHIP_LIK_BLOCK;
constexpr int kGradBlock = 128;
constexpr int kGradWaves = kGradBlock / 64;
constexpr int kGradEF = 12;     // per node: e^{lam_k t}[4], F01 F02 F03 F12 F13 F23, t, pad
constexpr int kGradSlots = 4;   // LDS accumulator addresses per (wave, branch); fewer (GradParams.nslots) on big trees
constexpr size_t kValueWorkspaceBytes = (size_t)1 << 30;
constexpr int kValueTipRow = 20;     // doubles per taxon in the LDS tip table: 4 rows of P^T + a row of ones
constexpr int kValueMaxDepth = 5;   // deepest register stack instantiated (a Sethi-Ullman-ordered tree of 2^(D+1) tips needs D)
constexpr int kGrad2Block = 128;
constexpr int kGrad2Waves = kGrad2Block / 64;
constexpr int kGrad2EF = 12;        // per (candidate, node): e^{lam_k t}[4], F01 F02 F03 F12 F13 F23, t, pad
constexpr int kGrad2MaxRDepth = 8;  // parked adjoints of the reverse sweep (LDS): log2(taxa) on a balanced tree

// ---- classification and PI kernels (pi_kernels.hpp) ----
constexpr int kPiBlock = 256;
constexpr int kPiColsPerThread = 4;
constexpr int kPiChunk = kPiBlock * kPiColsPerThread;  // 1024 columns per workgroup

// ---- site-pattern de-duplication (dedup_kernels.hpp) ----
enum : int32_t { DEDUP_AUTO = 0, DEDUP_OFF = 1, DEDUP_ON = 2 };
// Batches below this many columns are not de-duplicated in automatic mode: they run in the latency-bound small-batch
// modes of site_rate_kernel (a launch lasts as long as its slowest wave), where fewer columns hardly shorten the kernel and the four extra
// launches cost more than they save (C2, 5e5 columns: 0.50 -> 0.53 ms per step with the machinery idling).
constexpr int64_t kDedupAutoMinColumns = 1 << 20;

}  // namespace tphip

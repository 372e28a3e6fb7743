// locus_launch_plan.hpp -- how the stage-1 kernels of a plan (locus likelihood, value, the two gradients) will run, decided on
// the host from the tree's sizes, the CU count, the kernels' answers about LDS and occupancy and two knobs; and the pure
// arithmetic of a call: column slices, candidate chunks, tape sizes and the layout of the gradient's outputs.  The stage-1
// sibling of site_launch_plan.hpp: no HIP header, no environment.  locus_driver.hip calls it, and
// tests/native/locus_launch_dump.cpp compiles it with g++ so that every decision is checked without a GPU
// (tests/test_locus_launch.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "launch_constants.hpp"
#include "site_launch_plan.hpp"   // PlanKnobs

namespace tphip {

// What the decision sees of a plan's tree and batch.
struct LocusShape {
    int32_t ntaxa = 0, nnodes = 0;
    int32_t nwords = 0;          // packed tip words per column: ceil(tips / 8)
    int32_t stack_depth = 0;     // TreeProgram::stack_depth
    int32_t ntape = 0;           // TreeProgram::ntape: tape slots of locus_grad_kernel's forward sweep
    int64_t max_locus_cols = 0;  // longest locus at plan creation
    int32_t value_nops = 0;      // records of locus_value_kernel's op stream, 0: the tree's program cannot be expressed in it
    bool grad2_built = false;    // locus_grad2_kernel's programs exist (binary tree, reverse depth within kGrad2MaxRDepth)
    int32_t grad2_rdepth = 0, grad2_ntape = 0;
};

// Launch configuration of the stage-1 kernels, fixed at plan creation.
struct LocusLaunch {
    size_t lik_lds = 0;          // locus_loglik_kernel (eigenbasis value kernel)
    bool lik_ok = false;
    int32_t value_cols = 0;      // columns per thread of locus_value_kernel (0: it does not run, the eigenbasis kernel does)
    size_t value_lds = 0;
    size_t grad_lds = 0;         // locus_grad_kernel: LDS bytes, whether it stages its state masks, accumulator addresses per
    int32_t grad_stage = 0;      // (wave, branch), resident workgroups per CU
    int32_t grad_slots = kGradSlots;
    int32_t grad_blocks_per_cu = 1;
    bool grad_ok = false;
    bool grad2_ok = false;       // locus_grad2_kernel
    size_t grad2_lds = 0;
    int32_t grad2_blocks_per_cu = 1;
};

enum LocusKernel : int { LOCUS_LIK = 0, LOCUS_VALUE = 1, LOCUS_GRAD = 2, LOCUS_GRAD2 = 3 };

// `allow_lds(kernel, cols, depth, lds_bytes)`: true when the kernel (for LOCUS_VALUE its <cols, depth> instance, for LOCUS_GRAD2 its
// <depth> instance) may be launched with that much dynamic LDS; asked only above 64 KiB, and only when the tests before it pass.
// `occupancy(kernel, depth, lds_bytes)`: resident workgroups per CU, 0 when the query failed; asked for a gradient kernel that runs.
template <typename AllowLds, typename Occupancy>
LocusLaunch decide_locus_launch(const LocusShape& shape, int num_cus, const PlanKnobs& knobs, AllowLds&& allow_lds, Occupancy&& occupancy) {
    LocusLaunch s;
    const size_t nnodes = (size_t)shape.nnodes, ntaxa = (size_t)shape.ntaxa, nwords = (size_t)shape.nwords;
    const int depth = shape.stack_depth;
    // locus likelihood (value) kernel: no staging of the state masks in LDS, which cost it more than it saved (measured
    // 13.6 ms vs 10.0 ms per 1616 candidates x 20000 columns x 64 taxa)
    s.lik_lds = (nnodes * 4 + (size_t)depth * 4 * kLikBlock) * sizeof(double);
    s.lik_ok = s.lik_lds <= 150 * 1024;
    if (s.lik_ok && s.lik_lds > 64 * 1024) s.lik_ok = allow_lds(LOCUS_LIK, 0, 0, (size_t)150 * 1024);
    // value kernel on transition matrices (locus_value_kernel.hpp): C columns per thread share the op decode and the
    // scalar loads of a branch's matrix; parked siblings live in registers (template depth), LDS holds the tip matrices
    // and the packed state masks.  (A tree whose two columns do not fit is not tried with one.)
    {
        int cols = shape.max_locus_cols >= 512 ? 2 : 1;
        if (knobs.value_cols) cols = *knobs.value_cols;
        if (shape.value_nops > 0 && depth <= kValueMaxDepth && !knobs.value_eigenbasis) {
            const size_t need = ntaxa * kValueTipRow * sizeof(double) + nwords * cols * kLikBlock * sizeof(uint32_t);
            if (need <= 96 * 1024 && (need <= 64 * 1024 || allow_lds(LOCUS_VALUE, cols, depth, (size_t)96 * 1024))) {
                s.value_cols = cols;
                s.value_lds = need;
            }
        }
    }
    // gradient kernel: staging helps it (95.6 -> 91.7 ms)
    s.grad_slots = kGradSlots;   // fewer accumulator addresses per branch when the tree would not fit otherwise
    while (s.grad_slots > 1 && nnodes * (kGradEF + 2 * kGradWaves * s.grad_slots) * sizeof(double) > 100 * 1024) s.grad_slots >>= 1;
    s.grad_lds = nnodes * (kGradEF + 2 * kGradWaves * s.grad_slots) * sizeof(double);
    const size_t grad_stage_bytes = ntaxa * kGradBlock;
    s.grad_stage = (grad_stage_bytes <= 48 * 1024 && s.grad_lds + grad_stage_bytes <= 150 * 1024) ? 1 : 0;
    if (s.grad_stage) s.grad_lds += grad_stage_bytes;
    s.grad_ok = s.grad_lds <= 150 * 1024;
    if (s.grad_ok && s.grad_lds > 64 * 1024) s.grad_ok = allow_lds(LOCUS_GRAD, 0, 0, (size_t)150 * 1024);
    if (s.grad_ok) {
        int bpc = occupancy(LOCUS_GRAD, 0, s.grad_lds);
        if (bpc < 1) bpc = 1;
        // the tape of the resident blocks should stay within reach of the 256 MB memory-side cache: with 64 taxa, 4
        // blocks per CU (390 MB of tape) ran slower than 3 (91 vs 85 ms); fewer than 3 loses more to latency
        const size_t tape_per_block = (size_t)std::max(1, shape.ntape + depth) * 4 * kGradBlock * sizeof(double);
        if (tape_per_block * (size_t)num_cus * (size_t)bpc > ((size_t)300 << 20)) bpc = std::min(bpc, 3);
        s.grad_blocks_per_cu = bpc;
    }
    // transition-matrix gradient kernel: LDS = tip table + tipY + parked adjoints + per-branch accumulators + state codes
    if (shape.grad2_built) {
        s.grad2_lds = (ntaxa * kValueTipRow + 64 + (size_t)shape.grad2_rdepth * 4 * kGrad2Block + 2 * (size_t)kGrad2Waves * nnodes) * sizeof(double) +
                      nwords * kGrad2Block * sizeof(uint32_t);
        s.grad2_ok = s.value_cols > 0 && s.grad2_lds <= 96 * 1024 &&
                     (s.grad2_lds <= 64 * 1024 || allow_lds(LOCUS_GRAD2, 0, depth, (size_t)96 * 1024));
        if (s.grad2_ok) {
            const int bpc = occupancy(LOCUS_GRAD2, depth, s.grad2_lds);
            s.grad2_blocks_per_cu = bpc < 1 ? 1 : bpc;
        }
    }
    return s;
}

// ---- per call (max_locus_cols is the plan's at the time of the call: a pattern view of stage 1 swaps it) ----

// Slices per candidate for the locus likelihood / gradient kernels: enough work items to fill the device even when
// only a few candidates are in flight (the general model's one point per locus), never more than a locus has blocks.
inline int lik_nsplit(int num_cus, int64_t max_locus_cols, int64_t ncand, int block) {
    const int64_t target = (int64_t)num_cus * 8;
    int64_t ns = (target + ncand - 1) / std::max<int64_t>(ncand, 1);
    const int64_t max_blocks = std::max<int64_t>(1, (max_locus_cols + block - 1) / block);
    ns = std::min(ns, max_blocks);
    return (int)std::max<int64_t>(1, std::min<int64_t>(ns, 4096));
}

constexpr int64_t kMaxGridX = (int64_t)1 << 30;   // work items of one launch

// Workspace per candidate and candidates per chunk of the value path (eigen-system [36] + transition matrices [nnodes][16]) ...
inline size_t value_ws_per_cand(int nnodes) { return ((size_t)nnodes * 16 + 36) * sizeof(double); }
inline int64_t value_chunk(int nnodes, int64_t ncand, int nsplit) {
    int64_t chunk = std::max<int64_t>(1, (int64_t)(kValueWorkspaceBytes / value_ws_per_cand(nnodes)));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, kMaxGridX / nsplit));
    return std::min<int64_t>(chunk, ncand);
}
// ... and of the transition-matrix gradient (the same + branch tables [nnodes][kGrad2EF]): 4 GiB of workspace at the most
inline size_t grad2_ws_per_cand(int nnodes) { return (36 + (size_t)nnodes * (16 + kGrad2EF)) * sizeof(double); }
inline int64_t grad2_chunk(int nnodes, int64_t ncand) {
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(((size_t)4 << 30) / grad2_ws_per_cand(nnodes)));
    return std::min<int64_t>(chunk, ncand);
}

// Tape of `grid` resident workgroups: locus_grad_kernel's forward slots and adjoint stack, locus_grad2_kernel's branch messages.
inline size_t grad_tape_bytes(int64_t grid, int ntape, int stack_depth) {
    return (size_t)grid * (size_t)std::max(1, ntape + stack_depth) * 4 * kGradBlock * sizeof(double);
}
inline size_t grad2_tape_bytes(int64_t grid, int grad2_ntape) {
    return (size_t)grid * (size_t)std::max(1, grad2_ntape) * 4 * kGrad2Block * sizeof(double);
}

// The gradient's outputs as one block of doubles: lnl[items] | sum_dlogt[items] | dexch[items][6] | dlogt[items][nnodes]
// (optional) | d2logt[items][nnodes] (optional).  items = candidates x slices for the kernels' partial sums, = candidates for the
// host wrapper's staging buffer.  An output that is not wanted has no room; its offset is not to be used.
struct GradOutLayout {
    size_t lnl = 0, sum_dlogt = 0, dexch = 0, dlogt = 0, d2logt = 0, total = 0;
    GradOutLayout(size_t items, size_t nnodes, bool want_dlogt, bool want_d2logt) {
        sum_dlogt = items;
        dexch = 2 * items;
        dlogt = 8 * items;
        d2logt = dlogt + (want_dlogt ? nnodes : 0) * items;
        total = d2logt + (want_d2logt ? nnodes : 0) * items;
    }
};

}  // namespace tphip

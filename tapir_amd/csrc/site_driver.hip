// site_driver.hip -- the device launches of stage 2 (site rates, then the PI tables) and their C entry points on device
// pointers, with the profiling slots and the evaluation counters; the front end of the empirical-Bayes calls, which runs the
// same classification and de-duplication kernels; and the stand-alone utilities on the kernels of pi_kernels.hpp (corrected
// rates, dense Townsend PI, QUADPACK probe, state histogram) and the eval diagnostic.  How a plan's site-rate kernel is
// launched is site_launch_plan.hpp's to say (decide_site_launch at plan creation, site_kernel_args here): nothing in this
// file reads the environment to choose anything.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "dedup_kernels.hpp"
#include "pi_kernels.hpp"
#include "tphip_internal.hpp"

extern "C" {

int tphip_profile_enable(tphip_plan* p, int32_t on) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    if (on && p->ev.empty()) {
        p->ev.resize(4 * kProfileRing);
        for (auto& e : p->ev) HIP_TRY(hipEventCreate(&e));
    }
    p->profile = on != 0;
    return TPHIP_OK;
}

static int profile_drain(tphip_plan* p) {
    for (int s = 0; s < p->ev_used; ++s) {
        float ms = 0;
        HIP_TRY(hipEventSynchronize(p->ev[4 * s + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, p->ev[4 * s + 0], p->ev[4 * s + 1]));
        p->acc_site_ms += ms;
        HIP_TRY(hipEventSynchronize(p->ev[4 * s + 3]));
        HIP_TRY(hipEventElapsedTime(&ms, p->ev[4 * s + 2], p->ev[4 * s + 3]));
        p->acc_pi_ms += ms;
        ++p->acc_launches;
    }
    p->ev_used = 0;
    return TPHIP_OK;
}

int tphip_profile_read(tphip_plan* p, double* site_ms, double* pi_ms, int64_t* launches, int32_t reset) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    int rc = profile_drain(p);
    if (rc) return rc;
    if (site_ms) *site_ms = p->acc_site_ms;
    if (pi_ms) *pi_ms = p->acc_pi_ms;
    if (launches) *launches = p->acc_launches;
    if (reset) { p->acc_site_ms = p->acc_pi_ms = 0; p->acc_launches = 0; }
    return TPHIP_OK;
}

// d_evals[which] of the last site-rate launch: [0] evaluations, [1] evaluation rounds
static int last_count(tphip_plan* p, int which, int64_t* out) {
    if (!p || !out) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long v = 0, w = 0;
    if (p->last_run_in_parts) {   // the last site-rate launch was a host-pointer pipeline of locus groups: their sum
        for (tphip_plan* q : p->parts) {
            HIP_TRY(hipMemcpy(&w, q->d_evals.p + which, sizeof w, hipMemcpyDeviceToHost));
            v += w;
        }
    } else {
        HIP_TRY(hipMemcpy(&v, p->d_evals.p + which, sizeof v, hipMemcpyDeviceToHost));
    }
    *out = (int64_t)v;
    return TPHIP_OK;
}

int tphip_last_eval_count(tphip_plan* p, int64_t* evals) {
    const int rc = last_count(p, 0, evals);
    if (rc == TPHIP_OK && !p->last_run_in_parts && getenv("TPHIP_SITE_TRACE_ROUNDS")) {   // meaningful in a -DTPHIP_SITE_TRACE_ROUNDS build only
        unsigned long long c[8];
        HIP_TRY(hipMemcpy(c, p->d_evals.p, sizeof c, hipMemcpyDeviceToHost));
        if (c[5]) fprintf(stderr, "site_rate_kernel: %llu waves with work, evaluations %llu, rounds mean %.1f max %llu (lane use %.1f %%), wave time mean %.1f us max %.1f us\n",
                          c[5], c[0], (double)c[1] / c[5], c[2], 100.0 * c[0] / (64.0 * c[1]), 0.01 * c[3] / c[5], 0.01 * c[4]);
    }
    return rc;
}

int tphip_last_round_count(tphip_plan* p, int64_t* rounds) { return last_count(p, 1, rounds); }

// ---- launches ------------------------------------------------------------------------------------

// classify_kernel's block: where its per-column results and the packed tip words go; `hash` null = no de-duplication
static ClassifyParams classify_params(const tphip_plan* p, const uint8_t* d_states, double* rate, double* subst, double* lnl, uint8_t* flag,
                                      int32_t* nres, uint32_t* packed, uint64_t* hash, double start_scale) {
    ClassifyParams C{};
    C.states = d_states; C.ncols_total = p->ncols; C.ntaxa = p->ntaxa; C.models = p->d_models.p;
    C.locus_offsets = p->d_offsets.p; C.chunk_locus = p->d_pi_chunk_locus.p; C.chunk_index = p->d_pi_chunk_index.p;
    C.rate = rate; C.subst = subst; C.lnl = lnl; C.flag = flag; C.nres = nres;
    C.chrono_length = p->prog.chrono_length;
    C.steps = (const int2*)p->d_cls_steps.p; C.tail_pops = p->prog.cls_tail_pops; C.max_pops = p->prog.cls_max_pops;
    C.packed = packed; C.start_scale = start_scale; C.hash = hash;
    return C;
}

// The de-duplication kernels' block, on what classify_kernel left (C.hash, C.packed, C.flag).  `results`: dedup_scatter_kernel
// copies C's rate / subst / lnl from the representatives (null pointers otherwise: that kernel is not run).
static DedupParams dedup_params(const tphip_plan* p, const ClassifyParams& C, int32_t* dup_of, unsigned long long* tab_key,
                                int32_t* tab_val, int32_t* on, int32_t mode, bool results) {
    DedupParams D{};
    D.locus_offsets = p->d_offsets.p; D.chunk_locus = p->d_pi_chunk_locus.p; D.chunk_index = p->d_pi_chunk_index.p;
    D.hash = C.hash; D.packed = C.packed; D.nwords = p->nwords; D.ncols_total = p->ncols; D.flag = C.flag;
    D.dup_of = dup_of; D.tab_key = tab_key; D.tab_val = tab_val; D.on = on; D.mode = mode;
    if (results) { D.rate = C.rate; D.subst = C.subst; D.lnl = C.lnl; }
    return D;
}

// The work list of long loci by the chunk-parallel kernels (pi_kernels.hpp).  work_class != null: with the class counts and
// the reserved tails of the hand-out by predicted work (compact_classes_kernel's list), else compact_kernel's plain list.
static void launch_compact_chunked(tphip_plan* p, const uint8_t* d_flag, const double* d_lnl, int32_t* work_cols, int32_t* work_count,
                                  int32_t* work_class, void* ws, hipStream_t st) {
    int2* cnt = (int2*)((char*)ws + p->ws.chunk_cnt);
    const dim3 chunks((unsigned)p->n_pi_chunks), loci((unsigned)p->nloci), block(kCompactChunkBlock);
    if (work_class) {
        compact_count_kernel<true><<<chunks, block, 0, st>>>(d_flag, d_lnl, p->d_offsets.p, p->d_pi_chunk_locus.p, p->d_pi_chunk_index.p, cnt);
        compact_scan_kernel<true><<<loci, block, 0, st>>>(p->d_locus_pichunk_offsets.p, cnt, work_count, work_class);
        compact_scatter_kernel<true><<<chunks, block, 0, st>>>(d_flag, d_lnl, p->d_offsets.p, p->d_pi_chunk_locus.p, p->d_pi_chunk_index.p, cnt,
                                                               work_count, work_class, p->site.reserve_q, work_cols);
    } else {
        compact_count_kernel<false><<<chunks, block, 0, st>>>(d_flag, nullptr, p->d_offsets.p, p->d_pi_chunk_locus.p, p->d_pi_chunk_index.p, cnt);
        compact_scan_kernel<false><<<loci, block, 0, st>>>(p->d_locus_pichunk_offsets.p, cnt, work_count, nullptr);
        compact_scatter_kernel<false><<<chunks, block, 0, st>>>(d_flag, nullptr, p->d_offsets.p, p->d_pi_chunk_locus.p, p->d_pi_chunk_index.p, cnt,
                                                                work_count, nullptr, 0, work_cols);
    }
}

int launch_site_rates(tphip_plan* p, const uint8_t* d_states, double* d_rate, double* d_subst, double* d_lnl,
                      uint8_t* d_flag, int32_t* d_nres, void* ws, hipStream_t st, int slot) {
    p->last_run_in_parts = false;
    const auto at = [ws](size_t offset) { return (void*)((char*)ws + offset); };   // a region of the workspace (p->ws)
    int32_t* work_cols = (int32_t*)at(p->ws.work_cols);
    int32_t* work_count = (int32_t*)at(p->ws.work_count);
    int64_t* work_prefix = (int64_t*)at(p->ws.work_prefix);
    int64_t* slice_prefix = (int64_t*)at(p->ws.slice_prefix);
    const bool dedup = p->site.dedup_mode != DEDUP_OFF && p->n_pi_chunks > 0;
    const ClassifyParams C = classify_params(p, d_states, d_rate, d_subst, d_lnl, d_flag, d_nres, (uint32_t*)at(p->ws.packed),
                                             dedup ? (uint64_t*)at(p->ws.hash) : nullptr,
                                             (p->site.start_rule == TPHIP_START_REFERENCE) ? 0.0 : 1.0);
    DedupParams D{};
    if (dedup) D = dedup_params(p, C, (int32_t*)at(p->ws.dup_of), (unsigned long long*)at(p->ws.tab_key), (int32_t*)at(p->ws.tab_val),
                                (int32_t*)at(p->ws.dedup_on), p->site.dedup_mode, true);
    if (p->n_pi_chunks > 0) {
        classify_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(kPiBlock), 0, st>>>(C);
        if (dedup) {   // one rate per unique site pattern (bf:1033-1044); loci that hardly repeat a column skip it
            if (p->max_locus_cols > 2048) dedup_estimate_kernel<1024><<<dim3((unsigned)p->nloci), dim3(1024), 0, st>>>(D);
            else dedup_estimate_kernel<256><<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(D);
            dedup_insert_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(D);
            dedup_resolve_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(D);
        }
        if (p->site.share_work) {
            // shares by predicted work: the list with class counts and reserved tails, and their scans (compact_classes_kernel
            // reads the marks, 8 more bytes per work column in its chain of barriers, and appends the tails: C3 47 -> 100 us;
            // long loci take the chunk-parallel kernels instead: 40 us)
            int32_t* work_class = (int32_t*)at(p->ws.work_class);
            if (p->site.compact_chunked) {
                launch_compact_chunked(p, d_flag, d_lnl, work_cols, work_count, work_class, ws, st);
            } else {
                int32_t* scratch = p->site.reserve_q > 0 ? (int32_t*)at(p->ws.work_cols2) : nullptr;
                if (p->max_locus_cols > 2048) compact_classes_kernel<1024><<<dim3((unsigned)p->nloci), dim3(1024), 0, st>>>(d_flag, p->d_offsets.p, work_cols, work_count, d_lnl, p->site.reserve_q, scratch, work_class);
                else compact_classes_kernel<256><<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(d_flag, p->d_offsets.p, work_cols, work_count, d_lnl, p->site.reserve_q, scratch, work_class);
            }
            ScanClasses SC;
            SC.cls = work_class; SC.reserve_q = p->site.reserve_q; SC.w_slow = p->site.w_slow; SC.w_easy = p->site.w_easy;
            SC.locus_offsets = p->d_offsets.p;
            SC.wprefix = (int64_t*)at(p->ws.work_wprefix); SC.part_prefix = (int64_t*)at(p->ws.part_prefix);
            SC.part_start = (int64_t*)at(p->ws.part_start);
            HIP_TRY(launch_scan_counts_kernel(st, work_count, p->nloci, p->site.chunk_cols, work_prefix, slice_prefix, &SC));
        } else {
            if (p->site.compact_chunked) launch_compact_chunked(p, d_flag, nullptr, work_cols, work_count, nullptr, ws, st);
            else if (p->max_locus_cols > 2048) compact_kernel<1024><<<dim3((unsigned)p->nloci), dim3(1024), 0, st>>>(d_flag, p->d_offsets.p, work_cols, work_count);
            else compact_kernel<256><<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(d_flag, p->d_offsets.p, work_cols, work_count);
            HIP_TRY(launch_scan_counts_kernel(st, work_count, p->nloci, p->site.chunk_cols, work_prefix, slice_prefix, nullptr));
        }
    }
    HIP_TRY(hipMemsetAsync(p->d_evals.p, 0, 8 * sizeof(unsigned long long), st));
    // how the kernel runs: site_launch_plan.hpp; the packed tip states are read with the fused-cherry stream (tree_program.hpp)
    const SiteKernelArgs A = site_kernel_args(p->site, p->nwords, p->prog.stack_depth, p->n_site_chunks);
    SiteParams S = plan_site_params(p, d_states, true);
    S.packed = C.packed; S.nwords = p->nwords;
    S.work_cols = work_cols; S.work_count = work_count;
    S.work_cols2 = A.second_list ? (int32_t*)at(p->ws.work_cols2) : nullptr;
    S.work_prefix = work_prefix; S.slice_prefix = slice_prefix;
    S.rate = d_rate; S.subst = d_subst; S.lnl = d_lnl; S.flag = d_flag; S.eval_counter = p->d_evals.p;
    S.lds_depth = p->site.lds_depth;
    S.spill = A.spill ? (double*)at(p->ws.spill) : nullptr;
    S.persistent = A.persistent; S.first_round = A.first_round; S.first_fraction = A.first_fraction;
    S.mixed_few_waves = p->site.mixed_few_waves; S.mixed_switch_cols = p->site.mixed_switch_cols;
    S.tail_order = A.tail_order; S.share_work = A.share_work; S.main_shares = A.main_shares;
    S.tail_shares = p->site.tail_shares;
    S.work_wprefix = (const int64_t*)at(p->ws.work_wprefix); S.part_prefix = (const int64_t*)at(p->ws.part_prefix);
    S.part_start = (const int64_t*)at(p->ws.part_start);
    // profiling brackets exactly the dominant kernel, so the figure matches rocprofv3's per-kernel average
    if (slot >= 0) HIP_TRY(hipEventRecord(p->ev[4 * slot + 0], st));
    if (p->n_site_chunks > 0)
        HIP_TRY(launch_site_rate_kernel(A.variant, p->model, dim3((unsigned)A.grid), A.lds_bytes, st, S));
    if (slot >= 0) HIP_TRY(hipEventRecord(p->ev[4 * slot + 1], st));
    if (dedup) dedup_scatter_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(D);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

// Where the empirical-Bayes fit of a locus' scale starts: the mean over ALL its columns of classify_kernel's parsimony start
// rate s0 (start_log_rate; 0 for the columns it answers in closed form), or 1 / tree length for a locus without a change.
// One workgroup per locus, thread-strided sums and a binary tree: the order depends on the locus alone.
__global__ __launch_bounds__(256) void eb_start_scale_kernel(const int64_t* __restrict__ locus_offsets, const uint8_t* __restrict__ flag,
                                                            const double* __restrict__ start_log, double chrono_length,
                                                            double* __restrict__ start) {
    __shared__ double red[256];
    const int locus = blockIdx.x;
    const int64_t lo = locus_offsets[locus], hi = locus_offsets[locus + 1];
    double sum = 0.0;
    for (int64_t c = lo + threadIdx.x; c < hi; c += 256)
        if (flag[c] == TPHIP_FLAG_OK) sum += exp(start_log[c]);
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) start[locus] = (red[0] > 0.0 && hi > lo) ? red[0] / (double)(hi - lo) : 1.0 / chrono_length;
}

// Front end of the empirical-Bayes calls (eb_driver.hip): classify_kernel for the informative-cell counts and the packed
// tip words, then -- every column takes part in the mixture, constant ones included -- either all columns, or the first
// column of every site pattern of a locus as a compacted work list (the stage-2 de-duplication kernels, forced on).
int tphip_internal_eb_prepare(tphip_plan* p, const uint8_t* d_states, const EbPrep* B, int32_t use_patterns, double* d_start,
                              void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (p->n_pi_chunks <= 0) return TPHIP_OK;
    const ClassifyParams C = classify_params(p, d_states, B->scratch[0], B->scratch[1], B->scratch[2], B->flag, B->nres, B->packed,
                                             use_patterns ? B->hash : nullptr, 1.0);
    classify_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(kPiBlock), 0, st>>>(C);
    if (d_start)   // before the flags are reset: they tell which columns carry a start rate
        eb_start_scale_kernel<<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(p->d_offsets.p, B->flag, B->scratch[0],
                                                                             p->prog.chrono_length, d_start);
    HIP_TRY(hipMemsetAsync(B->flag, TPHIP_FLAG_OK, (size_t)p->ncols, st));
    HIP_TRY(hipMemsetAsync(B->dup_of, 0xff, sizeof(int32_t) * (size_t)p->ncols, st));
    if (use_patterns) {
        const DedupParams D = dedup_params(p, C, B->dup_of, B->tab_key, B->tab_val, B->on, DEDUP_ON, false);
        if (p->max_locus_cols > 2048) dedup_estimate_kernel<1024><<<dim3((unsigned)p->nloci), dim3(1024), 0, st>>>(D);
        else dedup_estimate_kernel<256><<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(D);
        dedup_insert_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(D);
        dedup_resolve_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(D);
        // (this front end keeps the one-workgroup-per-locus list for long loci too: it runs once per empirical-Bayes call,
        //  not per step, and EbPrep carries no buffer for the chunk counts of launch_compact_chunked)
        if (p->max_locus_cols > 2048) compact_kernel<1024><<<dim3((unsigned)p->nloci), dim3(1024), 0, st>>>(B->flag, p->d_offsets.p, B->work_cols, B->work_count);
        else compact_kernel<256><<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(B->flag, p->d_offsets.p, B->work_cols, B->work_count);
    }
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int launch_pi_tables(tphip_plan* p, const double* d_rates, const int32_t* d_nres, double* d_tables, void* ws, hipStream_t st,
                     int slot) {
    PiParams Q = plan_pi_params(p, d_rates, d_nres);
    Q.partial = (double*)((char*)ws + p->ws.partial);
    if (slot >= 0) HIP_TRY(hipEventRecord(p->ev[4 * slot + 2], st));
    if (p->n_pi_chunks > 0) {
        const dim3 grid((unsigned)p->n_pi_chunks), block(kPiBlock);
        if (p->site.pi_split) {   // between them the two kernels write every entry of `partial`
            pi_net_kernel<<<grid, block, 0, st>>>(Q);
            if (p->n_i > 0) pi_interval_kernel<<<grid, block, 0, st>>>(Q);
        } else {
            pi_partial_kernel<<<grid, block, 0, st>>>(Q);
        }
    }
    pi_reduce_kernel<<<dim3((unsigned)p->nloci), dim3(kPiReduceBlock), 0, st>>>(Q.partial, p->d_locus_pichunk_offsets.p, p->T,
                                                                   p->d_times.p, p->n_t, p->n_i, d_tables);
    if (slot >= 0) HIP_TRY(hipEventRecord(p->ev[4 * slot + 3], st));
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

// The plan workspace's base (tphip_plan_workspace_bytes).  Its regions lie at multiples of 256 from it (layout_workspace) and are
// reached through their own types: int64_t prefixes, int2 chunk counts, the 64-bit keys of the de-duplication table (atomics)
// and, widest, classify_kernel's 16-byte stores into `packed`.  The three entry points below refuse any other base before
// anything is enqueued.
constexpr uintptr_t kPlanWsAlign = 16;
static const char* const kPlanWsAlignMessage = "workspace must be 16-byte aligned";
static bool plan_ws_aligned(const void* ws) { return ((uintptr_t)ws & (kPlanWsAlign - 1)) == 0; }

static int take_slot(tphip_plan* p) {
    if (!p->profile) return -1;
    if (p->ev_used >= kProfileRing) {
        if (profile_drain(p)) return -1;
    }
    return p->ev_used++;
}

int tphip_run_dev(tphip_plan* p, const uint8_t* d_states, double* d_rate, double* d_subst, double* d_lnl, uint8_t* d_flag,
                  int32_t* d_nres, double* d_tables, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!d_states || !d_rate || !d_subst || !d_lnl || !d_flag || !d_nres || !d_tables || !ws)
        return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ws_bytes < p->ws.total) return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than tphip_plan_workspace_bytes()");
    if (!plan_ws_aligned(ws)) return fail(TPHIP_ERR_INVALID, kPlanWsAlignMessage);
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    int slot = take_slot(p);
    int rc = launch_site_rates(p, d_states, d_rate, d_subst, d_lnl, d_flag, d_nres, ws, st, slot);
    if (rc) return rc;
    return launch_pi_tables(p, d_rate, d_nres, d_tables, ws, st, slot);
}

int tphip_site_rates_dev(tphip_plan* p, const uint8_t* d_states, double* d_rate, double* d_subst, double* d_lnl,
                         uint8_t* d_flag, int32_t* d_nres, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!d_states || !d_rate || !d_subst || !d_lnl || !d_flag || !d_nres || !ws)
        return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ws_bytes < p->ws.total) return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than tphip_plan_workspace_bytes()");
    if (!plan_ws_aligned(ws)) return fail(TPHIP_ERR_INVALID, kPlanWsAlignMessage);
    HIP_TRY(hipSetDevice(p->device));
    int slot = take_slot(p);
    int rc = launch_site_rates(p, d_states, d_rate, d_subst, d_lnl, d_flag, d_nres, ws, (hipStream_t)stream, slot);
    if (rc == 0 && slot >= 0) {  // keep the pi event pair of this slot valid (zero-length)
        HIP_TRY(hipEventRecord(p->ev[4 * slot + 2], (hipStream_t)stream));
        HIP_TRY(hipEventRecord(p->ev[4 * slot + 3], (hipStream_t)stream));
    }
    return rc;
}

int tphip_pi_tables_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, double* d_tables, void* ws,
                        size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!d_rates || !d_tables || !ws) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ws_bytes < p->ws.total) return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than tphip_plan_workspace_bytes()");
    if (!plan_ws_aligned(ws)) return fail(TPHIP_ERR_INVALID, kPlanWsAlignMessage);
    HIP_TRY(hipSetDevice(p->device));
    int slot = take_slot(p);
    if (slot >= 0) {
        HIP_TRY(hipEventRecord(p->ev[4 * slot + 0], (hipStream_t)stream));
        HIP_TRY(hipEventRecord(p->ev[4 * slot + 1], (hipStream_t)stream));
    }
    return launch_pi_tables(p, d_rates, d_nres, d_tables, ws, (hipStream_t)stream, slot);
}

int tphip_corrected_rates_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, double* d_out, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (p->ncols && (!d_rates || !d_out)) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    if (p->ncols) {
        corrected_rates_kernel<<<dim3((unsigned)((p->ncols + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
            plan_pi_params(p, d_rates, d_nres), p->ncols, d_out);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

int tphip_corrected_rates(tphip_plan* p, const double* rates, const int32_t* nres, double* out) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (p->ncols == 0) return TPHIP_OK;
    if (!rates || !out) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const size_t n = (size_t)p->ncols;
    const double* d_r = S.in(rates, n);
    double* d_o = S.out(out, n);
    const int32_t* d_n = S.in(nres, n);
    if (S.rc) return S.rc;
    int rc = tphip_corrected_rates_dev(p, d_r, d_n, d_o, nullptr);
    return rc ? rc : S.finish();
}

int tphip_townsend_pi_dense_dev(int32_t device, const double* d_rates, int64_t n, const double* d_times, int32_t n_times,
                                double* d_out, void* stream) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (n < 0 || n_times < 0 || (n && n_times && (!d_rates || !d_out || !d_times))) return fail(TPHIP_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(device));
    if (n && n_times) {
        townsend_dense_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(d_rates, n, d_times,
                                                                                                    n_times, d_out);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

int tphip_quad_townsend_dev(int32_t device, const double* d_rates, int64_t n, double a, double b, int32_t integ_mode,
                            double* d_integral, double* d_abserr, void* stream) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (n < 0 || (n && (!d_rates || !d_integral || !d_abserr))) return fail(TPHIP_ERR_INVALID, "bad arguments");
    if (!(a < b)) return fail(TPHIP_ERR_INVALID, "Start time is sooner than end time in an interval");
    if (integ_mode != TPHIP_INTEG_QUADPACK && integ_mode != TPHIP_INTEG_CLOSED) return fail(TPHIP_ERR_INVALID, "unknown integ_mode");
    HIP_TRY(hipSetDevice(device));
    if (n) {
        quad_sites_kernel<<<dim3((unsigned)((n + 127) / 128)), dim3(128), 0, (hipStream_t)stream>>>(d_rates, n, a, b, integ_mode,
                                                                                                d_integral, d_abserr);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

int tphip_state_histogram_dev(int32_t device, const uint8_t* d_states, int64_t ncols_total, int32_t ntaxa,
                              const int64_t* d_locus_offsets, int64_t nloci, int64_t* d_hist, void* stream) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (!d_states || !d_locus_offsets || !d_hist || nloci < 1 || ntaxa < 1) return fail(TPHIP_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(device));
    state_histogram_kernel<<<dim3((unsigned)nloci), dim3(256), 0, (hipStream_t)stream>>>(
        d_states, ncols_total, ntaxa, d_locus_offsets, (unsigned long long*)d_hist);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int tphip_townsend_pi_dense(int32_t device, const double* rates, int64_t n, const double* times, int32_t n_times, double* out) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (n < 0 || n_times < 0) return fail(TPHIP_ERR_INVALID, "bad arguments");
    if (n == 0 || n_times == 0) return TPHIP_OK;
    if (!rates || !times || !out) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(device));
    Scratch S;
    double* d_r = S.get<double>((size_t)n);
    double* d_t = S.get<double>((size_t)n_times);
    double* d_o = S.get<double>((size_t)n * (size_t)n_times);
    if (!d_r || !d_t || !d_o) return fail(TPHIP_ERR_HIP, "hipMalloc failed for the dense PI matrix");
    HIP_TRY(hipMemcpy(d_r, rates, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_t, times, sizeof(double) * (size_t)n_times, hipMemcpyHostToDevice));
    int rc = tphip_townsend_pi_dense_dev(device, d_r, n, d_t, n_times, d_o, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, d_o, sizeof(double) * (size_t)n * (size_t)n_times, hipMemcpyDeviceToHost));
    return TPHIP_OK;
}

int tphip_quad_townsend(int32_t device, const double* rates, int64_t n, double a, double b, int32_t integ_mode,
                        double* integral, double* abserr) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (n < 0) return fail(TPHIP_ERR_INVALID, "bad arguments");
    if (n == 0) return TPHIP_OK;
    if (!rates || !integral || !abserr) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(device));
    Staging S;
    const double* d_r = S.in(rates, (size_t)n);
    double* d_i = S.out(integral, (size_t)n);
    double* d_e = S.out(abserr, (size_t)n);
    if (S.rc) return S.rc;
    int rc = tphip_quad_townsend_dev(device, d_r, n, a, b, integ_mode, d_i, d_e, nullptr);
    return rc ? rc : S.finish();
}

int tphip_eval_columns_dev(tphip_plan* p, const uint8_t* d_s, const double* d_u, double* d_f, double* d_g, double* d_h,
                           void* stream) {
    if (!p || !d_s || !d_u || !d_f || !d_g || !d_h) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    EvalParams E{};
    E.S = plan_site_params(p, d_s, false);   // reads the states, not packed tip words: the plain op stream
    E.u = d_u; E.f = d_f; E.g = d_g; E.h = d_h;
    if (p->n_site_chunks > 0)
        HIP_TRY(launch_eval_columns_kernel(p->model, dim3((unsigned)p->n_site_chunks), site_lds_bytes(p->prog.stack_depth), (hipStream_t)stream, E));
    return TPHIP_OK;
}

int tphip_eval_columns(tphip_plan* p, const uint8_t* states, const double* u, double* f, double* g, double* h) {
    if (!p || !states || !u || !f || !g || !h) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    const size_t n = (size_t)p->ncols;
    uint8_t* d_s = S.get<uint8_t>(n * (size_t)p->ntaxa);
    double* d_u = S.get<double>(n);
    double* d_f = S.get<double>(n);
    double* d_g = S.get<double>(n);
    double* d_h = S.get<double>(n);
    if (!d_s || !d_u || !d_f || !d_g || !d_h) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_s, states, n * (size_t)p->ntaxa, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_u, u, sizeof(double) * n, hipMemcpyHostToDevice));
    int rc = tphip_eval_columns_dev(p, d_s, d_u, d_f, d_g, d_h, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(f, d_f, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(g, d_g, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h, d_h, sizeof(double) * n, hipMemcpyDeviceToHost));
    return TPHIP_OK;
}

int tphip_state_histogram(int32_t device, const uint8_t* states, int64_t ncols_total, int32_t ntaxa,
                          const int64_t* locus_offsets, int64_t nloci, int64_t* hist) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (!states || !locus_offsets || !hist || nloci < 1 || ntaxa < 1 || ncols_total < 0) return fail(TPHIP_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(device));
    Staging S;
    const uint8_t* d_s = S.in(states, (size_t)ncols_total * (size_t)ntaxa);
    const int64_t* d_o = S.in(locus_offsets, (size_t)nloci + 1);
    int64_t* d_h = S.out(hist, 16 * (size_t)nloci);
    if (S.rc) return S.rc;
    int rc = tphip_state_histogram_dev(device, d_s, ncols_total, ntaxa, d_o, nloci, d_h, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

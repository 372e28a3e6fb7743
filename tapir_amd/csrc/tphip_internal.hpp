// tphip_internal.hpp -- what the translation units of the host side share: the plan object behind include/tphip.h,
// the error channel and small device-buffer helpers.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "band_blocks.hpp"   // align_up
#include "gtr_model.hpp"
#include "locus_lik_params.hpp"
#include "locus_value_params.hpp"
#include "locus_grad2_params.hpp"
#include "locus_launch_plan.hpp"
#include "pi_rate.hpp"
#include "site_launch_plan.hpp"
#include "site_rate_params.hpp"
#include "tphip.h"
#include "tree_program.hpp"

using namespace tphip;

// thread-local message behind tphip_last_error() (defined in tphip.hip)
extern thread_local std::string g_tphip_err;

inline int fail(int code, const std::string& msg) {
    g_tphip_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return fail(TPHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

constexpr int kProfileRing = 1024;
constexpr double kPiFloor = 1e-12;

// device array of a fixed size, freed with its owner (on the device that is current then: tphip_plan_destroy sets the plan's)
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        n = count;
        return hipMalloc((void**)&p, (count ? count : 1) * sizeof(T));
    }
    hipError_t upload(const std::vector<T>& h) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess) return e;
        if (h.empty()) return hipSuccess;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

// device buffer grown on demand (its contents are not kept), freed with its owner
struct DevGrow {
    void* p = nullptr;
    size_t bytes = 0;
    DevGrow() = default;
    DevGrow(const DevGrow&) = delete;
    DevGrow& operator=(const DevGrow&) = delete;
    ~DevGrow() { if (p) (void)hipFree(p); }
    int reserve(size_t need) {
        if (need <= bytes && p) return TPHIP_OK;
        if (p) { HIP_TRY(hipFree(p)); p = nullptr; bytes = 0; }
        HIP_TRY(hipMalloc(&p, need ? need : 1));
        bytes = need;
        return TPHIP_OK;
    }
};

// grow-only device arena + pinned host mirror of the same size (arena_reserve in locus_driver.hip: doubling)
struct HostArena {
    char* d = nullptr;
    char* h = nullptr;
    size_t bytes = 0;
    HostArena() = default;
    HostArena(const HostArena&) = delete;
    HostArena& operator=(const HostArena&) = delete;
    ~HostArena() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
    }
};

// small RAII set of device buffers for the host-pointer conveniences
struct Scratch {
    std::vector<void*> bufs;
    ~Scratch() { for (void* q : bufs) if (q) (void)hipFree(q); }
    template <typename T> T* get(size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return nullptr;
        bufs.push_back(q);
        return (T*)q;
    }
};

// The device side of a host-pointer convenience: declare the inputs and outputs, check rc, make the _dev call, finish().
// After a failure (rc != 0: TPHIP_ERR_HIP, "hipMalloc failed" for an allocation) nothing more is allocated or copied.
struct Staging {
    Scratch S;
    struct Download { void* host; const void* dev; size_t bytes; };
    std::vector<Download> downloads;
    int rc = TPHIP_OK;
    // device buffer of `count` elements, its contents undefined (a workspace)
    template <typename T> T* scratch(size_t count) {
        T* d = rc ? nullptr : S.get<T>(count);
        if (!d && !rc) rc = fail(TPHIP_ERR_HIP, "hipMalloc failed");
        return d;
    }
    // device copy of host[count]; a null host pointer gives a null device pointer, count 0 copies nothing
    template <typename T> T* in(const T* host, size_t count) {
        T* d = host ? scratch<T>(count) : nullptr;
        if (d && count) rc = upload(d, host, sizeof(T) * count);
        return d;
    }
    // device buffer that finish() copies to host[count]; a null host pointer gives a null device pointer
    template <typename T> T* out(T* host, size_t count) {
        T* d = host ? scratch<T>(count) : nullptr;
        if (d && count) downloads.push_back({host, d, sizeof(T) * count});
        return d;
    }
    int upload(void* d, const void* host, size_t bytes) {
        HIP_TRY(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        return TPHIP_OK;
    }
    int finish() {
        for (const Download& o : downloads) HIP_TRY(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
        return TPHIP_OK;
    }
};

struct tphip_host_buffers;
struct tphip_saved_desc;

struct tphip_plan {
    tphip_host_buffers* hostbuf = nullptr;   // device buffers, streams and events of the host-pointer entry points
    // host-pointer entry points on big batches: the loci are cut into `host_split` groups, each a plan of its own with its
    // own streams, so that the upload of group k + 1 runs under the kernels of group k (host_run)
    tphip_saved_desc* saved = nullptr;       // deep copy of the descriptor the plan was created from
    std::vector<tphip_plan*> parts;
    std::vector<int64_t> part_locus;         // [parts + 1] locus boundaries
    int32_t host_split = 1;
    bool is_part = false;
    bool last_run_in_parts = false;
    int32_t device = 0;
    int32_t ntaxa = 0;
    int64_t nloci = 0, ncols = 0;
    int32_t T = 0, n_t = 0, n_i = 0, integ_mode = 0, threshold = 0, round_decimals = -1;
    double correction = 1.0;
    TreeProgram prog;
    std::vector<int64_t> h_offsets;
    int64_t n_site_chunks = 0, n_pi_chunks = 0;
    DevBuf<TreeOp> d_ops, d_fused_ops;
    DevBuf<LocusModel> d_models;
    DevBuf<int64_t> d_offsets, d_locus_pichunk_offsets;
    DevBuf<int32_t> d_tip_taxon, d_op_node;
    DevBuf<int32_t> d_cls_steps;   // TreeProgram::cls_steps, read as int2 by classify_kernel
    // launch configuration of the locus likelihood / gradient kernels, fixed at plan creation (locus_launch_plan.hpp:
    // decide_locus_launch)
    LocusLaunch locus;
    int32_t ncat = 0;
    DevBuf<double> d_cat;     // [2 * ncat] category rates, then log weights
    DevBuf<int4> d_lik_ops;   // {code, taxon, node, tape slot} per op for the locus likelihood / gradient kernels
    DevGrow tape;       // reverse-mode tape of the gradient kernels
    DevGrow grad_eig;   // per-candidate eigen-systems for locus_grad_kernel
    DevGrow value_ws;   // per-candidate eigen-systems + transition matrices of locus_value_kernel (one chunk)
    const uint8_t* lib_states = nullptr;   // the device copy of the alignment the library made itself (stage_alignment) ...
    uint32_t* d_value_packed = nullptr;    // ... and its state codes packed for locus_value_kernel (valid for exactly that copy)
    DevBuf<int4> d_value_ops;       // fused op stream of locus_value_kernel
    DevBuf<int32_t> d_value_tip_node;
    int32_t value_nops = 0;
    // the host-pointer likelihood / gradient calls stage through it: the optimiser makes thousands of small calls, so they
    // must not hipMalloc or issue a dozen pageable copies each
    HostArena arena;
    DevGrow grad_params;   // device copy of the gradient kernel's parameter block
    // transition-matrix gradient kernel (locus_grad2_kernel.hpp): binary trees with the value kernel's packed state codes
    bool grad2_built = false;        // its programs are on the device (whether it runs: locus.grad2_ok)
    DevBuf<int4> d_grad2_fops, d_grad2_rops;
    int32_t grad2_nrops = 0, grad2_ntape = 0, grad2_rdepth = 0;
    DevGrow grad2_ws;       // per-candidate transition matrices + branch tables of one chunk of candidates
    DevGrow grad2_params;   // ring of 64 parameter blocks
    DevGrow eb_ws;          // workspace of the empirical-Bayes calls (eb_driver.hip)
    // simulation kernel (simulate_driver.hip), made on first use: the tree as SimNode[nnodes], the workgroup size at which the
    // packed states of its internal nodes fit the LDS and their words per column; the stream ids of a call with locus_ids
    void* d_sim_nodes = nullptr;
    int32_t sim_block = 0, sim_words = 0;
    int64_t* d_sim_ids = nullptr;
    double* d_col_weight = nullptr;  // optional column multiplicities for the locus likelihood / gradient kernels
    DevGrow part;   // per-slice partial sums of the locus likelihood / gradient kernels
    int64_t max_locus_cols = 0;
    int32_t nnodes = 0;
    int32_t nwords = 0;
    DevBuf<int32_t> d_site_chunk_locus, d_site_chunk_index, d_pi_chunk_locus, d_pi_chunk_index, d_times, d_intervals;
    DevBuf<unsigned long long> d_evals;
    // how the site-rate stage runs and where its regions lie in the caller's workspace: decided once, at plan creation
    // (site_launch_plan.hpp: decide_site_launch, layout_workspace)
    SiteLaunch site;
    WorkspaceLayout ws;
    int32_t model = 0;        // TPHIP_MODEL_GTR / TPHIP_MODEL_F81 (tphip_plan_desc.model): the site-rate kernels' messages
    int32_t num_cus = 256;
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev;  // 4 events per slot: site start/stop, pi start/stop
    int ev_used = 0;
    double acc_site_ms = 0, acc_pi_ms = 0;
    int64_t acc_launches = 0;
};

// Device buffers tphip_internal_eb_prepare fills for eb_driver.hip: what classify_kernel leaves (informative-cell counts,
// packed tip words) and, with site patterns, the pattern representatives as a compacted work list per locus.
struct EbPrep {
    uint32_t* packed;             // [nwords][ncols]
    int32_t* nres;                // [ncols]
    uint8_t* flag;                // [ncols] scratch
    double* scratch[3];           // [ncols] each: classify_kernel's rate / subst / lnl slots (overwritten later)
    uint64_t* hash;               // [ncols]       (patterns)
    int32_t* dup_of;              // [ncols] representative column of a repeated pattern, or -1
    unsigned long long* tab_key;  // [2 * ncols]   (patterns)
    int32_t* tab_val;             // [2 * ncols]   (patterns)
    int32_t* on;                  // [nloci]       (patterns)
    int32_t* work_cols;           // [ncols]       (patterns)
    int32_t* work_count;          // [nloci]       (patterns)
};

// What every launch of a kernel that takes SiteParams shares (site_rate_kernel and the eval diagnostic in site_driver.hip,
// the posterior kernels of eb_driver.hip): the batch, the tree's op stream -- the fused-cherry stream goes with the packed tip
// words, the plain one with the diagnostic that reads the states -- the site chunk tables and the rate categories, with the
// whole stack in LDS and equal shares.  Work lists, outputs and scheduling are the caller's.
inline SiteParams plan_site_params(const tphip_plan* p, const uint8_t* d_states, bool fused) {
    SiteParams S{};
    S.states = d_states; S.ncols_total = p->ncols; S.models = p->d_models.p;
    S.ops = fused ? p->d_fused_ops.p : p->d_ops.p;
    S.nops = (int32_t)(fused ? p->prog.fused_ops.size() : p->prog.ops.size());
    S.stack_depth = p->prog.stack_depth; S.chrono_length = p->prog.chrono_length;
    S.locus_offsets = p->d_offsets.p; S.chunk_locus = p->d_site_chunk_locus.p; S.chunk_index = p->d_site_chunk_index.p;
    S.chunk_cols = p->site.chunk_cols;
    S.nloci = p->nloci; S.ncat = p->ncat; S.cat = p->d_cat.p;
    S.lds_depth = p->prog.stack_depth; S.first_fraction = 1.0;
    return S;
}

// The PI stage's view of the plan (finalize_rate's inputs, the schedule and the PI chunk tables); launch_pi_tables sets `partial`.
inline PiParams plan_pi_params(const tphip_plan* p, const double* d_rates, const int32_t* d_nres) {
    PiParams Q{};
    Q.rates = d_rates; Q.nres = d_nres; Q.locus_offsets = p->d_offsets.p;
    Q.chunk_locus = p->d_pi_chunk_locus.p; Q.chunk_index = p->d_pi_chunk_index.p;
    Q.T = p->T; Q.intervals = p->d_intervals.p; Q.n_i = p->n_i; Q.integ_mode = p->integ_mode;
    Q.correction = p->correction; Q.threshold = p->threshold;
    Q.round_scale = (p->round_decimals >= 0) ? std::pow(10.0, (double)p->round_decimals) : 0.0;
    return Q;
}

// launch configuration of the stage-1 kernels of a new plan, from its tree and batch (locus_driver.hip, for tphip_plan_create)
__attribute__((visibility("hidden"))) void configure_locus_launch(tphip_plan* p, const PlanKnobs& knobs);

// helpers of tphip.hip, site_driver.hip, pattern_driver.hip and locus_driver.hip for the other translation units of the library
// (not declared in include/tphip.h; hidden visibility: the shared library exports exactly what include/tphip.h declares)
extern "C" {
// the two stage-2 launchers (site_driver.hip), for the host-pointer paths of tphip.hip; slot = profiling slot or -1
__attribute__((visibility("hidden"))) int launch_site_rates(tphip_plan* p, const uint8_t* d_states, double* d_rate, double* d_subst,
                                                          double* d_lnl, uint8_t* d_flag, int32_t* d_nres, void* ws, hipStream_t st,
                                                          int slot);
__attribute__((visibility("hidden"))) int launch_pi_tables(tphip_plan* p, const double* d_rates, const int32_t* d_nres, double* d_tables,
                                                         void* ws, hipStream_t st, int slot);
__attribute__((visibility("hidden"))) int tphip_internal_stage_alignment(tphip_plan* p, const uint8_t* states, void** d_states_cache,
                                                                       uint8_t** d_s);
__attribute__((visibility("hidden"))) const tphip_plan_desc* tphip_internal_saved_desc(const tphip_plan* p);
__attribute__((visibility("hidden"))) int tphip_internal_compress_dev(const uint8_t* d_s, int64_t ncols_total, int32_t ntaxa,
                                                                    const int64_t* d_off, int64_t nloci, uint8_t** d_out,
                                                                    int64_t** d_newoff, double** d_w, int64_t* npat);
__attribute__((visibility("hidden"))) int tphip_internal_eb_prepare(tphip_plan* p, const uint8_t* d_states, const EbPrep* B,
                                                                  int32_t use_patterns, double* d_start, void* stream);
// posterior_pi_driver.hip, for tphip_eb_posterior_table: d_post holds f_k + log w_k of the representatives on entry
__attribute__((visibility("hidden"))) int tphip_internal_posterior_normalize(tphip_plan* p, const int32_t* d_dup_of, const double* d_f,
                                                                           double* d_post, int32_t K, void* stream);
__attribute__((visibility("hidden"))) int tphip_internal_store_pi(tphip_plan* p, const double* pi);
__attribute__((visibility("hidden"))) int tphip_internal_set_models_dev(tphip_plan* p, const double* d_pi, const double* d_exch,
                                                                      void* stream);
}

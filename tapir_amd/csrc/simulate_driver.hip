// simulate_driver.hip -- parametric bootstrap of site rates and PI rows: the C entry points
// tphip_simulate_columns (+ _dev), tphip_pi_parametric_bootstrap (+ _dev) and tphip_parboot_workspace_bytes.  The kernels
// are in simulate_kernels.hpp, the summary at the end in bootstrap_driver.hip, the workspace's layout in band_blocks.hpp.
//
// A replicate is three enqueues on the caller's stream: simulate every column at its fitted rate with the observed pattern of
// missing cells, the plan's own site-rate and PI-table stages on the simulated states (tphip_run_dev: de-duplication and start
// rule as the plan says), and the copy of the table into the replicate's row with the Welford update of the rate moments.
// The locus' model and the tree are held fixed -- no stage-1 refit per replicate: the bands are conditional on the fitted
// substitution model.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "band_driver_common.hpp"
#include "simulate_kernels.hpp"

namespace {

constexpr BandOptsRules kParbootOptsRules{band_seed_end<tphip_parboot_opts>(), band_ids_end<tphip_parboot_opts>(), "null tphip_parboot_opts",
                                          "tphip_parboot_opts.struct_size is too small: set it to sizeof(tphip_parboot_opts)",
                                          "parametric bootstrap replicates must be in 2..4096",
                                          "parametric bootstrap level must be in (0, 1)"};

struct SimOpts { int32_t replicate = 0; uint64_t seed = 0; const int64_t* locus_ids = nullptr; };

int sim_read_opts(const tphip_simulate_opts* o, SimOpts* out) {
    if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_simulate_opts");
    if (o->struct_size < band_seed_end<tphip_simulate_opts>())
        return fail(TPHIP_ERR_INVALID, "tphip_simulate_opts.struct_size is too small: set it to sizeof(tphip_simulate_opts)");
    out->replicate = o->replicate; out->seed = o->seed;
    out->locus_ids = o->struct_size >= band_ids_end<tphip_simulate_opts>() ? o->locus_ids : nullptr;
    if (out->replicate < 0 || out->replicate >= kSimMaxReplicate) return fail(TPHIP_ERR_INVALID, "replicate must be in 0..65535");
    return TPHIP_OK;
}

// what the plan must be for the simulation, and its tree as the kernel reads it (made once per plan)
int sim_prepare(tphip_plan* p) {
    if (p->ncat > 1)
        return fail(TPHIP_ERR_INVALID, "the simulation has no rate mixture: a plan with ncat > 1 cannot be simulated from");
    if (p->max_locus_cols >= ((int64_t)1 << 32)) return fail(TPHIP_ERR_INVALID, "a locus of 2^32 columns or more cannot be simulated");
    if (p->d_sim_nodes) return TPHIP_OK;
    const tphip_plan_desc* d = tphip_internal_saved_desc(p);
    if (!d) return fail(TPHIP_ERR_INVALID, "plan without a saved descriptor");
    const int32_t nn = d->nnodes;
    if (nn >= kSimMaxNodes) return fail(TPHIP_ERR_INVALID, "trees of 2^17 nodes or more cannot be simulated");
    std::vector<int32_t> slot((size_t)nn, -1);
    int32_t nint = 0;
    for (int32_t n = nn - 1; n >= 0; --n)
        if (d->leaf_taxon[n] < 0) slot[(size_t)n] = nint++;
    std::vector<SimNode> nodes((size_t)nn);
    for (int32_t n = 0; n < nn; ++n) {
        SimNode& s = nodes[(size_t)n];
        s.pslot = d->parent[n] < 0 ? -1 : slot[(size_t)d->parent[n]];
        s.self = d->leaf_taxon[n] >= 0 ? d->leaf_taxon[n] : ~slot[(size_t)n];
        s.t = d->parent[n] < 0 ? 0.0 : d->branch_len[n];
    }
    int32_t words = 0, block = 0;
    if (!sim_launch_shape(nint, &words, &block))
        return fail(TPHIP_ERR_INVALID, "tree has " + std::to_string(nint) + " internal nodes: the simulation kernel keeps the 2-bit states of at "
                                       "most 10240 per column (64 columns in 160 KiB of LDS)");
    HIP_TRY(hipSetDevice(p->device));
    void* dn = nullptr;
    HIP_TRY(hipMalloc(&dn, sizeof(SimNode) * (size_t)nn));
    hipError_t e = hipMemcpy(dn, nodes.data(), sizeof(SimNode) * (size_t)nn, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dn);
        return fail(TPHIP_ERR_HIP, std::string("hipMemcpy of the simulation tree: ") + hipGetErrorString(e));
    }
    p->d_sim_nodes = dn;
    p->sim_block = block;
    p->sim_words = words;
    return TPHIP_OK;
}

// stream ids into the plan's own buffer, made on first use; *d_ids = null without ids
int sim_stage_ids(tphip_plan* p, const int64_t* locus_ids, hipStream_t st, const int64_t** d_ids) {
    if (locus_ids && !p->d_sim_ids) HIP_TRY(hipMalloc((void**)&p->d_sim_ids, sizeof(int64_t) * (size_t)p->nloci));
    return band_stage_ids(p->d_sim_ids, locus_ids, p->nloci, st, d_ids);
}

int sim_launch(const tphip_plan* p, const double* d_rates, const uint8_t* d_mask, const int64_t* d_ids, uint32_t replicate,
               uint64_t seed, uint8_t* d_out, hipStream_t st) {
    if (p->n_pi_chunks == 0) return TPHIP_OK;
    SimParams S;
    S.rates = d_rates; S.mask = d_mask; S.out = d_out; S.ncols = p->ncols;
    S.models = p->d_models.p; S.locus_offsets = p->d_offsets.p;
    S.chunk_locus = p->d_pi_chunk_locus.p; S.chunk_index = p->d_pi_chunk_index.p;
    S.locus_ids = d_ids;
    S.nodes = (const SimNode*)p->d_sim_nodes;
    S.nnodes = tphip_internal_saved_desc(p)->nnodes;
    S.f81 = p->model == TPHIP_MODEL_F81 ? 1 : 0;
    S.replicate = replicate;
    S.key0 = (uint32_t)seed ^ kSimKeyTag;
    S.key1 = (uint32_t)(seed >> 32);
    const size_t lds = sim_lds_bytes(p->sim_words, p->sim_block);
    if (lds > kSimLdsDefaultBytes)
        HIP_TRY(hipFuncSetAttribute((const void*)simulate_columns_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    simulate_columns_kernel<<<dim3((unsigned)p->n_pi_chunks, (unsigned)(kSimChunk / p->sim_block)), dim3((unsigned)p->sim_block), lds, st>>>(S);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

// workspace of tphip_pi_parametric_bootstrap_dev: struct ParbootLayout of band_blocks.hpp on the plan's sizes
inline int32_t parboot_width(const tphip_plan* p) { return p->T + p->n_i; }
ParbootLayout parboot_layout(const tphip_plan* p, int32_t B) {
    return tphip::parboot_layout((size_t)p->ntaxa, (size_t)p->ncols, (size_t)p->nloci, (size_t)(p->T + p->n_t + 2 * p->n_i),
                                 (size_t)parboot_width(p), (size_t)B, p->ws.total);
}

}  // namespace

extern "C" {

int tphip_simulate_columns_dev(tphip_plan* p, const double* d_rates, const uint8_t* d_mask, const tphip_simulate_opts* opts,
                               uint8_t* d_states_out, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    SimOpts o;
    int rc = sim_read_opts(opts, &o);
    if (rc) return rc;
    rc = sim_prepare(p);
    if (rc) return rc;
    if (p->ncols == 0) return TPHIP_OK;
    if (!d_rates || !d_states_out) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t* d_ids = nullptr;
    rc = sim_stage_ids(p, o.locus_ids, st, &d_ids);
    if (rc) return rc;
    return sim_launch(p, d_rates, d_mask, d_ids, (uint32_t)o.replicate, o.seed, d_states_out, st);
}

int tphip_simulate_columns(tphip_plan* p, const double* rates, const uint8_t* mask, const tphip_simulate_opts* opts, uint8_t* states_out) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    SimOpts o;
    int rc = sim_read_opts(opts, &o);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, cells = (size_t)p->ntaxa * n;
    if (n && (!rates || !states_out)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const double* d_r = S.in(rates, n);
    const uint8_t* d_m = S.in(mask, cells);
    uint8_t* d_o = S.out(states_out, cells);
    if (S.rc) return S.rc;
    rc = tphip_simulate_columns_dev(p, d_r, d_m, opts, d_o, nullptr);
    return rc ? rc : S.finish();
}

int tphip_parboot_workspace_bytes(const tphip_plan* p, const tphip_parboot_opts* opts, size_t* bytes) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int rc = band_read_opts(opts, kParbootOptsRules, &o);
    if (rc) return rc;
    if (bytes) *bytes = parboot_layout(p, o.replicates).total;
    return TPHIP_OK;
}

int tphip_pi_parametric_bootstrap_dev(tphip_plan* p, const double* d_rates, const uint8_t* d_states_observed,
                                      const tphip_parboot_opts* opts, double* d_summary, double* d_rows, double* d_rate_mean,
                                      double* d_rate_sd, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int rc = band_read_opts(opts, kParbootOptsRules, &o);
    if (rc) return rc;
    rc = sim_prepare(p);
    if (rc) return rc;
    if (!d_states_observed && p->ncols) return fail(TPHIP_ERR_INVALID, "null observed alignment: its pattern of missing cells is part of the bootstrap");
    if (!d_summary || !ws || (p->ncols && !d_rates)) return fail(TPHIP_ERR_INVALID, "null device pointer");
    const int32_t B = o.replicates, Wb = parboot_width(p), W = p->T + p->n_t + 2 * p->n_i;
    const ParbootLayout L = parboot_layout(p, B);
    if (ws_bytes < L.total) return fail(TPHIP_ERR_INVALID, "workspace smaller than tphip_parboot_workspace_bytes()");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    char* base = band_ws_base(ws, ws_bytes);
    const int64_t* d_ids = nullptr;
    rc = sim_stage_ids(p, o.locus_ids, st, &d_ids);
    if (rc) return rc;
    uint8_t* states = (uint8_t*)(base + L.states);
    double* rate = (double*)(base + L.rate);
    double* subst = (double*)(base + L.subst);
    double* lnl = (double*)(base + L.lnl);
    uint8_t* flag = (uint8_t*)(base + L.flag);
    int32_t* nres = (int32_t*)(base + L.nres);
    double* tables = (double*)(base + L.tables);
    double* rows = d_rows ? d_rows : (double*)(base + L.rows);
    MomentParams M;
    M.pi = plan_pi_params(p, rate, nres);
    M.ncols = p->ncols; M.B = B;
    M.mean = (double*)(base + L.mean); M.m2 = (double*)(base + L.m2);
    M.out_mean = d_rate_mean; M.out_sd = d_rate_sd;
    for (int32_t b = 0; b < B; ++b) {
        rc = sim_launch(p, d_rates, d_states_observed, d_ids, (uint32_t)b, o.seed, states, st);
        if (rc) return rc;
        // (the plan's own workspace: `base` and L.plan_ws are multiples of 256, which meets tphip_run_dev's 16-byte rule)
        rc = tphip_run_dev(p, states, rate, subst, lnl, flag, nres, tables, base + L.plan_ws, p->ws.total, stream);
        if (rc) return rc;
        if (Wb > 0) parboot_rows_kernel<<<dim3((unsigned)p->nloci), dim3(256), 0, st>>>(tables, W, p->T, p->n_t, p->n_i, b, B, rows);
        if (p->ncols > 0) {
            M.b = b;
            rate_moments_kernel<<<dim3((unsigned)((p->ncols + 255) / 256)), dim3(256), 0, st>>>(M);
        }
        HIP_TRY(hipGetLastError());
    }
    return band_summarize(rows, p->nloci, B, Wb, o.level, d_summary, st);
}

int tphip_pi_parametric_bootstrap(tphip_plan* p, const double* rates, const uint8_t* states_observed, const tphip_parboot_opts* opts,
                                  double* summary, double* rows, double* rate_mean, double* rate_sd) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int rc = band_read_opts(opts, kParbootOptsRules, &o);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, cells = (size_t)p->ntaxa * n, Wb = (size_t)parboot_width(p), L = (size_t)p->nloci,
                 B = (size_t)o.replicates;
    if (!states_observed && n) return fail(TPHIP_ERR_INVALID, "null observed alignment: its pattern of missing cells is part of the bootstrap");
    if (!summary || (n && !rates)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t ws_bytes = parboot_layout(p, o.replicates).total;
    Staging S;
    const double* d_r = S.in(rates, n);
    const uint8_t* d_s = S.in(states_observed, cells);
    double* d_sum = S.out(summary, L * 4 * Wb);
    double* d_rows = S.out(rows, L * B * Wb);
    double* d_mean = S.out(rate_mean, n);
    double* d_sd = S.out(rate_sd, n);
    char* ws = S.scratch<char>(ws_bytes);
    if (S.rc) return S.rc;
    rc = tphip_pi_parametric_bootstrap_dev(p, d_r, d_s, opts, d_sum, d_rows, d_mean, d_sd, ws, ws_bytes, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

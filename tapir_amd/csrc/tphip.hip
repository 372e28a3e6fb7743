// tphip.hip -- the plan behind the C ABI (include/tphip.h): validation, the one-off tree compilation and table uploads of
// tphip_plan_create, the accessors and the per-locus models, and the host-pointer entry points with their pipeline of locus
// groups.  There is no CPU compute path.  The device launches are in the drivers: stage 2 in site_driver.hip (called from here
// through launch_site_rates / launch_pi_tables), the column compression in pattern_driver.hip, stage 1 in locus_driver.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gtr_setup_kernel.hpp"
#include "tphip_internal.hpp"

using namespace tphip;

thread_local std::string g_tphip_err;

static void free_host_buffers(struct tphip_plan* p);
static void free_parts(struct tphip_plan* p);

extern "C" {

int tphip_version(void) { return TPHIP_VERSION; }

const char* tphip_last_error(void) { return g_tphip_err.c_str(); }

int tphip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tphip_plan_destroy(tphip_plan* plan) {
    if (!plan) return TPHIP_OK;
    (void)hipSetDevice(plan->device);
    free_host_buffers(plan);
    free_parts(plan);
    // what a pattern view of stage 1 swaps stays a raw pointer (stage1_driver.hip), as do the simulation's arrays
    for (void* q : {(void*)plan->d_col_weight, (void*)plan->d_value_packed, plan->d_sim_nodes, (void*)plan->d_sim_ids}) if (q) (void)hipFree(q);
    for (hipEvent_t e : plan->ev) (void)hipEventDestroy(e);
    delete plan;   // its buffers free themselves, on the plan's device
    return TPHIP_OK;
}

struct tphip_saved_desc {
    tphip_plan_desc d;
    std::vector<int32_t> parent, leaf, times, intervals;
    std::vector<double> blen, pi, exch, cat_rate, cat_weight;
    std::vector<int64_t> offsets;
};

static tphip_saved_desc* save_desc(const tphip_plan_desc* d) {
    tphip_saved_desc* s = new tphip_saved_desc();
    s->d = *d;
    s->parent.assign(d->parent, d->parent + d->nnodes);
    s->blen.assign(d->branch_len, d->branch_len + d->nnodes);
    s->leaf.assign(d->leaf_taxon, d->leaf_taxon + d->nnodes);
    s->offsets.assign(d->locus_offsets, d->locus_offsets + d->nloci + 1);
    s->pi.assign(d->pi, d->pi + 4 * d->nloci);
    if (d->model == TPHIP_MODEL_F81) s->exch.assign(6 * (size_t)d->nloci, 1.0);   // what the library uses; d.exch stays NULL
    else s->exch.assign(d->exch, d->exch + 6 * d->nloci);
    if (d->n_t) s->times.assign(d->times, d->times + d->n_t);
    if (d->n_i) s->intervals.assign(d->intervals, d->intervals + 2 * (size_t)d->n_i);
    if (d->ncat > 0 && d->cat_rate && d->cat_weight) {
        s->cat_rate.assign(d->cat_rate, d->cat_rate + d->ncat);
        s->cat_weight.assign(d->cat_weight, d->cat_weight + d->ncat);
    }
    // the saved descriptor points at its own copies (the caller's arrays may be gone after tphip_plan_create returns)
    s->d.parent = s->parent.data(); s->d.branch_len = s->blen.data(); s->d.leaf_taxon = s->leaf.data();
    s->d.locus_offsets = s->offsets.data(); s->d.pi = s->pi.data();
    s->d.exch = d->model == TPHIP_MODEL_F81 ? nullptr : s->exch.data();
    s->d.times = s->times.empty() ? nullptr : s->times.data();
    s->d.intervals = s->intervals.empty() ? nullptr : s->intervals.data();
    s->d.cat_rate = s->cat_rate.empty() ? nullptr : s->cat_rate.data();
    s->d.cat_weight = s->cat_weight.empty() ? nullptr : s->cat_weight.data();
    return s;
}

// for the other translation units of the library (stage1_driver.hip)
const tphip_plan_desc* tphip_internal_saved_desc(const tphip_plan* p) { return (p && p->saved) ? &p->saved->d : nullptr; }

// the locus groups of the host-pointer pipeline (make_parts): gone with the plan, and rebuilt on next use after its models changed
static void drop_parts(tphip_plan* p) {
    for (tphip_plan* q : p->parts) (void)tphip_plan_destroy(q);
    p->parts.clear();
}

static void free_parts(tphip_plan* p) {
    drop_parts(p);
    delete p->saved;
    p->saved = nullptr;
}

// F81 models (TPHIP_MODEL_F81) on the host, exact: Q = Pi - I has the eigenvalue 0 (right vector 1, left vector pi) and -1
// three times, whose right eigenvectors are the vectors orthogonal to pi -- here e_k - pi_k 1 (k = 1..3), with the rows
// e_k - e_0 of the inverse.  Needs no floor (nothing divides by pi); pi normalised to sum 1, kappa = 1 - sum pi_i^2 (=
// 2 sum_{i<j} pi_i pi_j, what gtr_setup_kernel computes for exchangeabilities of 1).  The site-rate kernels read pi and
// kappa only; classify_kernel's start rule reads -Q_xx = 1 - pi_x from the eigen-form.
static void f81_models(const double* pi_in, int64_t L, std::vector<LocusModel>* out) {
    out->assign((size_t)L, LocusModel{});
    for (int64_t l = 0; l < L; ++l) {
        LocusModel& m = (*out)[(size_t)l];
        double pi[4], sum = 0.0, sq = 0.0;
        for (int i = 0; i < 4; ++i) sum += pi_in[4 * l + i];
        for (int i = 0; i < 4; ++i) { pi[i] = pi_in[4 * l + i] / sum; sq += pi[i] * pi[i]; }
        for (int k = 1; k < 4; ++k) {
            m.lam[k - 1] = -1.0;
            for (int i = 0; i < 4; ++i) m.U[i * 3 + k - 1] = (i == k ? 1.0 : 0.0) - pi[k];
            for (int j = 0; j < 4; ++j) m.Ui[(k - 1) * 4 + j] = (j == k ? 1.0 : 0.0) - (j == 0 ? 1.0 : 0.0);
        }
        for (int i = 0; i < 4; ++i) m.pi[i] = pi[i];
        m.kappa = 1.0 - sq;
    }
}

// The plans of the locus groups of a host-pointer run (created on first use): boundaries at the loci nearest to equal
// column counts; each group is an ordinary plan over its own loci (same tree, schedule and options).
static int make_parts(tphip_plan* p) {
    if (!p->parts.empty()) return TPHIP_OK;
    const tphip_saved_desc& S = *p->saved;
    const int64_t L = p->nloci, n = p->ncols;
    const int K = (int)std::min<int64_t>(p->host_split, L);
    std::vector<int64_t> cut(1, 0);
    for (int k = 1; k < K; ++k) {
        const int64_t target = n * k / K;
        int64_t l = std::lower_bound(S.offsets.begin(), S.offsets.end(), target) - S.offsets.begin();
        l = std::max<int64_t>(cut.back() + 1, std::min<int64_t>(l, L - (K - k)));
        cut.push_back(l);
    }
    cut.push_back(L);
    for (size_t k = 0; k + 1 < cut.size(); ++k)
        if (S.offsets[cut[k + 1]] == S.offsets[cut[k]]) { p->host_split = 1; return TPHIP_OK; }   // a group without columns: no pipeline
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const int64_t l0 = cut[k], l1 = cut[k + 1];
        std::vector<int64_t> off(S.offsets.begin() + l0, S.offsets.begin() + l1 + 1);
        for (int64_t& o : off) o -= S.offsets[l0];
        tphip_plan_desc d = S.d;
        d.parent = S.parent.data(); d.branch_len = S.blen.data(); d.leaf_taxon = S.leaf.data();
        d.nloci = l1 - l0; d.locus_offsets = off.data(); d.pi = S.pi.data() + 4 * l0;
        d.exch = S.d.model == TPHIP_MODEL_F81 ? nullptr : S.exch.data() + 6 * l0;
        d.times = S.times.empty() ? nullptr : S.times.data();
        d.intervals = S.intervals.empty() ? nullptr : S.intervals.data();
        d.cat_rate = S.cat_rate.empty() ? nullptr : S.cat_rate.data();
        d.cat_weight = S.cat_weight.empty() ? nullptr : S.cat_weight.data();
        tphip_plan* q = nullptr;
        const int rc = tphip_plan_create(&d, &q);
        if (rc) {   // whatever stops a group's plan: run the batch whole (the plain path reports real errors itself)
            drop_parts(p);
            p->host_split = 1;
            return TPHIP_OK;
        }
        q->is_part = true;
        p->parts.push_back(q);
    }
    p->part_locus = cut;
    return TPHIP_OK;
}

// Base frequencies and exchangeabilities of locus l as a caller gave them (either array may be null: not checked).
static int check_locus_model(const double* pi, const double* exch, int64_t l) {
    if (pi) {
        int npos = 0;
        for (int k = 0; k < 4; ++k) {
            if (!(pi[l * 4 + k] >= 0.0) || !std::isfinite(pi[l * 4 + k]))
                return fail(TPHIP_ERR_INVALID, "base frequencies of locus " + std::to_string(l) + " must be finite and >= 0");
            npos += pi[l * 4 + k] > 0.0;
        }
        if (npos < 2) return fail(TPHIP_ERR_INVALID, "locus " + std::to_string(l) + " has fewer than two bases with a positive frequency");
    }
    for (int k = 0; k < 6 && exch; ++k)
        if (!(exch[l * 6 + k] >= 0.0)) return fail(TPHIP_ERR_INVALID, "exchangeabilities must be >= 0");
    return TPHIP_OK;
}

// A base that never occurs in a (short) locus has empirical frequency 0 (HarvestFrequencies, bf:968); HyPhy takes
// that as it is: the state is unreachable and no tip carries it, so the likelihood is that of the three-state
// model.  The eigen-form used here needs D^-1/2, so the zero is floored at kPiFloor before the renormalisation in
// gtr_setup_kernel: the dead state then enters every likelihood with weight O(1e-12), below the 1e-9 the parity
// tests resolve.
static void floor_pi(std::vector<double>* hpi) {
    for (size_t l = 0; 4 * l < hpi->size(); ++l) {
        double sum = 0;
        for (int k = 0; k < 4; ++k) sum += (*hpi)[4 * l + k];
        for (int k = 0; k < 4; ++k) (*hpi)[4 * l + k] = std::max((*hpi)[4 * l + k], kPiFloor * sum);
    }
}

// The tuning knobs of plan creation (site_launch_plan.hpp), read from the environment once per plan.
static PlanKnobs knobs_from_env() {
    PlanKnobs k;
    for (const char* name : kPlanKnobNames)
        if (const char* text = getenv(name)) set_plan_knob(&k, name, text);
    return k;
}

// The tree programs, the locus and chunk tables, the schedule and the per-locus models, onto the plan's device.
static hipError_t upload_plan(tphip_plan* p, const tphip_plan_desc* d, const std::vector<double>& cat, const ChunkTables& chunks) {
    hipError_t e = hipSuccess;
    std::vector<int32_t> times(d->times, d->times + d->n_t), iv(d->intervals, d->intervals + 2 * (size_t)d->n_i);
    DevBuf<double> d_pi, d_exch;
    std::vector<double> hpi(d->pi, d->pi + 4 * (size_t)d->nloci), hex(6 * (size_t)d->nloci, 1.0);
    if (d->exch) hex.assign(d->exch, d->exch + 6 * (size_t)d->nloci);
    std::vector<LocusModel> f81;
    if (d->model == TPHIP_MODEL_F81) f81_models(d->pi, d->nloci, &f81);
    floor_pi(&hpi);
    std::vector<int32_t> tip_taxon;
    for (const TreeOp& op : p->prog.ops) if (op.code <= OP_TIP_MUL) tip_taxon.push_back(op.taxon);
    while (tip_taxon.size() % 8) tip_taxon.push_back(tip_taxon.back());   // read eight at a time
    if (e == hipSuccess) e = p->d_tip_taxon.upload(tip_taxon);
    if (e == hipSuccess) e = p->d_cls_steps.upload(p->prog.cls_steps);
    if (e == hipSuccess) e = p->d_op_node.upload(p->prog.op_node);
    if (e == hipSuccess && !cat.empty()) e = p->d_cat.upload(cat);
    if (e == hipSuccess) {
        std::vector<int4> lops(p->prog.ops.size());
        for (size_t i = 0; i < lops.size(); ++i) {
            const int32_t code = p->prog.ops[i].code;
            lops[i] = make_int4(code, p->prog.ops[i].taxon, p->prog.op_node[i],
                                code == OP_POP_MUL ? p->prog.op_partner[i] : p->prog.op_tape[i]);
        }
        e = p->d_lik_ops.upload(lops);
    }
    if (e == hipSuccess) {
        // locus_value_kernel's stream (build_value_program, locus_value_params.hpp)
        const auto& ops = p->prog.ops;
        std::vector<int4> vops;
        std::vector<int32_t> tip_node;
        const bool ok = build_value_program(p->prog, d->ntaxa, d->nnodes, &vops, &tip_node);
        if (ok) e = p->d_value_tip_node.upload(tip_node);
        p->value_nops = ok ? (int32_t)vops.size() : 0;
        if (ok && e == hipSuccess) e = p->d_value_ops.upload(vops);
        // the transition-matrix gradient kernel's programs: the same forward stream with a tape slot on every BRANCH, and the
        // pre-order walk over the internal nodes for the reverse sweep (binary trees only)
        if (ok && e == hipSuccess) {
            std::vector<int4> fops(vops);
            std::vector<int32_t> tape_slot(d->nnodes, -1), tip_pos(d->ntaxa, -1);
            int32_t nslot = 0, pos = 0;
            for (int4& o : fops)
                if ((o.x & OP_CODE_MASK) == OP_BRANCH) { tape_slot[o.y / 128] = nslot; o.z = nslot++; }
            for (size_t i = 0; i < ops.size(); ++i)
                if (ops[i].code <= OP_TIP_MUL) tip_pos[ops[i].taxon] = pos++;
            std::vector<int4> rops;
            int32_t rdepth = 0;
            const std::string gerr = build_grad2_program(d->nnodes, d->parent, d->leaf_taxon, tape_slot, tip_pos, &rops, &rdepth);
            if (gerr.empty() && rdepth <= kGrad2MaxRDepth) {
                e = p->d_grad2_fops.upload(fops);
                if (e == hipSuccess) e = p->d_grad2_rops.upload(rops);
                p->grad2_nrops = (int32_t)(rops.size() / 2);
                p->grad2_ntape = nslot;
                p->grad2_rdepth = rdepth;
                p->grad2_built = e == hipSuccess;
            }
        }
    }
    if (e == hipSuccess) e = p->d_ops.upload(p->prog.ops);
    if (e == hipSuccess) e = p->d_fused_ops.upload(p->prog.fused_ops);
    if (e == hipSuccess) e = p->d_offsets.upload(p->h_offsets);
    if (e == hipSuccess) e = p->d_locus_pichunk_offsets.upload(chunks.locus_pichunk_offsets);
    if (e == hipSuccess) e = p->d_site_chunk_locus.upload(chunks.site_chunk_locus);
    if (e == hipSuccess) e = p->d_site_chunk_index.upload(chunks.site_chunk_index);
    if (e == hipSuccess) e = p->d_pi_chunk_locus.upload(chunks.pi_chunk_locus);
    if (e == hipSuccess) e = p->d_pi_chunk_index.upload(chunks.pi_chunk_index);
    if (e == hipSuccess) e = p->d_times.upload(times);
    if (e == hipSuccess) e = p->d_intervals.upload(iv);
    if (e == hipSuccess) e = p->d_models.alloc((size_t)d->nloci);
    if (e == hipSuccess) e = p->d_evals.alloc(8);   // [0] evaluations; [1] evaluation rounds; [2..5] diagnostics of a TPHIP_SITE_TRACE_ROUNDS build
    if (e == hipSuccess) e = hipMemset(p->d_evals.p, 0, 8 * sizeof(unsigned long long));
    if (e == hipSuccess && d->model == TPHIP_MODEL_F81)
        e = hipMemcpy(p->d_models.p, f81.data(), sizeof(LocusModel) * f81.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && d->model == TPHIP_MODEL_GTR) e = d_pi.upload(hpi);
    if (e == hipSuccess && d->model == TPHIP_MODEL_GTR) e = d_exch.upload(hex);
    if (e == hipSuccess && d->model == TPHIP_MODEL_GTR) {
        const int bs = 128;
        gtr_setup_kernel<<<dim3((unsigned)((d->nloci + bs - 1) / bs)), dim3(bs)>>>(d_pi.p, d_exch.p, d->nloci, p->d_models.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

static int plan_setup_failed(tphip_plan* p, hipError_t e) {
    std::string m = std::string("plan setup: ") + hipGetErrorString(e);
    tphip_plan_destroy(p);
    return fail(TPHIP_ERR_HIP, m);
}

int tphip_plan_create(const tphip_plan_desc* d_in, tphip_plan** out) {
    // 1. validate
    if (!d_in || !out) return fail(TPHIP_ERR_INVALID, "null plan descriptor");
    *out = nullptr;
    // the caller's struct may be shorter (built against an older header): its missing trailing fields are zero
    if (d_in->struct_size < offsetof(tphip_plan_desc, round_decimals) + sizeof(int32_t) || d_in->struct_size > 4096)
        return fail(TPHIP_ERR_INVALID, "tphip_plan_desc.struct_size not set (zero-initialise the struct, then set it to sizeof)");
    tphip_plan_desc d_copy;
    memset(&d_copy, 0, sizeof(d_copy));
    memcpy(&d_copy, d_in, std::min<size_t>(d_in->struct_size, sizeof(d_copy)));
    d_copy.struct_size = (uint32_t)sizeof(d_copy);
    const tphip_plan_desc* d = &d_copy;
    int ndev = tphip_device_count();
    if (ndev <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (d->device < 0 || d->device >= ndev) return fail(TPHIP_ERR_INVALID, "device ordinal out of range");
    if (d->ntaxa < 2) return fail(TPHIP_ERR_INVALID, "ntaxa must be >= 2");
    if (!d->parent || !d->branch_len || !d->leaf_taxon) return fail(TPHIP_ERR_INVALID, "null tree arrays");
    if (d->model != TPHIP_MODEL_GTR && d->model != TPHIP_MODEL_F81) return fail(TPHIP_ERR_INVALID, "unknown model");
    if (d->model == TPHIP_MODEL_F81 && d->exch)
        return fail(TPHIP_ERR_INVALID, "exch must be NULL with TPHIP_MODEL_F81 (its exchangeabilities are all 1)");
    if (d->nloci < 1 || !d->locus_offsets || !d->pi || (d->model == TPHIP_MODEL_GTR && !d->exch))
        return fail(TPHIP_ERR_INVALID, "null or empty locus arrays");
    if (d->T < 0 || d->n_t < 0 || d->n_i < 0) return fail(TPHIP_ERR_INVALID, "negative schedule size");
    if ((d->n_t && !d->times) || (d->n_i && !d->intervals)) return fail(TPHIP_ERR_INVALID, "null times/intervals");
    if (!(d->correction > 0.0)) return fail(TPHIP_ERR_INVALID, "correction must be > 0");
    if (d->integ_mode != TPHIP_INTEG_QUADPACK && d->integ_mode != TPHIP_INTEG_CLOSED)
        return fail(TPHIP_ERR_INVALID, "unknown integ_mode");
    if (d->start_rule != TPHIP_START_AUTO && d->start_rule != TPHIP_START_PARSIMONY && d->start_rule != TPHIP_START_REFERENCE)
        return fail(TPHIP_ERR_INVALID, "unknown start_rule");
    if (d->pattern_dedup != TPHIP_DEDUP_AUTO && d->pattern_dedup != TPHIP_DEDUP_OFF && d->pattern_dedup != TPHIP_DEDUP_ON)
        return fail(TPHIP_ERR_INVALID, "unknown pattern_dedup");
    for (int i = 0; i < d->n_t; ++i)
        if (d->times[i] < 0 || d->times[i] >= d->T)  // numpy would raise IndexError (tapir/compute.py:78)
            return fail(TPHIP_ERR_INVALID, "a --times value is outside 0..T-1 (index out of bounds for the net PI vector)");
    for (int i = 0; i < d->n_i; ++i)
        if (!(d->intervals[2 * i] < d->intervals[2 * i + 1]))  // assert at tapir/compute.py:90-91
            return fail(TPHIP_ERR_INVALID, "Start time is sooner than end time in an interval");
    if (d->locus_offsets[0] != 0) return fail(TPHIP_ERR_INVALID, "locus_offsets[0] must be 0");
    for (int64_t l = 0; l < d->nloci; ++l) {
        if (d->locus_offsets[l + 1] < d->locus_offsets[l]) return fail(TPHIP_ERR_INVALID, "locus_offsets not monotone");
        if (const int rc = check_locus_model(d->pi, d->exch, l)) return rc;
    }
    const int64_t ncols = d->locus_offsets[d->nloci];
    if (ncols >= (int64_t)1 << 31) return fail(TPHIP_ERR_INVALID, "more than 2^31-1 columns in one batch");
    std::vector<double> cat;
    if (d->ncat > 1) {
        if (d->ncat > 16) return fail(TPHIP_ERR_INVALID, "at most 16 rate categories");
        if (!d->cat_rate || !d->cat_weight) return fail(TPHIP_ERR_INVALID, "rate categories need cat_rate and cat_weight");
        double wsum = 0;
        for (int k = 0; k < d->ncat; ++k) {
            if (!(d->cat_rate[k] > 0.0) || !(d->cat_weight[k] > 0.0) || !std::isfinite(d->cat_rate[k]) || !std::isfinite(d->cat_weight[k]))
                return fail(TPHIP_ERR_INVALID, "category rates and weights must be positive and finite");
            wsum += d->cat_weight[k];
        }
        cat.resize(2 * (size_t)d->ncat);
        for (int k = 0; k < d->ncat; ++k) { cat[k] = d->cat_rate[k]; cat[d->ncat + k] = std::log(d->cat_weight[k] / wsum); }
    }
    const PlanKnobs knobs = knobs_from_env();

    // 2. the tree programs
    tphip_plan* p = new tphip_plan();
    p->device = d->device; p->ntaxa = d->ntaxa; p->nnodes = d->nnodes; p->nloci = d->nloci; p->ncols = ncols;
    p->T = d->T; p->n_t = d->n_t; p->n_i = d->n_i; p->integ_mode = d->integ_mode;
    p->threshold = d->threshold; p->round_decimals = d->round_decimals; p->correction = d->correction;
    p->model = d->model;
    p->ncat = cat.empty() ? 0 : d->ncat;
    std::string terr = build_tree_program(d->ntaxa, d->nnodes, d->parent, d->branch_len, d->leaf_taxon, &p->prog);
    if (!terr.empty()) { delete p; return fail(TPHIP_ERR_INVALID, "tree: " + terr); }
    if (p->prog.nleaves != d->ntaxa) {  // HyPhy refuses a tree / alignment mismatch as well
        delete p;
        return fail(TPHIP_ERR_INVALID, "tree: the number of leaves differs from the number of alignment rows");
    }
    if (site_lds_bytes(p->prog.stack_depth) > 160 * 1024) { delete p; return fail(TPHIP_ERR_INVALID, "tree needs a deeper LDS stack than 160 KiB allows"); }
    int64_t ntips = 0;
    for (const TreeOp& op : p->prog.ops) ntips += op.code <= OP_TIP_MUL;
    p->nwords = (int32_t)((ntips + 7) / 8);
    p->h_offsets.assign(d->locus_offsets, d->locus_offsets + d->nloci + 1);
    for (int64_t l = 0; l < d->nloci; ++l)
        p->max_locus_cols = std::max<int64_t>(p->max_locus_cols, d->locus_offsets[l + 1] - d->locus_offsets[l]);

    // 3. how the site-rate stage will run (site_launch_plan.hpp)
    hipError_t e = hipSetDevice(d->device);
    if (e != hipSuccess) return plan_setup_failed(p, e);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) != hipSuccess) { tphip_plan_destroy(p); return fail(TPHIP_ERR_HIP, "hipGetDeviceProperties failed"); }
    p->num_cus = prop.multiProcessorCount;
    SiteShape shape;
    shape.ncols = ncols; shape.nloci = d->nloci; shape.max_locus_cols = p->max_locus_cols; shape.ntaxa = d->ntaxa;
    shape.nwords = p->nwords; shape.stack_depth = p->prog.stack_depth; shape.model = d->model; shape.ncat = d->ncat;
    shape.start_rule = d->start_rule; shape.pattern_dedup = d->pattern_dedup; shape.T = d->T; shape.n_i = d->n_i;
    p->site = decide_site_launch(shape, p->num_cus, knobs, [&](int variant, size_t lds_bytes) {
        int per_cu = 0;
        return site_rate_kernel_occupancy(variant, shape.model, lds_bytes, &per_cu) == hipSuccess ? per_cu : 0;
    });
    p->host_split = host_split_groups(knobs);

    // 4. the chunk tables and the workspace layout
    const ChunkTables chunks = build_chunk_tables(p->h_offsets.data(), d->nloci, p->site.chunk_cols);
    p->n_site_chunks = (int64_t)chunks.site_chunk_locus.size();
    p->n_pi_chunks = (int64_t)chunks.pi_chunk_locus.size();
    p->ws = layout_workspace(shape, p->site, p->n_pi_chunks);

    // 5. upload
    e = upload_plan(p, d, cat, chunks);
    if (e != hipSuccess) return plan_setup_failed(p, e);

    // 6. the stage-1 kernels (locus_launch_plan.hpp)
    configure_locus_launch(p, knobs);
    p->saved = save_desc(d);
    *out = p;
    return TPHIP_OK;
}

int32_t tphip_plan_table_width(const tphip_plan* p) { return p ? p->T + p->n_t + 2 * p->n_i : 0; }
int64_t tphip_plan_ncols(const tphip_plan* p) { return p ? p->ncols : 0; }
size_t tphip_plan_workspace_bytes(const tphip_plan* p) { return p ? p->ws.total : 0; }
double tphip_plan_chrono_length(const tphip_plan* p) { return p ? p->prog.chrono_length : 0.0; }
int32_t tphip_plan_stack_depth(const tphip_plan* p) { return p ? p->prog.stack_depth : 0; }

int tphip_plan_op_counts(const tphip_plan* p, int32_t* counts) {
    if (!p || !counts) return fail(TPHIP_ERR_INVALID, "null argument");
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    for (const TreeOp& op : p->prog.ops) ++counts[op.code];
    return TPHIP_OK;
}

int32_t tphip_plan_cherry_count(const tphip_plan* p) {
    if (!p) return 0;
    int32_t n = 0;
    for (const TreeOp& op : p->prog.fused_ops) n += ((op.code & OP_CODE_MASK) == OP_CHERRY);
    return n;
}

int tphip_plan_get_models(const tphip_plan* p, double* lam, double* U, double* Uinv, double* kappa) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    std::vector<LocusModel> h((size_t)p->nloci);
    HIP_TRY(hipMemcpy(h.data(), p->d_models.p, sizeof(LocusModel) * h.size(), hipMemcpyDeviceToHost));
    for (int64_t l = 0; l < p->nloci; ++l) {  // expand the packed device layout to full 4x4 matrices
        const LocusModel& m = h[l];
        if (lam) { lam[4 * l] = 0.0; for (int k = 1; k < 4; ++k) lam[4 * l + k] = m.lam[k - 1]; }
        if (U) for (int i = 0; i < 4; ++i) { U[16 * l + 4 * i] = 1.0; for (int k = 1; k < 4; ++k) U[16 * l + 4 * i + k] = m.U[i * 3 + k - 1]; }
        if (Uinv) for (int j = 0; j < 4; ++j) { Uinv[16 * l + j] = m.pi[j]; for (int k = 1; k < 4; ++k) Uinv[16 * l + 4 * k + j] = m.Ui[(k - 1) * 4 + j]; }
        if (kappa) kappa[l] = m.kappa;
    }
    return TPHIP_OK;
}

// ---- host-pointer wrappers -------------------------------------------------------------------------

// Host-pointer calls keep their device buffers in the plan (grown on demand, freed with the plan): a hipMalloc /
// hipFree pair per buffer per call cost more than the kernels of a small batch.  Copies are asynchronous on a second
// stream where the caller's memory allows it (pinned: tphip_host_alloc, or registered by the caller): the per-column
// outputs leave the device while the PI kernels run, and rate / flag / nres leave as soon as the site-rate stage ends.
// Pageable memory is copied by the runtime's own staged hipMemcpy (same code path, no overlap).
namespace {
struct HostBuffers {
    DevGrow states;
    DevGrow percol;    // rate | subst | lnl | nres | flag, one allocation
    DevGrow tables;
    DevGrow ws;
    hipStream_t copy_stream = nullptr, run_stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_site = nullptr;
};

bool is_pinned(const void* q) {   // host memory the DMA engines can reach directly
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
}  // namespace

struct tphip_host_buffers : HostBuffers {};

static void free_host_buffers(tphip_plan* p) {
    tphip_host_buffers* B = p->hostbuf;
    if (!B) return;
    if (B->copy_stream) (void)hipStreamDestroy(B->copy_stream);
    if (B->run_stream) (void)hipStreamDestroy(B->run_stream);
    if (B->ev_in) (void)hipEventDestroy(B->ev_in);
    if (B->ev_site) (void)hipEventDestroy(B->ev_site);
    delete B;   // and with it the four device buffers
    p->hostbuf = nullptr;
}

// Queues one host-pointer pass on the plan's own streams (no wait).  `spitch` = bytes between taxon rows of `states` at the
// caller (= the plan's column count unless the plan is a locus group of a bigger batch); `after` = an event the upload must
// wait for (the previous group's upload: the DMA engine serves one upload after the other, not all of them slowly).
static int host_enqueue(tphip_plan* p, const uint8_t* states, size_t spitch, hipEvent_t after, const double* rates_in,
                        const int32_t* nres_in, double* rate, double* subst, double* lnl, uint8_t* flag, int32_t* nres,
                        double* tables, bool do_site, bool do_pi) {
    HIP_TRY(hipSetDevice(p->device));
    if (!p->hostbuf) {
        p->hostbuf = new tphip_host_buffers();
        HIP_TRY(hipStreamCreateWithFlags(&p->hostbuf->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&p->hostbuf->run_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&p->hostbuf->ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&p->hostbuf->ev_site, hipEventDisableTiming));
    }
    HostBuffers& B = *p->hostbuf;
    const size_t n = (size_t)p->ncols, W = (size_t)tphip_plan_table_width(p);
    // per-column block: rate | subst | lnl (8 B each) | nres (4 B) | flag (1 B), each part 256-byte aligned
    const size_t o_rate = 0, o_subst = align_up(8 * n, 256), o_lnl = o_subst + align_up(8 * n, 256),
                 o_nres = o_lnl + align_up(8 * n, 256), o_flag = o_nres + align_up(4 * n, 256);
    int rc = B.percol.reserve(o_flag + align_up(n, 256));
    if (rc) return rc;
    rc = B.ws.reserve(p->ws.total);
    if (rc) return rc;
    char* percol = (char*)B.percol.p;
    double* d_rate = (double*)(percol + o_rate);
    double* d_subst = (double*)(percol + o_subst);
    double* d_lnl = (double*)(percol + o_lnl);
    int32_t* d_nres = (int32_t*)(percol + o_nres);
    uint8_t* d_flag = (uint8_t*)(percol + o_flag);
    hipStream_t cs = B.copy_stream, rs = B.run_stream;
    if (do_site) {
        if (!states || !rate || !subst || !lnl || !flag || !nres) return fail(TPHIP_ERR_INVALID, "null host pointer");
        // (+ 1, and + 8 for the tables below: redundant guards against an empty allocation, which DevGrow::reserve handles
        //  itself; no kernel writes past the states matrix or the tables: tests/test_gpu_abi_contract.py)
        rc = B.states.reserve(n * (size_t)p->ntaxa + 1);
        if (rc) return rc;
        uint8_t* d_states = (uint8_t*)B.states.p;
        if (after) HIP_TRY(hipStreamWaitEvent(rs, after, 0));
        if (spitch == n) HIP_TRY(hipMemcpyAsync(d_states, states, n * (size_t)p->ntaxa, hipMemcpyHostToDevice, rs));
        else HIP_TRY(hipMemcpy2DAsync(d_states, n, states, spitch, n, (size_t)p->ntaxa, hipMemcpyHostToDevice, rs));
        HIP_TRY(hipEventRecord(B.ev_in, rs));
        rc = launch_site_rates(p, d_states, d_rate, d_subst, d_lnl, d_flag, d_nres, B.ws.p, rs, -1);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(B.ev_site, rs));
    } else {
        if (!rates_in) return fail(TPHIP_ERR_INVALID, "null host pointer");
        HIP_TRY(hipMemcpyAsync(d_rate, rates_in, sizeof(double) * n, hipMemcpyHostToDevice, rs));
        if (nres_in) HIP_TRY(hipMemcpyAsync(d_nres, nres_in, sizeof(int32_t) * n, hipMemcpyHostToDevice, rs));
    }
    if (do_pi) {
        if (!tables) return fail(TPHIP_ERR_INVALID, "null host pointer");
        rc = B.tables.reserve(sizeof(double) * W * (size_t)p->nloci + 8);
        if (rc) return rc;
        rc = launch_pi_tables(p, d_rate, (do_site || nres_in) ? d_nres : nullptr, (double*)B.tables.p, B.ws.p, rs, -1);
        if (rc) return rc;
    }
    if (do_site) {
        // the per-column results go home on the copy stream while the PI kernels (which only read them) run; with
        // pageable destinations the runtime stages the copies itself and they simply run in order
        const bool overlap = is_pinned(rate) && is_pinned(subst) && is_pinned(lnl) && is_pinned(flag) && is_pinned(nres);
        hipStream_t os = overlap ? cs : rs;
        if (overlap) HIP_TRY(hipStreamWaitEvent(cs, B.ev_site, 0));
        HIP_TRY(hipMemcpyAsync(rate, d_rate, sizeof(double) * n, hipMemcpyDeviceToHost, os));
        HIP_TRY(hipMemcpyAsync(subst, d_subst, sizeof(double) * n, hipMemcpyDeviceToHost, os));
        HIP_TRY(hipMemcpyAsync(lnl, d_lnl, sizeof(double) * n, hipMemcpyDeviceToHost, os));
        HIP_TRY(hipMemcpyAsync(flag, d_flag, n, hipMemcpyDeviceToHost, os));
        HIP_TRY(hipMemcpyAsync(nres, d_nres, sizeof(int32_t) * n, hipMemcpyDeviceToHost, os));
    }
    if (do_pi) HIP_TRY(hipMemcpyAsync(tables, B.tables.p, sizeof(double) * W * (size_t)p->nloci, hipMemcpyDeviceToHost, rs));
    return TPHIP_OK;
}

static int host_wait(tphip_plan* p) {
    if (!p->hostbuf) return TPHIP_OK;
    HIP_TRY(hipStreamSynchronize(p->hostbuf->run_stream));
    HIP_TRY(hipStreamSynchronize(p->hostbuf->copy_stream));
    return TPHIP_OK;
}

constexpr int64_t kHostSplitMinColumns = (int64_t)1 << 21;   // below this a pass is too short for the pipeline to pay

static int host_run(tphip_plan* p, const uint8_t* states, const double* rates_in, const int32_t* nres_in, double* rate,
                    double* subst, double* lnl, uint8_t* flag, int32_t* nres, double* tables, bool do_site, bool do_pi,
                    size_t row_pitch = 0) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    const size_t pitch = row_pitch ? row_pitch : (size_t)p->ncols;   // bytes between taxon rows of `states` at the caller
    if (pitch < (size_t)p->ncols) return fail(TPHIP_ERR_INVALID, "row_pitch smaller than the plan's column count");
    // Big batches from pinned host memory: locus groups in a pipeline -- the upload of group k + 1 (and the download of group
    // k - 1) run while group k computes.  Results do not depend on how a batch is cut (per-column results depend on the
    // column and its locus' model only, a locus' PI row on its own columns in a fixed order).
    const bool split = do_site && !p->is_part && p->saved && p->host_split > 1 && p->nloci >= 2 * p->host_split &&
                       p->ncols >= kHostSplitMinColumns && states && rate && subst && lnl && flag && nres &&
                       is_pinned(states) && is_pinned(rate) && is_pinned(subst) && is_pinned(lnl) && is_pinned(flag) &&
                       is_pinned(nres) && (!do_pi || (tables && is_pinned(tables)));
    int rc = split ? make_parts(p) : TPHIP_OK;
    if (rc) return rc;
    if (!split || p->parts.empty()) {   // the whole batch at once (also when it does not cut into groups with columns)
        // always drain: a failed enqueue may already have copies in flight that touch the caller's buffers
        rc = host_enqueue(p, states, pitch, nullptr, rates_in, nres_in, rate, subst, lnl, flag, nres, tables, do_site, do_pi);
        const int rw = host_wait(p);
        return rc ? rc : rw;
    }
    const size_t W = (size_t)tphip_plan_table_width(p);
    p->last_run_in_parts = true;
    hipEvent_t after = nullptr;
    for (size_t k = 0; k < p->parts.size(); ++k) {
        tphip_plan* q = p->parts[k];
        const int64_t l0 = p->part_locus[k], c0 = p->h_offsets[l0];
        rc = host_enqueue(q, states + c0, pitch, after, nullptr, nullptr, rate + c0, subst + c0, lnl + c0, flag + c0,
                          nres + c0, do_pi ? tables + (size_t)l0 * W : nullptr, true, do_pi);
        if (rc) break;
        after = q->hostbuf->ev_in;
    }
    for (tphip_plan* q : p->parts) {
        const int rw = host_wait(q);
        if (!rc) rc = rw;
    }
    return rc;
}

void* tphip_host_alloc(size_t bytes) {
    void* q = nullptr;
    if (tphip_device_count() <= 0) { fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path"); return nullptr; }
    if (hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { fail(TPHIP_ERR_HIP, "hipHostMalloc failed"); return nullptr; }
    return q;
}

int tphip_host_free(void* ptr) {
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return TPHIP_OK;
}

int tphip_site_rates(tphip_plan* p, const uint8_t* states, double* rate, double* subst, double* lnl, uint8_t* flag,
                     int32_t* nres) {
    return host_run(p, states, nullptr, nullptr, rate, subst, lnl, flag, nres, nullptr, true, false);
}

int tphip_pi_tables(tphip_plan* p, const double* rates, const int32_t* nres, double* tables) {
    return host_run(p, nullptr, rates, nres, nullptr, nullptr, nullptr, nullptr, nullptr, tables, false, true);
}

int tphip_run_fused(tphip_plan* p, const uint8_t* states, double* rate, double* subst, double* lnl, uint8_t* flag,
                    int32_t* nres, double* tables) {
    return host_run(p, states, nullptr, nullptr, rate, subst, lnl, flag, nres, tables, true, true);
}

int tphip_run_fused_pitched(tphip_plan* p, const uint8_t* states, int64_t row_pitch, double* rate, double* subst, double* lnl,
                            uint8_t* flag, int32_t* nres, double* tables) {
    if (row_pitch < 0) return fail(TPHIP_ERR_INVALID, "negative row_pitch");
    return host_run(p, states, nullptr, nullptr, rate, subst, lnl, flag, nres, tables, true, true, (size_t)row_pitch);
}

// per-locus eigen-systems from DEVICE arrays pi [L][4] (floored, any scale) and exch [L][6]; for stage1_driver.hip
int tphip_internal_set_models_dev(tphip_plan* p, const double* d_pi, const double* d_exch, void* stream) {
    const int bs = 64;
    gtr_setup_kernel<<<dim3((unsigned)((p->nloci + bs - 1) / bs)), dim3(bs), 0, (hipStream_t)stream>>>(d_pi, d_exch, p->nloci, p->d_models.p);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

// the plan's record of its base frequencies after they were replaced on the device (stage1_driver.hip: empirical_pi)
int tphip_internal_store_pi(tphip_plan* p, const double* pi) {
    if (!p || !p->saved) return fail(TPHIP_ERR_INVALID, "plan has no saved descriptor");
    p->saved->pi.assign(pi, pi + 4 * (size_t)p->nloci);
    p->saved->d.pi = p->saved->pi.data();
    drop_parts(p);
    return TPHIP_OK;
}

int tphip_plan_set_models(tphip_plan* p, const double* pi, const double* exch) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!p->saved) return fail(TPHIP_ERR_INVALID, "plan has no saved descriptor");
    const size_t L = (size_t)p->nloci;
    if (p->model == TPHIP_MODEL_F81 && exch)
        return fail(TPHIP_ERR_INVALID, "exch must be NULL on a TPHIP_MODEL_F81 plan (its exchangeabilities are all 1)");
    if (pi) {
        for (int64_t l = 0; l < p->nloci; ++l)
            if (const int rc = check_locus_model(pi, nullptr, l)) return rc;
        p->saved->pi.assign(pi, pi + 4 * L);
    }
    if (exch) {
        for (int64_t l = 0; l < p->nloci; ++l)
            if (const int rc = check_locus_model(nullptr, exch, l)) return rc;
        p->saved->exch.assign(exch, exch + 6 * L);
    }
    p->saved->d.pi = p->saved->pi.data();
    HIP_TRY(hipSetDevice(p->device));
    if (p->model == TPHIP_MODEL_F81) {
        std::vector<LocusModel> f81;
        f81_models(p->saved->pi.data(), p->nloci, &f81);
        HIP_TRY(hipMemcpy(p->d_models.p, f81.data(), sizeof(LocusModel) * L, hipMemcpyHostToDevice));
        drop_parts(p);
        return TPHIP_OK;
    }
    p->saved->d.exch = p->saved->exch.data();
    std::vector<double> hpi(p->saved->pi);
    floor_pi(&hpi);   // as at plan creation
    Scratch S;
    double* d_pi = S.get<double>(4 * L);
    double* d_ex = S.get<double>(6 * L);
    if (!d_pi || !d_ex) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_pi, hpi.data(), sizeof(double) * 4 * L, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ex, p->saved->exch.data(), sizeof(double) * 6 * L, hipMemcpyHostToDevice));
    int rc = tphip_internal_set_models_dev(p, d_pi, d_ex, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    // locus groups of the pipelined host path were built from the old models: rebuilt on next use
    drop_parts(p);
    return TPHIP_OK;
}

}  // extern "C"

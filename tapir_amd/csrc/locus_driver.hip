// locus_driver.hip -- the stage-1 entry points of the C ABI (include/tphip.h): per-locus likelihood and gradient on device
// pointers, their host-pointer wrappers, and what those keep in the plan (alignment cache, column weights).  No kernels here:
// they live in the launch units (locus_lik_launch.hip, locus_value_launch.hip, locus_grad2_launch.hip); what is launched how
// is decided in locus_launch_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "locus_grad2_params.hpp"
#include "locus_launch_plan.hpp"
#include "locus_lik_params.hpp"
#include "locus_value_params.hpp"
#include "tphip.h"
#include "tphip_internal.hpp"

using namespace tphip;

// Launch configuration of the stage-1 kernels of a new plan (decide_locus_launch over the launch units' own queries).
void configure_locus_launch(tphip_plan* p, const PlanKnobs& knobs) {
    LocusShape shape;
    shape.ntaxa = p->ntaxa; shape.nnodes = p->nnodes; shape.nwords = p->nwords; shape.stack_depth = p->prog.stack_depth;
    shape.ntape = p->prog.ntape; shape.max_locus_cols = p->max_locus_cols; shape.value_nops = p->value_nops;
    shape.grad2_built = p->grad2_built; shape.grad2_rdepth = p->grad2_rdepth; shape.grad2_ntape = p->grad2_ntape;
    p->locus = decide_locus_launch(
        shape, p->num_cus, knobs,
        [](LocusKernel k, int cols, int depth, size_t lds) {
            return (k == LOCUS_LIK     ? locus_loglik_kernel_allow_lds(lds)
                    : k == LOCUS_VALUE ? locus_value_kernel_allow_lds(cols, depth, lds)
                    : k == LOCUS_GRAD  ? locus_grad_kernel_allow_lds(lds)
                                       : locus_grad2_kernel_allow_lds(depth, lds)) == hipSuccess;
        },
        [](LocusKernel k, int depth, size_t lds) {
            int bpc = 0;
            const hipError_t e = k == LOCUS_GRAD ? locus_grad_kernel_occupancy(lds, &bpc) : locus_grad2_kernel_occupancy(depth, lds, &bpc);
            return e == hipSuccess ? bpc : 0;
        });
}

namespace {

// The candidates of a call (device arrays); at(done) = the same from candidate `done` on.
struct CandPtrs {
    const int32_t* locus;
    const double* exch;     // [ncand][6]
    const double* blen_vecs;
    const int32_t* vec;
    const double* scale;
    const int32_t* pidx;
    const double* pfac;
    CandPtrs at(int64_t done) const { return {locus + done, exch + done * 6, blen_vecs, vec + done, scale + done, pidx + done, pfac + done}; }
};

// LikParams of the eigenbasis kernels for the plan as it stands (a pattern view of stage 1 may have swapped its columns)
LikParams lik_params(const tphip_plan* p, const uint8_t* d_states, const CandPtrs& c, double* d_out) {
    LikParams L;
    L.states = d_states; L.ncols_total = p->ncols; L.locus_offsets = p->d_offsets.p; L.models = p->d_models.p;
    L.col_weight = p->d_col_weight;
    L.lops = p->d_lik_ops.p; L.nops = (int32_t)p->prog.ops.size(); L.nnodes = p->nnodes; L.ntaxa = p->ntaxa;
    L.stack_depth = p->prog.stack_depth; L.cand_locus = c.locus; L.cand_exch = c.exch;
    L.blen_vecs = c.blen_vecs; L.cand_vec = c.vec; L.cand_scale = c.scale; L.cand_pidx = c.pidx;
    L.cand_pfac = c.pfac; L.out = d_out;
    return L;
}

// Eigen-systems and transition matrices of the `n` candidates of a chunk (transition-matrix kernels)
int launch_chunk_matrices(hipStream_t st, const tphip_plan* p, const CandPtrs& c, int64_t n, double* d_eig, double* d_pmat) {
    HIP_TRY(launch_lik_eigen_kernel(st, p->d_models.p, c.locus, c.exch, n, d_eig));
    HIP_TRY(launch_lik_pmat_kernel(st, d_eig, c.blen_vecs, c.vec, c.scale, c.pidx, c.pfac, n, p->nnodes, d_pmat));
    return TPHIP_OK;
}

}  // namespace

extern "C" {

int tphip_locus_loglik_dev(tphip_plan* p, const uint8_t* d_states, int64_t ncand, const int32_t* d_cand_locus,
                           const double* d_cand_exch, const double* d_blen_vecs, const int32_t* d_cand_vec,
                           const double* d_cand_scale, const int32_t* d_cand_pidx, const double* d_cand_pfac, double* d_out,
                           void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (ncand < 0 || (ncand && (!d_states || !d_cand_locus || !d_cand_exch || !d_blen_vecs || !d_cand_vec || !d_cand_scale ||
                                !d_cand_pidx || !d_cand_pfac || !d_out)))
        return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ncand == 0) return TPHIP_OK;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const CandPtrs cand{d_cand_locus, d_cand_exch, d_blen_vecs, d_cand_vec, d_cand_scale, d_cand_pidx, d_cand_pfac};
    if (p->locus.value_cols > 0) {
        // transition-matrix form: eigen-systems and matrices of a chunk of candidates, then the pruning kernel
        const int C = p->locus.value_cols;
        const int nsplit = lik_nsplit(p->num_cus, p->max_locus_cols, ncand, kLikBlock * C);
        if (nsplit > 1) {
            int rc = p->part.reserve((size_t)ncand * nsplit * sizeof(double));
            if (rc) return rc;
        }
        double* d_part = (double*)p->part.p;
        const int64_t chunk = value_chunk(p->nnodes, ncand, nsplit);
        int rc = p->value_ws.reserve((size_t)chunk * value_ws_per_cand(p->nnodes));
        if (rc) return rc;
        double* d_eig = (double*)p->value_ws.p;
        double* d_pmat = d_eig + (size_t)chunk * 36;
        ValueParams V;
        V.states = d_states; V.ncols_total = p->ncols; V.locus_offsets = p->d_offsets.p; V.col_weight = p->d_col_weight;
        V.models = p->d_models.p; V.vops = p->d_value_ops.p; V.nvops = p->value_nops; V.ntaxa = p->ntaxa;
        V.nnodes = p->nnodes; V.pmat = d_pmat; V.nsplit = nsplit;
        V.tip_taxon = p->d_tip_taxon.p; V.nwords = p->nwords; V.tip_node = p->d_value_tip_node.p;
        V.packed = (d_states == p->lib_states) ? p->d_value_packed : nullptr;
        for (int64_t done = 0; done < ncand; done += chunk) {
            const int64_t n = std::min<int64_t>(ncand - done, chunk);
            const CandPtrs c = cand.at(done);
            rc = launch_chunk_matrices(st, p, c, n, d_eig, d_pmat);
            if (rc) return rc;
            V.cand_locus = c.locus;
            V.out = (nsplit > 1 ? d_part : d_out) + done * nsplit;
            HIP_TRY(launch_locus_value_kernel(C, p->prog.stack_depth, dim3((unsigned)(n * nsplit)), p->locus.value_lds, st, V));
        }
        HIP_TRY(hipGetLastError());
        if (nsplit > 1) {
            HIP_TRY(launch_split_sum_kernel(st, d_part, d_out, ncand, nsplit, 1));
        }
        return TPHIP_OK;
    }
    if (!p->locus.lik_ok) return fail(TPHIP_ERR_INVALID, "tree too large for the locus-likelihood kernel's LDS tables");
    const int nsplit = lik_nsplit(p->num_cus, p->max_locus_cols, ncand, kLikBlock);
    if (nsplit > 1) {
        int rc = p->part.reserve((size_t)ncand * nsplit * sizeof(double));
        if (rc) return rc;
    }
    double* d_part = (double*)p->part.p;
    double* out = nsplit > 1 ? d_part : d_out;
    const int64_t per_launch = std::max<int64_t>(1, kMaxGridX / nsplit);
    for (int64_t done = 0; done < ncand; done += per_launch) {
        const int64_t n = std::min<int64_t>(ncand - done, per_launch);
        LikParams Q = lik_params(p, d_states, cand.at(done), out + done * nsplit);
        Q.nsplit = nsplit;
        HIP_TRY(launch_locus_loglik_kernel(dim3((unsigned)(n * nsplit)), p->locus.lik_lds, st, Q));
    }
    HIP_TRY(hipGetLastError());
    if (nsplit > 1) {
        HIP_TRY(launch_split_sum_kernel(st, d_part, d_out, ncand, nsplit, 1));
    }
    return TPHIP_OK;
}

int tphip_locus_gradient_dev(tphip_plan* p, const uint8_t* d_states, int64_t ncand, const int32_t* d_cand_locus,
                             const double* d_cand_exch, const double* d_blen_vecs, const int32_t* d_cand_vec,
                             const double* d_cand_scale, const int32_t* d_cand_pidx, const double* d_cand_pfac, double* d_lnl,
                             double* d_dexch, double* d_dlogt, double* d_sum_dlogt, double* d_d2logt, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (ncand < 0 || (ncand && (!d_states || !d_cand_locus || !d_cand_exch || !d_blen_vecs || !d_cand_vec || !d_cand_scale ||
                                !d_cand_pidx || !d_cand_pfac || !d_lnl || !d_dexch || !d_sum_dlogt)))
        return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ncand == 0) return TPHIP_OK;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const CandPtrs cand{d_cand_locus, d_cand_exch, d_blen_vecs, d_cand_vec, d_cand_scale, d_cand_pidx, d_cand_pfac};
    const bool grad2 = p->locus.grad2_ok && d_states == p->lib_states && p->d_value_packed;
    if (!grad2 && !p->locus.grad_ok) return fail(TPHIP_ERR_INVALID, "tree too large for the locus-gradient kernel's LDS tables");
    // where the kernel writes: the caller's arrays, or with a column split the partial sums of every (candidate, slice) item
    const size_t nn = (size_t)p->nnodes;
    const int nsplit = lik_nsplit(p->num_cus, p->max_locus_cols, ncand, grad2 ? kGrad2Block : kGradBlock);
    const size_t items = (size_t)ncand * nsplit;
    double *o_lnl = d_lnl, *o_sum = d_sum_dlogt, *o_dex = d_dexch, *o_dlt = d_dlogt, *o_d2 = d_d2logt;
    if (nsplit > 1) {
        const GradOutLayout part(items, nn, d_dlogt != nullptr, d_d2logt != nullptr);
        int rc = p->part.reserve(part.total * sizeof(double));
        if (rc) return rc;
        double* d_part = (double*)p->part.p;
        o_lnl = d_part + part.lnl; o_sum = d_part + part.sum_dlogt; o_dex = d_part + part.dexch;
        o_dlt = d_dlogt ? d_part + part.dlogt : nullptr;
        o_d2 = d_d2logt ? d_part + part.d2logt : nullptr;
    }
    if (grad2) {
        // transition-matrix gradient kernel (locus_grad2_kernel.hpp): eigen-systems, matrices and branch tables of a chunk
        // of candidates, then resident workgroups loop over (candidate, column slice) items, each with its own tape
        const int64_t chunk = grad2_chunk(p->nnodes, ncand);
        int rc = p->grad2_ws.reserve((size_t)chunk * grad2_ws_per_cand(p->nnodes));
        if (rc) return rc;
        double* d_eig = (double*)p->grad2_ws.p;
        double* d_pmat = d_eig + (size_t)chunk * 36;
        double* d_ef = d_pmat + (size_t)chunk * nn * 16;
        const int64_t grid_max = (int64_t)p->num_cus * p->locus.grad2_blocks_per_cu;
        rc = p->tape.reserve(grad2_tape_bytes(std::min<int64_t>(chunk * nsplit, grid_max), p->grad2_ntape));
        if (rc) return rc;
        rc = p->grad2_params.reserve(sizeof(Grad2Params) * 64);
        if (rc) return rc;
        int slot = 0;
        for (int64_t done = 0; done < ncand; done += chunk, ++slot) {
            const int64_t n = std::min<int64_t>(ncand - done, chunk);
            const CandPtrs c = cand.at(done);
            rc = launch_chunk_matrices(st, p, c, n, d_eig, d_pmat);
            if (rc) return rc;
            HIP_TRY(launch_grad2_ef_kernel(st, d_eig, c.blen_vecs, c.vec, c.scale, c.pidx, c.pfac, n, p->nnodes, d_ef));
            Grad2Params G2;
            G2.packed = p->d_value_packed; G2.ncols_total = p->ncols; G2.locus_offsets = p->d_offsets.p; G2.col_weight = p->d_col_weight;
            G2.models = p->d_models.p; G2.fops = p->d_grad2_fops.p; G2.rops = p->d_grad2_rops.p; G2.nrops = p->grad2_nrops;
            G2.ntaxa = p->ntaxa; G2.nnodes = p->nnodes; G2.nwords = p->nwords; G2.ntape = p->grad2_ntape; G2.rdepth = p->grad2_rdepth;
            G2.tip_node = p->d_value_tip_node.p; G2.cand_locus = c.locus; G2.eig = d_eig; G2.pmat = d_pmat; G2.ef = d_ef;
            G2.ncand = n; G2.nsplit = nsplit; G2.tape = (double*)p->tape.p;
            const size_t o = (size_t)done * nsplit;
            G2.out_lnl = o_lnl + o; G2.out_sum_dlogt = o_sum + o; G2.out_dexch = o_dex + o * 6;
            G2.out_dlogt = o_dlt ? o_dlt + o * nn : nullptr; G2.out_d2logt = o_d2 ? o_d2 + o * nn : nullptr;
            if (slot >= 64) { HIP_TRY(hipStreamSynchronize(st)); slot = 0; }   // the parameter blocks in flight are a ring of 64
            Grad2Params* d_par = (Grad2Params*)p->grad2_params.p + slot;
            HIP_TRY(hipMemcpyAsync(d_par, &G2, sizeof(Grad2Params), hipMemcpyHostToDevice, st));
            const int64_t grid = std::min<int64_t>(n * nsplit, grid_max);
            HIP_TRY(launch_locus_grad2_kernel(p->prog.stack_depth, dim3((unsigned)grid), p->locus.grad2_lds, st, d_par));
        }
    } else {
        // reverse-mode kernel in the eigenbasis (locus_lik_kernel.hpp): resident workgroups loop over the items; each owns one tape
        GradParams G;
        G.L = lik_params(p, d_states, cand, o_lnl);
        G.L.stage_states = p->locus.grad_stage;
        G.L.nsplit = nsplit;
        G.ntape = p->prog.ntape; G.ncand = ncand; G.nslots = p->locus.grad_slots;
        G.out_dexch = o_dex; G.out_dlogt = o_dlt; G.out_sum_dlogt = o_sum; G.out_d2logt = o_d2;
        const int64_t grid = std::min<int64_t>((int64_t)items, (int64_t)p->num_cus * p->locus.grad_blocks_per_cu);
        int rc = p->tape.reserve(grad_tape_bytes(grid, p->prog.ntape, p->prog.stack_depth));
        if (rc) return rc;
        G.tape = (double*)p->tape.p;
        // eigen-systems of the candidates by one thread each (locus_value_launch.hip) instead of thread 0 of every work item
        rc = p->grad_eig.reserve((size_t)ncand * 36 * sizeof(double));
        if (rc) return rc;
        HIP_TRY(launch_lik_eigen_kernel(st, p->d_models.p, d_cand_locus, d_cand_exch, ncand, (double*)p->grad_eig.p));
        G.cand_eig = (const double*)p->grad_eig.p;
        rc = p->grad_params.reserve(sizeof(GradParams));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(p->grad_params.p, &G, sizeof(GradParams), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_locus_grad_kernel(dim3((unsigned)grid), p->locus.grad_lds, st, (const GradParams*)p->grad_params.p));
    }
    if (nsplit > 1) {
        (void)launch_split_sum_kernel(st, o_lnl, d_lnl, ncand, nsplit, 1);
        (void)launch_split_sum_kernel(st, o_sum, d_sum_dlogt, ncand, nsplit, 1);
        (void)launch_split_sum_kernel(st, o_dex, d_dexch, ncand, nsplit, 6);
        if (d_dlogt) (void)launch_split_sum_kernel(st, o_dlt, d_dlogt, ncand, nsplit, (int)nn);
        if (d_d2logt) (void)launch_split_sum_kernel(st, o_d2, d_d2logt, ncand, nsplit, (int)nn);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

int tphip_plan_set_column_weights(tphip_plan* p, const double* weights) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    if (p->d_col_weight) { HIP_TRY(hipFree(p->d_col_weight)); p->d_col_weight = nullptr; }
    if (!weights || p->ncols == 0) return TPHIP_OK;
    for (int64_t c = 0; c < p->ncols; ++c)
        if (!(weights[c] >= 0.0)) return fail(TPHIP_ERR_INVALID, "column weights must be >= 0");
    HIP_TRY(hipMalloc((void**)&p->d_col_weight, sizeof(double) * (size_t)p->ncols));
    HIP_TRY(hipMemcpy(p->d_col_weight, weights, sizeof(double) * (size_t)p->ncols, hipMemcpyHostToDevice));
    return TPHIP_OK;
}

int tphip_free_device(tphip_plan* p, void* d_ptr) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    if (d_ptr && d_ptr == (void*)p->lib_states) {   // the alignment cache goes: so do the codes packed from it
        if (p->d_value_packed) { HIP_TRY(hipFree(p->d_value_packed)); p->d_value_packed = nullptr; }
        p->lib_states = nullptr;
    }
    if (d_ptr) HIP_TRY(hipFree(d_ptr));
    return TPHIP_OK;
}

}  // extern "C"

// ---- host-pointer wrappers -------------------------------------------------------------------------

// Candidate batch staged through the plan's arena: one pinned buffer, one H2D copy in, one D2H copy out.
namespace {
struct CandBatch {
    size_t off_locus, off_exch, off_blen, off_vec, off_scale, off_pidx, off_pfac, in_bytes;
    size_t off_out, out_bytes, total;
    CandPtrs on(const char* base) const {   // the staged candidates in the arena at `base`
        return {(const int32_t*)(base + off_locus), (const double*)(base + off_exch), (const double*)(base + off_blen),
                (const int32_t*)(base + off_vec), (const double*)(base + off_scale), (const int32_t*)(base + off_pidx),
                (const double*)(base + off_pfac)};
    }
};

int arena_reserve(tphip_plan* p, size_t bytes) {
    HostArena& A = p->arena;
    if (bytes <= A.bytes) return TPHIP_OK;
    const size_t want = std::max(bytes, A.bytes * 2);
    if (A.d) { HIP_TRY(hipFree(A.d)); A.d = nullptr; }
    if (A.h) { HIP_TRY(hipHostFree(A.h)); A.h = nullptr; }
    A.bytes = 0;
    HIP_TRY(hipMalloc((void**)&A.d, want));
    HIP_TRY(hipHostMalloc((void**)&A.h, want, hipHostMallocDefault));
    A.bytes = want;
    return TPHIP_OK;
}

int check_candidates(const tphip_plan* p, int64_t nvec, int64_t ncand, const int32_t* cand_locus, const int32_t* cand_vec,
                     const int32_t* cand_pidx) {
    for (int64_t c = 0; c < ncand; ++c) {
        if (cand_locus[c] < 0 || cand_locus[c] >= p->nloci) return fail(TPHIP_ERR_INVALID, "cand_locus out of range");
        if (cand_vec[c] < 0 || cand_vec[c] >= nvec) return fail(TPHIP_ERR_INVALID, "cand_vec out of range");
        if (cand_pidx[c] >= p->nnodes) return fail(TPHIP_ERR_INVALID, "cand_pidx out of range");
    }
    return TPHIP_OK;
}

// device copy of the alignment: the caller's cache, or a scratch buffer for this call
int stage_alignment(tphip_plan* p, const uint8_t* states, void** d_states_cache, Scratch& S, uint8_t** d_s) {
    const size_t nb = (size_t)p->ncols * (size_t)p->ntaxa;
    *d_s = d_states_cache ? (uint8_t*)*d_states_cache : nullptr;
    if (*d_s) return TPHIP_OK;
    if (d_states_cache) {
        HIP_TRY(hipMalloc((void**)d_s, nb ? nb : 1));
        *d_states_cache = *d_s;
    } else {
        *d_s = S.get<uint8_t>(nb);
        if (!*d_s) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    }
    HIP_TRY(hipMemcpy(*d_s, states, nb, hipMemcpyHostToDevice));
    if (d_states_cache && p->locus.value_cols > 0 && p->ncols > 0) {
        // a copy that stays: pack its state codes once for locus_value_kernel (8 per word, tip order) instead of once per
        // likelihood evaluation.  Only for the copy made here -- the library cannot know when a caller's own device array changes.
        if (p->d_value_packed) { HIP_TRY(hipFree(p->d_value_packed)); p->d_value_packed = nullptr; }
        p->lib_states = nullptr;
        HIP_TRY(hipMalloc((void**)&p->d_value_packed, sizeof(uint32_t) * (size_t)p->nwords * (size_t)p->ncols));
        HIP_TRY(launch_value_pack_codes_kernel(nullptr, *d_s, p->ncols, p->d_tip_taxon.p, p->nwords, p->d_value_packed));
        HIP_TRY(hipStreamSynchronize(nullptr));   // later launches may come on any stream
        p->lib_states = *d_s;
    }
    return TPHIP_OK;
}

int stage_candidates(tphip_plan* p, int64_t nvec, const double* blen_vecs, int64_t ncand, const int32_t* cand_locus,
                     const double* cand_exch, const int32_t* cand_vec, const double* cand_scale, const int32_t* cand_pidx,
                     const double* cand_pfac, size_t out_doubles, CandBatch* B) {
    const size_t n = (size_t)ncand, nn = (size_t)p->nnodes;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    B->off_locus = take(sizeof(int32_t) * n);
    B->off_exch = take(sizeof(double) * n * 6);
    B->off_blen = take(sizeof(double) * (size_t)nvec * nn);
    B->off_vec = take(sizeof(int32_t) * n);
    B->off_scale = take(sizeof(double) * n);
    B->off_pidx = take(sizeof(int32_t) * n);
    B->off_pfac = take(sizeof(double) * n);
    B->in_bytes = off;
    B->off_out = take(sizeof(double) * out_doubles);
    B->out_bytes = sizeof(double) * out_doubles;
    B->total = off;
    int rc = arena_reserve(p, B->total);
    if (rc) return rc;
    char* h = p->arena.h;
    memcpy(h + B->off_locus, cand_locus, sizeof(int32_t) * n);
    memcpy(h + B->off_exch, cand_exch, sizeof(double) * n * 6);
    memcpy(h + B->off_blen, blen_vecs, sizeof(double) * (size_t)nvec * nn);
    memcpy(h + B->off_vec, cand_vec, sizeof(int32_t) * n);
    memcpy(h + B->off_scale, cand_scale, sizeof(double) * n);
    memcpy(h + B->off_pidx, cand_pidx, sizeof(int32_t) * n);
    memcpy(h + B->off_pfac, cand_pfac, sizeof(double) * n);
    HIP_TRY(hipMemcpyAsync(p->arena.d, h, B->in_bytes, hipMemcpyHostToDevice, nullptr));
    return TPHIP_OK;
}
}  // namespace

extern "C" {

// device copy of the alignment in the caller's cache slot, for the other translation units (stage1_driver.hip)
int tphip_internal_stage_alignment(tphip_plan* p, const uint8_t* states, void** d_states_cache, uint8_t** d_s) {
    Scratch S;
    return stage_alignment(p, states, d_states_cache, S, d_s);
}

int tphip_locus_loglik(tphip_plan* p, const uint8_t* states, void** d_states_cache, int64_t nvec, const double* blen_vecs,
                       int64_t ncand, const int32_t* cand_locus, const double* cand_exch, const int32_t* cand_vec,
                       const double* cand_scale, const int32_t* cand_pidx, const double* cand_pfac, double* out) {
    if (!p || !states || ncand < 0 || nvec < 0 ||
        (ncand && (!blen_vecs || !cand_locus || !cand_exch || !cand_vec || !cand_scale || !cand_pidx || !cand_pfac || !out)))
        return fail(TPHIP_ERR_INVALID, "null argument");
    if (ncand == 0) return TPHIP_OK;
    int rc = check_candidates(p, nvec, ncand, cand_locus, cand_vec, cand_pidx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    uint8_t* d_s = nullptr;
    rc = stage_alignment(p, states, d_states_cache, S, &d_s);
    if (rc) return rc;
    CandBatch B;
    rc = stage_candidates(p, nvec, blen_vecs, ncand, cand_locus, cand_exch, cand_vec, cand_scale, cand_pidx, cand_pfac,
                          (size_t)ncand, &B);
    if (rc) return rc;
    char* d = p->arena.d;
    const CandPtrs c = B.on(d);
    rc = tphip_locus_loglik_dev(p, d_s, ncand, c.locus, c.exch, c.blen_vecs, c.vec, c.scale, c.pidx, c.pfac, (double*)(d + B.off_out),
                                nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p->arena.h + B.off_out, d + B.off_out, B.out_bytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    memcpy(out, p->arena.h + B.off_out, B.out_bytes);
    return TPHIP_OK;
}

int tphip_locus_gradient(tphip_plan* p, const uint8_t* states, void** d_states_cache, int64_t nvec, const double* blen_vecs,
                         int64_t ncand, const int32_t* cand_locus, const double* cand_exch, const int32_t* cand_vec,
                         const double* cand_scale, const int32_t* cand_pidx, const double* cand_pfac, double* lnl,
                         double* dexch, double* dlogt, double* sum_dlogt, double* d2logt) {
    if (!p || !states || ncand < 0 || nvec < 0 ||
        (ncand && (!blen_vecs || !cand_locus || !cand_exch || !cand_vec || !cand_scale || !cand_pidx || !cand_pfac || !lnl ||
                   !dexch || !sum_dlogt)))
        return fail(TPHIP_ERR_INVALID, "null argument");
    if (ncand == 0) return TPHIP_OK;
    int rc = check_candidates(p, nvec, ncand, cand_locus, cand_vec, cand_pidx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    uint8_t* d_s = nullptr;
    rc = stage_alignment(p, states, d_states_cache, S, &d_s);
    if (rc) return rc;
    const size_t n = (size_t)ncand, nn = (size_t)p->nnodes;
    const GradOutLayout lay(n, nn, dlogt != nullptr, d2logt != nullptr);   // the outputs, staged as one block
    CandBatch B;
    rc = stage_candidates(p, nvec, blen_vecs, ncand, cand_locus, cand_exch, cand_vec, cand_scale, cand_pidx, cand_pfac, lay.total, &B);
    if (rc) return rc;
    char* d = p->arena.d;
    const CandPtrs c = B.on(d);
    double* d_o = (double*)(d + B.off_out);
    rc = tphip_locus_gradient_dev(p, d_s, ncand, c.locus, c.exch, c.blen_vecs, c.vec, c.scale, c.pidx, c.pfac, d_o + lay.lnl,
                                  d_o + lay.dexch, dlogt ? d_o + lay.dlogt : nullptr, d_o + lay.sum_dlogt,
                                  d2logt ? d_o + lay.d2logt : nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p->arena.h + B.off_out, d + B.off_out, B.out_bytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    const double* h_o = (const double*)(p->arena.h + B.off_out);
    memcpy(lnl, h_o + lay.lnl, sizeof(double) * n);
    memcpy(sum_dlogt, h_o + lay.sum_dlogt, sizeof(double) * n);
    memcpy(dexch, h_o + lay.dexch, sizeof(double) * n * 6);
    if (dlogt) memcpy(dlogt, h_o + lay.dlogt, sizeof(double) * n * nn);
    if (d2logt) memcpy(d2logt, h_o + lay.d2logt, sizeof(double) * n * nn);
    return TPHIP_OK;
}

}  // extern "C"

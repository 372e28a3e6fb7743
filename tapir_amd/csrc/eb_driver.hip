// eb_driver.hip -- empirical-Bayes site rates under a discrete-gamma prior: the per-locus reduction
// and scale-step kernels, and the C entry points tphip_eb_fit_scale / tphip_eb_posterior.
//
// Division of labour (as in stage1_driver.hip): the kernels do the arithmetic, the host sequences launches and reads one
// counter per round.  A round of the fit is  site_posterior_kernel (per column: log m_c and its two u-derivatives)
// -> locus_marginal_reduce_kernel (per locus: l, dl/du, d2l/du2 in a fixed order) -> eb_scale_step_kernel (per locus:
// safeguarded Newton step in u = log mu).  No per-column array crosses PCIe during the fit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "site_posterior_params.hpp"
#include "tphip_internal.hpp"

namespace tphip {

constexpr int kEbDefaultMaxIt = 60;
constexpr double kEbDefaultTol = 1e-9;

struct EbLocusState {
    double* u;          // [L] log mu (the posterior kernel's log_scale)
    double* lo;         // [L] bracket of the maximiser: slope > 0 at lo ...
    double* hi;         // [L] ... slope <= 0 at hi
    double* sums;       // [L][3] l, dl/du, d2l/du2 at u
    int32_t* done;      // [L] 0 = iterating, 1 = converged, 2 = iteration limit
    int32_t* iters;     // [L] evaluations so far
    int32_t* active;    // [1] loci still iterating after this round
};

// l = sum_c n_c f_c and its two u-derivatives for one locus.  The sum always runs over the locus' COLUMNS, a repeated
// pattern read through its representative (n_c is thereby implicit), in a fixed order: thread t adds columns t, t + 256,
// ... of the locus in sequence, then a binary tree over the 256 partial sums.  The order depends on nothing but the
// locus' own columns, so a locus gives the same bits whatever the batch around it, with or without site patterns.
__global__ __launch_bounds__(kEbReduceBlock) void locus_marginal_reduce_kernel(const int64_t* __restrict__ locus_offsets,
                                                                               const int32_t* __restrict__ dup_of,
                                                                               const double* __restrict__ f,
                                                                               const double* __restrict__ g,
                                                                               const double* __restrict__ h,
                                                                               const int32_t* __restrict__ done,
                                                                               double* __restrict__ sums) {
    __shared__ double red[3][kEbReduceBlock];
    const int locus = blockIdx.x;
    if (done && done[locus]) return;
    const int64_t lo = locus_offsets[locus], hi = locus_offsets[locus + 1];
    double sf = 0.0, sg = 0.0, sh = 0.0;
    for (int64_t c = lo + threadIdx.x; c < hi; c += kEbReduceBlock) {
        const int32_t r = dup_of[c];
        const int64_t src = r >= 0 ? (int64_t)r : c;
        sf += f[src]; sg += g[src]; sh += h[src];
    }
    red[0][threadIdx.x] = sf; red[1][threadIdx.x] = sg; red[2][threadIdx.x] = sh;
    __syncthreads();
    for (int o = kEbReduceBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
            red[2][threadIdx.x] += red[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) sums[(int64_t)locus * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// One thread per locus: a safeguarded Newton step on u = log mu from (l, l', l'') at u.  The sign of l' moves one end of
// the bracket [lo, hi] (initially [kUMin, kUMax]) to u.  A Newton step is taken only where the curvature is negative and
// only if it lands inside the bracket, limited to kStepMax; anywhere else (l flattens out as mu -> infinity: every
// category saturated, l' and l'' -> 0) the step halves the distance to the bracket's end on the uphill side, again at
// most kStepMax.  Converged when a Newton step is below tol (the step is then NOT applied: u, l and l'' are reported at
// the point that was evaluated) or the bracket has closed.
__global__ void eb_scale_step_kernel(EbLocusState X, int64_t nloci, double tol, int32_t maxit) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nloci || X.done[l]) return;
    const double u = X.u[l], G = X.sums[l * 3 + 1], H = X.sums[l * 3 + 2];
    double lo = X.lo[l], hi = X.hi[l];
    const int32_t it = X.iters[l] + 1;
    X.iters[l] = it;
    if (G == 0.0 && H == 0.0) { X.done[l] = 1; return; }   // no column, or nothing but gaps: l does not depend on mu
    const bool uphill = G > 0.0;
    if (uphill) lo = u; else hi = u;
    X.lo[l] = lo; X.hi[l] = hi;
    bool newton = H < 0.0;
    double step = 0.0;
    if (newton) {
        step = fmin(fmax(-G / H, -kStepMax), kStepMax);
        const double cand = u + step;
        newton = cand > lo && cand < hi;
        if (fabs(step) < tol) { X.done[l] = 1; return; }   // (step = 0 where G = 0: inside the bracket or not, this is the maximum)
    }
    if (!newton) step = uphill ? fmin(kStepMax, 0.5 * (hi - u)) : -fmin(kStepMax, 0.5 * (u - lo));
    if (hi - lo < tol) { X.done[l] = 1; return; }
    if (it >= maxit) { X.done[l] = 2; return; }
    X.u[l] = u + step;
    atomicAdd(X.active, 1);
}

// rate = kappa mu E[rho | column], sd = kappa mu sd[rho | column], ll = log m_c; repeated patterns copy their representative
__global__ __launch_bounds__(256) void eb_finish_kernel(const int64_t* __restrict__ locus_offsets, const int32_t* __restrict__ chunk_locus,
                                                       const int32_t* __restrict__ chunk_index, const LocusModel* __restrict__ models,
                                                       const int32_t* __restrict__ dup_of, const double* __restrict__ log_scale,
                                                       const double* __restrict__ f, const double* __restrict__ mean,
                                                       const double* __restrict__ second, double* __restrict__ rate,
                                                       double* __restrict__ sd, double* __restrict__ lnl) {
    const int locus = chunk_locus[blockIdx.x];
    const int64_t hi = locus_offsets[locus + 1];
    const int64_t base = locus_offsets[locus] + (int64_t)chunk_index[blockIdx.x] * 1024;
    const double km = models[locus].kappa * exp(log_scale[locus]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t c = base + j * 256 + threadIdx.x;
        if (c >= hi) continue;
        const int32_t r = dup_of[c];
        const int64_t src = r >= 0 ? (int64_t)r : c;
        const double m = mean[src];
        rate[c] = km * m;
        sd[c] = km * sqrt(fmax(second[src] - m * m, 0.0));
        lnl[c] = f[src];
    }
}

}  // namespace tphip

namespace {

struct EbWorkspace {
    EbPrep prep;
    PosteriorParams E;
    EbLocusState X;
    double* cat_rate;
    double* cat_logw;
};

// the next `count` elements of the workspace at base + off (base may be null: sizing pass)
template <typename T>
T* carve(void* base, size_t& off, size_t count) {
    T* r = (T*)((uintptr_t)base + off);
    off += align_up(sizeof(T) * (count ? count : 1), 256);
    return r;
}

size_t eb_layout(void* base, size_t n, size_t L, size_t K, size_t nw, EbWorkspace& W) {
    size_t off = 0;
    EbPrep& B = W.prep;
    PosteriorParams& E = W.E;
    B.packed = carve<uint32_t>(base, off, nw * n); B.nres = carve<int32_t>(base, off, n); B.flag = carve<uint8_t>(base, off, n);
    E.f = carve<double>(base, off, n); E.g = carve<double>(base, off, n); E.h = carve<double>(base, off, n);
    E.mean = carve<double>(base, off, n); E.second = carve<double>(base, off, n);
    B.scratch[0] = E.f; B.scratch[1] = E.g; B.scratch[2] = E.h;
    B.hash = carve<uint64_t>(base, off, n); B.dup_of = carve<int32_t>(base, off, n);
    B.tab_key = carve<unsigned long long>(base, off, 2 * n); B.tab_val = carve<int32_t>(base, off, 2 * n);
    B.on = carve<int32_t>(base, off, L); B.work_cols = carve<int32_t>(base, off, n); B.work_count = carve<int32_t>(base, off, L);
    W.X.u = carve<double>(base, off, L); W.X.lo = carve<double>(base, off, L); W.X.hi = carve<double>(base, off, L);
    W.X.sums = carve<double>(base, off, 3 * L); W.X.done = carve<int32_t>(base, off, L); W.X.iters = carve<int32_t>(base, off, L);
    W.X.active = carve<int32_t>(base, off, 1);
    W.cat_rate = carve<double>(base, off, L * K); W.cat_logw = carve<double>(base, off, L * K);
    return off;
}

int eb_check(const tphip_plan* p, const tphip_eb_opts* o, const double* cat_rate, const double* cat_weight, const double* scale) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_eb_opts");
    if (o->struct_size < sizeof(tphip_eb_opts)) return fail(TPHIP_ERR_INVALID, "tphip_eb_opts.struct_size is smaller than this library's struct");
    if (o->ncat < 2 || o->ncat > kEbMaxCat) return fail(TPHIP_ERR_INVALID, "tphip_eb_opts.ncat must be in 2..16");
    if (o->maxit_scale < 0 || !(o->tol_scale >= 0.0)) return fail(TPHIP_ERR_INVALID, "tphip_eb_opts.maxit_scale / tol_scale must be >= 0");
    if (!cat_rate || !cat_weight) return fail(TPHIP_ERR_INVALID, "null category table");
    if (!scale) return fail(TPHIP_ERR_INVALID, "null scale");
    for (int64_t i = 0; i < p->nloci * o->ncat; ++i) {
        if (!(cat_rate[i] > 0.0) || !std::isfinite(cat_rate[i])) return fail(TPHIP_ERR_INVALID, "category rates must be positive and finite");
        if (!(cat_weight[i] > 0.0) || !std::isfinite(cat_weight[i])) return fail(TPHIP_ERR_INVALID, "category weights must be positive and finite");
    }
    for (int64_t l = 0; l < p->nloci; ++l)
        if (!(scale[l] > 0.0) || !std::isfinite(scale[l])) return fail(TPHIP_ERR_INVALID, "scales must be positive and finite");
    return TPHIP_OK;
}

// workspace + uploads + classification; after it returns W.E is ready for launch_posterior
int eb_setup(tphip_plan* p, const uint8_t* d_states, const tphip_eb_opts* o, const double* cat_rate, const double* cat_weight,
             const double* scale, hipStream_t st, EbWorkspace& W) {
    const size_t n = (size_t)p->ncols, L = (size_t)p->nloci, K = (size_t)o->ncat;
    const size_t nw = (size_t)(p->nwords > 0 ? p->nwords : 1);
    const size_t need = eb_layout(nullptr, n, L, K, nw, W);
    if (const int rc = p->eb_ws.reserve(need)) return rc;
    eb_layout(p->eb_ws.p, n, L, K, nw, W);
    EbPrep& B = W.prep;
    PosteriorParams& E = W.E;

    std::vector<double> h_logw(L * K), h_u(L);
    for (size_t i = 0; i < L * K; ++i) h_logw[i] = std::log(cat_weight[i]);
    for (size_t l = 0; l < L; ++l) h_u[l] = std::min(std::max(std::log(scale[l]), kUMin), kUMax);
    HIP_TRY(hipMemcpyAsync(W.cat_rate, cat_rate, sizeof(double) * L * K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.cat_logw, h_logw.data(), sizeof(double) * L * K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.X.u, h_u.data(), sizeof(double) * L, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the staging vectors leave scope
    int rc = tphip_internal_eb_prepare(p, d_states, &B, o->use_patterns ? 1 : 0, nullptr, st);
    if (rc) return rc;

    SiteParams& S = E.S;
    S = plan_site_params(p, d_states, true);   // the packed tip words go with the fused-cherry stream
    S.packed = B.packed; S.nwords = p->nwords;
    S.work_cols = o->use_patterns ? B.work_cols : nullptr;
    S.work_count = o->use_patterns ? B.work_count : nullptr;
    E.ncat = o->ncat; E.cat_rate = W.cat_rate; E.cat_logw = W.cat_logw; E.log_scale = W.X.u; E.done = nullptr;
    return TPHIP_OK;
}

int launch_posterior(tphip_plan* p, const PosteriorParams& E, hipStream_t st) {
    if (p->n_site_chunks <= 0) return TPHIP_OK;
    const size_t lds = site_lds_bytes(p->prog.stack_depth);
    HIP_TRY(launch_site_posterior_kernel(site_variant(p->nwords), p->model, dim3((unsigned)p->n_site_chunks), lds, st, E));
    return TPHIP_OK;
}

// the posterior-table variant: the same launch with the categories' f_k + log w_k stored at logp [K][ncols]
int launch_posterior_table(tphip_plan* p, const PosteriorParams& E, double* logp, hipStream_t st) {
    if (p->n_site_chunks <= 0) return TPHIP_OK;
    PosteriorTableParams T;
    static_cast<PosteriorParams&>(T) = E;
    T.logp = logp;
    const size_t lds = site_lds_bytes(p->prog.stack_depth);
    HIP_TRY(launch_site_posterior_table_kernel(site_variant(p->nwords), p->model, dim3((unsigned)p->n_site_chunks), lds, st, T));
    return TPHIP_OK;
}

}  // namespace

extern "C" {

int tphip_eb_fit_scale_dev(tphip_plan* p, const uint8_t* d_states, const tphip_eb_opts* o, const double* cat_rate,
                           const double* cat_weight, double* scale, double* locus_lnl, double* curvature, int32_t* iters,
                           void* stream) {
    int rc = eb_check(p, o, cat_rate, cat_weight, scale);
    if (rc) return rc;
    if (!d_states) return fail(TPHIP_ERR_INVALID, "null states");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t L = (size_t)p->nloci;
    if (L == 0) return TPHIP_OK;
    EbWorkspace W;
    rc = eb_setup(p, d_states, o, cat_rate, cat_weight, scale, st, W);
    if (rc) return rc;
    const int32_t maxit = o->maxit_scale > 0 ? o->maxit_scale : kEbDefaultMaxIt;
    const double tol = o->tol_scale > 0.0 ? o->tol_scale : kEbDefaultTol;
    std::vector<double> h_lo(L, kUMin), h_hi(L, kUMax);
    HIP_TRY(hipMemcpyAsync(W.X.lo, h_lo.data(), sizeof(double) * L, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.X.hi, h_hi.data(), sizeof(double) * L, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(W.X.done, 0, sizeof(int32_t) * L, st));
    HIP_TRY(hipMemsetAsync(W.X.iters, 0, sizeof(int32_t) * L, st));
    W.E.done = W.X.done;
    for (int32_t round = 0; round < maxit; ++round) {
        HIP_TRY(hipMemsetAsync(W.X.active, 0, sizeof(int32_t), st));
        rc = launch_posterior(p, W.E, st);
        if (rc) return rc;
        locus_marginal_reduce_kernel<<<dim3((unsigned)L), dim3(kEbReduceBlock), 0, st>>>(p->d_offsets.p, W.prep.dup_of, W.E.f, W.E.g,
                                                                                        W.E.h, W.X.done, W.X.sums);
        eb_scale_step_kernel<<<dim3((unsigned)((L + 63) / 64)), dim3(64), 0, st>>>(W.X, (int64_t)L, tol, maxit);
        HIP_TRY(hipGetLastError());
        int32_t active = 0;   // the round's convergence record
        HIP_TRY(hipMemcpyAsync(&active, W.X.active, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (active == 0) break;
    }
    std::vector<double> h_u(L), h_sums(3 * L);
    std::vector<int32_t> h_done(L), h_it(L);
    HIP_TRY(hipMemcpyAsync(h_u.data(), W.X.u, sizeof(double) * L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_sums.data(), W.X.sums, sizeof(double) * 3 * L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_done.data(), W.X.done, sizeof(int32_t) * L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_it.data(), W.X.iters, sizeof(int32_t) * L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t l = 0; l < L; ++l) {
        scale[l] = std::exp(h_u[l]);
        if (locus_lnl) locus_lnl[l] = h_sums[3 * l];
        if (curvature) curvature[l] = h_sums[3 * l + 2];
        if (iters) iters[l] = h_done[l] == 1 ? h_it[l] : -h_it[l];
    }
    return TPHIP_OK;
}

int tphip_eb_posterior_dev(tphip_plan* p, const uint8_t* d_states, const tphip_eb_opts* o, const double* cat_rate,
                           const double* cat_weight, const double* scale, double* d_rate, double* d_rate_sd, double* d_lnl,
                           int32_t* d_nres, void* stream) {
    int rc = eb_check(p, o, cat_rate, cat_weight, scale);
    if (rc) return rc;
    if (!d_states || !d_rate || !d_rate_sd || !d_lnl || !d_nres) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (p->nloci == 0 || p->n_pi_chunks <= 0) return TPHIP_OK;
    EbWorkspace W;
    rc = eb_setup(p, d_states, o, cat_rate, cat_weight, scale, st, W);
    if (rc) return rc;
    rc = launch_posterior(p, W.E, st);
    if (rc) return rc;
    eb_finish_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(p->d_offsets.p, p->d_pi_chunk_locus.p, p->d_pi_chunk_index.p,
                                                                          p->d_models.p, W.prep.dup_of, W.X.u, W.E.f, W.E.mean,
                                                                          W.E.second, d_rate, d_rate_sd, d_lnl);
    HIP_TRY(hipMemcpyAsync(d_nres, W.prep.nres, sizeof(int32_t) * (size_t)p->ncols, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

// tphip_eb_posterior_dev with the category posterior besides: the table variant of the mixture kernel
// leaves f_k + log w_k in d_post, eb_finish_kernel gives rate / sd / lnl as above, and the normalisation (a kernel of
// posterior_pi_driver.hip) turns d_post into p_ck in place, repeats copying their representatives.
int tphip_eb_posterior_table_dev(tphip_plan* p, const uint8_t* d_states, const tphip_eb_opts* o, const double* cat_rate,
                                 const double* cat_weight, const double* scale, double* d_post, double* d_rate, double* d_rate_sd,
                                 double* d_lnl, int32_t* d_nres, void* stream) {
    int rc = eb_check(p, o, cat_rate, cat_weight, scale);
    if (rc) return rc;
    if (!d_states || !d_post || !d_rate || !d_rate_sd || !d_lnl || !d_nres) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (p->nloci == 0 || p->n_pi_chunks <= 0) return TPHIP_OK;
    EbWorkspace W;
    rc = eb_setup(p, d_states, o, cat_rate, cat_weight, scale, st, W);
    if (rc) return rc;
    rc = launch_posterior_table(p, W.E, d_post, st);
    if (rc) return rc;
    eb_finish_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(p->d_offsets.p, p->d_pi_chunk_locus.p, p->d_pi_chunk_index.p,
                                                                          p->d_models.p, W.prep.dup_of, W.X.u, W.E.f, W.E.mean,
                                                                          W.E.second, d_rate, d_rate_sd, d_lnl);
    HIP_TRY(hipMemcpyAsync(d_nres, W.prep.nres, sizeof(int32_t) * (size_t)p->ncols, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    return tphip_internal_posterior_normalize(p, W.prep.dup_of, W.E.f, d_post, o->ncat, stream);
}

int tphip_eb_posterior_table(tphip_plan* p, const uint8_t* states, const tphip_eb_opts* o, const double* cat_rate,
                             const double* cat_weight, const double* scale, double* post, double* rate, double* rate_sd, double* lnl,
                             int32_t* nres) {
    int rc = eb_check(p, o, cat_rate, cat_weight, scale);
    if (rc) return rc;
    if (!states || !post || !rate || !rate_sd || !lnl || !nres) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    const size_t nc = (size_t)p->ncols, K = (size_t)o->ncat;
    Staging S;
    const uint8_t* d_s = S.in(states, nc * (size_t)p->ntaxa);
    double* d_p = S.out(post, K * nc);
    double* d_r = S.out(rate, nc);
    double* d_sd = S.out(rate_sd, nc);
    double* d_l = S.out(lnl, nc);
    int32_t* d_n = S.out(nres, nc);
    if (S.rc) return S.rc;
    rc = tphip_eb_posterior_table_dev(p, d_s, o, cat_rate, cat_weight, scale, d_p, d_r, d_sd, d_l, d_n, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return S.finish();
}

int tphip_eb_start_scale_dev(tphip_plan* p, const uint8_t* d_states, double* scale, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!d_states || !scale) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t L = (size_t)p->nloci;
    if (L == 0) return TPHIP_OK;
    EbWorkspace W;
    const size_t nw = (size_t)(p->nwords > 0 ? p->nwords : 1);
    const size_t need = eb_layout(nullptr, (size_t)p->ncols, L, 2, nw, W);
    if (const int rc = p->eb_ws.reserve(need)) return rc;
    eb_layout(p->eb_ws.p, (size_t)p->ncols, L, 2, nw, W);
    if (p->n_pi_chunks <= 0) {   // no column at all
        for (size_t l = 0; l < L; ++l) scale[l] = 1.0 / p->prog.chrono_length;
        return TPHIP_OK;
    }
    int rc = tphip_internal_eb_prepare(p, d_states, &W.prep, 0, W.X.u, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(scale, W.X.u, sizeof(double) * L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TPHIP_OK;
}

int tphip_eb_start_scale(tphip_plan* p, const uint8_t* states, double* scale) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (!states || !scale) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    const size_t n = (size_t)p->ncols * (size_t)p->ntaxa;
    uint8_t* d_s = S.get<uint8_t>(n);
    if (!d_s) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_s, states, n, hipMemcpyHostToDevice));
    int rc = tphip_eb_start_scale_dev(p, d_s, scale, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    return rc;
}

int tphip_eb_fit_scale(tphip_plan* p, const uint8_t* states, const tphip_eb_opts* o, const double* cat_rate, const double* cat_weight,
                       double* scale, double* locus_lnl, double* curvature, int32_t* iters) {
    int rc = eb_check(p, o, cat_rate, cat_weight, scale);
    if (rc) return rc;
    if (!states) return fail(TPHIP_ERR_INVALID, "null states");
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    const size_t n = (size_t)p->ncols * (size_t)p->ntaxa;
    uint8_t* d_s = S.get<uint8_t>(n);
    if (!d_s) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_s, states, n, hipMemcpyHostToDevice));
    rc = tphip_eb_fit_scale_dev(p, d_s, o, cat_rate, cat_weight, scale, locus_lnl, curvature, iters, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    return rc;
}

int tphip_eb_posterior(tphip_plan* p, const uint8_t* states, const tphip_eb_opts* o, const double* cat_rate, const double* cat_weight,
                       const double* scale, double* rate, double* rate_sd, double* lnl, int32_t* nres) {
    int rc = eb_check(p, o, cat_rate, cat_weight, scale);
    if (rc) return rc;
    if (!states || !rate || !rate_sd || !lnl || !nres) return fail(TPHIP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    Scratch S;
    const size_t nc = (size_t)p->ncols, n = nc * (size_t)p->ntaxa;
    uint8_t* d_s = S.get<uint8_t>(n);
    double* d_r = S.get<double>(nc);
    double* d_sd = S.get<double>(nc);
    double* d_l = S.get<double>(nc);
    int32_t* d_n = S.get<int32_t>(nc);
    if (!d_s || !d_r || !d_sd || !d_l || !d_n) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_s, states, n, hipMemcpyHostToDevice));
    rc = tphip_eb_posterior_dev(p, d_s, o, cat_rate, cat_weight, scale, d_r, d_sd, d_l, d_n, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(rate, d_r, sizeof(double) * nc, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rate_sd, d_sd, sizeof(double) * nc, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lnl, d_l, sizeof(double) * nc, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nres, d_n, sizeof(int32_t) * nc, hipMemcpyDeviceToHost));
    return TPHIP_OK;
}

}  // extern "C"

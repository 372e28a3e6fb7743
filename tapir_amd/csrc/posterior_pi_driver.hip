// posterior_pi_driver.hip -- the empirical-Bayes rate posterior carried into the per-locus PI rows:
// the C entry points tphip_posterior_pi / tphip_posterior_pi_workspace_bytes and the launch that turns the mixture kernel's
// f_k + log w_k into the category posterior for tphip_eb_posterior_table (eb_driver.hip).  The kernels are in
// posterior_pi_kernels.hpp, the blocking of loci over the caller's workspace in band_blocks.hpp; this unit is built with the
// compiler's defaults.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "band_driver_common.hpp"
#include "posterior_pi_kernels.hpp"

namespace {

constexpr int64_t kPpTargetGroups = 1024;   // workgroups a draw launch aims at before it cuts loci into segments
constexpr int64_t kPpMaxSegCols = 0x40000000;   // columns of a segment at most (2^30: seg_cols is an int32)
constexpr BandOptsRules kPpOptsRules{sizeof(tphip_posterior_pi_opts), sizeof(tphip_posterior_pi_opts), "null tphip_posterior_pi_opts",
                                     "tphip_posterior_pi_opts.struct_size is smaller than this library's struct",
                                     "posterior replicates must be in 2..4096", "posterior level must be in (0, 1)"};

// the shared fields, then K = ncat
int pp_read_opts(const tphip_posterior_pi_opts* opts, BandOpts* o, int32_t* K) {
    int rc = band_read_opts(opts, kPpOptsRules, o);
    if (rc) return rc;
    *K = opts->ncat;
    if (*K < 2 || *K > kPpMaxCat) return fail(TPHIP_ERR_INVALID, "tphip_posterior_pi_opts.ncat must be in 2..16");
    return TPHIP_OK;
}

inline size_t pp_width(const tphip_plan* p) { return (size_t)(p->T + p->n_i); }
inline BandBytes pp_workspace(const tphip_plan* p, const BandOpts& o, int32_t K) {
    return posterior_bytes(p->nloci, (size_t)K, (size_t)o.replicates, pp_width(p));
}

}  // namespace

extern "C" {

// logp (f_k + log w_k of the representatives, [K][ncols]) -> the category posterior, in place; for eb_driver.hip
int tphip_internal_posterior_normalize(tphip_plan* p, const int32_t* d_dup_of, const double* d_f, double* d_post, int32_t K,
                                       void* stream) {
    if (p->n_pi_chunks <= 0) return TPHIP_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int pass = 0; pass < 2; ++pass)
        posterior_normalize_kernel<<<dim3((unsigned)p->n_pi_chunks), dim3(256), 0, st>>>(p->d_offsets.p, p->d_pi_chunk_locus.p,
                                                                                        p->d_pi_chunk_index.p, d_dup_of, d_f, d_post,
                                                                                        K, p->ncols, pass);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int tphip_posterior_pi_workspace_bytes(const tphip_plan* p, const tphip_posterior_pi_opts* opts, size_t* min_bytes,
                                       size_t* preferred_bytes) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int32_t K = 0;
    int rc = pp_read_opts(opts, &o, &K);
    if (rc) return rc;
    const BandBytes W = pp_workspace(p, o, K);
    if (min_bytes) *min_bytes = W.min;
    if (preferred_bytes) *preferred_bytes = W.preferred;
    return TPHIP_OK;
}

int tphip_posterior_pi_dev(tphip_plan* p, const double* d_post, const int32_t* d_nres, const double* d_scale, const double* d_cat_rate,
                           const tphip_posterior_pi_opts* opts, double* d_analytic, double* d_expected_counts, double* d_summary,
                           double* d_rows, int32_t* d_counts, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int32_t K = 0;
    int rc = pp_read_opts(opts, &o, &K);
    if (rc) return rc;
    const size_t Wb = pp_width(p), L = (size_t)p->nloci;
    const int32_t B = o.replicates;
    if (L == 0 || Wb == 0) return TPHIP_OK;
    if (!d_analytic || !d_expected_counts || !d_summary || !d_scale || !d_cat_rate || !ws || (p->ncols && !d_post))
        return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ws_bytes < pp_workspace(p, o, K).min)
        return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than the minimum of tphip_posterior_pi_workspace_bytes()");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    size_t usable = 0;
    char* base = band_ws_base(ws, ws_bytes, &usable);
    const int64_t* d_ids = nullptr;
    rc = band_stage_ids((int64_t*)base, o.locus_ids, p->nloci, st, &d_ids);
    if (rc) return rc;
    base += band_ids_bytes(p->nloci);
    usable -= band_ids_bytes(p->nloci);
    const size_t nb = posterior_block_loci(L, (size_t)K, (size_t)B, Wb, usable);   // at least one: ws_bytes >= the minimum
    PostPiParams Q{};
    Q.pi = plan_pi_params(p, nullptr, d_nres);
    Q.models = p->d_models.p; Q.scale = d_scale; Q.cat_rate = d_cat_rate; Q.post = d_post; Q.ncols_total = p->ncols;
    Q.K = K; Q.B = B; Q.analytic = d_analytic; Q.expected = d_expected_counts;
    PostDrawParams D{};
    D.locus_offsets = p->d_offsets.p; D.locus_ids = d_ids; D.nres = d_nres; D.threshold = p->threshold; D.post = d_post;
    D.ncols_total = p->ncols; D.K = K; D.B = B; D.seed = o.seed;
    const unsigned draw_block = (unsigned)std::min(kPpBlock, (B + 63) / 64 * 64);
    const int64_t rep_tiles = (B + draw_block - 1) / draw_block;
    for (size_t l0 = 0; l0 < L; l0 += nb) {
        const size_t n = std::min(nb, L - l0);
        double* ptab = (double*)base;
        int32_t* ws_counts = (int32_t*)(base + pp_ptab_bytes(n, (size_t)K, Wb));
        double* ws_rows = (double*)(base + pp_ptab_bytes(n, (size_t)K, Wb) + pp_counts_bytes(n, (size_t)B, (size_t)K));
        int32_t* counts = d_counts ? d_counts + l0 * (size_t)B * K : ws_counts;
        double* rows = d_rows ? d_rows + l0 * (size_t)B * Wb : ws_rows;
        Q.locus0 = (int32_t)l0; Q.ptab = ptab; Q.counts = counts; Q.rows = rows;
        posterior_category_rows_kernel<<<dim3((unsigned)n), dim3(kPpBlock), 0, st>>>(Q);
        posterior_moments_kernel<<<dim3((unsigned)n, (unsigned)((Wb + kPpWTile - 1) / kPpWTile)), dim3(kPpBlock), 0, st>>>(Q);
        HIP_TRY(hipGetLastError());
        int64_t max_cols = 0;
        for (size_t l = l0; l < l0 + n; ++l) max_cols = std::max(max_cols, p->h_offsets[l + 1] - p->h_offsets[l]);
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t) * n * (size_t)B * K, st));
        if (max_cols > 0) {
            // a long locus with few replicates is cut into column segments: whole staging tiles, integer partial counts
            const int64_t tiles = (max_cols + kPpTile - 1) / kPpTile;
            const int64_t groups = (int64_t)n * rep_tiles;
            const int64_t segs = std::min(tiles, std::max<int64_t>(1, (kPpTargetGroups + groups - 1) / groups));
            const int64_t seg_tiles = (tiles + segs - 1) / segs;
            D.seg_cols = (int32_t)std::min<int64_t>(seg_tiles * kPpTile, kPpMaxSegCols);
            const int64_t gz = (max_cols + D.seg_cols - 1) / D.seg_cols;
            if (gz > 65535) return fail(TPHIP_ERR_INVALID, "locus too long for one posterior draw launch");
            D.locus0 = (int32_t)l0; D.counts = counts;
            const dim3 grid((unsigned)rep_tiles, (unsigned)n, (unsigned)gz), block(draw_block);
            if (K <= 2) posterior_draw_kernel<2><<<grid, block, 0, st>>>(D);
            else if (K <= 4) posterior_draw_kernel<4><<<grid, block, 0, st>>>(D);
            else if (K <= 8) posterior_draw_kernel<8><<<grid, block, 0, st>>>(D);
            else posterior_draw_kernel<16><<<grid, block, 0, st>>>(D);
            HIP_TRY(hipGetLastError());
        }
        const int64_t entries = (int64_t)B * (int64_t)Wb;
        posterior_rows_kernel<<<dim3((unsigned)n, (unsigned)((entries + kPpBlock - 1) / kPpBlock)), dim3(kPpBlock), 0, st>>>(Q);
        HIP_TRY(hipGetLastError());
        rc = band_summarize(rows, (int64_t)n, B, (int32_t)Wb, o.level, d_summary + l0 * 4 * Wb, st);
        if (rc) return rc;
    }
    return TPHIP_OK;
}

int tphip_posterior_pi(tphip_plan* p, const double* post, const int32_t* nres, const double* scale, const double* cat_rate,
                       const tphip_posterior_pi_opts* opts, double* analytic, double* expected_counts, double* summary, double* rows,
                       int32_t* counts) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int32_t ncat = 0;
    int rc = pp_read_opts(opts, &o, &ncat);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, Wb = pp_width(p), L = (size_t)p->nloci, B = (size_t)o.replicates, K = (size_t)ncat;
    if (L * Wb == 0) return TPHIP_OK;
    if (!analytic || !expected_counts || !summary || !scale || !cat_rate || (n && !post)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t pf = pp_workspace(p, o, ncat).preferred;
    Staging S;
    const double* d_post = S.in(post, K * n);
    const int32_t* d_nres = S.in(nres, n);
    const double* d_scale = S.in(scale, L);
    const double* d_cat = S.in(cat_rate, L * K);
    double* d_an = S.out(analytic, L * 2 * Wb);
    double* d_ex = S.out(expected_counts, L * K);
    double* d_sum = S.out(summary, L * 4 * Wb);
    double* d_rows = S.out(rows, L * B * Wb);
    int32_t* d_counts = S.out(counts, L * B * K);
    char* ws = S.scratch<char>(pf);
    if (S.rc) return S.rc;
    rc = tphip_posterior_pi_dev(p, d_post, d_nres, d_scale, d_cat, opts, d_an, d_ex, d_sum, d_rows, d_counts, ws, pf, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

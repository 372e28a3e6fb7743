// bootstrap_driver.hip -- site bootstrap of the per-locus PI rows: the C entry points
// tphip_pi_resample / tphip_pi_bootstrap / tphip_bootstrap_counts and the summary launch of every band stage.  The kernels are
// in bootstrap_kernels.hpp; how loci and replicate ranges are blocked over the caller's workspace is in band_blocks.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "band_driver_common.hpp"
#include "bootstrap_kernels.hpp"

namespace {

constexpr int32_t kBsMaxResampleReps = 1 << 20;
constexpr BandOptsRules kBsOptsRules{band_seed_end<tphip_bootstrap_opts>(), band_ids_end<tphip_bootstrap_opts>(), "null tphip_bootstrap_opts",
                                     "tphip_bootstrap_opts.struct_size is too small: set it to sizeof(tphip_bootstrap_opts)",
                                     "bootstrap replicates must be in 2..4096", "bootstrap level must be in (0, 1)"};

inline int32_t bs_width(const tphip_plan* p) { return p->T + p->n_i; }
inline BandBytes bs_workspace(const tphip_plan* p, int64_t B) {
    return bootstrap_bytes(p->h_offsets.data(), p->nloci, p->n_i, bs_width(p), B, kBsRepTile);
}

// numpy.quantile's default rule for n sorted values: virtual index n q + (1 + q (1 - 1 - 1)) - 1 evaluated as numpy does,
// lower neighbour = its floor, weight of the upper neighbour = the fractional part
void bs_quantile_index(int32_t n, double q, int32_t* idx, double* frac) {
    volatile double nq = (double)n * q;
    volatile double inner = 1.0 + q * -1.0;
    volatile double sum = nq + inner;
    const double vi = sum - 1.0;
    double fl = std::floor(vi);
    if (fl < 0.0) { *idx = 0; *frac = 0.0; return; }
    if (vi >= (double)(n - 1)) { *idx = n - 1; *frac = 0.0; return; }
    *idx = (int32_t)fl;
    *frac = vi - fl;
}

// integrals of the columns [c0, c1) into `integ`
int bs_launch_integrals(const tphip_plan* p, const PiParams& Q, int64_t c0, int64_t c1, double* integ, hipStream_t st) {
    if (c1 > c0 && p->n_i > 0) {
        bootstrap_integrals_kernel<<<dim3((unsigned)((c1 - c0 + 127) / 128)), dim3(128), 0, st>>>(Q, c0, c1 - c0, integ);
        HIP_TRY(hipGetLastError());
    }
    return TPHIP_OK;
}

// rows of the loci [l0, l1) for `nrep` replicates whose counts are counts[r * pitch + (column - col_base)]
int bs_launch_matrix(const tphip_plan* p, const PiParams& Q, int64_t l0, int64_t l1, const uint16_t* counts, int64_t pitch,
                     int64_t col_base, const double* integ, int64_t integ_col_base, double* rows, int64_t rows_reps,
                     int64_t rows_rep0, int32_t nrep, hipStream_t st) {
    const int32_t Wb = bs_width(p);
    if (l1 <= l0 || nrep <= 0 || Wb <= 0) return TPHIP_OK;
    BootMatParams M;
    M.pi = Q; M.counts = counts; M.count_pitch = pitch; M.col_base = col_base;
    M.integ = integ; M.integ_col_base = integ_col_base;
    M.rows = rows; M.rows_reps = rows_reps; M.rows_rep0 = rows_rep0;
    M.locus0 = (int32_t)l0; M.nrep = nrep; M.Tp = (p->T + 15) & ~15;
    const int Wi = M.Tp + p->n_i;
    bootstrap_matrix_kernel<<<dim3((unsigned)(l1 - l0), (unsigned)((nrep + kBsRepTile - 1) / kBsRepTile),
                                   (unsigned)((Wi + kBsOutTile - 1) / kBsOutTile)), dim3(kBsBlock), 0, st>>>(M);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

int bs_launch_draw(const int64_t* d_offsets, const int64_t* d_ids, int64_t single_n, int64_t single_id, int64_t l0, int64_t l1,
                   int64_t max_cols, int64_t rep0, int32_t nrep, uint64_t seed, uint16_t* counts, int64_t pitch,
                   int64_t col_base, hipStream_t st) {
    if (l1 <= l0 || nrep <= 0 || max_cols <= 0) return TPHIP_OK;
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(uint16_t) * (size_t)pitch * (size_t)nrep, st));
    DrawParams D;
    D.locus_offsets = d_offsets; D.locus_ids = d_ids; D.single_n = single_n; D.single_id = single_id;
    D.locus0 = (int32_t)l0; D.nrep = nrep; D.rep0 = rep0; D.seed = seed;
    D.words = (uint32_t*)counts; D.pitch = pitch; D.col_base = col_base;
    const int64_t calls = (max_cols + 1) / 2;
    const int64_t gx = (l1 - l0) * (int64_t)nrep, gy = (calls + kBsDrawBlock - 1) / kBsDrawBlock;
    if (gx > 0x7fffffffll || gy > 65535) return fail(TPHIP_ERR_INVALID, "bootstrap block too large for one launch");
    bootstrap_draw_kernel<<<dim3((unsigned)gx, (unsigned)gy), dim3(kBsDrawBlock), 0, st>>>(D);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

}  // namespace

int band_summarize(const double* d_rows, int64_t nloci, int32_t B, int32_t Wb, double level, double* d_summary, hipStream_t st) {
    if (nloci == 0 || Wb == 0) return TPHIP_OK;
    if (nloci * (int64_t)Wb > 0x7fffffffll) return fail(TPHIP_ERR_INVALID, "nloci * Wb beyond 2^31 - 1 entries");
    SummaryParams S;
    S.rows = d_rows; S.summary = d_summary;
    S.B = B; S.Wb = Wb;
    S.npow2 = 2;
    while (S.npow2 < B) S.npow2 <<= 1;
    const double q_lo = (1.0 - level) / 2.0, q_hi = 1.0 - (1.0 - level) / 2.0;
    bs_quantile_index(B, q_lo, &S.idx_lo, &S.frac_lo);
    bs_quantile_index(B, q_hi, &S.idx_hi, &S.frac_hi);
    bootstrap_summary_kernel<<<dim3((unsigned)(nloci * Wb)), dim3(256), 0, st>>>(S);
    HIP_TRY(hipGetLastError());
    return TPHIP_OK;
}

extern "C" {

int32_t tphip_bootstrap_width(const tphip_plan* p) { return p ? bs_width(p) : 0; }

int tphip_bootstrap_workspace_bytes(const tphip_plan* p, const tphip_bootstrap_opts* opts, size_t* min_bytes, size_t* preferred_bytes) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandBytes W = resample_bytes(p->max_locus_cols, p->ncols, p->n_i);   // no opts: tphip_pi_resample_dev, whatever nrep
    if (opts) {
        BandOpts o;
        int rc = band_read_opts(opts, kBsOptsRules, &o);
        if (rc) return rc;
        W = bs_workspace(p, o.replicates);
    }
    if (min_bytes) *min_bytes = W.min;
    if (preferred_bytes) *preferred_bytes = W.preferred;
    return TPHIP_OK;
}

int tphip_pi_resample_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const uint16_t* d_counts, int32_t nrep,
                          double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (nrep < 1 || nrep > kBsMaxResampleReps) return fail(TPHIP_ERR_INVALID, "nrep must be in 1..2^20");
    const int32_t Wb = bs_width(p);
    if (p->nloci == 0 || Wb == 0) return TPHIP_OK;
    if (!d_rows || (p->ncols && (!d_rates || !d_counts))) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    size_t usable = 0;
    char* base = ws ? band_ws_base(ws, ws_bytes, &usable) : nullptr;
    const PiParams Q = plan_pi_params(p, d_rates, d_nres);
    int64_t l0 = 0;
    while (l0 < p->nloci) {
        const int64_t l1 = resample_next_block(p->h_offsets.data(), p->nloci, l0, p->n_i, usable);
        const int64_t c0 = p->h_offsets[l0], c1 = p->h_offsets[l1];
        if (p->n_i > 0 && c1 > c0 && (!base || bs_integ_bytes(c1 - c0, p->n_i) > usable))
            return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than the minimum of tphip_bootstrap_workspace_bytes()");
        int rc = bs_launch_integrals(p, Q, c0, c1, (double*)base, st);
        if (rc) return rc;
        rc = bs_launch_matrix(p, Q, l0, l1, d_counts, p->ncols, 0, (const double*)base, c0,
                              d_rows + (size_t)l0 * (size_t)nrep * (size_t)Wb, nrep, 0, nrep, st);
        if (rc) return rc;
        l0 = l1;
    }
    return TPHIP_OK;
}

int tphip_pi_bootstrap_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_bootstrap_opts* opts,
                           double* d_summary, double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int rc = band_read_opts(opts, kBsOptsRules, &o);
    if (rc) return rc;
    const int32_t Wb = bs_width(p), B = o.replicates;
    if (p->nloci == 0 || Wb == 0) return TPHIP_OK;
    if (!d_summary || !ws || (p->ncols && !d_rates)) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (ws_bytes < bs_workspace(p, B).min)
        return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than the minimum of tphip_bootstrap_workspace_bytes()");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    size_t usable = 0;
    char* base = band_ws_base(ws, ws_bytes, &usable);
    const int64_t* d_ids = nullptr;
    rc = band_stage_ids((int64_t*)base, o.locus_ids, p->nloci, st, &d_ids);
    if (rc) return rc;
    base += band_ids_bytes(p->nloci);
    usable -= band_ids_bytes(p->nloci);
    const PiParams Q = plan_pi_params(p, d_rates, d_nres);
    int64_t l0 = 0;
    while (l0 < p->nloci) {
        const BsBlock blk = bootstrap_next_block(p->h_offsets.data(), p->nloci, l0, p->n_i, Wb, B, kBsRepTile, usable);
        const int64_t l1 = blk.l1, range = blk.range;
        const int64_t c0 = p->h_offsets[l0], c1 = p->h_offsets[l1], n = c1 - c0;
        int64_t max_cols = 0;
        for (int64_t l = l0; l < l1; ++l) max_cols = std::max(max_cols, p->h_offsets[l + 1] - p->h_offsets[l]);
        double* integ = (double*)base;
        uint16_t* counts = (uint16_t*)(base + bs_integ_bytes(n, p->n_i));
        double* ws_rows = (double*)(base + bs_integ_bytes(n, p->n_i) + bs_counts_bytes(n, range));
        double* rows = d_rows ? d_rows + (size_t)l0 * (size_t)B * (size_t)Wb : ws_rows;
        rc = bs_launch_integrals(p, Q, c0, c1, integ, st);
        if (rc) return rc;
        for (int64_t r0 = 0; r0 < B; r0 += range) {
            const int32_t nr = (int32_t)std::min<int64_t>(range, B - r0);
            rc = bs_launch_draw(p->d_offsets.p, d_ids, 0, 0, l0, l1, max_cols, r0, nr, o.seed, counts, (int64_t)bs_pitch(n), c0, st);
            if (rc) return rc;
            rc = bs_launch_matrix(p, Q, l0, l1, counts, (int64_t)bs_pitch(n), c0, integ, c0, rows, B, r0, nr, st);
            if (rc) return rc;
        }
        rc = band_summarize(rows, l1 - l0, B, Wb, o.level, d_summary + (size_t)l0 * 4 * (size_t)Wb, st);
        if (rc) return rc;
        l0 = l1;
    }
    return TPHIP_OK;
}

int tphip_pi_resample(tphip_plan* p, const double* rates, const int32_t* nres, const uint16_t* counts, int32_t nrep, double* rows) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    if (nrep < 1 || nrep > kBsMaxResampleReps) return fail(TPHIP_ERR_INVALID, "nrep must be in 1..2^20");
    const size_t n = (size_t)p->ncols, Wb = (size_t)bs_width(p), nrows = (size_t)p->nloci * (size_t)nrep * Wb;
    if (nrows == 0) return TPHIP_OK;
    if (!rows || (n && (!rates || !counts))) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    Staging S;
    const double* d_r = S.in(rates, n);
    const int32_t* d_n = S.in(nres, n);
    const uint16_t* d_c = S.in(counts, n * (size_t)nrep);
    double* d_rows = S.out(rows, nrows);
    const size_t ws_bytes = resample_bytes(p->max_locus_cols, p->ncols, p->n_i).preferred;
    char* ws = S.scratch<char>(ws_bytes);
    if (S.rc) return S.rc;
    int rc = tphip_pi_resample_dev(p, d_r, d_n, d_c, nrep, d_rows, ws, ws_bytes, nullptr);
    return rc ? rc : S.finish();
}

int tphip_pi_bootstrap(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_bootstrap_opts* opts, double* summary,
                       double* rows) {
    if (!p) return fail(TPHIP_ERR_INVALID, "null plan");
    BandOpts o;
    int rc = band_read_opts(opts, kBsOptsRules, &o);
    if (rc) return rc;
    const size_t n = (size_t)p->ncols, Wb = (size_t)bs_width(p), L = (size_t)p->nloci, B = (size_t)o.replicates;
    if (L * Wb == 0) return TPHIP_OK;
    if (!summary || (n && !rates)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t pf = bs_workspace(p, o.replicates).preferred;
    Staging S;
    const double* d_r = S.in(rates, n);
    const int32_t* d_n = S.in(nres, n);
    double* d_sum = S.out(summary, L * 4 * Wb);
    double* d_rows = S.out(rows, L * B * Wb);
    char* ws = S.scratch<char>(pf);
    if (S.rc) return S.rc;
    rc = tphip_pi_bootstrap_dev(p, d_r, d_n, opts, d_sum, d_rows, ws, pf, nullptr);
    return rc ? rc : S.finish();
}

int tphip_bootstrap_counts(int32_t device, uint64_t seed, int64_t locus_id, int64_t n, int64_t rep0, int32_t nrep, uint16_t* counts_out) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (n < 0 || nrep < 0 || rep0 < 0 || rep0 + nrep > ((int64_t)1 << 32)) return fail(TPHIP_ERR_INVALID, "bad arguments");
    if (n == 0 || nrep == 0) return TPHIP_OK;
    if (!counts_out) return fail(TPHIP_ERR_INVALID, "null host pointer");
    if ((double)n * (double)nrep > 2147483648.0) return fail(TPHIP_ERR_INVALID, "n * nrep beyond 2^31 counts");
    HIP_TRY(hipSetDevice(device));
    Scratch S;
    const size_t pitch = bs_pitch(n);
    uint16_t* d_c = S.get<uint16_t>(pitch * (size_t)nrep);
    if (!d_c) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    int rc = bs_launch_draw(nullptr, nullptr, n, locus_id, 0, 1, n, rep0, nrep, seed, d_c, (int64_t)pitch, 0, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2D(counts_out, sizeof(uint16_t) * (size_t)n, d_c, sizeof(uint16_t) * pitch, sizeof(uint16_t) * (size_t)n,
                        (size_t)nrep, hipMemcpyDeviceToHost));
    return TPHIP_OK;
}

// The summary kernel on any [L][B][Wb] rows
int tphip_summarize_rows_dev(int32_t device, const double* d_rows, int64_t nloci, int32_t B, int32_t Wb, double level,
                             double* d_summary, void* stream) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (B < 2 || B > kBandMaxReplicates) return fail(TPHIP_ERR_INVALID, "replicates must be in 2..4096");
    if (!(level > 0.0 && level < 1.0)) return fail(TPHIP_ERR_INVALID, "level must be in (0, 1)");
    if (nloci < 0 || Wb < 0) return fail(TPHIP_ERR_INVALID, "negative size");
    if (nloci == 0 || Wb == 0) return TPHIP_OK;
    if (!d_rows || !d_summary) return fail(TPHIP_ERR_INVALID, "null device pointer");
    HIP_TRY(hipSetDevice(device));
    return band_summarize(d_rows, nloci, B, Wb, level, d_summary, (hipStream_t)stream);
}

int tphip_summarize_rows(int32_t device, const double* rows, int64_t nloci, int32_t B, int32_t Wb, double level, double* summary) {
    if (nloci < 0 || Wb < 0 || B < 0) return fail(TPHIP_ERR_INVALID, "negative size");
    const size_t nrows = (size_t)nloci * (size_t)B * (size_t)Wb, nsum = (size_t)nloci * 4 * (size_t)Wb;
    if (nsum && (!rows || !summary)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    Staging S;
    const double* d_rows = S.in(rows, nrows);
    double* d_sum = S.out(summary, nsum);
    if (S.rc) return S.rc;
    int rc = tphip_summarize_rows_dev(device, d_rows, nloci, B, Wb, level, d_sum, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

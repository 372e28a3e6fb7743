// quartet_driver.hip -- quartet signal and noise probabilities for per-locus site rates: the C entry
// points tphip_quartet_tables / tphip_quartet_sites (+ _dev) and tphip_quartet_workspace_bytes.  The kernels are in
// quartet_kernels.hpp, the entry points' bodies in quartet_driver_common.hpp: this unit is the family's traits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "quartet_kernels.hpp"
#include "quartet_driver_common.hpp"

namespace {

constexpr int32_t kQtMaxQuartets = 256;

struct EqualTips {
    using Opts = tphip_quartet_opts;
    using Params = QuartetParams;
    using Batch = QuartetBatch;
    static constexpr int kBatch = kQtBatch, kBlock = kQtBlock, kReduceBlock = kQtReduceBlock;
    static constexpr int kSums = kQtSums, kRow = kQtRow, kPlanes = 2;
    static constexpr auto partial_kernel = quartet_partial_kernel;
    static constexpr auto sites_kernel = quartet_sites_kernel;
    static constexpr auto reduce_kernel = quartet_reduce_kernel;

    static int read_opts(const Opts* o, int32_t* n_q) {
        if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_quartet_opts");
        if (o->struct_size < offsetof(tphip_quartet_opts, internode) + sizeof(const double*))
            return fail(TPHIP_ERR_INVALID, "tphip_quartet_opts.struct_size is too small: set it to sizeof(tphip_quartet_opts)");
        if (o->n_q < 1 || o->n_q > kQtMaxQuartets) return fail(TPHIP_ERR_INVALID, "n_q must be in 1..256");
        if (!o->tip || !o->internode) return fail(TPHIP_ERR_INVALID, "null quartet lengths");
        for (int32_t q = 0; q < o->n_q; ++q) {
            if (!(o->tip[q] >= 0.0) || !std::isfinite(o->tip[q]))
                return fail(TPHIP_ERR_INVALID, "quartet " + std::to_string(q) + ": the tip length T must be finite and >= 0");
            if (!(o->internode[q] > 0.0) || !std::isfinite(o->internode[q]))
                return fail(TPHIP_ERR_INVALID, "quartet " + std::to_string(q) + ": the internode length t_o must be finite and > 0");
        }
        *n_q = o->n_q;
        return TPHIP_OK;
    }

    static void fill_batch(Batch& B, const Opts* o, int32_t q0, int32_t nq) {
        for (int32_t k = 0; k < kBatch; ++k) {
            B.tip[k] = k < nq ? o->tip[q0 + k] : 0.0;
            B.internode[k] = k < nq ? o->internode[q0 + k] : 0.0;
        }
    }

    static int workspace_too_small() { return fail(TPHIP_ERR_WORKSPACE, "workspace smaller than tphip_quartet_workspace_bytes()"); }
};

}  // namespace

extern "C" {

int tphip_quartet_workspace_bytes(const tphip_plan* p, const tphip_quartet_opts* opts, size_t* bytes) {
    return quartet_workspace_bytes<EqualTips>(p, opts, bytes);
}

int tphip_quartet_tables_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_quartet_opts* opts,
                             double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    return quartet_tables_dev<EqualTips>(p, d_rates, d_nres, opts, d_rows, ws, ws_bytes, stream);
}

int tphip_quartet_sites_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_quartet_opts* opts,
                            double* d_sites, void* stream) {
    return quartet_sites_dev<EqualTips>(p, d_rates, d_nres, opts, d_sites, stream);
}

int tphip_quartet_tables(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_quartet_opts* opts, double* rows) {
    return quartet_tables<EqualTips>(p, rates, nres, opts, rows);
}

int tphip_quartet_sites(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_quartet_opts* opts, double* sites) {
    return quartet_sites<EqualTips>(p, rates, nres, opts, sites);
}

}  // extern "C"

// unequal_quartet_driver.hip -- signal and noise of quartets with four unequal tip branches: the C entry
// points tphip_unequal_quartet_tables / tphip_unequal_quartet_sites (+ _dev) and tphip_unequal_quartet_workspace_bytes.  The
// kernels are in unequal_quartet_kernels.hpp, the entry points' bodies in quartet_driver_common.hpp: this unit is the family's
// traits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "unequal_quartet_kernels.hpp"
#include "quartet_driver_common.hpp"

namespace {

constexpr int32_t kUqMaxQuartets = 256;

struct UnequalTips {
    using Opts = tphip_unequal_quartet_opts;
    using Params = UnequalQuartetParams;
    using Batch = UnequalQuartetBatch;
    static constexpr int kBatch = kUqBatch, kBlock = kUqBlock, kReduceBlock = kUqReduceBlock;
    static constexpr int kSums = kUqSums, kRow = kUqRow, kPlanes = 3;
    static constexpr auto partial_kernel = uquartet_partial_kernel;
    static constexpr auto sites_kernel = uquartet_sites_kernel;
    static constexpr auto reduce_kernel = uquartet_reduce_kernel;

    static int read_opts(const Opts* o, int32_t* n_q) {
        if (!o) return fail(TPHIP_ERR_INVALID, "null tphip_unequal_quartet_opts");
        if (o->struct_size < offsetof(tphip_unequal_quartet_opts, internode) + sizeof(const double*))
            return fail(TPHIP_ERR_INVALID, "tphip_unequal_quartet_opts.struct_size is too small: set it to sizeof(tphip_unequal_quartet_opts)");
        if (o->n_q < 1 || o->n_q > kUqMaxQuartets) return fail(TPHIP_ERR_INVALID, "n_q must be in 1..256");
        if (!o->tips || !o->internode) return fail(TPHIP_ERR_INVALID, "null quartet lengths (tips, internode)");
        static const char* const kTip[4] = {"Ta", "Tb", "Tc", "Td"};
        for (int32_t q = 0; q < o->n_q; ++q) {
            for (int t = 0; t < 4; ++t) {
                const double v = o->tips[4 * (size_t)q + t];
                if (!(v >= 0.0) || !std::isfinite(v))
                    return fail(TPHIP_ERR_INVALID, "quartet " + std::to_string(q) + ": the tip length " + kTip[t] + " (tips) must be finite and >= 0");
            }
            if (!(o->internode[q] > 0.0) || !std::isfinite(o->internode[q]))
                return fail(TPHIP_ERR_INVALID, "quartet " + std::to_string(q) + ": the internode length t_o (internode) must be finite and > 0");
        }
        *n_q = o->n_q;
        return TPHIP_OK;
    }

    static void fill_batch(Batch& B, const Opts* o, int32_t q0, int32_t nq) {
        for (int32_t k = 0; k < kBatch; ++k) {
            for (int t = 0; t < 4; ++t) B.tip[t][k] = k < nq ? o->tips[4 * (size_t)(q0 + k) + t] : 0.0;
            B.internode[k] = k < nq ? o->internode[q0 + k] : 0.0;
        }
    }

    static int workspace_too_small() {
        return fail(TPHIP_ERR_INVALID, "ws_bytes: workspace smaller than tphip_unequal_quartet_workspace_bytes()");
    }
};

}  // namespace

extern "C" {

int tphip_unequal_quartet_workspace_bytes(const tphip_plan* p, const tphip_unequal_quartet_opts* opts, size_t* bytes) {
    return quartet_workspace_bytes<UnequalTips>(p, opts, bytes);
}

int tphip_unequal_quartet_tables_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_unequal_quartet_opts* opts,
                                     double* d_rows, void* ws, size_t ws_bytes, void* stream) {
    return quartet_tables_dev<UnequalTips>(p, d_rates, d_nres, opts, d_rows, ws, ws_bytes, stream);
}

int tphip_unequal_quartet_sites_dev(tphip_plan* p, const double* d_rates, const int32_t* d_nres, const tphip_unequal_quartet_opts* opts,
                                    double* d_sites, void* stream) {
    return quartet_sites_dev<UnequalTips>(p, d_rates, d_nres, opts, d_sites, stream);
}

int tphip_unequal_quartet_tables(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_unequal_quartet_opts* opts, double* rows) {
    return quartet_tables<UnequalTips>(p, rates, nres, opts, rows);
}

int tphip_unequal_quartet_sites(tphip_plan* p, const double* rates, const int32_t* nres, const tphip_unequal_quartet_opts* opts, double* sites) {
    return quartet_sites<UnequalTips>(p, rates, nres, opts, sites);
}

}  // extern "C"

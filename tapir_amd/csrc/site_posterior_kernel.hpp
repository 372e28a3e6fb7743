// site_posterior_kernel.hpp -- empirical-Bayes site rates: the discrete-gamma mixture over a locus-wide
// scale, evaluated per column with the posterior moments of the rate category.
//
// Model: site rate s = mu rho, rho in K equiprobable gamma categories (rho_k, w_k from the host), mu the locus' scale.
// Per column c the kernel walks the K categories through evaluate_column (site_rate_kernel.hpp: the same tree-program
// interpreter, tip tables, rescaling and LDS stack the ML kernel uses) and keeps, in one running log-sum-exp scale,
//   z = sum w_k L_k,  a = sum w_k L_k g_k,  b = sum w_k L_k (h_k + g_k^2),  m1 = sum w_k L_k rho_k,  m2 = sum w_k L_k rho_k^2
// so that f = log m_c, g and h (derivatives in u = log mu: d/du of L(mu rho_k) is the category's own g_k, because
// log(mu rho_k) = u + log rho_k) and the posterior mean and second moment of rho come out of one pass.  The [ncols][K]
// likelihood table is never materialised.
//
// The kernels are further overloads of eval_columns_kernel on their parameter type and live in site_rate_launch.hip, the
// unit built with -structurizecfg-skip-uniform-regions: the streamed-words path of evaluate_column keeps a hand-issued
// global load in flight in one register, and without the switch the structurizer's Flow blocks copy that register
// before the load has landed (profiles/r05_eb_resource_usage.txt).
//
// Mapping: one column per lane, one wavefront per workgroup, all of one locus (the model, the category table and mu are
// wave-uniform).  The column's packed tip words are loaded once, before the category loop, and stay in registers for
// all K evaluations (up to 64 tips; beyond, word 0 stays and the others are streamed from L2 as in site_rate_kernel).
// Work: the site chunk tables cut a locus' work list (all columns, or the representatives of its site patterns) into
// slices; there is no lane refill because every lane does exactly K evaluations.
// A category whose log(mu rho_k) is below kUMin is evaluated at kUMin (the likelihood is flat to fp64 there).
#pragma once
#include "site_rate_kernel.hpp"
#include "site_posterior_params.hpp"

namespace tphip {

// TABLE = true is the posterior-table variant: besides the moments it stores every category's
// f_k + log w_k at logp[k * ncols_total + col] (category-major: a wave's lanes write neighbouring columns).  It is a
// template parameter so that the TABLE = false instantiations keep their code (profiles/r21_device_asm_unchanged.txt).
template <int NW, int MODEL, bool TABLE = false>
__device__ __forceinline__ void site_posterior_body(const PosteriorParams& E, double* __restrict__ logp = nullptr) {
    extern __shared__ double lds[];
    double* wtab = lds;
    double* mtab = lds + 64;
    double* etab = lds + 96;
    double* stack = lds + kSiteLdsHeader;
    const SiteParams& P = E.S;
    const int chunk = blockIdx.x;
    const int locus = P.chunk_locus[chunk];
    if (E.done && E.done[locus]) return;   // wave-uniform
    etab[threadIdx.x] = kExp2Table[threadIdx.x];
    const LocusModel* __restrict__ M = P.models + locus;
    const int lane = threadIdx.x;
    using Regs = typename std::conditional<MODEL == TPHIP_MODEL_F81, F81Regs, ModelRegs>::type;
    Regs R;
    if constexpr (MODEL == TPHIP_MODEL_F81) {
        build_tip_table_f81(M, wtab, mtab, lane);
        R = load_model_f81(M, mtab, lane);
    } else {
        build_tip_table(M, wtab, lane);
        R = load_model(M, mtab, lane);
    }
    const int64_t lo = P.locus_offsets[locus], hi = P.locus_offsets[locus + 1];
    const int64_t S = hi - lo;
    int64_t ns = (S + P.chunk_cols / 2) / P.chunk_cols;  // = workgroups launched for this locus
    ns = ns < 1 ? 1 : ns;
    const int64_t W = P.work_count ? (int64_t)P.work_count[locus] : S;   // entries on the locus' work list
    const int64_t j = P.chunk_index[chunk];
    const int64_t first = j * W / ns, last = (j + 1) * W / ns;
    if (first >= last) return;
    const int K = E.ncat;
    const double u = E.log_scale[locus];
    const double* __restrict__ rho = E.cat_rate + (int64_t)locus * K;
    const double* __restrict__ logw = E.cat_logw + (int64_t)locus * K;
    for (int64_t base = first; base < last; base += kSiteBlock) {
        const int64_t want = base + lane;
        const bool active = want < last;
        const int64_t idx = active ? want : first;
        const int64_t col = P.work_cols ? (int64_t)P.work_cols[lo + idx] : lo + idx;
        uint32_t pk[NW > 0 ? NW : 1];
        if constexpr (NW > 0) {
#pragma unroll
            for (int w = 0; w < NW; ++w) pk[w] = (w < P.nwords) ? P.packed[(int64_t)w * P.ncols_total + col] : 0u;
        } else {
            pk[0] = P.packed[col];
        }
        double top = -INFINITY, z = 0.0, a = 0.0, b = 0.0, m1 = 0.0, m2 = 0.0;
        for (int k = 0; k < K; ++k) {
            const double rk = rho[k];
            const double uk = fmax(u + log(rk), kUMin);
            double fk, gk, hk;
            evaluate_column<NW, false, Regs>(P, R, wtab, etab, stack, col, pk, exp(uk), fk, gk, hk);
            fk += logw[k];
            if constexpr (TABLE) {
                if (active) logp[(int64_t)k * P.ncols_total + col] = fk;
            }
            if (fk > top) {
                const double r = exp(top - fk);   // exp(-inf) = 0 on the first category
                z *= r; a *= r; b *= r; m1 *= r; m2 *= r;
                top = fk;
            }
            const double p = exp(fk - top);
            z += p;
            a = fma(p, gk, a);
            b = fma(p, fma(gk, gk, hk), b);
            const double pr = p * rk;
            m1 += pr;
            m2 = fma(pr, rk, m2);
        }
        if (active) {
            const double iz = 1.0 / z;
            const double g = a * iz;
            E.f[col] = top + log(z);
            E.g[col] = g;
            E.h[col] = b * iz - g * g;
            E.mean[col] = m1 * iz;
            E.second[col] = m2 * iz;
        }
    }
}

// One parameter type per instantiation, so that all of them keep the name eval_columns_kernel (the names
// tools/flag_containment.py admits in this unit); NW = 2 / 8 words in registers or kStreamWords.
template <int NW, int MODEL>
struct PosteriorArgs : PosteriorParams {};
#define TPHIP_POSTERIOR_KERNEL(NW, MODEL) \
    __global__ __launch_bounds__(kSiteBlock) void eval_columns_kernel(PosteriorArgs<NW, MODEL> E) { site_posterior_body<NW, MODEL>(E); }
TPHIP_POSTERIOR_KERNEL(2, TPHIP_MODEL_GTR)
TPHIP_POSTERIOR_KERNEL(8, TPHIP_MODEL_GTR)
TPHIP_POSTERIOR_KERNEL(kStreamWords, TPHIP_MODEL_GTR)
TPHIP_POSTERIOR_KERNEL(2, TPHIP_MODEL_F81)
TPHIP_POSTERIOR_KERNEL(8, TPHIP_MODEL_F81)
TPHIP_POSTERIOR_KERNEL(kStreamWords, TPHIP_MODEL_F81)
#undef TPHIP_POSTERIOR_KERNEL

// the posterior-table variant: six more overloads, for the reason above
template <int NW, int MODEL>
struct PosteriorTableArgs : PosteriorTableParams {};
#define TPHIP_POSTERIOR_TABLE_KERNEL(NW, MODEL)                                                               \
    __global__ __launch_bounds__(kSiteBlock) void eval_columns_kernel(PosteriorTableArgs<NW, MODEL> E) {      \
        site_posterior_body<NW, MODEL, true>(E, E.logp);                                                      \
    }
TPHIP_POSTERIOR_TABLE_KERNEL(2, TPHIP_MODEL_GTR)
TPHIP_POSTERIOR_TABLE_KERNEL(8, TPHIP_MODEL_GTR)
TPHIP_POSTERIOR_TABLE_KERNEL(kStreamWords, TPHIP_MODEL_GTR)
TPHIP_POSTERIOR_TABLE_KERNEL(2, TPHIP_MODEL_F81)
TPHIP_POSTERIOR_TABLE_KERNEL(8, TPHIP_MODEL_F81)
TPHIP_POSTERIOR_TABLE_KERNEL(kStreamWords, TPHIP_MODEL_F81)
#undef TPHIP_POSTERIOR_TABLE_KERNEL

}  // namespace tphip

/*
 * tphip.h -- C ABI of libtphip.so: the MI355X (gfx950) site-rate + phylogenetic-informativeness engine.
 *
 * This is the drop-in boundary for ONE hot path of faircloth-lab/tapir: what `worker()` in
 * bin/tapir_compute.py:84-123 does per locus -- the shell-out to HyPhy (per-site substitution-rate ML,
 * tapir/data/models_and_rates.bf:978-1070) followed by Townsend's PI(t), its per-locus sums and its
 * scipy.integrate.quad interval integrals (tapir/compute.py:46-52, 76-94, 96-110) -- computed for ALL
 * loci in one column-parallel batch on the GPU.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  No exceptions cross the boundary.
 *   - every function returns 0 on success, non-zero on error; tphip_last_error() gives the message
 *     (thread-local, owned by the library).
 *   - there is NO CPU backend: a call fails with TPHIP_ERR_NO_DEVICE when no gfx950 device is usable.
 *   - the caller owns every data buffer.  `*_dev` entry points take DEVICE pointers (the hot path: inputs
 *     already resident in HBM, nothing leaves the device); the plain entry points take HOST pointers and
 *     do the H2D/D2H copies themselves.  The library keeps no pointer past the return of a host-pointer
 *     call; a plan keeps only its own small device tables (tree program, per-locus models, schedule).
 *   - state codes: one byte per alignment cell, bit mask A=1 C=2 G=4 T=8; gap/?/N = 15; IUPAC codes are
 *     unions (HyPhy resolves ambiguities as sets in the likelihood and fractionally in
 *     HarvestFrequencies, bf:968).  Layout is TAXON-MAJOR over the flattened batch:
 *     states[taxon * ncols_total + column]; loci are concatenated along the column axis and
 *     locus_offsets[L+1] gives their column ranges.  A wave reads 64 consecutive bytes of one taxon row.
 *   - tree: nodes in post-order (children before parents, root last); parent[root] = -1; leaf_taxon[n] =
 *     alignment row of leaf n, -1 for internal nodes; branch_len[n] = length of the branch above n,
 *     ALREADY divided by the correction factor (tapir/compute.py:59-74).  Multifurcations allowed.
 *   - PI table row for a locus: [ net PI at t=0..T-1 | PI at each of n_t times | sum(integral) per
 *     interval | sum(error) per interval ],  W = T + n_t + 2*n_i doubles (what tapir/db.py:44-61 stores).
 */
#ifndef TPHIP_H
#define TPHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPHIP_VERSION 110 /* 0.1.1: tphip_plan_desc.struct_size, TPHIP_START_AUTO, tphip_stage1_fit, tphip_plan_set_models;
                              tphip_plan_desc.model (TPHIP_MODEL_F81), a trailing field that struct_size makes safe to add */

enum {
    TPHIP_OK = 0,
    TPHIP_ERR_INVALID = 1,   /* bad argument (message says which) */
    TPHIP_ERR_NO_DEVICE = 2, /* no usable GPU: the library has no CPU path */
    TPHIP_ERR_HIP = 3,       /* a HIP runtime call failed */
    TPHIP_ERR_WORKSPACE = 4  /* caller's workspace is too small */
};

/* per-column flags written by the site-rate kernel */
enum {
    TPHIP_FLAG_OK = 0,        /* interior optimum                                                   */
    TPHIP_FLAG_FLAT = 1,      /* <= 1 resolved taxon: L independent of the rate; s stays 1 (bf:1050)  */
    TPHIP_FLAG_SATURATED = 2, /* log L flat to fp64 on the way to s -> inf (or uphill at s = 1e4): s = 1e4 */
    TPHIP_FLAG_ZERO = 3,      /* all resolved taxa share one base: optimum exactly at s = 0          */
    TPHIP_FLAG_MAXIT = 4      /* iteration limit                                                     */
};

/* integral modes for the interval sums (tapir/compute.py:50-52, 81-94) */
enum {
    TPHIP_INTEG_QUADPACK = 0, /* emulates scipy.integrate.quad: QUADPACK dqagse, GK21, eps 1.49e-8, limit 50;
                                 also yields sum(error) for the sqlite `interval.error` column          */
    TPHIP_INTEG_CLOSED = 1    /* analytic antiderivative -(4rt+1)exp(-4rt); error column = 0            */
};

/* tphip_plan_desc.start_rule: where the per-site optimiser starts (HyPhy: siteRate = 1 before every Optimize, bf:1050) */
enum {
    TPHIP_START_AUTO = 0,      /* default: HyPhy's start on trees of fewer than 32 taxa, the parsimony start from 32 on
                                  (and with the rate-mixture extension, which HyPhy's script does not have)                */
    TPHIP_START_REFERENCE = 1, /* siteRate = 1 on every tree                                                            */
    TPHIP_START_PARSIMONY = 2  /* the column's parsimony rate on every tree (one evaluation fewer per column)           */
};

/* tphip_plan_desc.pattern_dedup */
enum { TPHIP_DEDUP_AUTO = 0, TPHIP_DEDUP_OFF = 1, TPHIP_DEDUP_ON = 2 };

/* tphip_plan_desc.model: the per-site substitution model */
enum {
    TPHIP_MODEL_GTR = 0, /* default: the locus' GTR model, pi and exch per locus (HyPhy's, bf:978-1001)                      */
    TPHIP_MODEL_F81 = 1  /* all six exchangeabilities 1 (exch must be NULL), pi per locus: Q = Pi - I, P(t) = e^-t I +
                            (1 - e^-t) Pi in closed form (a cheaper site-rate kernel).  Jukes-Cantor = F81 with pi = 1/4 each */
};

int tphip_version(void);
const char *tphip_last_error(void);
/* number of usable HIP devices (0 if none; never fails) */
int tphip_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Plan: everything that is small and shared by a batch -- the tree's traversal program, the per-locus
 * GTR models (eigen-systems are computed on the device), the column ranges and the PI schedule.
 * Replaces: the three stdin lines + in-script constants HyPhy is configured with (bf:4-9, 966-1013) and
 * the per-locus `params` list of bin/tapir_compute.py:148-152.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tphip_plan tphip_plan;

typedef struct tphip_plan_desc {
    uint32_t struct_size;      /* sizeof(tphip_plan_desc) as the caller compiled it.  Zero-initialise the struct, then set
                                  this: fields the caller's header did not have yet take their zero defaults instead of being
                                  read from beyond the caller's struct                                   */
    int32_t device;            /* HIP device ordinal (>= 0)                                            */
    /* tree (host pointers) */
    int32_t ntaxa;             /* rows of the alignment                                                */
    int32_t nnodes;            /* nodes of the tree, post-order                                        */
    const int32_t *parent;     /* [nnodes]                                                             */
    const double *branch_len;  /* [nnodes], already / correction                                       */
    const int32_t *leaf_taxon; /* [nnodes]                                                             */
    /* loci (host pointers) */
    int64_t nloci;
    const int64_t *locus_offsets; /* [nloci+1] column ranges in the flattened batch                    */
    const double *pi;          /* [nloci*4] A,C,G,T base frequencies (bf:968 HarvestFrequencies)       */
    const double *exch;        /* [nloci*6] AC,AG,AT,CG,CT,GT exchangeabilities (bf:970-976; AG == 1)  */
    /* PI schedule */
    int32_t T;                 /* net PI is evaluated at t = 0..T-1, T = int(tree depth) (compute.py:54-57) */
    const int32_t *times;      /* [n_t] --times, each < T (compute.py:76-79)                           */
    int32_t n_t;
    const int32_t *intervals;  /* [n_i*2] --intervals as (start, stop), start < stop (compute.py:90-91) */
    int32_t n_i;
    int32_t integ_mode;        /* TPHIP_INTEG_*                                                        */
    /* rate post-processing between the two stages (bin/tapir_compute.py:100-102) */
    double correction;         /* rates are divided by this (parse_site_rates, compute.py:38-39)       */
    int32_t threshold;         /* columns with fewer A/C/G/T cells become NaN (compute.py:96-110)      */
    int32_t round_decimals;    /* 4 = round rates as HyPhy's Format(x,0,4) does before PI (bf:1093-1095);
                                  < 0 = keep full precision                                            */
    /* Opt-in extension, NOT in the reference (its script has no rate mixture): a discrete mixture of
     * rate categories on top of the per-site rate, L(s) = sum_k cat_weight[k] L(s * cat_rate[k]) -- the "+G" of
     * GTR+G when the categories are the discrete gamma of Yang (1994).  ncat <= 1 = the reference's model. */
    int32_t ncat;              /* number of categories, at most 16                                    */
    const double *cat_rate;    /* [ncat] rate multipliers > 0 (mean 1 keeps `rate` = kappa * s interpretable) */
    const double *cat_weight;  /* [ncat] weights > 0 (normalised by the library)                       */
    /* Where the per-site optimiser starts.  HyPhy starts every column at siteRate = 1 (bf:1050) and returns the local
     * optimum uphill of that point.  The parsimony start (the column's parsimony rate) saves one evaluation
     * per column and reaches the same maximum on every unimodal column; on the rare multimodal ones it may end on another
     * local optimum than a search from 1 would -- measured: 0 of 4e5 columns at 64 taxa, 6e-5 at 16 taxa, 1e-3 of noisy
     * 5-taxon columns.  TPHIP_START_AUTO therefore uses it only on trees of 32 taxa or more, where no
     * deviation was ever seen, and HyPhy's own start below; the other two values force one rule on every tree. */
    int32_t start_rule;        /* TPHIP_START_*                                                        */
    /* HyPhy fits one rate per UNIQUE column pattern of a locus and reports it for every column that carries it
     * (bf:1033-1044: GetDataInfo(dupInfo...), alreadyDone[siteMap]).  TPHIP_DEDUP_AUTO does the same wherever a cheap
     * per-locus estimate says at least ~15 % of the columns that need the optimiser are repeats (real loci; the synthetic
     * alignments with random gaps hardly repeat a column), in batches of at least 2^20 columns (smaller ones are
     * latency-bound: nothing to gain); ON / OFF force it.  The outputs are bit-identical either way. */
    int32_t pattern_dedup;     /* TPHIP_DEDUP_*                                                        */
    /* The substitution model of the per-site loop.  TPHIP_MODEL_GTR (0, the zero default of callers built against an older
     * header) is the locus' GTR model.  TPHIP_MODEL_F81: exch must be NULL (the library uses 1s), pi is required; rate is
     * kappa * s with kappa = 1 - sum pi_i^2.  tphip_plan_set_models then takes pi only, tphip_stage1_fit[_dev] is refused
     * (a fixed model has nothing to fit) and tphip_plan_get_models returns the eigen-system of Pi - I (lam = -1, -1, -1). */
    int32_t model;             /* TPHIP_MODEL_*                                                        */
} tphip_plan_desc;

int tphip_plan_create(const tphip_plan_desc *desc, tphip_plan **out);
int tphip_plan_destroy(tphip_plan *plan);
/* width W of a PI table row, and total columns */
int32_t tphip_plan_table_width(const tphip_plan *plan);
int64_t tphip_plan_ncols(const tphip_plan *plan);
/* bytes of device scratch the *_dev entry points need (compacted column list, per-chunk PI partials).
 * Alignment: tphip_site_rates_dev, tphip_pi_tables_dev and tphip_run_dev need d_workspace 16-byte aligned (the widest access
 * into it is a 16-byte store of packed tip words; its other regions hold 64-bit prefixes and the 64-bit keys of the
 * de-duplication table, which atomics reach) and return TPHIP_ERR_INVALID, "workspace must be 16-byte aligned", before anything
 * is enqueued otherwise.  Its content on entry is irrelevant and nothing beyond the stated size is touched.
 * Data arrays of every *_dev entry point need the natural alignment of their element type only (1 for states and flags, 2 for
 * 16-bit counts, 4 for int32, 8 for double and the 64-bit integers): a caller may slice one big buffer.  Nothing before or
 * beyond an array's extent is written. */
size_t tphip_plan_workspace_bytes(const tphip_plan *plan);
/* chronogram length = sum of branch lengths (bf:1006-1013) and LDS stack depth of the program */
double tphip_plan_chrono_length(const tphip_plan *plan);
int32_t tphip_plan_stack_depth(const tphip_plan *plan);
/* op mix of the compiled tree program: counts[5] = TIP_SET, TIP_MUL, BRANCH, PUSH, POP_MUL (for FLOP models) */
int tphip_plan_op_counts(const tphip_plan *plan, int32_t *counts);
/* number of TIP_SET + TIP_MUL pairs the site-rate kernel executes as one fused CHERRY op (equal branch lengths:
 * one set of exponentials for both tips) */
int32_t tphip_plan_cherry_count(const tphip_plan *plan);
/* copy the per-locus eigen-systems back (tests): lam[L*4], U[L*16], Uinv[L*16], kappa[L] */
int tphip_plan_get_models(const tphip_plan *plan, double *lam, double *U, double *Uinv, double *kappa);
/* Replace the per-locus models of an existing plan: pi [nloci*4] and / or exch [nloci*6] (host; NULL keeps the current
 * values).  The eigen-systems are recomputed on the device.  What it is for: one plan per batch through both stages of
 * HyPhy's script -- tphip_stage1_fit estimates the exchangeabilities (bf:405-897), the per-site loop then runs on them
 * (bf:970-976) -- instead of a second plan.  Same validation as tphip_plan_create. */
int tphip_plan_set_models(tphip_plan *plan, const double *pi, const double *exch);

/* ------------------------------------------------------------------------------------------------
 * Device-pointer entry points (the hot path).  `stream` is a hipStream_t (NULL = default stream).
 * Kernels are enqueued and the call returns without synchronising.
 * ---------------------------------------------------------------------------------------------- */

/* Stage 1 -- replaces Popen([hyphy, template]) for every locus at once (bin/tapir_compute.py:92-99).
 * Per column: rate = kappa*s_hat, subst = rate*chronoLength, lnl, flag, nres = #A/C/G/T cells. */
int tphip_site_rates_dev(tphip_plan *plan, const uint8_t *d_states, double *d_rate, double *d_subst,
                         double *d_lnl, uint8_t *d_flag, int32_t *d_nres, void *d_workspace,
                         size_t workspace_bytes, void *stream);

/* Stage 2 -- replaces get_townsend_pi + nansum + get_net_pi_for_periods + get_net_integral_for_epochs
 * (bin/tapir_compute.py:114-122).  d_rates are the raw stage-1 rates; rounding, /correction and the
 * informative-site cull (d_nres may be NULL = no cull, the --site-rates path, bin/tapir_compute.py:103-104)
 * are applied on the fly.  d_tables is [nloci][W]. */
int tphip_pi_tables_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres, double *d_tables,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/* Both stages back to back on one stream: the whole worker() body for the whole batch. */
int tphip_run_dev(tphip_plan *plan, const uint8_t *d_states, double *d_rate, double *d_subst, double *d_lnl,
                  uint8_t *d_flag, int32_t *d_nres, double *d_tables, void *d_workspace,
                  size_t workspace_bytes, void *stream);

/* parse_site_rates + cull_uninformative_rates as the PI stage applies them to a raw rate (tapir/compute.py:24-44,
 * 108-110; bin/tapir_compute.py:100-102): d_out[c] = R4(d_rates[c]) / correction, NaN where d_nres[c] < threshold
 * (d_nres may be NULL: no cull -- what parse_site_rates alone returns and writes as `corrected_rates`).  R4 is the
 * round trip through HyPhy's Format(x,0,4) (bf:1093-1095): the double nearest to the decimal that printf-style
 * rounding of the exact binary value gives (skipped when round_decimals < 0). */
int tphip_corrected_rates_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres, double *d_out,
                              void *stream);

/* tapir/compute.py:46-48 get_townsend_pi(time, rates) as a dense (n_times, n) matrix, row-major:
 * out[k*n + i] = 16 r_i^2 t_k exp(-4 r_i t_k).  NaN rates propagate (numpy semantics). */
int tphip_townsend_pi_dense_dev(int32_t device, const double *d_rates, int64_t n, const double *d_times,
                                int32_t n_times, double *d_out, void *stream);

/* tapir/compute.py:50-52 vectorised over sites: (integral, abserr) of scipy.integrate.quad(
 * get_townsend_pi, a, b, args=(rate)) for every rate (QUADPACK dqagse emulation, or the closed form with
 * abserr = 0 when integ_mode == TPHIP_INTEG_CLOSED).  Non-finite rates give NaN. */
int tphip_quad_townsend_dev(int32_t device, const double *d_rates, int64_t n, double a, double b,
                            int32_t integ_mode, double *d_integral, double *d_abserr, void *stream);

/* HarvestFrequencies(Freqs, filter, 1, 1, 1) (bf:968): per-locus counts of each of the 16 state masks;
 * d_hist is [nloci][16] int64 (pi follows on the host: each mask adds 1/popcount to its bases).
 * d_locus_offsets is a DEVICE array [nloci+1].  HBM-bound byte kernel: ntaxa bytes read per column. */
int tphip_state_histogram_dev(int32_t device, const uint8_t *d_states, int64_t ncols_total, int32_t ntaxa,
                              const int64_t *d_locus_offsets, int64_t nloci, int64_t *d_hist, void *stream);

/* Whole-locus log-likelihood for a batch of candidate parameter sets: the objective HyPhy's stage 1 maximises in
 * every `Optimize(lf_MLES, lf)` (models_and_rates.bf:487-520, 647-655): sum over the columns of locus
 * cand_locus[c] of log L(column | exchangeabilities cand_exch[c][6] = AC,AG,AT,CG,CT,GT, branch lengths, base
 * frequencies = the plan's pi for that locus), every site at rate 1.  Branch lengths (above each node, post-order
 * numbering of the plan's tree, root entry ignored) of candidate c are
 *     blen_vecs[cand_vec[c]][b] * cand_scale[c] * (b == cand_pidx[c] ? cand_pfac[c] : 1)
 * so a finite-difference stencil, or the rate-class models that only rescale stashed lengths (bf:613-619), share
 * one stored vector.  One workgroup per candidate; the optimiser runs on the host (tapir_amd/stage1.py). */
int tphip_locus_loglik_dev(tphip_plan *plan, const uint8_t *d_states, int64_t ncand, const int32_t *d_cand_locus,
                           const double *d_cand_exch, const double *d_blen_vecs, const int32_t *d_cand_vec,
                           const double *d_cand_scale, const int32_t *d_cand_pidx, const double *d_cand_pfac,
                           double *d_out, void *stream);

/* Value AND gradient of the same objective from one forward + one reverse sweep of the pruning recursion
 * (reverse-mode differentiation; replaces a finite-difference stencil of 2 x (5 + 2N-3) likelihood evaluations).
 * Candidates are described exactly as for tphip_locus_loglik_dev.  Outputs per candidate:
 *   d_lnl[c]; d_dexch[c][6] = d lnL / d (AC, AG, AT, CG, CT, GT) with branch lengths held fixed;
 *   d_dlogt[c][nnodes] = d lnL / d log t_b (root entry 0; may be NULL); d_sum_dlogt[c] = its sum over branches
 *   (the only branch-length derivative a rate-class model needs: bf:613-619 ties all lengths to one factor);
 *   d_d2logt[c][nnodes] = d2 lnL / d (log t_b)^2, the diagonal of the Hessian in the branch lengths (may be NULL;
 *   the optimiser's preconditioner). */
int tphip_locus_gradient_dev(tphip_plan *plan, const uint8_t *d_states, int64_t ncand, const int32_t *d_cand_locus,
                             const double *d_cand_exch, const double *d_blen_vecs, const int32_t *d_cand_vec,
                             const double *d_cand_scale, const int32_t *d_cand_pidx, const double *d_cand_pfac,
                             double *d_lnl, double *d_dexch, double *d_dlogt, double *d_sum_dlogt, double *d_d2logt,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * HyPhy's stage 1 as one call: model-averaged exchangeabilities for every locus of the plan.
 * Replaces, per locus, models_and_rates.bf:487-520 (general reversible model: Optimize over AC, AT, CG, CT, GT
 * and every branch length), :522-540 (branch lengths stashed as expected substitutions), :542-661 (the other 202
 * partitions of the six rates into classes, Optimize over at most four class rates each) and :806-847 (Akaike weights
 * w_m ~ exp(lnL_m - k_m), model-averaged rates).  The optimisers run on the device (stage1_opt_kernels.hpp: L-BFGS for
 * the general model, dense BFGS for the rate-class models, a quadratic screen that decides which of the 202 can carry
 * weight); the host sequences launches.  The plan's own exchangeabilities are ignored, its pi and tree are used; with
 * column weights set (tphip_plan_set_column_weights) the plan's columns are site patterns, as HyPhy evaluates them.
 * Models are indexed 0..202: 0 = "012345" (the general model), then the other restricted growth strings over
 * (AC, AG, AT, CG, CT, GT) in lexicographic order = the order of the loops at bf:544-566.
 * Outputs are HOST arrays (the call synchronises `stream` before it returns); all but exch may be NULL:
 *   exch[L][6]           model-averaged AC, AG (= 1), AT, CG, CT, GT -- what stage 2 takes (bf:838-847)
 *   pi[L][4]             the base frequencies used (the plan's, or the empirical ones: opts.empirical_pi)
 *   weights[L][203]      Akaike weights;  lnl[L][203] maximised log-likelihoods;  model_exch[L][203][6] fitted rates
 *   grm_blen[L][nnodes]  branch lengths t_b of the general model (stash / totalFactor)
 *   grm_iters[L], sub_iters[L][202]  optimiser iterations;  stats[8] = likelihood evaluations, gradients, evaluations and
 *                        gradients of the general model, models abandoned, models fitted, outer iterations (general, class) */
typedef struct tphip_stage1_opts {
    uint32_t struct_size;   /* sizeof(tphip_stage1_opts) as the caller compiled it; fields beyond it take their defaults.
                               Zero-initialise the struct, then set this.                                          */
    int32_t maxit_grm;      /* iteration limit of the general model, 0 = max(300, 4 * (5 + branches))              */
    int32_t maxit_sub;      /* iteration limit of a rate-class model, 0 = 100                                      */
    int32_t no_prune;       /* 1 = fit all 202 models to convergence (default 0: a model whose Akaike weight cannot
                               exceed e^-21 is abandoned with the likelihood it has reached, a lower bound)          */
    double fd_step;         /* step of the central differences of the rate-class fits in log-rate, 0 = 1e-4         */
    int32_t free_root_pair; /* 1 = the two branches below a bifurcating root are separate coordinates, as in HyPhy's
                               parameter list (default 0: one coordinate for their sum, which is all a reversible
                               model's likelihood depends on; the reported pair keeps the input tree's proportion)  */
    int32_t compress_patterns; /* 1 = the plan's columns are raw alignment columns: collapse them on the device into unique
                               site patterns with counts first, which is what HyPhy's likelihood function sums over
                               (GetDataInfo(dupInfo...), bf:960-963).  0 = evaluate the plan's columns as they are (with
                               the plan's column weights, if set)                                                    */
    int32_t empirical_pi;   /* 1 = base frequencies from the alignment itself, HarvestFrequencies(.., 1, 1, 1) (bf:968):
                               every cell adds 1 / popcount(mask) to each base it may be.  They replace the plan's pi
                               (as tphip_plan_set_models would) and are returned in `pi`.  0 = the plan's pi          */
    int64_t row_pitch;      /* host-pointer call only: bytes between taxon rows of `states` (0 = the plan's column count).
                               Lets a caller pass a column range of a bigger taxon-major array without copying it.   */
} tphip_stage1_opts;

int tphip_stage1_fit_dev(tphip_plan *plan, const uint8_t *d_states, const tphip_stage1_opts *opts, double *exch, double *pi,
                         double *weights, double *lnl, double *model_exch, double *grm_blen, int32_t *grm_iters,
                         int32_t *sub_iters, int64_t *stats, void *stream);
/* host-pointer twin: `states` is uploaded once (a 2-D copy when opts.row_pitch is set); d_states_cache as for
 * tphip_locus_loglik (it must be NULL when row_pitch or compress_patterns is used: nothing of the upload is kept) */
int tphip_stage1_fit(tphip_plan *plan, const uint8_t *states, void **d_states_cache, const tphip_stage1_opts *opts,
                     double *exch, double *pi, double *weights, double *lnl, double *model_exch, double *grm_blen,
                     int32_t *grm_iters, int32_t *sub_iters, int64_t *stats);

/* Profiling hooks for bench.py: when enabled the library brackets its dominant kernel (site rates) with
 * HIP events on the caller's stream and accumulates the elapsed time. */
int tphip_profile_enable(tphip_plan *plan, int32_t on);
/* sums since the last reset; *launches = number of bracketed launches; the call synchronises the events */
int tphip_profile_read(tphip_plan *plan, double *site_rate_ms, double *pi_ms, int64_t *launches, int32_t reset);
/* total likelihood evaluations (Newton iterations summed over columns) of the last site-rate launch */
int tphip_last_eval_count(tphip_plan *plan, int64_t *evals);
/* evaluation rounds of the last site-rate launch summed over its wavefronts (a round = one likelihood evaluation issued for all
 * 64 lanes of a wavefront, busy or not): evals / (64 * rounds) is the fraction of issued lane-evaluations that carried a column */
int tphip_last_round_count(tphip_plan *plan, int64_t *rounds);

/* ------------------------------------------------------------------------------------------------
 * Host-pointer entry points: same stages, library does the copies (PCIe time included by construction).
 * ---------------------------------------------------------------------------------------------- */
/* Pinned host memory for the buffers of the host-pointer calls: with it the copies are direct DMA and the per-column
 * results travel while the PI kernels run; ordinary (pageable) memory works too, through the runtime's staged copies.
 * When EVERY buffer of a tphip_site_rates / tphip_run_fused call is pinned (the input `states` too) and the batch has
 * at least 2^21 columns, the library runs it as a pipeline of two locus groups (the second upload under the first
 * group's kernels); outputs are identical to the unsplit run.  NULL (and tphip_last_error) when the allocation fails.
 * Free with tphip_host_free. */
void *tphip_host_alloc(size_t bytes);
int tphip_host_free(void *ptr);
int tphip_site_rates(tphip_plan *plan, const uint8_t *states, double *rate, double *subst, double *lnl,
                     uint8_t *flag, int32_t *nres);
int tphip_pi_tables(tphip_plan *plan, const double *rates, const int32_t *nres, double *tables);
int tphip_corrected_rates(tphip_plan *plan, const double *rates, const int32_t *nres, double *out);
int tphip_run_fused(tphip_plan *plan, const uint8_t *states, double *rate, double *subst, double *lnl,
                    uint8_t *flag, int32_t *nres, double *tables);
/* tphip_run_fused on a column range of a bigger taxon-major array: `states` points at the range's first column of taxon 0,
 * consecutive taxon rows are row_pitch bytes apart (0 = the plan's column count).  The upload is one 2-D copy; from pinned
 * memory no host copy is made.  With tphip_stage1_fit (opts.row_pitch) and tphip_plan_set_models this lets a caller stream a
 * big batch block by block -- stage 1, the per-site loop and PI of block k while the host still writes block k - 1's files. */
int tphip_run_fused_pitched(tphip_plan *plan, const uint8_t *states, int64_t row_pitch, double *rate, double *subst,
                            double *lnl, uint8_t *flag, int32_t *nres, double *tables);
int tphip_townsend_pi_dense(int32_t device, const double *rates, int64_t n, const double *times, int32_t n_times,
                            double *out);
int tphip_quad_townsend(int32_t device, const double *rates, int64_t n, double a, double b, int32_t integ_mode,
                        double *integral, double *abserr);
int tphip_state_histogram(int32_t device, const uint8_t *states, int64_t ncols_total, int32_t ntaxa,
                          const int64_t *locus_offsets, int64_t nloci, int64_t *hist);
/* Unique site patterns per locus (HyPhy: GetDataInfo(dupInfo, filteredData), models_and_rates.bf:960-963; its stage 1
 * sums pattern likelihoods weighted by counts and its stage 2 fits one rate per pattern).  Columns of a locus that are
 * identical after normalising the state masks (0 -> 15) collapse into one pattern.  Outputs: out_states
 * [ntaxa][*out_npatterns] taxon-major (the buffer must hold ntaxa * ncols_total bytes), out_offsets [nloci+1] pattern
 * offsets per locus, out_weight [*out_npatterns] column counts (buffer of ncols_total doubles), out_map [ncols_total]
 * column -> pattern index (may be NULL).  Patterns of a locus are in hash order, deterministic for given input.
 * Exact: equality is decided on the full columns, hashes only group candidates.  Guaranteed:
 *   - columns that differ are NEVER merged into one pattern, whatever their hashes;
 *   - the columns of a pattern are never split over several patterns, except when another pattern of the same locus
 *     shares BOTH of the library's hashes with it (40 bits of the first and all 64 of the second, ~2^-104 per pair of
 *     patterns); the counts then still add up to the locus' columns, so weighted likelihoods stay right.
 * Plan-less, host pointers. */
int tphip_compress_columns(int32_t device, const uint8_t *states, int64_t ncols_total, int32_t ntaxa,
                           const int64_t *locus_offsets, int64_t nloci, uint8_t *out_states, int64_t *out_offsets,
                           double *out_weight, int64_t *out_map, int64_t *out_npatterns);
/* host-pointer twin of tphip_locus_loglik_dev; d_states_cache may keep the alignment on the device between calls:
 * pass the address of a NULL void* the first time and free it with tphip_free_device when done (NULL = copy the
 * alignment on every call) */
int tphip_locus_loglik(tphip_plan *plan, const uint8_t *states, void **d_states_cache, int64_t nvec,
                       const double *blen_vecs, int64_t ncand, const int32_t *cand_locus, const double *cand_exch,
                       const int32_t *cand_vec, const double *cand_scale, const int32_t *cand_pidx,
                       const double *cand_pfac, double *out);
/* host-pointer twin of tphip_locus_gradient_dev (dlogt and d2logt may be NULL) */
int tphip_locus_gradient(tphip_plan *plan, const uint8_t *states, void **d_states_cache, int64_t nvec,
                         const double *blen_vecs, int64_t ncand, const int32_t *cand_locus, const double *cand_exch,
                         const int32_t *cand_vec, const double *cand_scale, const int32_t *cand_pidx,
                         const double *cand_pfac, double *lnl, double *dexch, double *dlogt, double *sum_dlogt,
                         double *d2logt);
int tphip_free_device(tphip_plan *plan, void *d_ptr);
/* Column multiplicities [ncols] (host) for tphip_locus_loglik / tphip_locus_gradient of this plan: the plan's columns
 * are then site patterns (tphip_compress_columns) and every pattern's log-likelihood counts weight times.
 * NULL removes them.  The site-rate path ignores them. */
int tphip_plan_set_column_weights(tphip_plan *plan, const double *weights);

/* Diagnostic (tests): log L and its first two derivatives with respect to u = log(siteRate) for every
 * column at a caller-chosen u[ncols]; no classification, no optimiser.  Host pointers. */
int tphip_eval_columns(tphip_plan *plan, const uint8_t *states, const double *u, double *f, double *g, double *h);
/* device-pointer twin (full-size property tests: nothing crosses PCIe); enqueues on `stream`, does not synchronise */
int tphip_eval_columns_dev(tphip_plan *plan, const uint8_t *d_states, const double *d_u, double *d_f, double *d_g,
                           double *d_h, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Empirical-Bayes site rates under a discrete-gamma prior (Yang 1994; the Rate4Site estimator): an opt-in alternative
 * to the per-column maximum-likelihood rate of tphip_site_rates.  Per locus the site rate is s = mu rho with rho in
 * ncat categories (rates cat_rate[l][k], weights cat_weight[l][k], both [nloci][ncat], HOST arrays, positive; the
 * caller builds them, e.g. equiprobable gamma(alpha, alpha) categories) and mu = scale[l].  With L_c(s) the column
 * likelihood of the site-rate stage (tphip_eval_columns with a one-category plan), m_c = sum_k w_k L_c(mu rho_k).
 * A category whose log(mu rho_k) is below log(1e-10) is evaluated there (the likelihood is flat to fp64).
 * Works on TPHIP_MODEL_GTR and TPHIP_MODEL_F81 plans; the plan's own ncat / cat_rate / cat_weight are ignored, as are
 * column weights.  Every column of a locus takes part, whatever its count of informative cells.
 *
 * tphip_eb_start_scale: scale[l] (HOST, out) = where the fit of mu should start: the mean over the locus' columns of the
 *   parsimony start rate the site-rate stage gives each column (0 for columns without a change), or 1 / tree length for a
 *   locus without a change.  It lies on the near side of the plateau l reaches as mu grows, whatever the tree's units.
 * tphip_eb_fit_scale: for every locus at once, maximise l(mu) = sum over the locus' columns of log m_c over log mu,
 *   starting from scale[l] (in/out; tphip_eb_start_scale gives a start), by a safeguarded Newton
 *   iteration on the device.  locus_lnl[l] = l and curvature[l] = d2l/d(log mu)2 at the returned scale (may be NULL);
 *   iters[l] (may be NULL) = evaluations used, negated if the limit was reached first.  The alpha search is the caller's.
 * tphip_eb_posterior: per column rate = kappa mu E[rho | column] (expected substitutions per unit of tree time, the
 *   unit of tphip_site_rates' rate), rate_sd = kappa mu sd[rho | column], lnl = log m_c, nres as tphip_site_rates
 *   reports it; tphip_corrected_rates / tphip_pi_tables take rate and nres unchanged.
 * use_patterns = 1 evaluates one column per site pattern of a locus; results are bit-identical either way.
 * The plain functions take HOST states; the _dev twins take DEVICE states (and device rate / rate_sd / lnl / nres), keep
 * the small per-locus arrays on the host, enqueue on `stream` and, for the fit, synchronise it before returning.
 * Thread-safety: as for every call that takes a plan -- calls on one plan must not overlap (they share the plan's
 * workspace); different plans may be used from different threads. */
typedef struct tphip_eb_opts {
    uint32_t struct_size;  /* sizeof(tphip_eb_opts) of the caller */
    int32_t ncat;          /* 2..16 */
    int32_t maxit_scale;   /* limit of the Newton iteration, 0 = default (60) */
    int32_t use_patterns;  /* 1 = compress columns to site patterns on the device first */
    double tol_scale;      /* stop when the Newton step in log mu is below this, 0 = default (1e-9) */
} tphip_eb_opts;

int tphip_eb_start_scale(tphip_plan *plan, const uint8_t *states, double *scale);
int tphip_eb_start_scale_dev(tphip_plan *plan, const uint8_t *d_states, double *scale, void *stream);
int tphip_eb_fit_scale(tphip_plan *plan, const uint8_t *states, const tphip_eb_opts *opts, const double *cat_rate,
                       const double *cat_weight, double *scale, double *locus_lnl, double *curvature, int32_t *iters);
int tphip_eb_fit_scale_dev(tphip_plan *plan, const uint8_t *d_states, const tphip_eb_opts *opts, const double *cat_rate,
                           const double *cat_weight, double *scale, double *locus_lnl, double *curvature,
                           int32_t *iters, void *stream);
int tphip_eb_posterior(tphip_plan *plan, const uint8_t *states, const tphip_eb_opts *opts, const double *cat_rate,
                       const double *cat_weight, const double *scale, double *rate, double *rate_sd, double *lnl,
                       int32_t *nres);
int tphip_eb_posterior_dev(tphip_plan *plan, const uint8_t *d_states, const tphip_eb_opts *opts, const double *cat_rate,
                           const double *cat_weight, const double *scale, double *d_rate, double *d_rate_sd,
                           double *d_lnl, int32_t *d_nres, void *stream);
/* tphip_eb_posterior with the category posterior besides: post[k * ncols + c] = p_ck = w_k L_c(mu rho_k) / m_c
 * ([ncat][ncols], category-major; the same clamp at log(1e-10); every column sums to 1 within rounding; under use_patterns a
 * column repeated in its locus reads its representative's p).  rate, rate_sd, lnl and nres are those of tphip_eb_posterior,
 * bit for bit. */
int tphip_eb_posterior_table(tphip_plan *plan, const uint8_t *states, const tphip_eb_opts *opts, const double *cat_rate,
                             const double *cat_weight, const double *scale, double *post, double *rate, double *rate_sd,
                             double *lnl, int32_t *nres);
int tphip_eb_posterior_table_dev(tphip_plan *plan, const uint8_t *d_states, const tphip_eb_opts *opts,
                                 const double *cat_rate, const double *cat_weight, const double *scale, double *d_post,
                                 double *d_rate, double *d_rate_sd, double *d_lnl, int32_t *d_nres, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The empirical-Bayes rate posterior carried into the per-locus PI rows (an extension).  PI(t) = 16 s^2 t e^(-4st) is not
 * linear in s, so the profile at a site's posterior mean rate is not the posterior expectation of the profile.  Given the
 * fitted scale mu_l and categories (rho_lk, w_lk), k < K, a site of locus l has one of K rates only:
 *   r_lk      = the plan's finalisation (the round_decimals round trip, then /correction, as tphip_corrected_rates
 *               treats a column's rate) of the raw rate (kappa_l mu_l) rho_lk;
 *   P_l[k][w] = the per-site values of the PI tables and the bootstrap at r_lk, w < Wb = T + n_i (tphip_bootstrap_width):
 *               16 r^2 t e^(-4rt) at t = 0..T-1, then the interval integrals under the plan's integ_mode;
 *   live      = nres[c] >= threshold, the cull of tphip_pi_tables (nres NULL: every column); a culled column
 *               contributes nothing below.
 * A posterior draw of the locus' row is sum_k N_k P_l[k][.], N_k = the live sites drawn into category k.
 *
 * Analytic moments per locus and entry, analytic[l][0][w] = mean, analytic[l][1][w] = sd:
 *   expected_counts[l][k] = n_lk = sum over live c of p_ck (a fixed-order sum per locus),
 *   mean[w] = sum_k n_lk P_l[k][w],
 *   var[w]  = sum over live c of ( sum_k p_ck P_l[k][w]^2 - (sum_k p_ck P_l[k][w])^2 ), every site's term >= 0 (it is
 *             evaluated in the centred form sum_k p_ck (P_l[k][w] - a_c)^2, a_c = sum_k p_ck P_l[k][w]),  sd = sqrt(var).
 *
 * Draws: replicate b < B, 2 <= B <= 4096.  Generator: Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter =
 * (j, b, locus_id & 0xffffffff, locus_id >> 32); word i of block j serves the column at index 4j + i WITHIN ITS LOCUS --
 * the column, not its pattern (repeats draw independently), and every column, culled or not (the stream does not move with
 * the cull).  With x that 32-bit word and c_k the fp64 running sum p_c0 + ... + p_ck added in that order, the drawn category
 * is the number of k <= K - 2 with (x + 0.5) 2^-32 >= c_k.  counts[l][b][k] = N_b[k] = the live columns drawn into k;
 * rows[l][b][w] = X_b[w] = sum_k N_b[k] P_l[k][w], added in ascending k.  summary[l][4][Wb] = mean, sd, lo, hi over the B
 * rows, by tphip_summarize_rows_dev.
 *
 * Determinism: a locus' category rows, counts and replicate rows depend on its columns, its model, (mu, rho, w), the seed,
 * the locus id and b only -- not on the other loci, on B, on the workspace size, on blocking or on the GPU count.
 * Everything is conditional on the fitted (mu_l, alpha_l), the model and the tree: the bands say nothing about the
 * uncertainty of those.
 *
 * post is tphip_eb_posterior_table's [ncat][ncols].  In the _dev call post, nres, scale [nloci] and cat_rate [nloci][ncat]
 * are DEVICE arrays; it enqueues on `stream` and does not synchronise when opts.locus_ids is NULL (with locus_ids set: as
 * tphip_pi_bootstrap_dev).  d_rows [nloci][B][Wb] and d_counts [nloci][B][ncat] (int32) may be NULL.  Any workspace >=
 * *min_bytes gives the same bits; *preferred_bytes (<= about 1 GiB, or the minimum) takes more loci per block.
 * Errors: TPHIP_ERR_INVALID for B outside 2..4096, level outside (0, 1), ncat outside 2..16. */
typedef struct tphip_posterior_pi_opts {
    uint32_t struct_size;      /* sizeof(tphip_posterior_pi_opts) of the caller */
    int32_t replicates;        /* B, 2..4096 */
    double level;              /* coverage of [lo, hi], in (0, 1) */
    uint64_t seed;
    const int64_t *locus_ids;  /* HOST [nloci] stream id per locus, NULL = the plan's locus index; read before the call returns */
    int32_t ncat;              /* K, 2..16: the categories of post and cat_rate */
} tphip_posterior_pi_opts;

int tphip_posterior_pi_workspace_bytes(const tphip_plan *plan, const tphip_posterior_pi_opts *opts, size_t *min_bytes,
                                       size_t *preferred_bytes);
int tphip_posterior_pi_dev(tphip_plan *plan, const double *d_post, const int32_t *d_nres, const double *d_scale,
                           const double *d_cat_rate, const tphip_posterior_pi_opts *opts, double *d_analytic,
                           double *d_expected_counts, double *d_summary, double *d_rows, int32_t *d_counts,
                           void *d_workspace, size_t workspace_bytes, void *stream);
/* host-pointer twin: the library allocates its own workspace */
int tphip_posterior_pi(tphip_plan *plan, const double *post, const int32_t *nres, const double *scale,
                       const double *cat_rate, const tphip_posterior_pi_opts *opts, double *analytic,
                       double *expected_counts, double *summary, double *rows, int32_t *counts);

/* ------------------------------------------------------------------------------------------------
 * Site bootstrap of the per-locus PI rows (an extension: the reference reports the rows without an error bar).
 * A column's final rate depends on the column and the locus' model only, so an alignment resampled with replacement has
 * the same per-site rates with multiplicities.  Replicate b of locus l draws n_l column indices with replacement from all
 * n_l columns of the locus (culled ones included); with c[b][i] the counts and p_i[w] site i's values -- 16 r^2 t e^(-4rt)
 * at t = 0..T-1, then the integral over each of the n_i intervals, by the device functions of the PI tables under the
 * plan's integ_mode; all zero for a NaN (culled) or zero rate -- the replicate row is X_b[w] = sum_i c[b][i] p_i[w],
 * w < Wb = T + n_i.  The sum(error) columns are not resampled and the --times entries are net[times[k]], left to the
 * caller.  The locus' model (and an empirical-Bayes prior) are held fixed: the bands are conditional on the fitted model.
 * Inputs are those of tphip_pi_tables: raw rates and an optional nres, finalised by the plan's rounding, correction, cull.
 *
 * Generator: Philox4x32-10 (Salmon et al. 2011), key = (seed & 0xffffffff, seed >> 32), counter = (j, b, locus_id &
 * 0xffffffff, locus_id >> 32); the output words (x0, x1, x2, x3) give draw 2j = ((x1 * 2^32 + x0) * n_l) >> 64 and draw
 * 2j + 1 likewise from (x3, x2), j = 0 .. ceil(n_l / 2) - 1; the last draw of an odd n_l is discarded.  Counts are 16-bit.
 *
 * Determinism: the replicate rows of a locus depend on seed, locus id, b, the locus' final rates and the schedule only --
 * not on the other loci of the plan, on the number of replicates, on the workspace size or on how a batch is sharded.
 *
 * Summary per locus and entry w over the B replicates, layout [L][4][Wb]: mean, sd (B - 1 in the denominator, two-pass),
 * lo and hi = the quantiles at (1 - level) / 2 and 1 - (1 - level) / 2 by numpy's default (linear) rule.
 * Calls on one plan must not overlap. */
typedef struct tphip_bootstrap_opts {
    uint32_t struct_size;      /* sizeof(tphip_bootstrap_opts) of the caller */
    int32_t replicates;        /* B, 2..4096 */
    double level;              /* coverage of [lo, hi], in (0, 1) */
    uint64_t seed;
    const int64_t *locus_ids;  /* HOST [nloci] stream id per locus, NULL = the plan's locus index 0..L-1; read before the
                                  call returns */
} tphip_bootstrap_opts;

/* Wb = T + n_i */
int32_t tphip_bootstrap_width(const tphip_plan *plan);
/* Device workspace of tphip_pi_bootstrap_dev: any size >= *min_bytes works and gives the same bits (the library blocks over
 * loci and, for a locus too long for the workspace, over replicate ranges); *preferred_bytes (<= about 1 GiB, or the
 * minimum) lets it take more loci per block.  opts = NULL sizes the workspace of tphip_pi_resample_dev instead, which holds
 * per-site integrals only and does not depend on nrep (a bootstrap workspace is always large enough for it too).
 * Alignment: none.  The replicate-band calls (tphip_pi_resample_dev, tphip_pi_bootstrap_dev, tphip_posterior_pi_dev,
 * tphip_pi_parametric_bootstrap_dev) start at the first multiple of 256 in d_workspace; *min_bytes, *preferred_bytes and
 * tphip_parboot_workspace_bytes() already contain the 256 bytes that can cost, so a workspace of exactly *min_bytes at an odd
 * address is enough. */
int tphip_bootstrap_workspace_bytes(const tphip_plan *plan, const tphip_bootstrap_opts *opts, size_t *min_bytes,
                                    size_t *preferred_bytes);
/* The weighted-sum core on caller-supplied counts (jackknife, delete-half, site weighting): d_counts is uint16
 * [nrep][ncols] over the plan's columns, d_rows [nloci][nrep][Wb].  Enqueues on `stream`, does not synchronise. */
int tphip_pi_resample_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres, const uint16_t *d_counts,
                          int32_t nrep, double *d_rows, void *d_workspace, size_t workspace_bytes, void *stream);
/* Draws the counts, runs the core and summarises, block by block.  d_summary [nloci][4][Wb]; d_rows [nloci][B][Wb] or NULL.
 * Enqueues on `stream` and does not synchronise when opts.locus_ids is NULL.  With locus_ids set the ids are copied to the
 * device first and `stream` is synchronised once before any kernel is enqueued (the caller's array need not outlive the
 * call): such a call blocks and cannot be captured into a graph. */
int tphip_pi_bootstrap_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres, const tphip_bootstrap_opts *opts,
                           double *d_summary, double *d_rows, void *d_workspace, size_t workspace_bytes, void *stream);
/* host-pointer twins: the library allocates its own workspace, as tphip_pi_tables does */
int tphip_pi_resample(tphip_plan *plan, const double *rates, const int32_t *nres, const uint16_t *counts, int32_t nrep,
                      double *rows);
int tphip_pi_bootstrap(tphip_plan *plan, const double *rates, const int32_t *nres, const tphip_bootstrap_opts *opts,
                       double *summary, double *rows);
/* The draw kernel alone (host pointers, plan-less): counts_out uint16 [nrep][n] = the counts of replicates rep0 .. rep0 +
 * nrep - 1 of a locus of n columns with stream id locus_id. */
int tphip_bootstrap_counts(int32_t device, uint64_t seed, int64_t locus_id, int64_t n, int64_t rep0, int32_t nrep,
                           uint16_t *counts_out);

/* ------------------------------------------------------------------------------------------------
 * Quartet signal and noise (an extension: Townsend, Su & Tekle 2012; Su et al. 2014).  For the four-taxon tree
 * ((a:T, b:T)u, (c:T, d:T)v) with the internode u-v of length t_o, both in the tree's original time units, a site of final
 * rate r under the locus' model normalised to one substitution has M = exp(Q r T / kappa), N = exp(Q r t_o / kappa) and,
 * with w_xy = pi_x N_xy,
 *   signal y = sum_xy w_xy sum_{i != j} M_xi^2 M_yj^2              (tip pattern iijj)
 *   noise  x = sum_xy w_xy 2 sum_{i < j} (M_xi M_yi)(M_xj M_yj)    (tip pattern ijij; ijji has the same probability).
 * A NaN (culled) or zero rate gives exactly 0 for both.  Inputs are those of tphip_pi_tables: raw rates and an optional
 * nres, finalised by the plan's rounding, correction and cull; the models are the plan's (GTR or F81).
 *
 * Row per (locus, quartet), 8 doubles, rows [nloci][n_q][8]: Y = sum y, X = sum x, Yy = sum y^2, Xx = sum x^2,
 * XY = sum x y over the locus' columns, then p_correct, p_incorrect, p_polytomy: the probabilities that the locus' counts
 * of signal sites S and of the two kinds of noise sites N1, N2 give S - N > 0.5 for both, N - S > 0.5 with that N ahead of the
 * other, or neither -- by a bivariate-normal approximation with continuity correction (Var S = Y - Yy, Var N = X - Xx,
 * Cov(S, N) = -XY, Cov(N1, N2) = -Xx; 64-point Gauss-Legendre for the bivariate integral); (0, 0, 1) when the variance is 0.
 *
 * Determinism: a row depends on the locus' final rates, its model and the quartet's (T, t_o) only -- not on the other loci
 * of the plan, on the other quartets of the list or on how a batch is sharded.  Calls on one plan must not overlap. */
typedef struct tphip_quartet_opts {
    uint32_t struct_size;      /* sizeof(tphip_quartet_opts) of the caller */
    int32_t n_q;               /* quartets, 1..256 */
    const double *tip;         /* HOST [n_q] T >= 0; read before the call returns */
    const double *internode;   /* HOST [n_q] t_o > 0; read before the call returns */
} tphip_quartet_opts;

/* bytes of device workspace (8-byte aligned) tphip_quartet_tables_dev needs for these options */
int tphip_quartet_workspace_bytes(const tphip_plan *plan, const tphip_quartet_opts *opts, size_t *bytes);
/* d_rows [nloci][n_q][8].  Enqueues on `stream`, does not synchronise. */
int tphip_quartet_tables_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres, const tphip_quartet_opts *opts,
                             double *d_rows, void *d_workspace, size_t workspace_bytes, void *stream);
/* the per-site values: d_sites [2][n_q][ncols], y then x.  Enqueues on `stream`, does not synchronise. */
int tphip_quartet_sites_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres, const tphip_quartet_opts *opts,
                            double *d_sites, void *stream);
/* host-pointer twins: the library allocates its own buffers, as tphip_pi_tables does */
int tphip_quartet_tables(tphip_plan *plan, const double *rates, const int32_t *nres, const tphip_quartet_opts *opts,
                         double *rows);
int tphip_quartet_sites(tphip_plan *plan, const double *rates, const int32_t *nres, const tphip_quartet_opts *opts,
                        double *sites);

/* ------------------------------------------------------------------------------------------------
 * Quartet signal and noise with unequal tips (an extension: Su & Townsend 2015).  The four-taxon tree is
 * ((a:Ta, b:Tb)u, (c:Tc, d:Td)v) with the internode u-v of length t_o, all in the tree's original time units.  A site of
 * final rate r under the locus' model normalised to one substitution has A = P(r Ta), B = P(r Tb), C = P(r Tc), D = P(r Td),
 * N = P(r t_o), P(tau) = exp(Q tau / kappa), and with R_u[i][j] = sum_v N_uv C_vi D_vj and i != j throughout
 *   signal y  = sum_u pi_u sum_i A_ui B_ui sum_{j != i} R_u[j][j]   (tip pattern iijj, supports ab|cd)
 *   noise  x1 = sum_u pi_u sum_{i != j} A_ui B_uj R_u[i][j]         (tip pattern ijij, supports ac|bd)
 *   noise  x2 = sum_u pi_u sum_{i != j} A_ui B_uj R_u[j][i]         (tip pattern ijji, supports ad|bc).
 * A NaN (culled) or zero rate gives exactly 0 for all three; all tips 0 gives x1 = x2 = 0 exactly.  Inputs are those of
 * tphip_quartet_tables.
 *
 * Row per (locus, quartet), 13 doubles, rows [nloci][n_q][13]: the sums over the locus' columns of y, x1, x2, y^2, x1^2,
 * x2^2, y x1, y x2, x1 x2, then p_correct, p_ac, p_ad, p_polytomy: the probabilities that the count of signal sites S, of
 * ijij sites N1 or of ijji sites N2 ends more than 0.5 ahead of both others, or that none does -- by the bivariate-normal
 * approximation of the section above (Var = sum - sum of squares, Cov = -(cross sum); the correlation is clamped to
 * [-0.999, 0.999] for p_correct and to [-0.999, 0.99] for the wrong topologies where the two thresholds differ);
 * (0, 0, 0, 1) for an empty or fully culled locus.
 *
 * Determinism: a row depends on the locus' final rates, its model and the quartet's (Ta, Tb, Tc, Td, t_o) only -- not on the
 * other loci of the plan, on the other quartets of the list or on how a batch is sharded.  Calls on one plan must not overlap.
 * Errors are TPHIP_ERR_INVALID throughout, a workspace below tphip_unequal_quartet_workspace_bytes() included. */
typedef struct tphip_unequal_quartet_opts {
    uint32_t struct_size;      /* sizeof(tphip_unequal_quartet_opts) of the caller */
    int32_t n_q;               /* quartets, 1..256 */
    const double *tips;        /* HOST [n_q][4] Ta, Tb, Tc, Td >= 0; read before the call returns */
    const double *internode;   /* HOST [n_q] t_o > 0; read before the call returns */
} tphip_unequal_quartet_opts;

/* bytes of device workspace (8-byte aligned) tphip_unequal_quartet_tables_dev needs for these options */
int tphip_unequal_quartet_workspace_bytes(const tphip_plan *plan, const tphip_unequal_quartet_opts *opts, size_t *bytes);
/* d_rows [nloci][n_q][13].  Enqueues on `stream`, does not synchronise. */
int tphip_unequal_quartet_tables_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres,
                                     const tphip_unequal_quartet_opts *opts, double *d_rows, void *d_workspace,
                                     size_t workspace_bytes, void *stream);
/* the per-site values: d_sites [3][n_q][ncols], y, x1, x2.  Enqueues on `stream`, does not synchronise. */
int tphip_unequal_quartet_sites_dev(tphip_plan *plan, const double *d_rates, const int32_t *d_nres,
                                    const tphip_unequal_quartet_opts *opts, double *d_sites, void *stream);
/* host-pointer twins: the library allocates its own buffers, as tphip_pi_tables does */
int tphip_unequal_quartet_tables(tphip_plan *plan, const double *rates, const int32_t *nres,
                                 const tphip_unequal_quartet_opts *opts, double *rows);
int tphip_unequal_quartet_sites(tphip_plan *plan, const double *rates, const int32_t *nres,
                                const tphip_unequal_quartet_opts *opts, double *sites);

/* ------------------------------------------------------------------------------------------------
 * Exact quartet resolution probabilities (an extension): the law of the counts themselves in place of the bivariate-normal
 * approximation of the two sections above.  Input: the dense per-site planes y, x1, x2, each [n_q][ncols], exactly as
 * tphip_unequal_quartet_sites_dev writes them (d_sites, d_sites + n_q * ncols, d_sites + 2 * n_q * ncols); an equal-tip
 * quartet passes the x plane of tphip_quartet_sites_dev for both x1 and x2.  The plan gives the loci's column ranges and the
 * device; its models and rates play no part.  Every entry must be a probability (y, x1, x2 >= 0, y + x1 + x2 <= 1).
 *
 * Per site, independently, (D1, D2) = (S - N1, S - N2) moves by (+1, +1) with probability y, by (-1, 0) with x1, by (0, -1)
 * with x2 and not at all otherwise.  The characteristic function on the M x M torus, Phi[k1, k2] = prod over the locus'
 * sites of (p0 + y z1 z2 + x1 conj(z1) + x2 conj(z2)), z_j = exp(2 pi i k_j / M), is summed against the separable weights of
 * the regions  correct: D1 > 0 and D2 > 0;  ac: D1 < 0 and D1 < D2;  ad: D2 < 0 and D2 < D1;  polytomy: the rest  -- over
 * windows of M values centred at the rounded means of D1, D2 and D2 - D1.  M is the smallest of 16, 32, ..., window_cap for
 * which Bernstein's bound on the mass outside the windows,
 *   tail_bound = sum over V in {Var D1, Var D2, Var (D2 - D1)} of 2 exp(-t^2 / (2 (V + t / 3))),  t = M / 2 - 1
 * (a variance of exactly 0 adds nothing), is at most tail_tolerance.
 *
 * Row per (locus, quartet), 6 doubles, rows [nloci][n_q][6]: p_correct, p_ac, p_ad, p_polytomy, window (M), tail_bound.  The
 * probabilities are exact up to tail_bound and rounding, each clamped to [0, 1], p_polytomy = max(0, 1 - the other three).
 * A pair for which no M up to window_cap meets the tolerance is not computed: NaN in the four probabilities, window = 0 and
 * tail_bound the bound at window_cap -- a truncated answer is never reported.  An empty or fully culled locus gives
 * (0, 0, 0, 1), window 16, tail_bound 0.
 *
 * Determinism: a row depends on its locus' planes and on window_cap and tail_tolerance only -- not on the other loci of the
 * plan, on the other quartets of the call or their order, on how a batch is sharded or on the GPU count.  Every sum has a
 * fixed shape and order; there are no floating-point atomics.  Calls on one plan may overlap if their workspaces differ.
 * Errors are TPHIP_ERR_INVALID throughout, a workspace below tphip_quartet_exact_workspace_bytes() included; nloci * n_q is
 * at most 2^24 per call. */
typedef struct tphip_quartet_exact_opts {
    uint32_t struct_size;      /* sizeof(tphip_quartet_exact_opts) of the caller */
    int32_t n_q;               /* quartets: the planes' row count, 1..256 */
    int32_t window_cap;        /* largest M allowed: a power of two in 16..512; 0 = 128 */
    double tail_tolerance;     /* in (0, 1); 0 = 1e-12 */
} tphip_quartet_exact_opts;

/* bytes of device workspace (8-byte aligned) tphip_quartet_exact_dev needs for these options */
int tphip_quartet_exact_workspace_bytes(const tphip_plan *plan, const tphip_quartet_exact_opts *opts, size_t *bytes);
/* d_rows [nloci][n_q][6].  Enqueues on `stream`, does not synchronise, copies nothing: it can be captured. */
int tphip_quartet_exact_dev(tphip_plan *plan, const double *d_y, const double *d_x1, const double *d_x2,
                            const tphip_quartet_exact_opts *opts, double *d_rows, void *d_workspace, size_t workspace_bytes,
                            void *stream);
/* host-pointer twin: the library allocates its own buffers; x1 == x2 is uploaded once */
int tphip_quartet_exact(tphip_plan *plan, const double *y, const double *x1, const double *x2,
                        const tphip_quartet_exact_opts *opts, double *rows);

/* ------------------------------------------------------------------------------------------------
 * Locus-set accumulation curves (an extension): how likely is a set of loci, analysed together, to resolve a quartet's
 * internode, and how many of the best loci are needed?  For quartet q the order o_q[0..n_k) lists distinct locus indices; the
 * set of size k is the concatenation of the columns of loci o_q[0] .. o_q[k-1].  Sites are independent, so the set's law is
 * that of one long locus: the per-locus probabilities do not combine, but the moment sums add and the characteristic
 * function is the product of the loci's.
 *
 * Normal rows (tphip_locus_set_rows): input the per-locus rows of tphip_quartet_tables ([nloci][n_q][8], family
 * TPHIP_LOCUS_SET_EQUAL) or of tphip_unequal_quartet_tables ([nloci][n_q][13], TPHIP_LOCUS_SET_UNEQUAL).  Row (q, k) of
 * rows [n_q][n_k][8 or 13], k = 1..n_k stored at index k - 1, has the layout of a per-locus row: its 5 or 9 sums are the
 * left-to-right sums of the loci's own sums in the order given, its probabilities the family's own rule applied to them.
 * The row k = 1 equals the per-locus row of locus o_q[0] bit for bit.
 *
 * Exact rows (tphip_locus_set_exact): input the per-site planes of tphip_quartet_exact.  All prefixes of a quartet share the
 * torus M = window_cap; the centres and the three variances of prefix k are the left-to-right sums over the order of the
 * loci's own six sums.  Prefix k is computed iff the tail bound of tphip_quartet_exact at M = window_cap is at most
 * tail_tolerance for it and for every prefix before it, and k <= n_head; a variance term is >= 0, so the computed prefixes
 * form a head k <= K_q.  Row (q, k) of rows [n_q][n_k][6]: p_correct, p_ac, p_ad, p_polytomy, window, tail_bound with the
 * regions, weights and clamps of tphip_quartet_exact; window = window_cap and tail_bound the bound at the cap for a computed
 * prefix.  A prefix that is not computed is never truncated: NaN in the four probabilities, window = 0, tail_bound the bound
 * at the cap.  When all three variances are 0 the row is read off the centres.
 *
 * Determinism: row (q, k) depends only on the per-locus rows, or the planes, of the first k loci of o_q in that order, and
 * (exact rows) on window_cap and tail_tolerance -- not on the loci after k, on n_k, on n_head as long as k <= n_head, on the
 * other quartets or their orders, on the workspace or on the GPU count.  No floating-point atomics.
 * Errors are TPHIP_ERR_INVALID throughout: a repeated or out-of-range index in `order` and a workspace below
 * tphip_locus_set_exact_workspace_bytes() included; nloci * n_q is at most 2^24 per call. */
#define TPHIP_LOCUS_SET_EQUAL 0
#define TPHIP_LOCUS_SET_UNEQUAL 1
typedef struct tphip_locus_set_opts {
    uint32_t struct_size;      /* sizeof(tphip_locus_set_opts) of the caller */
    int32_t n_q;               /* quartets, 1..256 */
    int32_t n_k;               /* K: entries of a quartet's order, 1..nloci */
    int32_t family;            /* TPHIP_LOCUS_SET_EQUAL or TPHIP_LOCUS_SET_UNEQUAL: the layout of the normal rows (the exact
                                  call reads planes and ignores it) */
    int32_t window_cap;        /* exact rows: M, a power of two in 16..512; 0 = 128 */
    double tail_tolerance;     /* exact rows: in (0, 1); 0 = 1e-12 */
    int32_t n_head;            /* exact rows: the most prefixes per quartet that are computed, 0 = n_k, else 1..n_k; it sizes
                                  the workspace, and prefixes beyond it are reported as not computed */
    const int32_t *order;     /* HOST [n_q][n_k] distinct locus indices per quartet; read and validated before the call
                                  returns */
} tphip_locus_set_opts;

/* d_locus_rows [nloci][n_q][8 or 13], d_rows [n_q][n_k][8 or 13] on `device`.  Needs no plan.  Enqueues its kernels on
 * `stream`; the order is copied to a buffer of the call's own, which is freed before the call returns (that waits for the
 * kernels). */
int tphip_locus_set_rows_dev(int32_t device, const double *d_locus_rows, int64_t nloci, const tphip_locus_set_opts *opts,
                             double *d_rows, void *stream);
/* host-pointer twin */
int tphip_locus_set_rows(int32_t device, const double *locus_rows, int64_t nloci, const tphip_locus_set_opts *opts,
                         double *rows);
/* bytes of device workspace (8-byte aligned) tphip_locus_set_exact_dev needs for these options (`order` is not read) */
int tphip_locus_set_exact_workspace_bytes(const tphip_plan *plan, const tphip_locus_set_opts *opts, size_t *bytes);
/* d_rows [n_q][n_k][6].  The order is validated, then written into the workspace by launches that carry it as kernel arguments
 * (960 indices each): the caller's array need not outlive the call.  Enqueues on `stream`, does not synchronise, copies nothing:
 * it can be captured; the head of every quartet is found on the device. */
int tphip_locus_set_exact_dev(tphip_plan *plan, const double *d_y, const double *d_x1, const double *d_x2,
                              const tphip_locus_set_opts *opts, double *d_rows, void *d_workspace, size_t workspace_bytes,
                              void *stream);
/* host-pointer twin: the library allocates its own buffers; x1 == x2 is uploaded once */
int tphip_locus_set_exact(tphip_plan *plan, const double *y, const double *x1, const double *x2,
                          const tphip_locus_set_opts *opts, double *rows);

/* ------------------------------------------------------------------------------------------------
 * Parametric bootstrap of the site rates and the PI rows (an extension).  The site bootstrap above resamples columns with
 * their rates held fixed; this one asks how noisy the rates themselves are: every column is simulated down the plan's tree
 * under the locus' model at the column's own rate, with the observed pattern of missing cells, its rate is re-estimated by
 * the site-rate stage and the PI row recomputed, B times.  The locus' model and the tree are held fixed -- there is no
 * stage-1 refit per replicate: the bands are conditional on the fitted substitution model.
 *
 * Simulation of column i of a locus with stream id `id`, replicate b, raw rate r (the unit of tphip_site_rates' rate,
 * kappa * s, used exactly as given, no rounding): the root's state is drawn from the locus' pi; a node with parent state x
 * and branch length t (the plan's) from row x of exp(Q r t / kappa) in the expm1 form of the quartet section (F81 in closed
 * form), so that r = 0 gives the identity exactly and every cell equals the root's state.  Draw d belongs to the node with
 * post-order index d: Philox4x32-10 with key ((seed & 0xffffffff) ^ 0x73696D75, seed >> 32) and counter
 * (i, b | ((d >> 1) << 16), id & 0xffffffff, id >> 32); u = (((x1 << 32) | x0) >> 11) * 2^-53 for an even d, the same from
 * (x3, x2) for an odd one.  Every node has its draw whether or not its cell is masked.  With the probabilities p[0..3]
 * (A, C, G, T) clamped at >= 0, c0 = p0, c1 = c0 + p1, c2 = c1 + p2, c3 = c2 + p3 and v = u * c3, the state is
 * (v >= c0) + (v >= c1) + (v >= c2): a state of probability exactly 0 is never drawn.  A NaN, infinite or negative r gives a
 * column of 15s.  With a mask (an alignment in the plan's layout, 0 read as 15) a cell whose mask byte is not one of
 * 1, 2, 4, 8 is copied through, every other cell is 1 << state; without one every cell is 1 << state.  Output: taxon-major
 * [ntaxa][ncols], the plan's layout.  Multifurcations work, the root's own branch length is ignored, column weights are
 * ignored.  Refused (TPHIP_ERR_INVALID): plans with ncat > 1, trees of 2^17 nodes or more or with more than 10240 internal
 * nodes (their 2-bit states no longer fit the LDS), b >= 65536.
 *
 * Determinism: a column's bytes depend on seed, id, i, b, r, the locus' model, the tree and the column's mask only -- not on
 * the other loci of the plan or on the launch shape.  Calls on one plan must not overlap. */
typedef struct tphip_simulate_opts {
    uint32_t struct_size;      /* sizeof(tphip_simulate_opts) of the caller */
    int32_t replicate;         /* b, 0..65535 */
    uint64_t seed;
    const int64_t *locus_ids;  /* HOST [nloci] stream id per locus, NULL = the plan's locus index; handled as by
                                  tphip_pi_bootstrap_dev: copied first, `stream` synchronised once */
} tphip_simulate_opts;

/* d_rates [ncols] raw rates; d_mask [ntaxa][ncols] or NULL; d_states_out [ntaxa][ncols].  Enqueues on `stream`. */
int tphip_simulate_columns_dev(tphip_plan *plan, const double *d_rates, const uint8_t *d_mask,
                               const tphip_simulate_opts *opts, uint8_t *d_states_out, void *stream);
int tphip_simulate_columns(tphip_plan *plan, const double *rates, const uint8_t *mask, const tphip_simulate_opts *opts,
                           uint8_t *states_out);

/* The replicate loop.  Per replicate b = 0..B-1: simulate with the observed alignment as mask; run the plan's site-rate stage
 * (de-duplication and start rule as the plan says) and its PI-table stage on the simulated states; copy net PI [0..T) and the
 * n_i integrals of every locus into rows[l][b][0..Wb), Wb = T + n_i (the layout of tphip_pi_bootstrap); fold every column's
 * final rate -- after the plan's rounding, correction and cull, what the PI stage sees -- into running moments (Welford, in
 * replicate order).  Then d_summary [nloci][4][Wb] = mean, sd, lo, hi as for tphip_pi_bootstrap.  d_rate_mean / d_rate_sd
 * [ncols] (B - 1 in the denominator) are NaN for a column whose final rate is NaN in any replicate; with the mask kept those
 * are exactly the culled columns.  d_rows [nloci][B][Wb], d_rate_mean and d_rate_sd may be NULL.  d_rates are the raw rates
 * the simulation runs at (NaN = a culled column: it comes out all missing and is culled again).
 * A site whose rate is 0 simulates constant and is estimated at 0 again: its mean and sd are exactly 0.
 * Errors are TPHIP_ERR_INVALID throughout, a workspace below tphip_parboot_workspace_bytes() included. */
typedef struct tphip_parboot_opts {
    uint32_t struct_size;      /* sizeof(tphip_parboot_opts) of the caller */
    int32_t replicates;        /* B, 2..4096 */
    double level;              /* coverage of [lo, hi], in (0, 1) */
    uint64_t seed;
    const int64_t *locus_ids;  /* as in tphip_simulate_opts */
} tphip_parboot_opts;

/* device workspace: one replicate of states, the per-column outputs of the site-rate stage, one table, the rows, the moments
 * and the plan's own workspace */
int tphip_parboot_workspace_bytes(const tphip_plan *plan, const tphip_parboot_opts *opts, size_t *bytes);
int tphip_pi_parametric_bootstrap_dev(tphip_plan *plan, const double *d_rates, const uint8_t *d_states_observed,
                                      const tphip_parboot_opts *opts, double *d_summary, double *d_rows,
                                      double *d_rate_mean, double *d_rate_sd, void *d_workspace, size_t workspace_bytes,
                                      void *stream);
/* host-pointer twin: the library allocates its own workspace */
int tphip_pi_parametric_bootstrap(tphip_plan *plan, const double *rates, const uint8_t *states_observed,
                                  const tphip_parboot_opts *opts, double *summary, double *rows, double *rate_mean,
                                  double *rate_sd);
/* The summary of tphip_pi_bootstrap on any rows [nloci][B][Wb] -> d_summary [nloci][4][Wb]: mean, sd (B - 1), and the
 * quantiles at (1 - level) / 2 and 1 - (1 - level) / 2 by numpy's default rule.  B in 2..4096.  Plan-less. */
int tphip_summarize_rows_dev(int32_t device, const double *d_rows, int64_t nloci, int32_t B, int32_t Wb, double level,
                             double *d_summary, void *stream);
int tphip_summarize_rows(int32_t device, const double *rows, int64_t nloci, int32_t B, int32_t Wb, double level,
                         double *summary);

/* ------------------------------------------------------------------------------------------------
 * Site concordance factors (an extension; Minh, Hahn & Lanfear 2020): what the alignment shows at an internode, beside what
 * the quartet sections predict for it.  Plan-less: the calls read the states, the loci's column ranges and the set tables.
 *
 * A set is four groups of taxon rows A, B | C, D.  counts[l][s] = (conc, disc1, disc2): summed over the columns of locus l,
 * the number of quartets (a, b, c, d) in A x B x C x D whose four cells are each exactly one base (mask 1, 2, 4 or 8) and
 * read xxyy (ab|cd), xyxy (ac|bd) or xyyx (ad|bc) with x != y.  A quartet with a gap, ?, N or an IUPAC union at the column is
 * not decisive there.  Per column the three numbers come from the groups' base counts a_x, b_x, c_x, d_x in closed form,
 * conc = (sum_x a_x b_x)(sum_y c_y d_y) - sum_x a_x b_x c_x d_x and the two other pairings likewise, in 64-bit integers (four
 * groups of 260 taxa pass 2^32 on one column); the sums over the columns wrap at 2^64.  Integer arithmetic throughout: the
 * counts do not depend on the launch, the loci beside a locus or the sets beside a set.
 *
 * Groups may be of any size >= 1 and name the taxa in any order; taxa may belong to no group of a set.  Refused
 * (TPHIP_ERR_INVALID, before any device is touched): n_sets < 1, ntaxa < 4, an empty group, a taxon row outside 0..ntaxa-1, a
 * taxon listed twice within one set, row_pitch < ncols_total. */
typedef struct tphip_concordance_sets {
    uint32_t struct_size;         /* sizeof(tphip_concordance_sets) of the caller */
    int64_t n_sets;
    const int64_t *group_offsets; /* HOST [4 * n_sets + 1]: CSR into group_taxa; groups A, B, C, D of set s are 4s .. 4s+3 */
    const int32_t *group_taxa;    /* HOST taxon rows */
} tphip_concordance_sets;

/* d_states [ntaxa][row_pitch] (row_pitch >= ncols_total: the rows may be longer than the batch), d_locus_offsets [nloci + 1],
 * d_counts [nloci][n_sets][3].  Enqueues on `stream`; the set tables are copied to a buffer of the call's own, which is freed
 * before the call returns (that waits for the kernels). */
int tphip_concordance_counts_dev(int32_t device, const uint8_t *d_states, int64_t ncols_total, int64_t row_pitch,
                                 int32_t ntaxa, const int64_t *d_locus_offsets, int64_t nloci,
                                 const tphip_concordance_sets *sets, uint64_t *d_counts, void *stream);
/* host-pointer twin */
int tphip_concordance_counts(int32_t device, const uint8_t *states, int64_t ncols_total, int64_t row_pitch, int32_t ntaxa,
                             const int64_t *locus_offsets, int64_t nloci, const tphip_concordance_sets *sets,
                             uint64_t *counts);
/* The rows of the internodes: internode i owns the sets node_sets[i] .. node_sets[i + 1] - 1 (HOST [n_nodes + 1], at least two
 * each): the first is its pooled set (the whole groups), the second its nearest-tip quartet, the rest its sampled quartets.
 * d_rows [nloci][n_nodes][12] = pooled_c, pooled_1, pooled_2, near_c, near_1, near_2, sCF, sDF1, sDF2, sN, n_decisive,
 * n_quartets.  Over the sampled quartets with dec = c + d1 + d2 > 0, in set order: sCF = (sum c / dec) / n_decisive, sDF1 and
 * sDF2 likewise, sN = (sum dec) / n_decisive; each sum a sequential fp64 addition, one division at the end; fractions, not
 * percentages; NaN when n_decisive is 0.  The counts are converted to fp64 exactly when they are below 2^53, which is the
 * caller's to see to.  Handled as the counts call: node_sets is copied, `stream` waited for. */
int tphip_concordance_rows_dev(int32_t device, const uint64_t *d_counts, int64_t nloci, int64_t n_sets,
                               const int64_t *node_sets, int64_t n_nodes, double *d_rows, void *stream);
int tphip_concordance_rows(int32_t device, const uint64_t *counts, int64_t nloci, int64_t n_sets, const int64_t *node_sets,
                           int64_t n_nodes, double *rows);

#ifdef __cplusplus
}
#endif
#endif /* TPHIP_H */

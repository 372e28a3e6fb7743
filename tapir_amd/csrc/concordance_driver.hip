// concordance_driver.hip -- site concordance factors: the C entry points tphip_concordance_counts /
// tphip_concordance_counts_dev (per locus and set of four taxon groups, the quartets its columns support each way) and
// tphip_concordance_rows / tphip_concordance_rows_dev (the per-internode rows from those counts).  The kernels are in
// concordance_kernels.hpp.  No plan: the calls read the states, the loci's column ranges and the set tables only.
//
// The set tables and node_sets are host arrays: they are validated here, before any device is touched, and copied into a buffer
// of the call's own, so a _dev call waits for its kernels before it returns and frees that buffer.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "concordance_kernels.hpp"
#include "tphip_internal.hpp"

namespace {

constexpr int64_t kCcMaxSets = (int64_t)65535 * kCcTile;   // the grid's second dimension

// The set tables as the kernel reads them: 32-bit offsets from the first group's start.  Refuses what the header says it refuses.
int cc_read_sets(const tphip_concordance_sets* s, int32_t ntaxa, std::vector<int32_t>* goff, const int32_t** taxa, size_t* n_taxa) {
    if (!s) return fail(TPHIP_ERR_INVALID, "null tphip_concordance_sets");
    if (s->struct_size < offsetof(tphip_concordance_sets, group_taxa) + sizeof(const int32_t*))
        return fail(TPHIP_ERR_INVALID, "tphip_concordance_sets.struct_size is too small: set it to sizeof(tphip_concordance_sets)");
    if (ntaxa < 4) return fail(TPHIP_ERR_INVALID, "ntaxa must be at least 4");
    if (s->n_sets < 1 || s->n_sets > kCcMaxSets) return fail(TPHIP_ERR_INVALID, "n_sets must be in 1..65535 * 1024");
    if (!s->group_offsets || !s->group_taxa) return fail(TPHIP_ERR_INVALID, "null set table");
    const int64_t n_groups = 4 * s->n_sets, base = s->group_offsets[0];
    if (base < 0) return fail(TPHIP_ERR_INVALID, "group_offsets: negative offset");
    goff->resize((size_t)n_groups + 1);
    for (int64_t g = 0; g <= n_groups; ++g) {
        const int64_t at = s->group_offsets[g];
        if (g && at <= s->group_offsets[g - 1]) return fail(TPHIP_ERR_INVALID, "group_offsets: an empty group (or offsets that decrease)");
        if (at - base > (int64_t)INT32_MAX) return fail(TPHIP_ERR_INVALID, "the sets name more than 2^31 - 1 taxa in all");
        (*goff)[(size_t)g] = (int32_t)(at - base);
    }
    *taxa = s->group_taxa + base;
    *n_taxa = (size_t)goff->back();
    std::vector<int64_t> seen((size_t)ntaxa, -1);
    for (int64_t q = 0; q < s->n_sets; ++q)
        for (int32_t t = (*goff)[(size_t)(4 * q)]; t < (*goff)[(size_t)(4 * q + 4)]; ++t) {
            const int32_t x = (*taxa)[t];
            if (x < 0 || x >= ntaxa) return fail(TPHIP_ERR_INVALID, "group_taxa: a taxon row is out of range");
            if (seen[(size_t)x] == q) return fail(TPHIP_ERR_INVALID, "group_taxa: a taxon is listed twice within one set");
            seen[(size_t)x] = q;
        }
    return TPHIP_OK;
}

int cc_check_batch(int64_t ncols_total, int64_t row_pitch, int64_t nloci) {
    if (ncols_total < 0 || nloci < 0) return fail(TPHIP_ERR_INVALID, "negative ncols_total or nloci");
    if (row_pitch < ncols_total) return fail(TPHIP_ERR_INVALID, "row_pitch is smaller than ncols_total");
    return TPHIP_OK;
}

int cc_check_node_sets(const int64_t* node_sets, int64_t n_nodes, int64_t n_sets) {
    if (n_nodes < 0 || n_sets < 0) return fail(TPHIP_ERR_INVALID, "negative n_nodes or n_sets");
    if (!node_sets) return fail(TPHIP_ERR_INVALID, "null node_sets");
    if (node_sets[0] < 0 || node_sets[n_nodes] > n_sets) return fail(TPHIP_ERR_INVALID, "node_sets: a set index is out of range");
    for (int64_t i = 0; i < n_nodes; ++i)
        if (node_sets[i + 1] - node_sets[i] < 2)
            return fail(TPHIP_ERR_INVALID, "node_sets: an internode needs its pooled set and its nearest-tip quartet");
    return TPHIP_OK;
}

}  // namespace

extern "C" {

int tphip_concordance_counts_dev(int32_t device, const uint8_t* d_states, int64_t ncols_total, int64_t row_pitch, int32_t ntaxa,
                                 const int64_t* d_locus_offsets, int64_t nloci, const tphip_concordance_sets* sets,
                                 uint64_t* d_counts, void* stream) {
    std::vector<int32_t> goff;
    const int32_t* taxa = nullptr;
    size_t n_taxa = 0;
    int rc = cc_read_sets(sets, ntaxa, &goff, &taxa, &n_taxa);
    if (rc) return rc;
    rc = cc_check_batch(ncols_total, row_pitch, nloci);
    if (rc) return rc;
    if (nloci == 0) return TPHIP_OK;
    if (!d_locus_offsets || !d_counts || (ncols_total && !d_states)) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_sets = sets->n_sets;
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint64_t) * 3 * (size_t)nloci * (size_t)n_sets, st));
    if (ncols_total == 0) return TPHIP_OK;
    Scratch S;   // freed on return: after the wait below
    int32_t* d_goff = S.get<int32_t>(goff.size());
    int32_t* d_taxa = S.get<int32_t>(n_taxa);
    if (!d_goff || !d_taxa) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpyAsync(d_goff, goff.data(), sizeof(int32_t) * goff.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_taxa, taxa, sizeof(int32_t) * n_taxa, hipMemcpyHostToDevice, st));
    CcParams P;
    P.states = d_states; P.ncols_total = ncols_total; P.row_pitch = row_pitch;
    P.locus_offsets = d_locus_offsets; P.nloci = nloci;
    P.goff = d_goff; P.taxa = d_taxa; P.n_sets = n_sets;
    P.counts = (unsigned long long*)d_counts;
    const dim3 grid((unsigned)((ncols_total + kCcChunk - 1) / kCcChunk), (unsigned)((n_sets + kCcTile - 1) / kCcTile));
    concordance_counts_kernel<<<grid, dim3(kCcBlock), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // the caller's tables and the copies of them have been read
    return TPHIP_OK;
}

int tphip_concordance_counts(int32_t device, const uint8_t* states, int64_t ncols_total, int64_t row_pitch, int32_t ntaxa,
                             const int64_t* locus_offsets, int64_t nloci, const tphip_concordance_sets* sets, uint64_t* counts) {
    std::vector<int32_t> goff;
    const int32_t* taxa = nullptr;
    size_t n_taxa = 0;
    int rc = cc_read_sets(sets, ntaxa, &goff, &taxa, &n_taxa);
    if (rc) return rc;
    rc = cc_check_batch(ncols_total, row_pitch, nloci);
    if (rc) return rc;
    if (nloci == 0) return TPHIP_OK;
    if (!locus_offsets || !counts || (ncols_total && !states)) return fail(TPHIP_ERR_INVALID, "null host pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    Staging S;
    // (the last row ends with its last column: the caller's array need not hold a whole pitch of it)
    const uint8_t* d_s = S.in(states, ncols_total ? (size_t)(ntaxa - 1) * (size_t)row_pitch + (size_t)ncols_total : 0);
    const int64_t* d_o = S.in(locus_offsets, (size_t)nloci + 1);
    uint64_t* d_c = S.out(counts, 3 * (size_t)nloci * (size_t)sets->n_sets);
    if (S.rc) return S.rc;
    rc = tphip_concordance_counts_dev(device, d_s, ncols_total, row_pitch, ntaxa, d_o, nloci, sets, d_c, nullptr);
    return rc ? rc : S.finish();
}

int tphip_concordance_rows_dev(int32_t device, const uint64_t* d_counts, int64_t nloci, int64_t n_sets, const int64_t* node_sets,
                               int64_t n_nodes, double* d_rows, void* stream) {
    int rc = cc_check_node_sets(node_sets, n_nodes, n_sets);
    if (rc) return rc;
    if (nloci < 0) return fail(TPHIP_ERR_INVALID, "negative nloci");
    if (nloci == 0 || n_nodes == 0) return TPHIP_OK;
    if (!d_counts || !d_rows) return fail(TPHIP_ERR_INVALID, "null device pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch S;
    int64_t* d_nodes = S.get<int64_t>((size_t)n_nodes + 1);
    if (!d_nodes) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpyAsync(d_nodes, node_sets, sizeof(int64_t) * ((size_t)n_nodes + 1), hipMemcpyHostToDevice, st));
    CcRowsParams P;
    P.counts = (const unsigned long long*)d_counts; P.nloci = nloci; P.n_sets = n_sets; P.n_nodes = n_nodes;
    P.node_sets = d_nodes; P.rows = d_rows;
    const int64_t n = nloci * n_nodes;
    concordance_rows_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // the caller's node_sets and the copy of it have been read
    return TPHIP_OK;
}

int tphip_concordance_rows(int32_t device, const uint64_t* counts, int64_t nloci, int64_t n_sets, const int64_t* node_sets,
                           int64_t n_nodes, double* rows) {
    int rc = cc_check_node_sets(node_sets, n_nodes, n_sets);
    if (rc) return rc;
    if (nloci < 0) return fail(TPHIP_ERR_INVALID, "negative nloci");
    if (nloci == 0 || n_nodes == 0) return TPHIP_OK;
    if (!counts || !rows) return fail(TPHIP_ERR_INVALID, "null host pointer");
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    HIP_TRY(hipSetDevice(device));
    Staging S;
    const uint64_t* d_c = S.in(counts, 3 * (size_t)nloci * (size_t)n_sets);
    double* d_r = S.out(rows, (size_t)kCcRow * (size_t)nloci * (size_t)n_nodes);
    if (S.rc) return S.rc;
    rc = tphip_concordance_rows_dev(device, d_c, nloci, n_sets, node_sets, n_nodes, d_r, nullptr);
    return rc ? rc : S.finish();
}

}  // extern "C"

// pattern_driver.hip -- unique site patterns of a batch of loci with their counts (pattern_kernels.hpp around hipcub's radix
// sort and scan): tphip_compress_columns on host pointers and its device-to-device twin for stage 1.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pattern_kernels.hpp"
#include <hipcub/hipcub.hpp>
#include "tphip_internal.hpp"

extern "C" {

// Unique site patterns of device-resident columns (see tphip_compress_columns): temporaries in `tmp`, results in `keep`.
static int compress_core(const uint8_t* d_s, int64_t ncols_total, int32_t ntaxa, const int64_t* d_off, int64_t nloci, bool want_map,
                         Scratch& tmp, Scratch& keep, uint8_t** d_out_p, int64_t** d_newoff_p, double** d_w_p, int64_t** d_map_p,
                         int64_t* npat_p) {
    const size_t n = (size_t)ncols_total;
    const int32_t nwords = (ntaxa + 7) / 8;
    uint32_t* d_packed = tmp.get<uint32_t>(n * (size_t)nwords);
    uint64_t* d_key = tmp.get<uint64_t>(n);
    uint64_t* d_key2 = tmp.get<uint64_t>(n);
    uint64_t* d_h2 = tmp.get<uint64_t>(n);
    uint64_t* d_h2_sorted = tmp.get<uint64_t>(n);
    uint32_t* d_col = tmp.get<uint32_t>(n);
    uint32_t* d_col2 = tmp.get<uint32_t>(n);
    int32_t* d_head = tmp.get<int32_t>(n);
    int64_t* d_incl = tmp.get<int64_t>(n);
    int64_t* d_newoff = keep.get<int64_t>((size_t)nloci + 1);
    int64_t* d_map = want_map ? keep.get<int64_t>(n) : nullptr;
    if (!d_packed || !d_key || !d_key2 || !d_h2 || !d_h2_sorted || !d_col || !d_col2 || !d_head || !d_incl || !d_newoff || (want_map && !d_map))
        return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    const unsigned blocks = (unsigned)((n + 255) / 256);
    pack_hash_kernel<<<dim3(blocks), dim3(256)>>>(d_s, ncols_total, ntaxa, nwords, d_off, nloci, d_packed, d_key, d_h2, d_col);
    HIP_TRY(hipGetLastError());
    int locus_bits = 1;
    while (((int64_t)1 << locus_bits) < nloci) ++locus_bits;
    const int end_bit = std::min(64, kPatHashBits + locus_bits);
    // Two stable passes: by the second hash, then by the key.  Within a key the positions are then ordered by hash 2 and, within
    // that, by column, so equal columns stay adjacent even when another pattern of their locus shares the 40-bit key (sorted by
    // the key alone, A B A B A would stay interleaved and head_flag_kernel, which looks at the predecessor only, would start
    // five patterns).
    size_t tmp_sort2 = 0, tmp_sort = 0, tmp_scan = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort2, d_h2, d_h2_sorted, d_col, d_col2, (int)n, 0, 64));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, d_key2, d_key, d_col2, d_col, (int)n, 0, end_bit));
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, d_head, d_incl, (int)n));
    const size_t tmp_bytes = std::max(std::max(tmp_sort2, tmp_sort), tmp_scan);
    void* d_tmp = tmp.get<char>(tmp_bytes);
    if (!d_tmp) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_sort2, d_h2, d_h2_sorted, d_col, d_col2, (int)n, 0, 64));
    gather_key_kernel<<<dim3(blocks), dim3(256)>>>(d_key, d_col2, ncols_total, d_key2);   // the keys in hash-2 order
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_sort, d_key2, d_key, d_col2, d_col, (int)n, 0, end_bit));
    head_flag_kernel<<<dim3(blocks), dim3(256)>>>(d_key, d_col, d_h2, d_packed, nwords, ncols_total, d_head);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tmp_scan, d_head, d_incl, (int)n));
    int64_t npat = 0;
    HIP_TRY(hipMemcpy(&npat, d_incl + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost));
    uint8_t* d_out = keep.get<uint8_t>((size_t)npat * (size_t)ntaxa);
    int32_t* d_count = tmp.get<int32_t>((size_t)npat);
    double* d_w = keep.get<double>((size_t)npat);
    if (!d_out || !d_count || !d_w) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemset(d_count, 0, sizeof(int32_t) * (size_t)npat));
    pattern_scatter_kernel<<<dim3(blocks), dim3(256)>>>(d_col, d_head, d_incl, d_packed, nwords, ntaxa, ncols_total, npat, d_out,
                                                      d_count, d_map);
    pattern_offsets_kernel<<<dim3((unsigned)((nloci + 256) / 256)), dim3(256)>>>(d_off, nloci, ncols_total, d_incl, npat, d_newoff);
    count_to_weight_kernel<<<dim3((unsigned)((npat + 255) / 256)), dim3(256)>>>(d_count, npat, d_w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    *d_out_p = d_out; *d_newoff_p = d_newoff; *d_w_p = d_w; *npat_p = npat;
    if (d_map_p) *d_map_p = d_map;
    return TPHIP_OK;
}

// device-to-device twin for the other translation units (stage1_driver.hip); the three result arrays are the caller's to hipFree
int tphip_internal_compress_dev(const uint8_t* d_s, int64_t ncols_total, int32_t ntaxa, const int64_t* d_off, int64_t nloci,
                                uint8_t** d_out, int64_t** d_newoff, double** d_w, int64_t* npat) {
    if (ncols_total >= ((int64_t)1 << 31)) return fail(TPHIP_ERR_INVALID, "too many columns for one call (2^31)");
    if (nloci >= ((int64_t)1 << (64 - kPatHashBits))) return fail(TPHIP_ERR_INVALID, "too many loci for one call");
    Scratch tmp, keep;
    int rc = compress_core(d_s, ncols_total, ntaxa, d_off, nloci, false, tmp, keep, d_out, d_newoff, d_w, nullptr, npat);
    if (!rc) keep.bufs.clear();   // ownership passes to the caller
    return rc;
}

int tphip_compress_columns(int32_t device, const uint8_t* states, int64_t ncols_total, int32_t ntaxa,
                           const int64_t* locus_offsets, int64_t nloci, uint8_t* out_states, int64_t* out_offsets,
                           double* out_weight, int64_t* out_map, int64_t* out_npatterns) {
    if (tphip_device_count() <= 0) return fail(TPHIP_ERR_NO_DEVICE, "no HIP device visible: libtphip has no CPU path");
    if (!states || !locus_offsets || !out_states || !out_offsets || !out_weight || !out_npatterns || nloci < 1 || ntaxa < 1 ||
        ncols_total < 0)
        return fail(TPHIP_ERR_INVALID, "bad arguments");
    if (ncols_total >= ((int64_t)1 << 31)) return fail(TPHIP_ERR_INVALID, "too many columns for one call (2^31)");
    if (nloci >= ((int64_t)1 << (64 - kPatHashBits))) return fail(TPHIP_ERR_INVALID, "too many loci for one call");
    if (locus_offsets[0] != 0 || locus_offsets[nloci] != ncols_total) return fail(TPHIP_ERR_INVALID, "locus_offsets must span the columns");
    for (int64_t l = 0; l < nloci; ++l)
        if (locus_offsets[l + 1] < locus_offsets[l]) return fail(TPHIP_ERR_INVALID, "locus_offsets must not decrease");
    if (ncols_total == 0) {
        for (int64_t l = 0; l <= nloci; ++l) out_offsets[l] = 0;
        *out_npatterns = 0;
        return TPHIP_OK;
    }
    HIP_TRY(hipSetDevice(device));
    Scratch S, K;
    const size_t n = (size_t)ncols_total;
    uint8_t* d_s = S.get<uint8_t>(n * (size_t)ntaxa);
    int64_t* d_off = S.get<int64_t>((size_t)nloci + 1);
    if (!d_s || !d_off) return fail(TPHIP_ERR_HIP, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_s, states, n * (size_t)ntaxa, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off, locus_offsets, sizeof(int64_t) * ((size_t)nloci + 1), hipMemcpyHostToDevice));
    uint8_t* d_out = nullptr; int64_t* d_newoff = nullptr; double* d_w = nullptr; int64_t* d_map = nullptr; int64_t npat = 0;
    int rc = compress_core(d_s, ncols_total, ntaxa, d_off, nloci, out_map != nullptr, S, K, &d_out, &d_newoff, &d_w, &d_map, &npat);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_states, d_out, (size_t)npat * (size_t)ntaxa, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_offsets, d_newoff, sizeof(int64_t) * ((size_t)nloci + 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_weight, d_w, sizeof(double) * (size_t)npat, hipMemcpyDeviceToHost));
    if (out_map) HIP_TRY(hipMemcpy(out_map, d_map, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    *out_npatterns = npat;
    return TPHIP_OK;
}

}  // extern "C"

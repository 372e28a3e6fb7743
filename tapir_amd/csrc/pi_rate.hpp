// pi_rate.hpp -- the PI stage's parameter block and the rate it sees per column: the stage-1 rate after the JSON round
// trip, the correction and the informative-site cull.  Shared by the PI-table kernels (pi_kernels.hpp) and the resampling
// kernels (bootstrap_kernels.hpp), so that both finalise a column's rate with the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace tphip {

struct PiParams {
    const double* rates;       // raw stage-1 rates (kappa * s) or user-supplied rates
    const int32_t* nres;       // may be null (no cull)
    const int64_t* locus_offsets;
    const int32_t* chunk_locus;
    const int32_t* chunk_index;
    int32_t T;
    const int32_t* intervals;  // [n_i][2]
    int32_t n_i;
    int32_t integ_mode;
    double correction;
    int32_t threshold;
    double round_scale;        // 10^decimals, or 0 for no rounding
    double* partial;           // [nchunks][T + 2 n_i]
};

// rate as tapir sees it after the JSON round trip, the /correction and the cull
// (bf:1093-1095 Format(x,0,4); tapir/compute.py:38-39; tapir/compute.py:96-110)
// HyPhy writes Format(x,0,4) (bf:1093-1095) and tapir parses the text back: the double nearest to the decimal that
// printf-style rounding of the EXACT binary value gives (ties to even).  rint(r * 10^4) / 10^4 is not that: the product
// is itself rounded, so it can land exactly on a half-integer the true product only comes close to (a false tie, decided
// by parity instead of by the discarded part) -- the rate would then differ by 1e-4 from what the .rates file says.
// The FMA recovers the discarded part exactly (r * scale = p + e), and only a half-integer p needs it: otherwise p is
// at least one ulp away from the half and |e| <= ulp/2 cannot carry it across.
// (Contraction must stay off here: fused into fma(r, scale, -n), "p - n" would be the exact product minus n, never
// exactly 0.5 on a false tie, and the correction below would never fire.)
__host__ __device__ __forceinline__ double round_like_printf(double r, double scale) {
#pragma clang fp contract(off)
    const double p = r * scale;
    const double e = fma(r, scale, -p);
    double n = rint(p);
    if (fabs(p - n) == 0.5 && e != 0.0) n = (e > 0.0) ? p + 0.5 : p - 0.5;
    return n / scale;   // correctly rounded quotient of two exact doubles = strtod of the decimal string
}

__device__ __forceinline__ double finalize_rate(const PiParams& P, int64_t col) {
    double r = P.rates[col];
    if (P.round_scale > 0.0) r = round_like_printf(r, P.round_scale);
    r = r / P.correction;
    if (P.nres && P.nres[col] < P.threshold) r = __longlong_as_double(0x7ff8000000000000ll);
    return r;
}

}  // namespace tphip

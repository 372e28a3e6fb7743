// quartet_probabilities.hpp -- the resolution probabilities of an equal-tip quartet from its five moment sums (DESIGN section
// 3.6): the bivariate normal with continuity correction.  No __global__ definition, so that the per-locus rows
// (quartet_kernels.hpp: quartet_reduce_kernel) and the locus-set rows (locus_set_kernels.hpp: section 3.11) share one copy.
#pragma once
#include <hip/hip_runtime.h>

#include "quartet_common.hpp"

namespace tphip {

// (the 64-point Gauss-Legendre rule: kGl64X / kGl64W of quartet_common.hpp)
__device__ __forceinline__ double quartet_bvn_integrand(double h, double k, double theta) {
    const double s = sin(theta);
    if (h == k) return exp(-(k * k) / (1.0 + s));          // smooth up to rho = 1
    const double c = cos(theta);
    return exp(-((h * h + k * k) - 2.0 * h * k * s) / (2.0 * c * c));
}

// B(h, k, rho) = P(Z1 > h, Z2 > k) = Phi(-h) Phi(-k) + (1 / 2 pi) int_0^{asin rho} integrand d theta
__device__ __forceinline__ double quartet_bvn_upper(double h, double k, double rho) {
    const double half = 0.5 * asin(fmin(1.0, fmax(-1.0, rho)));
    double sum = 0.0;
    for (int i = 0; i < 32; ++i) {
        const double d = half * kGl64X[i];
        sum += kGl64W[i] * (quartet_bvn_integrand(h, k, half - d) + quartet_bvn_integrand(h, k, half + d));
    }
    const double tail = (0.5 * erfc(h * 0.70710678118654752440)) * (0.5 * erfc(k * 0.70710678118654752440));
    return fmax(0.0, tail + half * sum * 0.15915494309189533577);   // 1 / (2 pi); rho < 0: the two terms cancel, never below 0
}

// o[0..5): Y, X, Yy, Xx, XY; o[5..8) receive p_correct, p_incorrect, p_polytomy: (0, 0, 1) when the variance is 0.
__device__ __forceinline__ void quartet_probabilities(double* o) {
    const double Y = o[0], X = o[1], Yy = o[2], Xx = o[3], XY = o[4];
    const double varS = Y - Yy, varN = X - Xx;
    const double sigma2 = (varS + varN) + 2.0 * XY;
    double pc = 0.0, pw = 0.0, pp = 1.0;
    if (sigma2 > 0.0) {
        const double sigma = sqrt(sigma2);
        const double k = (0.5 - (Y - X)) / sigma;
        pc = quartet_bvn_upper(k, k, ((varS + 2.0 * XY) - Xx) / sigma2);
        if (X > 0.0) pw = 2.0 * quartet_bvn_upper((0.5 - (X - Y)) / sigma, 0.5 / sqrt(2.0 * X), fmin(sqrt(X / 2.0) / sigma, 0.99));
        pp = fmax(0.0, (1.0 - pc) - pw);
    }
    o[5] = pc;
    o[6] = pw;
    o[7] = pp;
}

}  // namespace tphip

// unequal_quartet_probabilities.hpp -- the resolution probabilities of a quartet with unequal tips from its nine moment sums
// (DESIGN section 3.8): the bivariate normal with continuity correction in the form that does not cancel near theta = pi / 2.
// No __global__ definition, so that the per-locus rows (unequal_quartet_kernels.hpp: uquartet_reduce_kernel) and the
// locus-set rows (locus_set_kernels.hpp: section 3.11) share one copy.
#pragma once
#include <hip/hip_runtime.h>

#include "quartet_common.hpp"

namespace tphip {

// (the rule and constants of section 3.6: kGl64X / kGl64W of quartet_common.hpp)

// h != k: (h - k)^2 / (2 cos^2) + h k / (1 + sin) is (h^2 + k^2 - 2 h k sin) / (2 cos^2) without that numerator's
// cancellation near theta = pi / 2
__device__ __forceinline__ double uquartet_bvn_integrand(double h, double k, double theta) {
    const double s = sin(theta);
    if (h == k) return exp(-(k * k) / (1.0 + s));          // smooth up to rho = 1
    const double c = cos(theta);
    const double d = h - k;
    return exp(-((d * d) / (2.0 * c * c) + (h * k) / (1.0 + s)));
}

// B(h, k, rho) = P(Z1 > h, Z2 > k) = Phi(-h) Phi(-k) + (1 / 2 pi) int_0^{asin rho} integrand d theta; rho already clamped
__device__ __forceinline__ double uquartet_bvn_upper(double h, double k, double rho) {
    const double half = 0.5 * asin(rho);
    double sum = 0.0;
    for (int i = 0; i < 32; ++i) {
        const double d = half * kGl64X[i];
        sum += kGl64W[i] * (uquartet_bvn_integrand(h, k, half - d) + uquartet_bvn_integrand(h, k, half + d));
    }
    const double tail = (0.5 * erfc(h * 0.70710678118654752440)) * (0.5 * erfc(k * 0.70710678118654752440));
    return fmax(0.0, tail + half * sum * 0.15915494309189533577);   // 1 / (2 pi); rho < 0: the two terms cancel, never below 0
}

// The probability that W ends strictly ahead of O1 and of O2.  e / var: expectation and variance of the three counts,
// w_o1, w_o2, o1_o2: the cross sums (Cov = -cross sum).  cap: the upper clamp of rho where h != k.
__device__ __forceinline__ double uquartet_win(double eW, double eO1, double eO2, double varW, double varO1, double varO2,
                                               double w_o1, double w_o2, double o1_o2, double cap) {
    const double s1 = (varW + varO1) + 2.0 * w_o1;
    const double s2 = (varW + varO2) + 2.0 * w_o2;
    if (!(s1 > 0.0) || !(s2 > 0.0)) return 0.0;
    const double h = (0.5 - (eW - eO1)) / sqrt(s1);
    const double k = (0.5 - (eW - eO2)) / sqrt(s2);
    double rho = ((varW + (w_o1 + w_o2)) - o1_o2) / sqrt(s1 * s2);
    rho = fmin(1.0, fmax(-1.0, rho));
    if (h != k) rho = fmin(cap, fmax(-0.999, rho));
    return uquartet_bvn_upper(h, k, rho);
}

// o[0..9): the sums of y, x1, x2, y^2, x1^2, x2^2, y x1, y x2, x1 x2; o[9..13) receive p_correct, p_ac, p_ad, p_polytomy.
__device__ __forceinline__ void uquartet_probabilities(double* o) {
    const double Y = o[0], X1 = o[1], X2 = o[2], yx1 = o[6], yx2 = o[7], x1x2 = o[8];
    const double vS = Y - o[3], v1 = X1 - o[4], v2 = X2 - o[5];
    const double pc = uquartet_win(Y, X1, X2, vS, v1, v2, yx1, yx2, x1x2, 0.999);
    const double p1 = X1 > 0.0 ? uquartet_win(X1, Y, X2, v1, vS, v2, yx1, x1x2, yx2, 0.99) : 0.0;
    const double p2 = X2 > 0.0 ? uquartet_win(X2, Y, X1, v2, vS, v1, yx2, x1x2, yx1, 0.99) : 0.0;
    o[9] = pc;
    o[10] = p1;
    o[11] = p2;
    o[12] = fmax(0.0, ((1.0 - pc) - p1) - p2);
}

}  // namespace tphip

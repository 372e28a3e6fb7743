// exact_quartet_window.hpp -- the window rule of the exact quartet resolution probabilities: which torus
// size M carries the law of (D1, D2, E) of a (locus, quartet) pair with all but `tol` of its mass, from the three variances
// alone.  Plain C++ (no HIP type), so that tests/native/exact_window_dump.cpp runs on the host what the moment kernel runs on
// the device.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TPHIP_EQ_HD __host__ __device__
#else
#define TPHIP_EQ_HD
#endif

namespace tphip {

constexpr int32_t kEqMinWindow = 16;
constexpr int32_t kEqMaxWindow = 512;
constexpr int32_t kEqDefaultWindow = 128;
constexpr double kEqDefaultTail = 1e-12;

TPHIP_EQ_HD inline bool exact_window_valid(int32_t m) { return m >= kEqMinWindow && m <= kEqMaxWindow && (m & (m - 1)) == 0; }

// Bernstein's inequality for a sum of independent variables in [-1, 1] about their means (each site moves a count by at most
// one): P(|D - E D| >= t) <= 2 exp(-t^2 / (2 (V + t / 3))).  A count of variance 0 is constant: it adds nothing.
TPHIP_EQ_HD inline double exact_tail_term(double var, double t) {
    if (!(var > 0.0)) return 0.0;
    return 2.0 * exp(-(t * t) / (2.0 * (var + t / 3.0)));
}

// The mass that may lie outside the windows [c - M/2, c + M/2) of D1, D2 and E, c the rounded mean: a count outside its
// window is at least t = M/2 - 1 (in fact M/2 - 1/2) from its mean.
TPHIP_EQ_HD inline double exact_tail_bound(double v1, double v2, double ve, int32_t m) {
    const double t = (double)(m / 2 - 1);
    return (exact_tail_term(v1, t) + exact_tail_term(v2, t)) + exact_tail_term(ve, t);
}

// The smallest M in {16, 32, ..., cap} with exact_tail_bound <= tol, or 0 when none qualifies; *bound: the bound at that M
// (at the cap when none qualifies).
TPHIP_EQ_HD inline int32_t exact_window(double v1, double v2, double ve, int32_t cap, double tol, double* bound) {
    double b = 0.0;
    for (int32_t m = kEqMinWindow; m <= cap; m *= 2) {
        b = exact_tail_bound(v1, v2, ve, m);
        if (b <= tol) {
            *bound = b;
            return m;
        }
    }
    *bound = b;
    return 0;
}

}  // namespace tphip

// transition_row.hpp -- rows of P(tau) = exp(Q r tau / kappa) under a locus' model, in the form that stays accurate at
// r tau << 1.  Shared by the quartet kernels (quartet_kernels.hpp: all four rows) and the simulation kernel
// (simulate_kernels.hpp: the row of the parent's state), so that both compute an entry with the very same operations.
//
// expm1 form: I + sum_k U[:,k] expm1(lam_k s) U^-1[k,:], s = r tau / kappa, keeps the off-diagonal entries accurate relative
// to themselves when s << 1 ("accuracy at t s << 1").  F81: e I + (1 - e) Pi with 1 - e = -expm1(-s): no
// eigenvector enters, an absent base stays exactly absent.  At s = 0 both give the identity exactly.
//
// Written with explicit fma() under contract(off): an entry is a function of (model, s, row, column) alone, not of the
// kernel it is inlined into.
#pragma once
#include <hip/hip_runtime.h>

#include "gtr_model.hpp"

namespace tphip {

// s = r tau / kappa: the argument of the matrix exponential in units of the normalised generator
__device__ __forceinline__ double transition_scale(const LocusModel& m, double r, double tau) {
#pragma clang fp contract(off)
    return r * tau / m.kappa;
}

// What all rows of one matrix share.  GTR: e[k] = expm1(lam_k s); F81: e[0] = 1 - exp(-s), e[1] = exp(-s), e[2] unused.
__device__ __forceinline__ void transition_exps(const LocusModel& m, bool f81, double s, double* __restrict__ e) {
#pragma clang fp contract(off)
    if (f81) {
        e[0] = -expm1(-s);
        e[1] = 1.0 - e[0];
        e[2] = 0.0;
        return;
    }
    e[0] = expm1(m.lam[0] * s);
    e[1] = expm1(m.lam[1] * s);
    e[2] = expm1(m.lam[2] * s);
}

// one of four values by a row index that may differ between lanes: selects, so that a model held in scalar registers
// stays there (an index known at compile time folds them away)
__device__ __forceinline__ double transition_pick(int i, double a0, double a1, double a2, double a3) {
    return i == 0 ? a0 : i == 1 ? a1 : i == 2 ? a2 : a3;
}

// row i of the matrix whose shared part is e (transition_exps): row[j] = P_ij
__device__ __forceinline__ void transition_row(const LocusModel& m, bool f81, const double* __restrict__ e, int i,
                                               double* __restrict__ row) {
#pragma clang fp contract(off)
    if (f81) {
#pragma unroll
        for (int j = 0; j < 4; ++j) row[j] = (i == j) ? fma(e[0], m.pi[j], e[1]) : e[0] * m.pi[j];
        return;
    }
    const double a1 = transition_pick(i, m.U[0], m.U[3], m.U[6], m.U[9]) * e[0];
    const double a2 = transition_pick(i, m.U[1], m.U[4], m.U[7], m.U[10]) * e[1];
    const double a3 = transition_pick(i, m.U[2], m.U[5], m.U[8], m.U[11]) * e[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double v = fma(a3, m.Ui[8 + j], fma(a2, m.Ui[4 + j], a1 * m.Ui[j]));
        row[j] = (i == j) ? 1.0 + v : v;
    }
}

}  // namespace tphip

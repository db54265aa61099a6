// audit_block.h -- the per-record arithmetic of the leave-one-out audit of measurements that are in the graph,
// behind gate_relative: what k_audit (audit.hip) does with the relative pose and its covariance, in the primitives of gate_block.h.
// It compiles for the device and for the host, so the same text is checked on a machine without a GPU (tests/test_audit_host.py).
//
// A record is a measurement (i -> j, R~, t~, kappa, tau) that IS in the weighted graph, at weight w >= 0.  With R_ij, t_ij,
// Sigma_rel and xi of the gate (gate.hip):
//   scaling      s = (sqrt(2 kappa) x 3, sqrt(tau) x 3): diag(s)^2 = Sigma_meas^-1 = W0, the edge's Hessian at zero residual
//   whitened     z = s o xi,  C_ab = Sigma_rel,ab (s_a s_b), bitwise symmetric
//   matrices     A = I - w C (the redundancy matrix of the edge: PSD, singular where the graph knows a direction through this
//                edge alone),  B = I + (1 - w) C
//   redundancy   rho = 1 - w tr(C) / 6
//   testability  A = L L^T; p_min = the smallest pivot before the square root (pivots behind a non-positive one do not count);
//                testable when every pivot > min_redundancy
//   distance     u = A^-1 z by both triangular solves, v = B^-1 z by its own Cholesky, d2 = u^T v
//   left out     xi_loo = u / s, the innovation the edge would have shown had it been left out;
//                Sigma_loo = diag(1 / s) sym(A^-1 C) diag(1 / s) = (Sigma_rel^-1 - w W0)^-1, the relative covariance without it
//   failure      untestable, or a non-positive pivot of B: d2 = +inf, xi_loo = 0; untestable: Sigma_loo = 0 too
// In whitened coordinates taking w W0 out of the Hessian gives C_loo = A^-1 C and z_loo = A^-1 z (Woodbury), and the gate of
// those is z_loo^T (C_loo + I)^-1 z_loo = z^T A^-1 B^-1 z: A, B and C commute.  w = 0 is the gate itself; w = 1 the
// normalised residual.
#pragma once
#include "gate_block.h"

namespace dpgo {

constexpr int AUDIT_REC = 16;  // doubles of the measurement part of a record: R~ row-major (9), t~ (3), kappa, tau, w, one of padding

// what one record gives; sigma_loo is formed only where it is asked for
struct AuditOut {
  double xi[6], xi_loo[6], d2, rho, pmin;
  bool testable;
};

// One record.  M = R_ij, tij = t_ij, S = Sigma_rel (bitwise symmetric; overwritten), rec the AUDIT_REC doubles of the measurement.
// SIGMA: SL receives Sigma_loo, bitwise symmetric (else it is not touched).
template <bool SIGMA>
DPGO_HD void audit_record(const double M[3][3], const double tij[3], double S[6][6], const double *rec, double min_redundancy,
                          AuditOut &o, double SL[6][6]) {
  double v[AUDIT_REC];
  gate_load_pairs<AUDIT_REC / 2>(rec, v);
  const double w = v[14];
  gate_innovation(M, tij, v, o.xi);
  const double sr = sqrt(2.0 * v[12]), st = sqrt(v[13]);
  const double s[6] = {sr, sr, sr, st, st, st};
  const double isr = 1.0 / sr, ist = 1.0 / st;
  const double is[6] = {isr, isr, isr, ist, ist, ist};
  // C in S; A and B beside it
  double A[6][6], B[6][6], tr = 0.0;
  const double w1 = 1.0 - w;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      const double c = S[a][b] * (s[a] * s[b]), d = a == b ? 1.0 : 0.0;
      S[a][b] = S[b][a] = c;
      A[a][b] = A[b][a] = __builtin_fma(-w, c, d);
      B[a][b] = B[b][a] = __builtin_fma(w1, c, d);
      if (a == b) tr += c;
    }
  o.rho = __builtin_fma(-w, tr / 6.0, 1.0);
  bool okb;
  gate_cholesky(A, min_redundancy, o.testable, o.pmin);
  gate_cholesky(B, okb);
  double u[6], y[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) u[a] = y[a] = s[a] * o.xi[a];
  gate_solve(A, u);
  gate_solve(B, y);
  double dd = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) dd = __builtin_fma(u[a], y[a], dd);
  const bool ok = o.testable && okb;
  o.d2 = ok ? dd : (double)INFINITY;
#pragma unroll
  for (int a = 0; a < 6; ++a) o.xi_loo[a] = ok ? u[a] * is[a] : 0.0;
  if constexpr (SIGMA) {
    double X[6][6];  // A^-1 C, column by column
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double col[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) col[a] = S[a][b];
      gate_solve(A, col);
#pragma unroll
      for (int a = 0; a < 6; ++a) X[a][b] = col[a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) {
        const double x = 0.5 * (X[a][b] + X[b][a]) * (is[a] * is[b]);
        SL[a][b] = SL[b][a] = o.testable ? x : 0.0;
      }
  }
}

}  // namespace dpgo

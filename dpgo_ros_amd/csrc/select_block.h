// select_block.h -- the block arithmetic of the selection of candidate closures under a budget: what
// k_select_open and k_select_step (select.hip) do with the staged covariance blocks and with the rows of the factor, in the
// primitives of gate_block.h and gate_joint_block.h.  It compiles for the device and for the host, so the same text is checked on
// a machine without a GPU (tests/test_select_host.py).
//
// P candidates, candidate k joining the team poses i_k != j_k with the expected noise (kappa_k, tau_k); M = A Sigma A^T + R of
// gate_joint_block.h, of which only the diagonal blocks and, per selected pivot, one block column are ever formed.
//   gain        gain_k|A = (log det S_k|A - log det Sigma_meas,k) / 2 with S_k|A = M_kk - M_kA M_AA^-1 M_Ak and
//               log det Sigma_meas,k = -3 log(2 kappa_k) - 3 log tau_k; -inf where S_k|A has a non-positive pivot
//   rule        the open candidate of largest gain, the lower index on ties; -inf and NaN are never taken
//   elimination left-looking block Cholesky in the order the pivots are taken, the innovation left out.  With p the pivot of step
//               s and D_p = L L^T its conditional diagonal block, row r that is still open forms
//                 G = M_rp - sum_{q < s} W_q[r] W_q[p]^T,   W_s[r] = G L^-T,   D_r <- D_r - W_s[r] W_s[r]^T
//               and its new gain by a 6 x 6 Cholesky of D_r.  M_rp is formed on the fly (select_cross_order, select_cross).
#pragma once
#include "gate_joint_block.h"

namespace dpgo {

// log det Sigma_meas = -3 log(2 kappa) - 3 log tau
DPGO_HD double select_logdet_meas(double kappa, double tau) { return -3.0 * log(2.0 * kappa) - 3.0 * log(tau); }

// gain = (log det D - logdet_meas) / 2 of the symmetric D, which is left alone; -inf for a non-positive pivot
DPGO_HD double select_gain(const double D[6][6], double logdet_meas) {
  double L[6][6];
  bool ok;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) L[a][b] = D[a][b];
  gate_cholesky(L, ok);
  const double g = 0.5 * (joint_logdet(L) - logdet_meas);
  return ok && g == g ? g : -(double)INFINITY;  // (a NaN is no gain either)
}

// the candidate that a greedy step takes: the larger gain, the lower index on ties; an index < 0 is no candidate, and a gain
// that is -inf or NaN never becomes one
DPGO_HD void select_better(double g, int k, double &best, int &arg) {
  if (k >= 0 && g > -(double)INFINITY && (arg < 0 || g > best || (g == best && k < arg))) { best = g; arg = k; }
}

// Which of two different candidates the block M_rp is formed from, as joint_assemble decides it for the stored M: first and
// second are the records whose joint_block(first, second) is formed; the block (r, p) is that block, or its transpose when
// the return value is true.  sym: both join the same poses, the block is symmetrised
DPGO_HD bool select_cross_order(int r, int ir, int jr, int p, int ip, int jp, int &first, int &second, bool &sym) {
  const int way = joint_orientation(ir, jr, ip, jp);
  sym = way == 0;
  first = way < 0 ? p : r;
  second = way < 0 ? r : p;
  return way < 0;
}

// G = M_rp from the ends of the two records select_cross_order names
DPGO_HD void select_cross(const double *diag, const double *pairs, int m, const JointEnds &first, const JointEnds &second, bool transposed,
                          bool sym, double G[6][6]) {
  double B[6][6];
  joint_block(diag, pairs, m, first, second, B);
  if (sym) joint_symmetrise(B);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) G[a][b] = transposed ? B[b][a] : B[a][b];
}

// One open row behind a pivot.  G: M_rp less the earlier columns (overwritten by W = G L^-T); L: the pivot's factor as
// gate_cholesky leaves it; D: the row's conditional diagonal block, updated; returns the row's new gain
DPGO_HD double select_row_update(double G[6][6], const double L[6][6], double D[6][6], double logdet_meas) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) {  // w L^T = g, forward
      double v = G[a][c];
#pragma unroll
      for (int q = 0; q < c; ++q) v = __builtin_fma(-G[a][q], L[c][q], v);
      G[a][c] = v * L[c][c];
    }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      double s = D[a][b];
#pragma unroll
      for (int k = 0; k < 6; ++k) s = __builtin_fma(-G[a][k], G[b][k], s);
      D[a][b] = D[b][a] = s;
    }
  return select_gain(D, logdet_meas);
}

}  // namespace dpgo

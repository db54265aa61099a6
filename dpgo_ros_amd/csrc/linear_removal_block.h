// linear_removal_block.h -- the block arithmetic of the first-order removal or down-weighting of measurements that are in the
// graph: what k_lin_b<true>, k_lin_finish<true> (linear_frame.h), k_rem_n and k_rem_z (linear_removal.hip) do
// with the staged covariance blocks, with B~ and with U~.  In the idiom of linear_update_block.h, whose primitives it uses: statically indexed 6 x 6
// arrays, compiled for the device and for the host, so the same text is checked on a machine without a GPU
// (tests/test_linear_removal_host.py).
//
// T, Sigma, the perturbation, J_i, J_j, xi (no Log-Jacobian) and Sigma_meas are the gate's (gate.hip); A is the joint gate's
// (gate_joint.hip), B = Sigma A^T the update's.  Record k is in the graph at weight w_k and goes to w'_k, 0 <= w'_k < w_k:
// dw_k = w_k - w'_k > 0, R_k = Sigma_meas,k / dw_k, s_k = (sqrt(2 kappa_k dw_k) x 3, sqrt(tau_k dw_k) x 3), D = diag(s), R = D^-2.
//   B~          B D: B~_p,k = B_p,k with column c scaled by s_k[c]; column-major with leading dimension 6 N as B is
//   N~          D N D = I - (D A) B~ with N = R - A B: N~_kl = delta_kl I - s_k o (J_i^k B~_{i_k,l} + J_j^k B~_{j_k,l}), the rows
//               scaled; the diagonal blocks stored symmetrised, N~ stored bitwise symmetric as M is: one lane writes a block
//               and its transpose.  A block off the diagonal is never symmetrised: for two records on the same ordered pair
//               of poses A Sigma A^T is symmetric, but s_k o (.) o s_l is not unless their noise is proportional
//   G~, z~, U~  G~ = N~^-1, xi~ = s o xi, z~ = G~ xi~, U~ = B~ G~
//   removal     dx_p = +B~_p z~,  Sigma'_pp = Sigma_pp + U~_p B~_p^T (the upper triangle, mirrored),
//               Sigma'_pq = Sigma_pq + U~_p B~_q^T,  T'_p = upd_retract(T_p, dx_p),  xi_loo = z~ / s
//   figures     d2_joint = xi~^T z~,  log det R = sum_k -3 log(2 kappa_k) - 3 log tau_k - 6 log dw_k,
//               log det N = log det N~ + log det R
// Every sum runs in index order with __builtin_fma.
#pragma once
#include "linear_update_block.h"

namespace dpgo {

// What the removal knows of a record beside its GateRec (64 bytes, read in 16-byte loads): the noise, the weight w at which
// it is in the graph, the weight dw taken out, and the two whitening factors sqrt(2 kappa dw), sqrt(tau dw).  The GateRec is
// the update's: its own two words hold the ranks of the poses i and j among the sorted distinct endpoints.
constexpr int REM_REC = 8;
struct RemRec {
  double kappa, tau, w, dw, s_rot, s_trn, pad[2];
};
static_assert(sizeof(RemRec) == 8 * REM_REC && sizeof(RemRec) % 16 == 0, "RemRec is read in 16-byte loads");

// s_k[a] of a record: the first three rows are the rotation's
DPGO_HD double rem_s(int a, double s_rot, double s_trn) { return a < 3 ? s_rot : s_trn; }

// B~_p,k = B_p,k D_k: column c times s_k[c]
DPGO_HD void rem_scale_columns(double Bk[6][6], double s_rot, double s_trn) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) Bk[a][c] *= rem_s(c, s_rot, s_trn);
}

// G = -s_k o (J_i^k B~_{i_k,l} + J_j^k B~_{j_k,l}): the block (k, l) of N~ less the identity; B~ carries the scaling of l
DPGO_HD void rem_n_block(const double *Bt, size_t ld, const JointEnds &k, int l, double s_rot, double s_trn, double G[6][6]) {
  upd_m_block(Bt, ld, k, l, G);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) G[a][c] = -rem_s(a, s_rot, s_trn) * G[a][c];
}

// the diagonal block: S = I + (G + G^T) / 2, bitwise symmetric, G of rem_n_block
DPGO_HD void rem_diagonal(const double G[6][6], double S[6][6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      const double v = 0.5 * (G[a][b] + G[b][a]) + (a == b ? 1.0 : 0.0);
      S[a][b] = S[b][a] = v;
    }
}

// the smallest Cholesky pivot of the diagonal block S of N~, which is left alone: the audit's pivot_min at weight dw
DPGO_HD double rem_pivot_min(const double S[6][6]) {
  double L[6][6], pmin;
  bool ok;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) L[a][b] = S[a][b];
  gate_cholesky(L, 0.0, ok, pmin);
  return pmin;
}

// xi~ = s o xi
DPGO_HD void rem_whiten(const double x[6], double s_rot, double s_trn, double xt[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) xt[a] = rem_s(a, s_rot, s_trn) * x[a];
}

// log det R_k = log det Sigma_meas,k - 6 log dw_k
DPGO_HD double rem_logdet_r(double kappa, double tau, double dw) { return upd_logdet_meas(kappa, tau) - 6.0 * log(dw); }

}  // namespace dpgo

// linear_update_block.h -- the block arithmetic of the first-order update of a trajectory and its covariances for a set of
// new closures: what k_lin_b, k_lin_finish (linear_frame.h) and k_upd_m (linear_update.hip) do with the staged
// covariance blocks, with B and with U.  In the idiom of gate_block.h and gate_joint_block.h, whose primitives it uses: statically indexed 6 x 6
// arrays, compiled for the device and for the host, so the same text is checked on a machine without a GPU
// (tests/test_linear_update_host.py).
//
// T, Sigma, the perturbation, J_i, J_j, xi (no Log-Jacobian) and Sigma_meas are the gate's (gate.hip); A and R are the joint
// gate's (gate_joint.hip).  K closures on m distinct endpoint poses e_0 < ... < e_{m-1}, N poses.
//   staged      for each endpoint rank a and each pose p the pair block a N + p holds Sigma_{p, e_a} (36 doubles, row-major);
//               what names pose 0 is zero as staged
//   B           B_p,k = Sigma_{p,i_k} J_i^k^T + Sigma_{p,j_k} J_j^k^T, 6 x 6, p = 0 .. N - 1; B_0 = 0.  Column-major with
//               leading dimension 6 N: B_p,k[a][c] at B[(6 k + c) 6 N + 6 p + a]
//   M           M_kl = J_i^k B_{i_k,l} + J_j^k B_{j_k,l} + delta_kl Sigma_meas,k; the diagonal blocks stored symmetrised, M
//               stored bitwise symmetric; the side a block is formed from is chosen by the endpoints (joint_orientation)
//   G, z, U     G = M^-1, z = G xi, U = B G
//   update      dx_p = -B_p z,  Sigma'_pp = Sigma_pp - U_p B_p^T (the upper triangle, mirrored),
//               Sigma'_pq = Sigma_pq - U_p B_q^T,  T'_p = (R_p Exp(phi_p), t_p + delta_p) with dx_p = (phi_p, delta_p)
// Every sum runs in index order with __builtin_fma.
#pragma once
#include "gate_joint_block.h"

namespace dpgo {

// the staged block of (pose p, endpoint of rank a) among N poses
DPGO_HD size_t upd_block_index(int N, int a, int p) { return (size_t)a * N + (size_t)p; }

// Bk = Si Ji^T + Sj Jj^T: element [a][c] the twelve terms Si[a][y] Ji[c][y], y = 0 .. 5, then Sj[a][y] Jj[c][y]
DPGO_HD void upd_b_block(const double Si[6][6], const double Sj[6][6], const double Ji[6][6], const double Jj[6][6], double Bk[6][6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int y = 0; y < 6; ++y) s = __builtin_fma(Si[a][y], Ji[c][y], s);
#pragma unroll
      for (int y = 0; y < 6; ++y) s = __builtin_fma(Sj[a][y], Jj[c][y], s);
      Bk[a][c] = s;
    }
}

// X = B_{p,l} out of the column-major B (leading dimension ld = 6 N)
DPGO_HD void upd_load_b(const double *B, size_t ld, int p, int l, double X[6][6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int a = 0; a < 6; ++a) X[a][c] = GATE_LD(B, ((size_t)6 * l + c) * ld + (size_t)6 * p + a);
}

// G = J_i^k B_{i_k,l} + J_j^k B_{j_k,l}: element [a][c] the twelve terms Ji[a][y] Bi[y][c], then Jj[a][y] Bj[y][c]
DPGO_HD void upd_m_block(const double *B, size_t ld, const JointEnds &k, int l, double G[6][6]) {
  double Bi[6][6], Bj[6][6];
  upd_load_b(B, ld, k.i, l, Bi);
  upd_load_b(B, ld, k.j, l, Bj);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int y = 0; y < 6; ++y) s = __builtin_fma(k.Ji[a][y], Bi[y][c], s);
#pragma unroll
      for (int y = 0; y < 6; ++y) s = __builtin_fma(k.Jj[a][y], Bj[y][c], s);
      G[a][c] = s;
    }
}

// what one wave lane sums for a pose: the 21 elements of the upper triangle of U_p B_p^T (row by row) and the 6 of B_p z
constexpr int UPD_TRI = 21, UPD_SUMS = 27;

// one column c of the 6 K: acc[tri(a, b)] += u[a] b[b] for a <= b, acc[21 + a] += b[a] z
DPGO_HD void upd_accumulate(const double u[6], const double b[6], double z, double acc[UPD_SUMS]) {
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c, ++q) acc[q] = __builtin_fma(u[a], b[c], acc[q]);
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[UPD_TRI + a] = __builtin_fma(b[a], z, acc[UPD_TRI + a]);
}

// one column of a pair (p, q): acc[6 a + c] += u_p[a] b_q[c]
DPGO_HD void upd_accumulate_pair(const double u[6], const double b[6], double acc[36]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[6 * a + c] = __builtin_fma(u[a], b[c], acc[6 * a + c]);
}

// Sigma'_pp (36 doubles, row-major, bitwise symmetric) from Sigma_pp (36, row-major) and the 21 sums, and dx from the 6.  The
// update: Sigma_pp - the sums, dx = -(B_p z); Add, the removal (linear_removal_block.h): Sigma_pp + the sums, dx = +(B~_p z~)
template <bool Add>
DPGO_HD void lin_close_pose(const double *Spp, const double acc[UPD_SUMS], double Sn[6][6], double dx[6]) {
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c, ++q) {
      const double S = GATE_LD(Spp, 6 * a + c);
      Sn[a][c] = Sn[c][a] = Add ? S + acc[q] : S - acc[q];
    }
#pragma unroll
  for (int a = 0; a < 6; ++a) dx[a] = Add ? acc[UPD_TRI + a] : -acc[UPD_TRI + a];
}

// E = Exp(phi) by Rodrigues, I + a [phi]x + b [phi]x^2 with a = sin(th) / th and b = (1 - cos th) / th^2 formed without
// cancellation as (sin(th / 2) / (th / 2))^2 / 2; below th^2 = 1e-8 the series a = 1 - th^2 / 6, b = 1 / 2 - th^2 / 24, whose
// first neglected terms are below 1e-18
DPGO_HD void upd_exp_so3(const double w[3], double E[3][3]) {
  const double t2 = __builtin_fma(w[2], w[2], __builtin_fma(w[1], w[1], w[0] * w[0]));
  double a, b;
  if (t2 < 1e-8) {
    a = 1.0 - t2 / 6.0;
    b = 0.5 - t2 / 24.0;
  } else {
    const double th = sqrt(t2), h = 0.5 * th, sh = sin(h) / h;
    a = sin(th) / th;
    b = 0.5 * sh * sh;
  }
  // [w]x^2 = w w^T - th^2 I
  E[0][0] = 1.0 - b * (w[1] * w[1] + w[2] * w[2]);
  E[1][1] = 1.0 - b * (w[0] * w[0] + w[2] * w[2]);
  E[2][2] = 1.0 - b * (w[0] * w[0] + w[1] * w[1]);
  E[0][1] = __builtin_fma(b * w[0], w[1], -a * w[2]);
  E[1][0] = __builtin_fma(b * w[0], w[1], a * w[2]);
  E[0][2] = __builtin_fma(b * w[0], w[2], a * w[1]);
  E[2][0] = __builtin_fma(b * w[0], w[2], -a * w[1]);
  E[1][2] = __builtin_fma(b * w[1], w[2], -a * w[0]);
  E[2][1] = __builtin_fma(b * w[1], w[2], a * w[0]);
}

// (Rn, tn) = (R Exp(phi), t + delta) with dx = (phi, delta): the rotation in the body frame, the translation in the world frame
DPGO_HD void upd_retract(const double R[3][3], const double t[3], const double dx[6], double Rn[3][3], double tn[3]) {
  double E[3][3];
  upd_exp_so3(dx, E);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rn[a][c] = __builtin_fma(R[a][2], E[2][c], __builtin_fma(R[a][1], E[1][c], R[a][0] * E[0][c]));
    tn[a] = t[a] + dx[3 + a];
  }
}

// the 12 doubles of a pose in the layout of T: R column-major, then t
DPGO_HD void upd_store_pose(const double R[3][3], const double t[3], double out[12]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int b = 0; b < 3; ++b) out[3 * c + b] = R[b][c];
#pragma unroll
  for (int b = 0; b < 3; ++b) out[9 + b] = t[b];
}

// log det Sigma_meas = -3 log(2 kappa) - 3 log tau
DPGO_HD double upd_logdet_meas(double kappa, double tau) { return -3.0 * log(2.0 * kappa) - 3.0 * log(tau); }

}  // namespace dpgo

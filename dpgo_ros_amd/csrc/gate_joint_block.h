// gate_joint_block.h -- the block arithmetic of the joint gate of a set of candidates: what k_joint_blocks and
// k_joint_step (gate_joint.hip) do with the staged covariance blocks and with the rows of the factor.  It compiles for the
// device (global loads through gp) and for the host with plain loads, so the same text is checked on a machine without a
// GPU (tests/test_gate_joint_host.py).
//
// K candidates, candidate k joining the team poses i_k != j_k; R_ij, t_ij, J_i, J_j, xi and Sigma_meas of the gate (gate.hip).
//   blocks       the distinct endpoint poses sorted, pose of rank a < b: the staged pair block a m - a (a + 1) / 2 + b - a - 1
//                holds Sigma_ab; Sigma_ba is its transpose, Sigma_aa the diagonal block; what names pose 0 is zero as staged
//   M_kl         sum over a in {i_k, j_k}, b in {i_l, j_l} of J_a^k Sigma_ab J_b^l^T, plus Sigma_meas,k when k = l; the
//                diagonal block stored (G + G^T) / 2, the block (l, k) as the transpose of (k, l): M is bitwise symmetric.
//                Which of the two is formed follows from the endpoints (joint_orientation), so duplicates have equal rows
//   elimination  left-looking block Cholesky in the order the pivots are taken.  With p the pivot of step s, D_p = L L^T its
//                conditional diagonal block and y = L^-1 xi_p|A, row r that is still open forms
//                  G = M_rp - sum_{q < s} W_q[r] W_q[p]^T,   W_s[r] = G L^-T,
//                  D_r <- D_r - W_s[r] W_s[r]^T,   xi_r|A <- xi_r|A - W_s[r] y,   d2_r|A = xi_r|A^T D_r^-1 xi_r|A
//                by a 6 x 6 Cholesky; a non-positive pivot gives +inf.  M itself is only read.
#pragma once
#include "gate_block.h"

namespace dpgo {

#if defined(__HIP_DEVICE_COMPILE__)
#define JOINT_LD(p, i) (gp(p)[i])
#else
#define JOINT_LD(p, i) ((p)[i])
#endif

constexpr int JOINT_REC = 16;  // doubles of a record: the four ints (i, j, rank of i, rank of j), R~ row-major (9), t~ (3), kappa, tau

// the staged pair block of the poses of rank a < b among m
DPGO_HD size_t joint_pair_index(int m, int a, int b) { return (size_t)a * m - (size_t)a * (a + 1) / 2 + (size_t)(b - a - 1); }

// B = Sigma_ab for the poses (pa, pb) of ranks (a, b): the diagonal block, the staged pair block or its transpose
DPGO_HD void joint_load_sigma(const double *diag, const double *pairs, int m, int pa, int a, int b, double B[6][6]) {
  const bool tr = b < a;
  const double *p = a == b ? diag + (size_t)36 * pa : pairs + (size_t)36 * joint_pair_index(m, tr ? b : a, tr ? a : b);
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int y = 0; y < 6; ++y) B[x][y] = JOINT_LD(p, tr ? 6 * y + x : 6 * x + y);
}

// pose g of T: R[b][c] = T[(4 g + c) 3 + b], t[b] = T[(4 g + 3) 3 + b]
DPGO_HD void joint_load_pose(const double *T, int g, double R[3][3], double t[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[b][c] = JOINT_LD(T, (size_t)12 * g + 3 * c + b);
#pragma unroll
  for (int b = 0; b < 3; ++b) t[b] = JOINT_LD(T, (size_t)12 * g + 9 + b);
}

// the relative pose (M = R_ij, tij) of the poses (Ri, ti), (Rj, tj) and its Jacobians; the arithmetic of gate_relative
DPGO_HD void joint_jacobians(const double Ri[3][3], const double ti[3], const double Rj[3][3], const double tj[3], double M[3][3],
                             double tij[3], double Ji[6][6], double Jj[6][6]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) M[a][b] = __builtin_fma(Ri[2][a], Rj[2][b], __builtin_fma(Ri[1][a], Rj[1][b], Ri[0][a] * Rj[0][b]));
    tij[a] = __builtin_fma(Ri[2][a], tj[2] - ti[2], __builtin_fma(Ri[1][a], tj[1] - ti[1], Ri[0][a] * (tj[0] - ti[0])));
  }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) { Ji[a][b] = 0.0; Jj[a][b] = a == b && a < 3 ? 1.0 : 0.0; }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Ji[a][b] = -M[b][a];
      Ji[3 + a][3 + b] = -Ri[b][a];
      Jj[3 + a][3 + b] = Ri[b][a];
    }
  Ji[3][1] = -tij[2]; Ji[3][2] = tij[1];
  Ji[4][0] = tij[2];  Ji[4][2] = -tij[0];
  Ji[5][0] = -tij[1]; Ji[5][1] = tij[0];
}

// A += X B Y^T (6 x 6; the text of gate_sandwich, for both compilers)
DPGO_HD void joint_sandwich(const double X[6][6], const double B[6][6], const double Y[6][6], double A[6][6]) {
  double P[6][6];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = __builtin_fma(X[a][k], B[k][b], s);
      P[a][b] = s;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double s = A[a][b];
#pragma unroll
      for (int k = 0; k < 6; ++k) s = __builtin_fma(P[a][k], Y[b][k], s);
      A[a][b] = s;
    }
}

// one candidate's endpoints as a block needs them
struct JointEnds {
  int i, j, ri, rj;
  double Ji[6][6], Jj[6][6];
};

// G = the block (k, l) of A Sigma A^T from the staged blocks: the four sandwiches in the order (i, i), (i, j), (j, i), (j, j)
DPGO_HD void joint_block(const double *diag, const double *pairs, int m, const JointEnds &k, const JointEnds &l, double G[6][6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) G[a][b] = 0.0;
  double B[6][6];
  joint_load_sigma(diag, pairs, m, k.i, k.ri, l.ri, B);
  joint_sandwich(k.Ji, B, l.Ji, G);
  joint_load_sigma(diag, pairs, m, k.i, k.ri, l.rj, B);
  joint_sandwich(k.Ji, B, l.Jj, G);
  joint_load_sigma(diag, pairs, m, k.j, k.rj, l.ri, B);
  joint_sandwich(k.Jj, B, l.Ji, G);
  joint_load_sigma(diag, pairs, m, k.j, k.rj, l.rj, B);
  joint_sandwich(k.Jj, B, l.Jj, G);
}

// How the block of two different candidates is formed, by their endpoints and not by their indices, so that duplicated
// records have rows of identical bits whichever side of a third candidate their indices fall on: > 0 as joint_block(k, l);
// < 0 as the transpose of joint_block(l, k); 0, the same pair of poses (the block is symmetric): (G + G^T) / 2
DPGO_HD int joint_orientation(int ik, int jk, int il, int jl) {
  return ik != il ? (ik < il ? 1 : -1) : jk != jl ? (jk < jl ? 1 : -1) : 0;
}

// G <- (G + G^T) / 2
DPGO_HD void joint_symmetrise(double G[6][6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a + 1; b < 6; ++b) G[a][b] = G[b][a] = 0.5 * (G[a][b] + G[b][a]);
}

// the diagonal block: S = (G + G^T) / 2 + Sigma_meas, bitwise symmetric
DPGO_HD void joint_diagonal(const double G[6][6], double kappa, double tau, double S[6][6]) {
  const double nr = 1.0 / (2.0 * kappa), nt = 1.0 / tau;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      const double v = 0.5 * (G[a][b] + G[b][a]) + (a == b ? (a < 3 ? nr : nt) : 0.0);
      S[a][b] = S[b][a] = v;
    }
}

// xi = (Log(R~^T R_ij), t_ij - t~) from the 14 doubles of the measurement (R~ row-major, t~, kappa, tau)
DPGO_HD void joint_innovation(const double M[3][3], const double tij[3], const double *v, double x[6]) {
  const double *Rm = v, *tm = v + 9;
  double E[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) E[a][b] = __builtin_fma(Rm[6 + a], M[2][b], __builtin_fma(Rm[3 + a], M[1][b], Rm[a] * M[0][b]));
  gate_log_so3(E, x);
#pragma unroll
  for (int a = 0; a < 3; ++a) x[3 + a] = tij[a] - tm[a];
}

// Cholesky of the symmetric S in place: the lower triangle receives L with the RECIPROCALS of its diagonal.  ok: every pivot
// positive
DPGO_HD void joint_cholesky(double S[6][6], bool &ok) {
  ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double p = S[c][c];
#pragma unroll
    for (int q = 0; q < c; ++q) p = __builtin_fma(-S[c][q], S[c][q], p);
    ok = ok && p > 0.0;
    const double inv = 1.0 / sqrt(p);
    S[c][c] = inv;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double v = S[r][c];
#pragma unroll
      for (int q = 0; q < c; ++q) v = __builtin_fma(-S[r][q], S[c][q], v);
      S[r][c] = v * inv;
    }
  }
}

// log det S = 2 sum log L_cc from the factor joint_cholesky leaves
DPGO_HD double joint_logdet(const double L[6][6]) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) s -= log(L[c][c]);
  return 2.0 * s;
}

// y = L^-1 x with the factor joint_cholesky leaves; returns |y|^2
DPGO_HD double joint_forward(const double L[6][6], const double x[6], double y[6]) {
  double dd = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double v = x[c];
#pragma unroll
    for (int q = 0; q < c; ++q) v = __builtin_fma(-L[c][q], y[q], v);
    y[c] = v * L[c][c];
    dd = __builtin_fma(y[c], y[c], dd);
  }
  return dd;
}

// d2 = x^T D^-1 x of the symmetric D, which is left alone; +inf for a non-positive pivot
DPGO_HD double joint_distance(const double D[6][6], const double x[6]) {
  double L[6][6], y[6];
  bool ok;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) L[a][b] = D[a][b];
  joint_cholesky(L, ok);
  const double dd = joint_forward(L, x, y);
  return ok && dd >= 0.0 ? dd : (double)INFINITY;  // (a NaN is no distance either)
}

// G -= A B^T, A and B 36 doubles row-major in memory (one earlier column of the factor at this row and at the pivot's)
DPGO_HD void joint_subtract_product(const double *A, const double *B, double G[6][6]) {
  double a[6][6], b[6][6];
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int y = 0; y < 6; ++y) { a[x][y] = JOINT_LD(A, 6 * x + y); b[x][y] = JOINT_LD(B, 6 * x + y); }
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int y = 0; y < 6; ++y) {
      double s = G[x][y];
#pragma unroll
      for (int k = 0; k < 6; ++k) s = __builtin_fma(-a[x][k], b[y][k], s);
      G[x][y] = s;
    }
}

// One open row behind a pivot.  G: M_rp less the earlier columns (overwritten by W = G L^-T); L, y: the pivot's factor and
// whitened innovation; D, x: the row's conditional diagonal block and innovation, updated; returns the row's new d2
DPGO_HD double joint_row_update(double G[6][6], const double L[6][6], const double y[6], double D[6][6], double x[6]) {
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
  for (int a = 0; a < 6; ++a) {
    double v = x[a];
#pragma unroll
    for (int k = 0; k < 6; ++k) v = __builtin_fma(-G[a][k], y[k], v);
    x[a] = v;
#pragma unroll
    for (int b = a; b < 6; ++b) {
      double s = D[a][b];
#pragma unroll
      for (int k = 0; k < 6; ++k) s = __builtin_fma(-G[a][k], G[b][k], s);
      D[a][b] = D[b][a] = s;
    }
  }
  return joint_distance(D, x);
}

// the candidate that a greedy step takes: the smaller d2, the lower index on ties; an index < 0 is no candidate
DPGO_HD void joint_better(double d, int k, double &best, int &arg) {
  if (k >= 0 && (arg < 0 || d < best || (d == best && k < arg))) { best = d; arg = k; }
}

}  // namespace dpgo

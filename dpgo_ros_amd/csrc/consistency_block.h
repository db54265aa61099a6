// consistency_block.h -- the per-pair arithmetic of pairwise consistency maximisation: the loop through two
// candidates and the two robots' own trajectories, its Jacobians, its covariance and the Mahalanobis distance of its residual.
// It compiles for the device (k_consistency, consistency.hip) and for the host, with the loads of gate_block.h, so the same
// text is checked on a machine without a GPU (tests/test_consistency_host.py).
//
// Every factor X = (R, t) is perturbed as R <- R Exp(phi), t <- t + delta, and so is the loop E.  For candidates p < q
//   E = X1 X2 X3 X4,  X1 = Z_q^-1,  X2 = A = (T^A_{i_q})^-1 T^A_{i_p},  X3 = Z_p,  X4 = B = (T^B_{j_p})^-1 T^B_{j_q}.
// Factor m moves E by  phi_E = (R_{m+1} .. R_4)^T phi_m,  delta_E = R_1 .. R_{m-1} delta_m - R_1 .. R_m [s_m]x phi_m  with s_m the
// translation of X_{m+1} .. X_4: a Jacobian [[P, 0], [Q, W]] in 3 x 3 blocks, rotation first.  Z_q enters through its inverse,
// which (phi, delta) moves by (-R~ phi, -R~^T delta - [R~^T t~]x phi).
#pragma once
#include "gate_block.h"

namespace dpgo {

constexpr int PCM_CAND = 16;  // doubles of a candidate record: R~ row-major (9), t~ (3), kappa, tau, two of padding
constexpr int PCM_SEG = 48;   // doubles of a segment record: R row-major (9), t (3), Sigma_rel row-major (36)

// a candidate: R~, t~ and its noise diag(I / (2 kappa), I / tau)
struct PcmCand {
  double R[3][3], t[3], nr, nt;
};
// a segment's relative pose; the blocks of its bitwise symmetric covariance [[rr, rt], [rt^T, tt]] are loaded where they are used
struct PcmSeg {
  double R[3][3], t[3];
};

DPGO_HD void pcm_load_cand(const double *rec, PcmCand &z) {
  double v[GATE_MEAS];
  gate_load_meas(rec, v);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) z.R[a][b] = v[3 * a + b];
    z.t[a] = v[9 + a];
  }
  z.nr = 1.0 / (2.0 * v[12]);
  z.nt = 1.0 / v[13];
}

// present = false: the two poses of the segment coincide -- the identity with zero covariance (rec is still read: it must
// point at a record)
DPGO_HD void pcm_load_seg(const double *rec, bool present, PcmSeg &s) {
  double v[12];
  gate_load_pairs<6>(rec, v);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) s.R[a][b] = present ? v[3 * a + b] : (a == b ? 1.0 : 0.0);
    s.t[a] = present ? v[9 + a] : 0.0;
  }
}
DPGO_HD void pcm_load_sigma(const double *rec, bool present, double rr[3][3], double rt[3][3], double tt[3][3]) {
  double v[36];
  gate_load_pairs<18>(rec + 12, v);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      rr[a][b] = present ? v[6 * a + b] : 0.0;
      rt[a][b] = present ? v[6 * a + 3 + b] : 0.0;
      tt[a][b] = present ? v[6 * (3 + a) + 3 + b] : 0.0;
    }
}

// C = A B, C = A^T B, C = A B^T for 3 x 3; y = A x, y = A^T x
DPGO_HD void pcm_mm(const double A[3][3], const double B[3][3], double C[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) C[a][b] = __builtin_fma(A[a][2], B[2][b], __builtin_fma(A[a][1], B[1][b], A[a][0] * B[0][b]));
}
DPGO_HD void pcm_mtm(const double A[3][3], const double B[3][3], double C[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) C[a][b] = __builtin_fma(A[2][a], B[2][b], __builtin_fma(A[1][a], B[1][b], A[0][a] * B[0][b]));
}
DPGO_HD void pcm_mv(const double A[3][3], const double x[3], double y[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) y[a] = __builtin_fma(A[a][2], x[2], __builtin_fma(A[a][1], x[1], A[a][0] * x[0]));
}
DPGO_HD void pcm_mtv(const double A[3][3], const double x[3], double y[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) y[a] = __builtin_fma(A[2][a], x[2], __builtin_fma(A[1][a], x[1], A[0][a] * x[0]));
}
// C += A B^T
DPGO_HD void pcm_add_mmt(const double A[3][3], const double B[3][3], double C[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      C[a][b] = __builtin_fma(A[a][2], B[b][2], __builtin_fma(A[a][1], B[b][1], __builtin_fma(A[a][0], B[b][0], C[a][b])));
}
// Q = -M [v]x
DPGO_HD void pcm_neg_m_skew(const double M[3][3], const double v[3], double Q[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Q[a][0] = -__builtin_fma(M[a][1], v[2], -(M[a][2] * v[1]));
    Q[a][1] = -__builtin_fma(M[a][2], v[0], -(M[a][0] * v[2]));
    Q[a][2] = -__builtin_fma(M[a][0], v[1], -(M[a][1] * v[0]));
  }
}

// the blocks of S += J Sigma J^T, J = [[P, 0], [Q, W]], Sigma = [[rr, rt], [rt^T, tt]] symmetric: the upper blocks S11, S12 and
// S22 alone (S21 = S12^T)
DPGO_HD void pcm_sandwich(const double P[3][3], const double Q[3][3], const double W[3][3], const double rr[3][3],
                          const double rt[3][3], const double tt[3][3], double S11[3][3], double S12[3][3], double S22[3][3]) {
  double U1[3][3], U2[3][3], tr[3][3];
  pcm_mm(P, rr, U1);  // U11 = P rr
  pcm_mm(P, rt, U2);  // U12 = P rt
  pcm_add_mmt(U1, P, S11);
  pcm_add_mmt(U1, Q, S12);
  pcm_add_mmt(U2, W, S12);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) tr[a][b] = rt[b][a];
  pcm_mm(Q, rr, U1);  // U21 = Q rr + W rt^T
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) U1[a][b] = __builtin_fma(W[a][2], tr[2][b], __builtin_fma(W[a][1], tr[1][b], __builtin_fma(W[a][0], tr[0][b], U1[a][b])));
  pcm_mm(Q, rt, U2);  // U22 = Q rt + W tt
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) U2[a][b] = __builtin_fma(W[a][2], tt[2][b], __builtin_fma(W[a][1], tt[1][b], __builtin_fma(W[a][0], tt[0][b], U2[a][b])));
  pcm_add_mmt(U1, Q, S22);
  pcm_add_mmt(U2, W, S22);
}

// the same for the noise of a candidate, Sigma = diag(nr I, nt I)
DPGO_HD void pcm_noise(const double P[3][3], const double Q[3][3], const double W[3][3], double nr, double nt, double S11[3][3],
                       double S12[3][3], double S22[3][3]) {
  double U[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) U[a][b] = nr * P[a][b];
  pcm_add_mmt(U, P, S11);
  pcm_add_mmt(U, Q, S12);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) U[a][b] = nr * Q[a][b];
  pcm_add_mmt(U, Q, S22);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) U[a][b] = nt * W[a][b];
  pcm_add_mmt(U, W, S22);
}

// d^2 of the ordered pair p < q: cp, cq the records of the two candidates, ra, rb those of A_pq and B_pq (has_a / has_b false:
// the segment's poses coincide).  xi_out (6) and S_out (36, row-major) receive the residual and its covariance where they are
// not null.  A non-positive pivot gives +inf.
DPGO_HD double pcm_pair(const double *cp, const double *cq, const double *ra, bool has_a, const double *rb, bool has_b,
                        double *xi_out, double *S_out) {
  PcmCand zp, zq;
  PcmSeg sa, sb;
  pcm_load_cand(cp, zp);
  pcm_load_cand(cq, zq);
  pcm_load_seg(ra, has_a, sa);
  pcm_load_seg(rb, has_b, sb);
  // X1 = Z_q^-1 = (R1, -u), u = R_q^T t_q
  double R1[3][3], u[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R1[a][b] = zq.R[b][a];
  pcm_mtv(zq.R, zq.t, u);
  // suffix products: R34 = R_p R_B, s2 = t_p + R_p t_B, R234 = R_A R34, s1 = t_A + R_A s2; prefix products P12, P123
  double R34[3][3], R234[3][3], P12[3][3], P123[3][3], RE[3][3], s2[3], s1[3], tE[3], w[3];
  pcm_mm(zp.R, sb.R, R34);
  pcm_mv(zp.R, sb.t, w);
#pragma unroll
  for (int a = 0; a < 3; ++a) s2[a] = zp.t[a] + w[a];
  pcm_mm(sa.R, R34, R234);
  pcm_mv(sa.R, s2, w);
#pragma unroll
  for (int a = 0; a < 3; ++a) s1[a] = sa.t[a] + w[a];
  pcm_mm(R1, sa.R, P12);
  pcm_mm(P12, zp.R, P123);
  pcm_mm(P123, sb.R, RE);
  pcm_mv(R1, s1, w);
#pragma unroll
  for (int a = 0; a < 3; ++a) tE[a] = w[a] - u[a];
  double x[6];
  gate_log_so3(RE, x);
#pragma unroll
  for (int a = 0; a < 3; ++a) x[3 + a] = tE[a];

  double S11[3][3], S12[3][3], S22[3][3], P[3][3], Q[3][3], W[3][3], rr[3][3], rt[3][3], tt[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) S11[a][b] = S12[a][b] = S22[a][b] = 0.0;
  // candidate q, factor 1 behind the inverse: P = -R234^T R_q, Q = R1 [s1]x R_q - [u]x, W = -R1
  pcm_mtm(R234, zq.R, P);
  pcm_neg_m_skew(R1, s1, W);  // (-R1 [s1]x for the moment)
  pcm_mm(W, zq.R, Q);         // -R1 [s1]x R_q
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) { P[a][b] = -P[a][b]; Q[a][b] = -Q[a][b]; W[a][b] = -R1[a][b]; }
  Q[0][1] += u[2];  Q[0][2] -= u[1];
  Q[1][0] -= u[2];  Q[1][2] += u[0];
  Q[2][0] += u[1];  Q[2][1] -= u[0];
  pcm_noise(P, Q, W, zq.nr, zq.nt, S11, S12, S22);
  // candidate p, factor 3: P = R_B^T, Q = -P123 [t_B]x, W = P12
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a][b] = sb.R[b][a];
  pcm_neg_m_skew(P123, sb.t, Q);
  pcm_noise(P, Q, P12, zp.nr, zp.nt, S11, S12, S22);
  // the segment of team A, factor 2: P = R34^T, Q = -P12 [s2]x, W = R1
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a][b] = R34[b][a];
  pcm_neg_m_skew(P12, s2, Q);
  pcm_load_sigma(ra, has_a, rr, rt, tt);
  pcm_sandwich(P, Q, R1, rr, rt, tt, S11, S12, S22);
  // the segment of team B, factor 4: P = I, Q = 0, W = P123
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) { P[a][b] = a == b ? 1.0 : 0.0; Q[a][b] = 0.0; }
  pcm_load_sigma(rb, has_b, rr, rt, tt);
  pcm_sandwich(P, Q, P123, rr, rt, tt, S11, S12, S22);

  double S[6][6];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      S[a][b] = 0.5 * (S11[a][b] + S11[b][a]);
      S[3 + a][3 + b] = 0.5 * (S22[a][b] + S22[b][a]);
      S[a][3 + b] = S[3 + b][a] = S12[a][b];
    }
  if (xi_out) {
#pragma unroll
    for (int a = 0; a < 6; ++a) xi_out[a] = x[a];
  }
  if (S_out) {
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) S_out[6 * a + b] = S[a][b];
  }
  // Cholesky of S in place (lower), forward solve y = L^-1 xi, d2 = |y|^2
  bool ok = true;
  double y[6], dd = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double p = S[c][c];
#pragma unroll
    for (int q = 0; q < c; ++q) p = __builtin_fma(-S[c][q], S[c][q], p);
    ok = ok && p > 0.0;
    const double l = sqrt(p), inv = 1.0 / l;
    S[c][c] = l;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double v = S[r][c];
#pragma unroll
      for (int q = 0; q < c; ++q) v = __builtin_fma(-S[r][q], S[c][q], v);
      S[r][c] = v * inv;
    }
    double v = x[c];
#pragma unroll
    for (int q = 0; q < c; ++q) v = __builtin_fma(-S[c][q], y[q], v);
    y[c] = v * inv;
    dd = __builtin_fma(y[c], y[c], dd);
  }
  return ok ? dd : (double)INFINITY;
}

}  // namespace dpgo

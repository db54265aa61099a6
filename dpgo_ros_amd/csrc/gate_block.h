// gate_block.h -- the 6 x 6 block text of the Mahalanobis gate and of the calls built on it: the audit (5h,
// audit_block.h), the joint gate (5i, gate_joint_block.h), the linear update (5j, linear_update_block.h) and the segment kernel
// of pairwise consistency (5g, consistency.hip).  One text, so a pose, a relative covariance, an innovation or a distance has
// the same bits wherever it is formed.  Everything compiles for the device (global loads through gp() / ld2) and for the host
// with plain loads, so the same text is checked on a machine without a GPU (tests/test_*_host.py).
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define DPGO_HD __host__ __device__ __forceinline__
#else
#define DPGO_HD inline
#endif

// p[i], and the two doubles at the 16-byte aligned p
#if defined(__HIP_DEVICE_COMPILE__)
#define GATE_LD(p, i) (gp(p)[i])
#define GATE_LD2(p, lo, hi) do { const double2 w_ = ld2(p); (lo) = w_.x; (hi) = w_.y; } while (0)
#else
#define GATE_LD(p, i) ((p)[i])
#define GATE_LD2(p, lo, hi) do { (lo) = (p)[0]; (hi) = (p)[1]; } while (0)
#endif

namespace dpgo {

// One measurement on the device, 128 bytes read in 16-byte loads: team poses i != j, two words of the call's own (the gate:
// w0 = the staged pair block that holds S_ij; the joint gate and the update: the ranks of i and j among the sorted distinct
// endpoints), and the GATE_MEAS doubles R~ row-major (9), t~ (3), kappa, tau.  The audit's record has the same head and the
// weight behind it (audit_block.h).
constexpr int GATE_MEAS = 14;
struct GateRec {
  int i, j, w0, w1;
  double m[GATE_MEAS];
};
static_assert(sizeof(GateRec) == 128, "GateRec is read in 16-byte loads");

// Log of E in SO(3) as a vector.  a = vee of the antisymmetric part (|a| = sin theta), c = (tr - 1) / 2, theta = atan2(|a|, c).
// Away from pi: (theta / |a|) a, the limit 1 where |a|^2 underflows (zero in, zero out).  Within 0.1 rad of pi the direction
// of a is lost to cancellation: the axis comes from the symmetric part c I + (1 - c) n n^T, by its largest diagonal entry,
// signed like a; theta = pi gives a finite vector of norm pi.
DPGO_HD void gate_log_so3(const double E[3][3], double w[3]) {
  const double a0 = 0.5 * (E[2][1] - E[1][2]), a1 = 0.5 * (E[0][2] - E[2][0]), a2 = 0.5 * (E[1][0] - E[0][1]);
  const double c = 0.5 * (E[0][0] + E[1][1] + E[2][2] - 1.0);
  const double s = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  const double theta = atan2(s, c);
  if (c < 0.0 && s < 0.1) {
    const double omc = 1.0 - c;
    const double d0 = E[0][0], d1 = E[1][1], d2 = E[2][2];
    double n0, n1, n2;
    if (d0 >= d1 && d0 >= d2) {
      n0 = sqrt(fmax(d0 - c, 0.0) / omc);
      n1 = 0.5 * (E[0][1] + E[1][0]) / (omc * n0);
      n2 = 0.5 * (E[0][2] + E[2][0]) / (omc * n0);
    } else if (d1 >= d2) {
      n1 = sqrt(fmax(d1 - c, 0.0) / omc);
      n0 = 0.5 * (E[0][1] + E[1][0]) / (omc * n1);
      n2 = 0.5 * (E[1][2] + E[2][1]) / (omc * n1);
    } else {
      n2 = sqrt(fmax(d2 - c, 0.0) / omc);
      n0 = 0.5 * (E[0][2] + E[2][0]) / (omc * n2);
      n1 = 0.5 * (E[1][2] + E[2][1]) / (omc * n2);
    }
    const double f = (n0 * a0 + n1 * a1 + n2 * a2 < 0.0) ? -theta : theta;
    w[0] = f * n0; w[1] = f * n1; w[2] = f * n2;
    return;
  }
  const double f = s > 0.0 ? theta / s : 1.0;
  w[0] = f * a0; w[1] = f * a1; w[2] = f * a2;
}

// v = the 2 PAIRS doubles at the 16-byte aligned p
template <int PAIRS>
DPGO_HD void gate_load_pairs(const double *p, double *v) {
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) GATE_LD2(p + 2 * q, v[2 * q], v[2 * q + 1]);
}

// the GATE_MEAS doubles of a measurement
DPGO_HD void gate_load_meas(const double *m, double v[GATE_MEAS]) { gate_load_pairs<GATE_MEAS / 2>(m, v); }

// 36 doubles, row-major.  (8-byte loads: where a path stages its blocks depends on the parity of its scratch in front of them)
DPGO_HD void gate_load36(const double *p, double B[6][6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) B[a][b] = GATE_LD(p, 6 * a + b);
}

// pose g of T: R[b][c] = T[(4 g + c) 3 + b], t[b] = T[(4 g + 3) 3 + b]
DPGO_HD void gate_load_pose(const double *T, int g, double R[3][3], double t[3]) {
  double v[12];
  gate_load_pairs<6>(T + (size_t)12 * g, v);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[b][c] = v[3 * c + b];
#pragma unroll
  for (int b = 0; b < 3; ++b) t[b] = v[9 + b];
}

// A += X B Y^T (all 6 x 6, every index static after unrolling: the zeros of the Jacobians fold away)
DPGO_HD void gate_sandwich(const double X[6][6], const double B[6][6], const double Y[6][6], double A[6][6]) {
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

// the relative pose (M = R_ij, tij = t_ij) of the poses (Ri, ti), (Rj, tj) and its Jacobians J_i, J_j
DPGO_HD void gate_jacobians(const double Ri[3][3], const double ti[3], const double Rj[3][3], const double tj[3], double M[3][3],
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

// The relative pose of the team poses i != j of T (M = R_ij, tij = t_ij) and its covariance S = Sigma_rel, bitwise symmetric,
// from the staged blocks: diag (36 per pose) and the pair block blk of `pairs`, which holds Sigma_ij.
DPGO_HD void gate_relative(const double *T, const double *diag, const double *pairs, int i, int j, int blk, double M[3][3],
                           double tij[3], double S[6][6]) {
  double Ri[3][3], Rj[3][3], ti[3], tj[3], Ji[6][6], Jj[6][6];
  gate_load_pose(T, i, Ri, ti);
  gate_load_pose(T, j, Rj, tj);
  gate_jacobians(Ri, ti, Rj, tj, M, tij, Ji, Jj);
  // A = J_i S_ii J_i^T + J_j S_jj J_j^T + C + C^T with C = J_i S_ij J_j^T, then (A + A^T) / 2
  double A[6][6], C[6][6], B[6][6];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) A[a][b] = C[a][b] = 0.0;
  gate_load36(diag + (size_t)36 * i, B);
  gate_sandwich(Ji, B, Ji, A);
  gate_load36(diag + (size_t)36 * j, B);
  gate_sandwich(Jj, B, Jj, A);
  gate_load36(pairs + (size_t)36 * blk, B);
  gate_sandwich(Ji, B, Jj, C);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      const double v = 0.5 * (A[a][b] + A[b][a]) + (C[a][b] + C[b][a]);
      S[a][b] = S[b][a] = v;
    }
}

// xi = (Log(R~^T R_ij), t_ij - t~) from the doubles of the measurement (R~ row-major, t~, ...)
DPGO_HD void gate_innovation(const double M[3][3], const double tij[3], const double *v, double x[6]) {
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

// Cholesky of the symmetric S in place: the lower triangle receives L with the RECIPROCALS of its diagonal, which is what the
// solves use.  ok: every pivot > floor.  pmin: the smallest pivot, those behind a non-positive one left out
DPGO_HD void gate_cholesky(double S[6][6], double floor, bool &ok, double &pmin) {
  bool alive = true;
  ok = true;
  pmin = INFINITY;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double p = S[c][c];
#pragma unroll
    for (int q = 0; q < c; ++q) p = __builtin_fma(-S[c][q], S[c][q], p);
    ok = ok && p > floor;
    pmin = alive && !(p >= pmin) ? p : pmin;  // (a NaN pivot is kept: it compares false with every floor)
    alive = alive && p > 0.0;
    const double l = sqrt(p), inv = 1.0 / l;
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
// ok: every pivot positive
DPGO_HD void gate_cholesky(double S[6][6], bool &ok) {
  double pmin;
  gate_cholesky(S, 0.0, ok, pmin);
}

// y = L^-1 x with the factor gate_cholesky leaves; returns |y|^2
DPGO_HD double gate_forward(const double L[6][6], const double x[6], double y[6]) {
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

// x <- (L L^T)^-1 x with the factor gate_cholesky leaves: the forward solve, then the back solve
DPGO_HD void gate_solve(const double L[6][6], double x[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double v = x[c];
#pragma unroll
    for (int q = 0; q < c; ++q) v = __builtin_fma(-L[c][q], x[q], v);
    x[c] = v * L[c][c];
  }
#pragma unroll
  for (int c = 5; c >= 0; --c) {
    double v = x[c];
#pragma unroll
    for (int q = c + 1; q < 6; ++q) v = __builtin_fma(-L[q][c], x[q], v);
    x[c] = v * L[c][c];
  }
}

// d2 = x^T D^-1 x of the symmetric D, which is left alone; +inf for a non-positive pivot
DPGO_HD double gate_distance(const double D[6][6], const double x[6]) {
  double L[6][6], y[6];
  bool ok;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) L[a][b] = D[a][b];
  gate_cholesky(L, ok);
  const double dd = gate_forward(L, x, y);
  return ok && dd >= 0.0 ? dd : (double)INFINITY;  // (a NaN is no distance either)
}

}  // namespace dpgo

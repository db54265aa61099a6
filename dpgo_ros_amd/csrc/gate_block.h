// gate_block.h -- the relative-pose arithmetic of the Mahalanobis gate, shared by k_gate (gate.hip) and by the
// segment kernel of the pairwise-consistency call (consistency.hip): one text, so the relative covariance of a
// pose pair has the same bits wherever it is formed.  gate_log_so3 also compiles for the host (consistency_block.h).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DPGO_HD __host__ __device__ __forceinline__
#else
#define DPGO_HD inline
#endif

namespace dpgo {

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

#if defined(__HIPCC__)

// 36 doubles, row-major.  (8-byte loads: where a path stages its blocks depends on the parity of its scratch in front of them)
__device__ __forceinline__ void gate_load36(const double *p, double B[6][6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) B[a][b] = gp(p)[6 * a + b];
}

// pose g of T: R[b][c] = T[(4 g + c) 3 + b], t[b] = T[(4 g + 3) 3 + b]
__device__ __forceinline__ void gate_load_pose(const double *T, int g, double R[3][3], double t[3]) {
  double v[12];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double2 w = ld2(T + (size_t)12 * g + 2 * q);
    v[2 * q] = w.x;
    v[2 * q + 1] = w.y;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[b][c] = v[3 * c + b];
#pragma unroll
  for (int b = 0; b < 3; ++b) t[b] = v[9 + b];
}

// A += X B Y^T (all 6 x 6, every index static after unrolling: the zeros of the Jacobians fold away)
__device__ __forceinline__ void gate_sandwich(const double X[6][6], const double B[6][6], const double Y[6][6], double A[6][6]) {
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

// The relative pose of the team poses i != j of T (M = R_ij, tij = t_ij) and its covariance S = Sigma_rel, bitwise symmetric,
// from the staged blocks: diag (36 per pose) and the pair block blk of `pairs`, which holds Sigma_ij.
__device__ __forceinline__ void gate_relative(const double *T, const double *diag, const double *pairs, int i, int j, int blk,
                                              double M[3][3], double tij[3], double S[6][6]) {
  double Ri[3][3], Rj[3][3], ti[3], tj[3];
  gate_load_pose(T, i, Ri, ti);
  gate_load_pose(T, j, Rj, tj);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) M[a][b] = __builtin_fma(Ri[2][a], Rj[2][b], __builtin_fma(Ri[1][a], Rj[1][b], Ri[0][a] * Rj[0][b]));
    tij[a] = __builtin_fma(Ri[2][a], tj[2] - ti[2], __builtin_fma(Ri[1][a], tj[1] - ti[1], Ri[0][a] * (tj[0] - ti[0])));
  }
  double Ji[6][6], Jj[6][6];
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

#endif  // __HIPCC__

}  // namespace dpgo

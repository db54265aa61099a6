// gate_joint_block.h -- the block arithmetic of the joint gate of a set of candidates: what k_joint_blocks and
// k_joint_step (gate_joint.hip) do with the staged covariance blocks and with the rows of the factor, in the primitives of
// gate_block.h (poses, Jacobians, sandwich, innovation, Cholesky, solves, distance).  It compiles for the device and for the
// host, so the same text is checked on a machine without a GPU (tests/test_gate_joint_host.py).
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

// the staged pair block of the poses of rank a < b among m
DPGO_HD size_t joint_pair_index(int m, int a, int b) { return (size_t)a * m - (size_t)a * (a + 1) / 2 + (size_t)(b - a - 1); }

// B = Sigma_ab for the poses (pa, pb) of ranks (a, b): the diagonal block, the staged pair block or its transpose
DPGO_HD void joint_load_sigma(const double *diag, const double *pairs, int m, int pa, int a, int b, double B[6][6]) {
  const bool tr = b < a;
  const double *p = a == b ? diag + (size_t)36 * pa : pairs + (size_t)36 * joint_pair_index(m, tr ? b : a, tr ? a : b);
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int y = 0; y < 6; ++y) B[x][y] = GATE_LD(p, tr ? 6 * y + x : 6 * x + y);
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
  gate_sandwich(k.Ji, B, l.Ji, G);
  joint_load_sigma(diag, pairs, m, k.i, k.ri, l.rj, B);
  gate_sandwich(k.Ji, B, l.Jj, G);
  joint_load_sigma(diag, pairs, m, k.j, k.rj, l.ri, B);
  gate_sandwich(k.Jj, B, l.Ji, G);
  joint_load_sigma(diag, pairs, m, k.j, k.rj, l.rj, B);
  gate_sandwich(k.Jj, B, l.Jj, G);
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

// log det S = 2 sum log L_cc from the factor gate_cholesky leaves
DPGO_HD double joint_logdet(const double L[6][6]) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) s -= log(L[c][c]);
  return 2.0 * s;
}

// G -= A B^T, A and B 36 doubles row-major in memory (one earlier column of the factor at this row and at the pivot's)
DPGO_HD void joint_subtract_product(const double *A, const double *B, double G[6][6]) {
  double a[6][6], b[6][6];
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int y = 0; y < 6; ++y) { a[x][y] = GATE_LD(A, 6 * x + y); b[x][y] = GATE_LD(B, 6 * x + y); }
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
  return gate_distance(D, x);
}

#if defined(__HIPCC__)

// the endpoints of the record c (w0, w1: the ranks of its poses), their Jacobians, and the relative pose (Rij, tij)
__device__ __forceinline__ void joint_ends(const double *T, const GateRec *c, JointEnds &e, double Rij[3][3], double tij[3]) {
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  const v4i_t ids = *(const __attribute__((address_space(1))) v4i_t *)c;
  e.i = ids.x; e.j = ids.y; e.ri = ids.z; e.rj = ids.w;
  double Ri[3][3], Rj[3][3], ti[3], tj[3];
  gate_load_pose(T, e.i, Ri, ti);
  gate_load_pose(T, e.j, Rj, tj);
  gate_jacobians(Ri, ti, Rj, tj, Rij, tij, e.Ji, e.Jj);
}

// The assembly of M = A Sigma A^T + R (order 6 K, leading dimension 6 K) and of xi, the body of a kernel of 256 lanes: one lane
// per block (k, l) with k <= l, K^2 lanes of which the lower triangle rests, grid-stride.  fp64 in registers, no LDS, no
// atomics: the lane writes the block and its transpose, so M is bitwise symmetric.  Which of the two a lane forms, (kk, ll),
// follows from the endpoints (joint_orientation).  form(ek, ll, G): G = the block (kk, ll) less Sigma_meas, ek the ends of
// record kk.  The lanes of the diagonal hand S = (G + G^T) / 2 + Sigma_meas and xi_k to diagonal(k, S, x) for what the kernel
// writes beside them, and store both.
template <class Form, class Diagonal>
__device__ __forceinline__ void joint_assemble(const double *__restrict__ T, const GateRec *__restrict__ cand, int K, double *__restrict__ M,
                                               double *__restrict__ xi, Form form, Diagonal diagonal) {
  const size_t total = (size_t)K * K, ld = (size_t)6 * K;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int k = (int)(t / K), l = (int)(t % K);
    if (l < k) continue;
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const v2i_t pk = *(const __attribute__((address_space(1))) v2i_t *)(cand + k), pl = *(const __attribute__((address_space(1))) v2i_t *)(cand + l);
    const int way = joint_orientation(pk.x, pk.y, pl.x, pl.y);
    const int kk = way < 0 ? l : k, ll = way < 0 ? k : l;
    JointEnds ek;
    double Rij[3][3], tij[3], G[6][6];
    joint_ends(T, cand + kk, ek, Rij, tij);
    form(ek, ll, G);
    if (k != l) {
      if (way == 0) joint_symmetrise(G);
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          gp(M)[((size_t)6 * kk + a) * ld + (size_t)6 * ll + b] = G[a][b];
          gp(M)[((size_t)6 * ll + b) * ld + (size_t)6 * kk + a] = G[a][b];
        }
      continue;
    }
    double v[GATE_MEAS], S[6][6], x[6];
    gate_load_meas(cand[k].m, v);
    joint_diagonal(G, v[12], v[13], S);
    gate_innovation(Rij, tij, v, x);
    diagonal(k, S, x);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) gp(M)[((size_t)6 * k + a) * ld + (size_t)6 * k + b] = S[a][b];
      gp(xi)[(size_t)6 * k + a] = x[a];
    }
  }
}

#endif  // __HIPCC__

// the candidate that a greedy step takes: the smaller d2, the lower index on ties; an index < 0 is no candidate
DPGO_HD void joint_better(double d, int k, double &best, int &arg) {
  if (k >= 0 && (arg < 0 || d < best || (d == best && k < arg))) { best = d; arg = k; }
}

}  // namespace dpgo

// refine_block.h -- the per-pose and per-edge arithmetic of the Newton refinement of a trajectory on SE(3): what
// k_refine_grad, k_refine_trials and k_refine_cost (refine.hip) do with a pose.  In the idiom of apply_block.h and
// linear_update_block.h, whose retraction it uses: statically indexed arrays, compiled for the device and for the host, so the
// same text is checked on a machine without a GPU (tests/test_refine_host.py).
//
// T and E = T Q are K = 3 blocks of the iterate layout, 12 doubles per pose: R[b][c] at [3 c + b], t[b] at [9 + b].  Pose p is
// perturbed by xi_p = (phi_p, delta_p): R_p <- R_p Exp(phi_p) (body frame), t_p <- t_p + delta_p (world frame); pose 0 is fixed
// (across teams: the problem's pose 0 on its holder, no pose elsewhere -- the functions take the fixed team pose, -1 for none).
//   gradient   g_p = J_p^T vec(E_p).  Column c of Tdot_p is -R_p [e_c]x phi_p, so the rotation rows are
//              sum_c (-R_p [e_c]x)^T E_p^c = sum_c e_c x (R_p^T E_p^c): with M = R_p^T E_p,rot
//                  g_0 = M[2][1] - M[1][2],  g_1 = M[0][2] - M[2][0],  g_2 = M[1][0] - M[0][1],
//              each one chain of six fused multiply-adds (no difference of two rounded dot products); the translation rows are
//              the translation column of E_p; pose 0's rows are zero
//   trial      T_p [+] (-alpha x_p) by upd_retract (linear_update_block.h); pose 0 is copied
//   edge       w / 2 (kappa |R_j - R_i R~|_F^2 + tau |t_j - t_i - R_i t~|^2), the term of f = 1/2 <T, T Q> that belongs to one
//              measurement: not negative, so a sum of them is known to a multiple of u f
#pragma once
#include "linear_update_block.h"

namespace dpgo {

// the six rows of pose p (the fixed pose: zeros) from its R and the 12 doubles of E_p.  fixed: the team pose that is held fixed, or
// -1 for none (a participant of a split team that does not hold the problem's pose 0)
DPGO_HD void refine_grad_rows(int p, int fixed, const double R[3][3], const double Ep[12], double g[6]) {
  // M[k][c] = sum_b R[b][k] E[b][c],  E[b][c] = Ep[3 c + b]
  // g_a = M[a2][a1] - M[a1][a2] with (a, a1, a2) cyclic
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    double s = R[0][a2] * Ep[3 * a1];
    s = __builtin_fma(-R[0][a1], Ep[3 * a2], s);
    s = __builtin_fma(R[1][a2], Ep[3 * a1 + 1], s);
    s = __builtin_fma(-R[1][a1], Ep[3 * a2 + 1], s);
    s = __builtin_fma(R[2][a2], Ep[3 * a1 + 2], s);
    s = __builtin_fma(-R[2][a1], Ep[3 * a2 + 2], s);
    g[a] = p == fixed ? 0.0 : s;
    g[3 + a] = p == fixed ? 0.0 : Ep[9 + a];
  }
}
// (one team: its pose 0)
DPGO_HD void refine_grad_rows(int p, const double R[3][3], const double Ep[12], double g[6]) { refine_grad_rows(p, 0, R, Ep, g); }

// the 12 doubles of the trial pose T_p [+] (-alpha x): P in the layout of T; the fixed pose (-1: none) is copied
DPGO_HD void refine_trial_pose(int p, int fixed, const double R[3][3], const double t[3], const double x[6], double alpha, double P[12]) {
  double dx[6], Rn[3][3], tn[3];
#pragma unroll
  for (int a = 0; a < 6; ++a) dx[a] = -alpha * x[a];
  upd_retract(R, t, dx, Rn, tn);
  if (p == fixed) {
    upd_store_pose(R, t, P);
    return;
  }
  upd_store_pose(Rn, tn, P);
}
DPGO_HD void refine_trial_pose(int p, const double R[3][3], const double t[3], const double x[6], double alpha, double P[12]) {
  refine_trial_pose(p, 0, R, t, x, alpha, P);
}

// one measurement's term of the cost; v: R~ row-major (9), t~ (3), w kappa, w tau
DPGO_HD double refine_edge_cost(const double Ri[3][3], const double ti[3], const double Rj[3][3], const double tj[3], const double *v) {
  const double *Rm = v, *tm = v + 9;
  double sr = 0.0, st = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double r = Rj[a][b] - __builtin_fma(Ri[a][2], Rm[6 + b], __builtin_fma(Ri[a][1], Rm[3 + b], Ri[a][0] * Rm[b]));
      sr = __builtin_fma(r, r, sr);
    }
    const double d = (tj[a] - ti[a]) - __builtin_fma(Ri[a][2], tm[2], __builtin_fma(Ri[a][1], tm[1], Ri[a][0] * tm[0]));
    st = __builtin_fma(d, d, st);
  }
  return 0.5 * __builtin_fma(v[12], sr, v[13] * st);
}

}  // namespace dpgo

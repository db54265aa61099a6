// apply_block.h -- the right-hand side V = A^T of the first-order update on the solve: what
// k_apply_rhs_closures (linear_update.hip) writes for one closure.  In the idiom of linear_update_block.h, whose Jacobians it
// takes (gate_jacobians, as k_lin_b does): statically indexed 6 x 6 arrays, compiled for the device and for the host, so the
// same text is checked on a machine without a GPU (tests/test_apply_host.py).
//
// A is the joint gate's (gate_joint.hip): row block k holds J_i^k at the columns of pose i_k and J_j^k at those of pose j_k.
// V is 6 N x 6 K, column-major with leading dimension ld = 6 N, zero before the closures are written:
//   V[6 i_k + a, 6 k + c] = J_i^k[c][a],   V[6 j_k + a, 6 k + c] = J_j^k[c][a],   a, c = 0 .. 5,
// and the rows of pose 0 stay zero (the covariance paths do not read them: Sigma's rows and columns of pose 0 are zero).
// Column block k belongs to closure k alone, so duplicated closures and a pair and its reverse write disjoint elements.
#pragma once
#include "gate_block.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define APPLY_ST(p, i, v) (gp(p)[i] = (v))
#else
#define APPLY_ST(p, i, v) ((p)[i] = (v))
#endif

namespace dpgo {

// J^T into column block k of V at the rows of pose p; nothing for pose 0
DPGO_HD void apply_rhs_block(const double J[6][6], int p, int k, size_t ld, double *V) {
  if (p == 0) return;
  double *o = V + (size_t)6 * k * ld + (size_t)6 * p;
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int a = 0; a < 6; ++a) APPLY_ST(o, c * ld + a, J[c][a]);
}

// the two blocks of closure k, joining the poses i and j
DPGO_HD void apply_rhs_closure(const double Ji[6][6], const double Jj[6][6], int i, int j, int k, size_t ld, double *V) {
  apply_rhs_block(Ji, i, k, ld, V);
  apply_rhs_block(Jj, j, k, ld, V);
}

}  // namespace dpgo

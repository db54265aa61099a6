// linear_update.hip -- the estimate and its covariances updated to first order for a set of new closures, without a re-solve
// (DESIGN.md 5j): the information-filter update, in covariance form, of the whole trajectory.
//
// T, Sigma, the perturbation, J_i, J_j, xi with no Log-Jacobian, and Sigma_meas are 5f's (gate.hip): R_p <- R_p Exp(phi_p) in
// the body frame and t_p <- t_p + delta_p in the world frame, pose 0 fixed; as in the gate the weight of a closure is not read.
// A and R are 5i's (gate_joint.hip).  K closures on m distinct endpoint poses e_0 < ... < e_{m-1}.
//   B_p,k = Sigma_{p,i_k} J_i^k^T + Sigma_{p,j_k} J_j^k^T, a 6 x 6 block, p = 0 .. N - 1; a Sigma block that names pose 0 is zero,
//           so B_0 = 0
//   M_kl  = J_i^k B_{i_k,l} + J_j^k B_{j_k,l} + delta_kl Sigma_meas,k; the diagonal blocks stored symmetrised; M stored bitwise
//           symmetric: one lane writes a block and its transpose, the side from which a block is formed chosen by the
//           endpoints, as joint_orientation does
//   G     = M^-1 from dense_spd_inverse;  z = G xi;  U = B G
//   dx_p  = -B_p z;  xi_post = R z, which equals xi + A dx
//   Sigma'_pp = Sigma_pp - U_p B_p^T, the upper triangle formed and mirrored;  Sigma'_pq = Sigma_pq - U_p B_q^T per requested pair
//   T'_p  = (R_p Exp(phi_p), t_p + delta_p), Rodrigues, the series below a threshold angle
//   d2_joint = xi^T z;  logdet_M from the Cholesky factor;  logdet_R = sum_k -3 log(2 kappa_k) - 3 log tau_k;
//   information_gain = (logdet_M - logdet_R) / 2
// Every sum runs in index order with __builtin_fma; no floating-point atomics: two calls give the same bytes.
//
// The covariance path is asked for the rectangular set: for each endpoint rank a and each pose p the pair block a N + p =
// Sigma_{p, e_a}, the caller's own pairs behind them.  The step behind it is linear_frame.h's, shared with the removal
// (linear_removal.hip): k_lin_b<false> forms B (column-major, leading dimension 6 N) behind the staged blocks, k_upd_m forms M
// and xi, dense_spd_inverse inverts M in place of a copy (its factor stays for the log det), k_lin_u is U = B G on the fp64
// matrix cores through dgemm_tile, k_upd_z forms z and xi_post, k_upd_scalars the three figures, and k_lin_finish<false>, one
// wave per pose or requested pair, reduces the 6 K columns and writes T', dx and the blocks of Sigma'.
// B, U, M and G stay on the device; only the outputs go to the host.
//
// On the solve (dpgo_team_linear_update_solved) the path is asked for the caller's own pairs alone and is handed
// a CovApply: k_apply_rhs_closures writes V = A^T (apply_block.h) once T is on the device, the path forms X = Sigma V on its
// factors, and that X is B.  k_lin_b is skipped; k_upd_m onward runs unchanged on that B.  The sums of B come in another order
// than on the rectangular set, so the outputs of the two routes agree to round-off, not bitwise.
#include "linear_frame.h"
#include "apply_block.h"

namespace dpgo {

// V = A^T into a zeroed V (6 N x 6 K, column-major, leading dimension 6 N): one lane per closure, grid-stride; J_i^T and J_j^T
// of closure k go into column block k at the rows of its endpoints (apply_rhs_closure), pose 0's rows stay zero
__global__ __launch_bounds__(256) void k_apply_rhs_closures(const double *__restrict__ T, const GateRec *__restrict__ cand, int N, int K,
                                                            double *__restrict__ V) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
    JointEnds e;
    double Rij[3][3], tij[3];
    joint_ends(T, cand + k, e, Rij, tij);
    if (e.i < 0 || e.i >= N || e.j < 0 || e.j >= N) continue;  // (the call has checked the endpoints on the host)
    apply_rhs_closure(e.Ji, e.Jj, e.i, e.j, k, (size_t)6 * N, V);
  }
}

// M by joint_assemble from B (upd_m_block), and xi; the lanes of the diagonal write nothing else
__global__ __launch_bounds__(256) void k_upd_m(const double *__restrict__ T, const GateRec *__restrict__ cand, int K, int N,
                                               const double *__restrict__ B, double *__restrict__ M, double *__restrict__ xi) {
  const size_t ldb = (size_t)6 * N;
  joint_assemble(
      T, cand, K, M, xi,
      [=](const JointEnds &ek, int ll, double G[6][6]) __attribute__((always_inline)) { upd_m_block(B, ldb, ek, ll, G); },
      [](int, const double[6][6], const double[6]) __attribute__((always_inline)) {});
}

// z = G xi, one lane per row, the sum over the columns in index order (G is bitwise symmetric: the element (r, c) is read at
// (c, r), consecutive lanes consecutive addresses), and xi_post = R z beside it
__global__ __launch_bounds__(256) void k_upd_z(const double *__restrict__ G, const double *__restrict__ xi, const GateRec *__restrict__ cand,
                                               int n, double *__restrict__ z, double *__restrict__ xi_post) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s = __builtin_fma(gp(G)[(size_t)c * n + r], gp(xi)[c], s);
    gp(z)[r] = s;
    const double *rec = (const double *)(cand + r / 6);
    gp(xi_post)[r] = s * (r % 6 < 3 ? 1.0 / (2.0 * gp(rec)[14]) : 1.0 / gp(rec)[15]);
  }
}

// the three figures by one lane: d2_joint = xi^T z and logdet_R in index order, logdet_M as k_cov_logdet left it in ld
__global__ __launch_bounds__(64) void k_upd_scalars(const double *__restrict__ xi, const double *__restrict__ z, const GateRec *__restrict__ cand,
                                                    int K, const double *__restrict__ ld, double *__restrict__ scal) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double d = 0.0, lr = 0.0;
  for (int c = 0; c < 6 * K; ++c) d = __builtin_fma(gp(xi)[c], gp(z)[c], d);
  for (int k = 0; k < K; ++k) {
    const double *rec = (const double *)(cand + k);
    lr += upd_logdet_meas(gp(rec)[14], gp(rec)[15]);
  }
  gp(scal)[0] = d;
  gp(scal)[1] = gp(ld)[0];
  gp(scal)[2] = lr;
  gp(scal)[3] = 0.0;
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall UPDATE = {"linear_update", "closure"};

// the update behind the shared step: M and xi by k_upd_m, the refusal of a non-positive pivot, z, xi_post and the three
// figures.  d_out behind xi: xi_post (6 K), 4 figures.  d_work: z (6 K), the log det's 4
struct UpdateEpilogue : LinearEpilogue<false> {
  UpdateEpilogue() : LinearEpilogue<false>(UPDATE) {}
  size_t tail_doubles() const override { return 6 * K() + 4; }
  size_t work_doubles() const override { return 6 * K() + 4; }
  double bytes(double N, double K, double P) const override {
    return 2.0 * 288.0 * N * K + 3.0 * 288.0 * K * K + 8.0 * (54.0 * N + 36.0 * P + 18.0 * K + 8.0) + 128.0 * K + 8.0 * P;
  }
  void assemble(const CovStage &st, const double *B) override {
    const size_t k = K();
    k_upd_m<<<(unsigned)std::min<size_t>((k * k + 255) / 256, 2048), 256, 0, st.stream>>>(st.Td, d_cand.p, (int)k, N, B, d_M.p, oxi);
  }
  int after_inverse(hipStream_t, int fail) override {
    if (fail > 0)
      return call.refuse("non-positive pivot at row " + std::to_string(fail - 1) + " of M (pivot block " + std::to_string((fail - 1) / 6) +
                         ", the block of closure " + std::to_string((fail - 1) / 6) + "): M = A Sigma A^T + R is not positive definite at this T");
    return DPGO_OK;
  }
  void z_and_figures(hipStream_t s) override {
    const int n = (int)(6 * K());
    k_upd_z<<<(unsigned)std::min<size_t>((n + 255) / 256, 2048), 256, 0, s>>>(d_G.p, oxi, d_cand.p, n, z, otail);
    k_upd_scalars<<<1, 64, 0, s>>>(oxi, z, d_cand.p, (int)K(), ldet, otail + n);
  }
};

// the hook of the solve: the records to the device, V cleared, V = A^T
struct UpdateRhs : CovApply {
  UpdateEpilogue *e = nullptr;
  int rhs(const double *Td, int N, double *V, hipStream_t s) override {
    const size_t k = e->K();
    if (N != e->N) { set_err("linear_update: the covariance path's poses are not the call's"); return DPGO_ERR; }
    HIPC(hipMemcpyAsync(e->d_cand.p, e->cand.data(), sizeof(GateRec) * k, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(V, 0, sizeof(double) * 36 * (size_t)N * k, s));
    k_apply_rhs_closures<<<(unsigned)std::min<size_t>((k + 255) / 256, 2048), 256, 0, s>>>(Td, e->d_cand.p, N, (int)k, V);
    HIPC(hipGetLastError());
    return DPGO_OK;
  }
};

int linear_update_call(const LinearArgs &a, double *xi_post, double *scalars, bool solved) {
  const auto t_begin = std::chrono::steady_clock::now();
  UpdateEpilogue epi;
  UpdateRhs hook;
  hook.e = &epi;
  const auto no_schur_solve = [&]() -> int {
    if (solved && a.method == DPGO_GATE_SCHUR)
      return UPDATE.refuse("there is no solve on the robot-wise Schur path: DPGO_GATE_NESTED (method=\"nested\") with no robot split has "
                           "the Schur path's sets");
    return DPGO_OK;
  };
  if (const int rc = linear_call(a, !xi_post || !scalars, epi, solved ? &hook : nullptr, no_schur_solve,
                                 [](int, const dpgo_measurement_t &) { return DPGO_OK; }))
    return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing) {  // (the fields keep the names the profiles quote: k_upd_b, k_upd_u and k_upd_finish are linear_frame.h's kernels)
    float ms[6];
    for (int q = 0; q < 6; ++q) ms[q] = epi.ev.ms(q, q + 1);
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "linear_update: %d closures on %d of %d poses (%zu pair blocks), k_upd_b %.3f ms, k_upd_m %.3f ms, inverse %.3f ms, "
                         "k_upd_u %.3f ms, k_upd_z and figures %.3f ms, k_upd_finish %.3f ms, the whole call %.3f ms\n",
                 a.num, epi.m, epi.N, epi.rect() + (size_t)a.num_pairs, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], whole);
    if (solved)
      std::fprintf(stderr, "linear_update (solve): B = Sigma A^T of %d columns inside the path, the apply's products %.3f ms (%.2f TFLOP/s)\n",
                   6 * a.num, hook.ms_products, hook.flops / (1e9 * std::max(hook.ms_products, 1e-9)));
  }
  const size_t K = (size_t)a.num;
  const double *hp = a.copy_head(epi.h_out, epi.N);
  std::memcpy(xi_post, hp, sizeof(double) * 6 * K);
  std::memcpy(scalars, hp + 6 * K, sizeof(double) * 3);
  return DPGO_OK;
}
}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_linear_update(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                       const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new, double *delta,
                                       double *cov_diag, double *cov_pairs, double *xi, double *xi_post, double *scalars,
                                       dpgo_covariance_t *res) {
  return linear_update_call({t, T, method, max_block, num, closures, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, res}, xi_post,
                            scalars, false);
}

extern "C" int dpgo_team_linear_update_solved(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                              const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new,
                                              double *delta, double *cov_diag, double *cov_pairs, double *xi, double *xi_post,
                                              double *scalars, dpgo_covariance_t *res) {
  return linear_update_call({t, T, method, max_block, num, closures, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, res}, xi_post,
                            scalars, true);
}

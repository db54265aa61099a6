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
// Sigma_{p, e_a}, the caller's own pairs behind them.  k_upd_b forms B (column-major, leading dimension 6 N) behind the staged
// blocks, k_upd_m forms M and xi, dense_spd_inverse inverts M in place of a copy (its factor stays for the log det), k_upd_u is
// U = B G on the fp64 matrix cores through dgemm_tile, k_upd_z forms z and xi_post, k_upd_scalars the three figures, and
// k_upd_finish, one wave per pose or requested pair, reduces the 6 K columns and writes T', dx and the blocks of Sigma'.
// B, U, M and G stay on the device; only the outputs go to the host.
//
// On the solve (dpgo_team_linear_update_solved) the path is asked for the caller's own pairs alone and is handed
// a CovApply: k_apply_rhs_closures writes V = A^T (apply_block.h) once T is on the device, the path forms X = Sigma V on its
// factors, and that X is B.  k_upd_b is skipped; k_upd_m onward runs unchanged on that B.  The sums of B come in another order
// than on the rectangular set, so the outputs of the two routes agree to round-off, not bitwise.
#include <algorithm>
#include <chrono>

#include "closure_frame.h"
#include "covariance_schur.h"
#include "linear_update_block.h"
#include "apply_block.h"

namespace dpgo {

// One lane per (p, k), p the faster index, grid-stride: the closure's Jacobians from T, the two staged blocks Sigma_{p,i_k}
// and Sigma_{p,j_k}, the two products, and the block B_p,k.  Consecutive lanes read consecutive staged blocks and store
// consecutive runs of 48 bytes of every column of B.
__global__ __launch_bounds__(256) void k_upd_b(const double *__restrict__ T, const double *__restrict__ blocks,
                                               const GateRec *__restrict__ cand, int N, int K, double *__restrict__ B) {
  const size_t total = (size_t)N * K, ld = (size_t)6 * N;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int k = (int)(t / N), p = (int)(t % N);
    JointEnds e;
    double Rij[3][3], tij[3], Si[6][6], Sj[6][6], Bk[6][6];
    joint_ends(T, cand + k, e, Rij, tij);
    gate_load36(blocks + 36 * upd_block_index(N, e.ri, p), Si);
    gate_load36(blocks + 36 * upd_block_index(N, e.rj, p), Sj);
    upd_b_block(Si, Sj, e.Ji, e.Jj, Bk);
    double *o = B + (size_t)6 * k * ld + (size_t)6 * p;
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int a = 0; a < 6; ++a) gp(o)[c * ld + a] = Bk[a][c];
  }
}

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

// U = B G: B 6 N x 6 K and U column-major with leading dimension 6 N, G of order 6 K; one workgroup per 64 x 64 tile of U
__global__ __launch_bounds__(256) void k_upd_u(const double *__restrict__ B, const double *__restrict__ G, double *__restrict__ U, int m, int n) {
  dgemm_tile<false>(B, m, G, n, U, m, m, n, n, 0, 64 * (int)blockIdx.x, 64 * (int)blockIdx.y);
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

// The reduction over the 6 K columns, one wave per pose and, in a second range of waves, per requested pair.  Lane l takes
// the columns l, l + 64, ... in index order: rows 6 p .. 6 p + 5 of column c of U and of B are 48 contiguous bytes each.  A
// pose's lane accumulates the 21 sums of the upper triangle of U_p B_p^T and the 6 of B_p z; a pair's the 36 of U_p B_q^T.
// The lanes' sums meet in an xor butterfly of fixed order (addition commutes: every lane ends with the same bits), and lane 0
// subtracts from the staged block, retracts and writes T'_p, dx_p and Sigma'_pp, or Sigma'_pq.  fp64 in registers, no LDS.
__global__ __launch_bounds__(256) void k_upd_finish(const double *__restrict__ T, const double *__restrict__ diag,
                                                    const double *__restrict__ pair_blocks, const int *__restrict__ pairs, int N, int K,
                                                    int num_pairs, const double *__restrict__ B, const double *__restrict__ U,
                                                    const double *__restrict__ z, double *__restrict__ T_new, double *__restrict__ delta,
                                                    double *__restrict__ out_diag, double *__restrict__ out_pairs) {
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), ld = (size_t)6 * N;
  const int lane = threadIdx.x & 63, n = 6 * K;
  if (w >= (size_t)N + (size_t)num_pairs) return;
  if (w < (size_t)N) {
    const int p = (int)w;
    double acc[UPD_SUMS];
#pragma unroll
    for (int q = 0; q < UPD_SUMS; ++q) acc[q] = 0.0;
    for (int c = lane; c < n; c += 64) {
      double u[6], b[6];
      gate_load_pairs<3>(U + (size_t)c * ld + (size_t)6 * p, u);
      gate_load_pairs<3>(B + (size_t)c * ld + (size_t)6 * p, b);
      upd_accumulate(u, b, gp(z)[c], acc);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1)
#pragma unroll
      for (int q = 0; q < UPD_SUMS; ++q) acc[q] += __shfl_xor(acc[q], off);
    if (lane != 0) return;
    double Sn[6][6], dx[6], R[3][3], t[3], Rn[3][3], tn[3], P[12];
    upd_close_pose(diag + (size_t)36 * p, acc, Sn, dx);
    gate_load_pose(T, p, R, t);
    upd_retract(R, t, dx, Rn, tn);
    upd_store_pose(Rn, tn, P);
#pragma unroll
    for (int q = 0; q < 12; ++q) gp(T_new)[(size_t)12 * p + q] = P[q];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      gp(delta)[(size_t)6 * p + a] = dx[a];
#pragma unroll
      for (int c = 0; c < 6; ++c) gp(out_diag)[(size_t)36 * p + 6 * a + c] = Sn[a][c];
    }
    return;
  }
  const size_t e = w - (size_t)N;
  const int p = gp(pairs)[2 * e], q = gp(pairs)[2 * e + 1];
  double acc[36];
#pragma unroll
  for (int x = 0; x < 36; ++x) acc[x] = 0.0;
  for (int c = lane; c < n; c += 64) {
    double u[6], b[6];
    gate_load_pairs<3>(U + (size_t)c * ld + (size_t)6 * p, u);
    gate_load_pairs<3>(B + (size_t)c * ld + (size_t)6 * q, b);
    upd_accumulate_pair(u, b, acc);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1)
#pragma unroll
    for (int x = 0; x < 36; ++x) acc[x] += __shfl_xor(acc[x], off);
  if (lane != 0) return;
#pragma unroll
  for (int x = 0; x < 36; ++x) gp(out_pairs)[36 * e + x] = gp(pair_blocks)[36 * e + x] - acc[x];
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall UPDATE = {"linear_update", "closure"};

// the step behind a covariance path's staged blocks: upload the records, form B and M, invert, multiply, reduce, queue the
// copy of the outputs
struct UpdateEpilogue : ClosureEpilogue {
  std::vector<GateRec> cand;  // w0, w1: the ranks of i and j among the endpoints
  std::vector<int> user_pairs;  // the caller's pairs, behind the N m blocks of the call
  int m = 0, N = 0;
  const CovApply *solve = nullptr;  // on the solve: the path's X is B, and the records are already on the device
  DevBuf<GateRec> d_cand;
  DevBuf<double> d_B, d_U, d_M, d_W, d_G, d_work, d_out;
  DevBuf<int> d_pairs;
  std::vector<double> h_out;  // T' (12 N), dx (6 N), Sigma' diagonal (36 N), Sigma' pairs (36 P), xi (6 K), xi_post (6 K), 4 figures
  UpdateEpilogue() : ClosureEpilogue(7) {}
  size_t K() const { return cand.size(); }
  size_t P() const { return user_pairs.size() / 2; }
  size_t out_doubles() const { return (size_t)54 * N + 36 * P() + 12 * K() + 4; }
  static double bytes(double N, double K, double P) {
    return 2.0 * 288.0 * N * K + 3.0 * 288.0 * K * K + 8.0 * (54.0 * N + 36.0 * P + 18.0 * K + 8.0) + 128.0 * K + 8.0 * P;
  }
  int alloc() {
    const size_t k = K();
    if (d_cand.alloc(k) || (!solve && d_B.alloc((size_t)36 * N * k)) || d_U.alloc((size_t)36 * N * k) || d_M.alloc(36 * k * k) || d_W.alloc(36 * k * k) ||
        d_G.alloc(36 * k * k) || d_work.alloc(6 * k + 4) || d_out.alloc(out_doubles()) || d_pairs.alloc(2 * P())) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "linear_update: device allocation failed (%.0f bytes for %zu closures on %d poses)",
                    bytes(N, (double)k, (double)P()), k, N);
      set_err(buf);
      return DPGO_ERR;
    }
    return ev.create();
  }
  int run(const CovStage &st) override {
    const size_t k = K(), np = P();
    const size_t nrect = solve ? 0 : (size_t)N * m;
    if (solve && !solve->X) { set_err("linear_update: the covariance path formed no X"); return DPGO_ERR; }
    const double *B = solve ? solve->X : d_B.p;
    if (st.N != N || (size_t)st.num_pairs != nrect + np) {
      set_err("linear_update: the staged blocks are not the rectangular set of the endpoints");
      return DPGO_ERR;
    }
    for (const GateRec &c : cand)
      if (c.i < 0 || c.i >= N || c.j < 0 || c.j >= N || c.w0 < 0 || c.w0 >= m || c.w1 < 0 || c.w1 >= m || c.w0 == c.w1) {
        set_err("linear_update: a closure lies outside the staged blocks");
        return DPGO_ERR;
      }
    for (int p : user_pairs)
      if (p < 0 || p >= N) {
        set_err("linear_update: a pair lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    const int n = (int)(6 * k);
    if (!solve) HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateRec) * k, hipMemcpyHostToDevice, s));
    if (np) HIPC(hipMemcpyAsync(d_pairs.p, user_pairs.data(), sizeof(int) * 2 * np, hipMemcpyHostToDevice, s));
    double *oT = d_out.p, *odx = oT + (size_t)12 * N, *odiag = odx + (size_t)6 * N, *opairs = odiag + (size_t)36 * N;
    double *oxi = opairs + 36 * np, *opost = oxi + 6 * k, *oscal = opost + 6 * k;
    double *z = d_work.p, *ldet = z + 6 * k;
    HIPC(hipEventRecord(ev[0], s));
    // at most eight workgroups per CU of an MI355X: the lanes beyond stride over the rest
    if (!solve) k_upd_b<<<(unsigned)std::min<size_t>(((size_t)N * k + 255) / 256, 2048), 256, 0, s>>>(st.Td, st.pairs, d_cand.p, N, (int)k, d_B.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    k_upd_m<<<(unsigned)std::min<size_t>((k * k + 255) / 256, 2048), 256, 0, s>>>(st.Td, d_cand.p, (int)k, N, B, d_M.p, oxi);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[2], s));
    const int fail = dense_spd_inverse(s, d_M.p, d_W.p, d_G.p, n);  // (synchronises the stream; the factor stays in d_M)
    HIPC(hipGetLastError());
    if (fail < 0) { set_err("linear_update: scratch allocation of the inverse failed"); return DPGO_ERR; }
    if (fail > 0) {
      set_err("linear_update: non-positive pivot at row " + std::to_string(fail - 1) + " of M (pivot block " + std::to_string((fail - 1) / 6) +
              ", the block of closure " + std::to_string((fail - 1) / 6) + "): M = A Sigma A^T + R is not positive definite at this T");
      return DPGO_ERR;
    }
    HIPC(hipEventRecord(ev[3], s));
    if (launch_cov_logdet(s, d_M.p, n, ldet)) return DPGO_ERR;
    k_upd_u<<<dim3((unsigned)((6 * (size_t)N + 63) / 64), (unsigned)((n + 63) / 64), 1), 256, 0, s>>>(B, d_G.p, d_U.p, 6 * N, n);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[4], s));
    k_upd_z<<<(unsigned)std::min<size_t>((n + 255) / 256, 2048), 256, 0, s>>>(d_G.p, oxi, d_cand.p, n, z, opost);
    k_upd_scalars<<<1, 64, 0, s>>>(oxi, z, d_cand.p, (int)k, ldet, oscal);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[5], s));
    k_upd_finish<<<(unsigned)(((size_t)N + np + 3) / 4), 256, 0, s>>>(st.Td, st.diag, st.pairs + 36 * nrect, d_pairs.p, N, (int)k, (int)np,
                                                                     B, d_U.p, z, oT, odx, odiag, opairs);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[6], s));
    h_out.resize(out_doubles());
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, s));
    ran = true;
    return DPGO_OK;
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

int linear_update_call(dpgo_team_t *t, const double *T, int method, int max_block, int num, const dpgo_measurement_t *closures,
                       int num_pairs, const int *pairs, double *T_new, double *delta, double *cov_diag, double *cov_pairs, double *xi,
                       double *xi_post, double *scalars, dpgo_covariance_t *res, bool solved) {
  const auto t_begin = std::chrono::steady_clock::now();
  // ---- the refusals of the call itself: on the host, before any device work, no output touched
  if (!t || !T || !res || !T_new || !delta || !cov_diag || !xi || !xi_post || !scalars) return UPDATE.refuse("null argument");
  if (num <= 0) return UPDATE.refuse("num must be positive, not " + std::to_string(num));
  if (!closures) return UPDATE.refuse("null argument");
  if (num_pairs < 0) return UPDATE.refuse("num_pairs must not be negative, not " + std::to_string(num_pairs));
  if (num_pairs > 0 && (!pairs || !cov_pairs)) return UPDATE.refuse("null argument");
  if (UPDATE.check_method(method)) return DPGO_ERR;
  if (solved && method == DPGO_GATE_SCHUR)
    return UPDATE.refuse("there is no solve on the robot-wise Schur path: DPGO_GATE_NESTED (method=\"nested\") with no robot split has "
                         "the Schur path's sets");
  if (check_team_local(t, UPDATE.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  const int N = offs.back();
  UpdateEpilogue epi;
  epi.N = N;
  epi.cand.resize(num);
  for (int k = 0; k < num; ++k) {
    int g[2];
    if (UPDATE.endpoints(t, offs, k, closures[k], g) || UPDATE.check(k, closures[k])) return DPGO_ERR;
    GateRec &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    pack_measurement(closures[k], c.m);
  }
  for (int k = 0; k < 2 * num_pairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= N)
      return UPDATE.refuse("pair " + std::to_string(k / 2) + " names pose " + std::to_string(pairs[k]) + ", outside [0, " + std::to_string(N) + ")");
  const std::vector<int> poses = rank_endpoints(epi.cand);
  const int m = epi.m = (int)poses.size();
  const size_t K = (size_t)num, nb = solved ? 0 : (size_t)N * m, np = nb + (size_t)num_pairs;
  UpdateRhs hook;
  hook.e = &epi;
  hook.num_cols = 6 * num;
  if (solved) epi.solve = &hook;
  HIPC(hipSetDevice(t->device));
  {
    // the pair blocks the path stages for this call, B and U, M, the scratch of its inverse and G: the rest is the path's own
    // accounting
    const double blocks = 288.0 * (double)np, bu = 288.0 * (double)N * (double)K, mat = 288.0 * (double)K * (double)K;
    const double need = blocks + UpdateEpilogue::bytes(N, (double)K, num_pairs);
    double avail = 0.0;
    if (UPDATE.device_avail(t, &avail)) return DPGO_ERR;
    if (solved && (need - bu > avail || 36 * K * K > (size_t)1 << 40 || 6 * K > (size_t)INT32_MAX / 2)) {
      char buf[480];
      std::snprintf(buf, sizeof buf,
                    "%d closures on %d of %d poses: the %zu pair blocks, U (6 N x 6 K; V and B are the covariance path's) and the three "
                    "matrices of order %zu need %.0f bytes (%.0f + %.0f + 3 x %.0f and the working arrays), %.0f are available on the device",
                    num, m, N, np, 6 * K, need - bu, blocks, bu, mat, avail);
      return UPDATE.refuse(buf);
    }
    if (need > avail || np > (size_t)INT32_MAX || 36 * K * K > (size_t)1 << 40 || 6 * K > (size_t)INT32_MAX / 2) {
      char buf[480];
      std::snprintf(buf, sizeof buf,
                    "%d closures on %d of %d poses: the %zu pair blocks, B and U (6 N x 6 K each) and the three matrices of order %zu need "
                    "%.0f bytes (%.0f + 2 x %.0f + 3 x %.0f and the working arrays), %.0f are available on the device; the pair blocks must "
                    "number at most %d",
                    num, m, N, np, 6 * K, need, blocks, bu, mat, avail, INT32_MAX);
      return UPDATE.refuse(buf);
    }
  }
  // the rectangular set: block a N + p = Sigma_{p, e_a} (the paths check a pair for range only: p = e_a and p = 0 pass, the
  // first as the pair (i, i), which agrees with the diagonal block, the second as zeros); the caller's pairs behind them
  std::vector<int> all;
  all.reserve(2 * np);
  for (int a = 0; a < m && !solved; ++a)
    for (int p = 0; p < N; ++p) { all.push_back(p); all.push_back(poses[a]); }
  all.insert(all.end(), pairs, pairs + 2 * (size_t)num_pairs);
  epi.user_pairs.assign(pairs, pairs + 2 * (size_t)num_pairs);
  if (epi.alloc()) return DPGO_ERR;
  if (const int rc = UPDATE.path(t, T, method, max_block, (int)np, all.data(), res, epi, solved ? &hook : nullptr)) return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing) {
    float ms[6];
    for (int q = 0; q < 6; ++q) ms[q] = epi.ev.ms(q, q + 1);
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "linear_update: %d closures on %d of %d poses (%zu pair blocks), k_upd_b %.3f ms, k_upd_m %.3f ms, inverse %.3f ms, "
                         "k_upd_u %.3f ms, k_upd_z and figures %.3f ms, k_upd_finish %.3f ms, the whole call %.3f ms\n",
                 num, m, N, np, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], whole);
    if (solved)
      std::fprintf(stderr, "linear_update (solve): B = Sigma A^T of %d columns inside the path, the apply's products %.3f ms (%.2f TFLOP/s)\n",
                   6 * num, hook.ms_products, hook.flops / (1e9 * std::max(hook.ms_products, 1e-9)));
  }
  const double *h = epi.h_out.data();
  std::memcpy(T_new, h, sizeof(double) * 12 * (size_t)N);
  std::memcpy(delta, h + (size_t)12 * N, sizeof(double) * 6 * (size_t)N);
  std::memcpy(cov_diag, h + (size_t)18 * N, sizeof(double) * 36 * (size_t)N);
  const double *hp = h + (size_t)54 * N;
  if (num_pairs > 0) std::memcpy(cov_pairs, hp, sizeof(double) * 36 * (size_t)num_pairs);
  hp += 36 * (size_t)num_pairs;
  std::memcpy(xi, hp, sizeof(double) * 6 * K);
  std::memcpy(xi_post, hp + 6 * K, sizeof(double) * 6 * K);
  std::memcpy(scalars, hp + 12 * K, sizeof(double) * 3);
  return DPGO_OK;
}

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_linear_update(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                       const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new, double *delta,
                                       double *cov_diag, double *cov_pairs, double *xi, double *xi_post, double *scalars,
                                       dpgo_covariance_t *res) {
  return linear_update_call(t, T, method, max_block, num, closures, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, xi_post, scalars,
                            res, false);
}

extern "C" int dpgo_team_linear_update_solved(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                              const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new,
                                              double *delta, double *cov_diag, double *cov_pairs, double *xi, double *xi_post,
                                              double *scalars, dpgo_covariance_t *res) {
  return linear_update_call(t, T, method, max_block, num, closures, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, xi_post, scalars,
                            res, true);
}

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
//
// Across teams (dpgo_team_linear_update_across; DESIGN.md 5j, "across teams") the path is covariance_schur_across with its
// AcrossStep (UpdateAcross below) and the caller's pairs together.  k_upd_rhs_across writes this participant's rows of V = A^T from a compact table of the
// endpoint poses that an allgather has made identical everywhere; the step's X is B_loc.  A second allgather carries the rows
// of B at the poses the records and the pairs name, every participant runs k_upd_m onward on that compact B_C (N := C), and
// k_lin_u and k_lin_finish on B_loc for its own poses; k_upd_pairs_across forms the pair blocks from B_C and U_C.
#include "linear_frame.h"
#include "apply_block.h"
#include "covariance_apply.h"

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

// The same V across teams ("across teams"): one lane per closure, grid-stride.  Both endpoint poses come from
// the compact table TC that every participant holds in identical bytes (cand's i, j index it), so J_i and J_j are the same
// bits whoever holds the poses; row[c] is the team pose of compact pose c on this participant, or -1 for a pose that lives
// elsewhere and for the problem's pose 0, whose rows stay zero.  J^T goes into column block k of the zeroed V (leading
// dimension ld = 6 N_loc) only at the rows that are this participant's.
__global__ __launch_bounds__(256) void k_upd_rhs_across(const double *__restrict__ TC, const GateRec *__restrict__ cand,
                                                        const int *__restrict__ row, int C, int K, size_t ld, double *__restrict__ V) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const v2i_t ids = *(const __attribute__((address_space(1))) v2i_t *)(cand + k);
    if (ids.x < 0 || ids.x >= C || ids.y < 0 || ids.y >= C) continue;  // (the call has checked the endpoints on the host)
    JointEnds e;
    double Rij[3][3], tij[3];
    joint_ends(TC, cand + k, e, Rij, tij);
    const int pi = gp(row)[e.i], pj = gp(row)[e.j];
    if (pi >= 0) {
      double *o = V + (size_t)6 * k * ld + (size_t)6 * pi;
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int a = 0; a < 6; ++a) gp(o)[c * ld + a] = e.Ji[c][a];
    }
    if (pj >= 0) {
      double *o = V + (size_t)6 * k * ld + (size_t)6 * pj;
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int a = 0; a < 6; ++a) gp(o)[c * ld + a] = e.Jj[c][a];
    }
  }
}

// Sigma'_pq = Sigma_pq - U_p B_q^T for the requested pairs on the compact tables (B and U 6 C x 6 K, leading dimension ld;
// pairs index them): one wave per pair, k_lin_finish's pair range with its arithmetic and its order of summation
__global__ __launch_bounds__(256) void k_upd_pairs_across(const double *__restrict__ pair_blocks, const int *__restrict__ pairs, int num_pairs,
                                                          int K, size_t ld, const double *__restrict__ B, const double *__restrict__ U,
                                                          double *__restrict__ out_pairs) {
  const size_t e = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, n = 6 * K;
  if (e >= (size_t)num_pairs) return;
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

// ---- across teams (dpgo_team_linear_update_across; DESIGN.md 5j, "across teams")

const ClosureCall UPDATE_ACROSS = {"linear_update_across", "closure"};

// The step handed to covariance_schur_across together with the caller's pairs.  resolve(): the records' endpoints and the pairs
// in the global numbering, the compact set of C poses {endpoints} u {pair poses} sorted by global pose, and allgather E, T of
// those poses from their holders.  rhs(): V = A^T on this participant's rows.  taken(): this participant's rows of B_loc = X at
// the compact poses it holds, gathered on the device.  exchange(): allgather F carries them, every participant assembles B_C and runs
// everything of order 6 K on identical bytes, and its own poses on B_loc.
struct UpdateAcross : AcrossStep {
  dpgo_team_t *t = nullptr;
  const double *T_host = nullptr;
  const dpgo_measurement_t *meas = nullptr;
  const int *pairs_in = nullptr;
  int num = 0, npairs = 0, N = 0, C = 0, zero_local = -1;
  std::vector<int> offs;        // pose offsets of the local robots
  std::vector<GateRec> cand;    // i, j (and w0, w1): compact poses
  std::vector<int> comp;        // the compact poses, global ids, ascending
  std::vector<int> cpairs;      // the caller's pairs as compact poses
  std::vector<int> lpose;       // compact pose -> team pose here, or -1
  std::vector<int> vrow;        // the same with -1 for the problem's pose 0: the rows of V that are written
  std::vector<int> mine_pose;   // the team poses of the compact poses that live here, in compact order
  std::vector<int> holder, pos; // compact pose -> rank, and its place among the compact poses of that rank
  std::vector<int> held;        // per rank the number of compact poses it holds
  size_t max_held = 0;
  std::vector<double> T_C, h_send, h_BC, h_out;
  DevBuf<GateRec> d_cand;
  DevBuf<double> d_TC, d_send, d_BC, d_UC, d_U, d_M, d_W, d_G, d_work, d_out, d_pb;
  DevBuf<int> d_vrow, d_mp, d_cpairs;
  Events ev{4};
  hipStream_t stream = nullptr;
  bool took = false, ran = false;
  std::string pivot;            // the refusal of a non-positive pivot of M: the same on every participant
  size_t K() const { return (size_t)num; }
  size_t out_doubles() const { return (size_t)54 * N + 36 * (size_t)npairs + 12 * K() + 4; }
  int num_cols() const override { return argerr.empty() ? 6 * num : 0; }

  int resolve(Across &x, std::string &msg) override {
    const ClosureCall &A = UPDATE_ACROSS;
    const long long NG = x.nglob;
    cand.resize(num);
    for (int k = 0; k < num; ++k) {
      int g[2];
      if (A.global_endpoint(x, k, meas[k].r1, meas[k].p1, &g[0], msg) || A.global_endpoint(x, k, meas[k].r2, meas[k].p2, &g[1], msg)) return 1;
      GateRec &c = cand[k];
      std::memset(&c, 0, sizeof c);
      c.i = g[0]; c.j = g[1];
      pack_measurement(meas[k], c.m);
      comp.push_back(g[0]); comp.push_back(g[1]);
    }
    for (int k = 0; k < 2 * npairs; ++k) {
      if (pairs_in[k] < 0 || pairs_in[k] >= NG) {
        msg = "pair " + std::to_string(k / 2) + " names pose " + std::to_string(pairs_in[k]) + ", outside [0, " + std::to_string(NG) + ")";
        return 1;
      }
      comp.push_back(pairs_in[k]);
    }
    std::sort(comp.begin(), comp.end());
    comp.erase(std::unique(comp.begin(), comp.end()), comp.end());
    C = (int)comp.size();
    const auto rank_of = [&](int g) { return (int)(std::lower_bound(comp.begin(), comp.end(), g) - comp.begin()); };
    for (GateRec &c : cand) { c.i = c.w0 = rank_of(c.i); c.j = c.w1 = rank_of(c.j); }
    cpairs.resize(2 * (size_t)npairs);
    for (int k = 0; k < 2 * npairs; ++k) cpairs[k] = rank_of(pairs_in[k]);
    offs = pose_offsets(t);
    N = offs.back();
    lpose.assign(C, -1); vrow.assign(C, -1); holder.assign(C, 0); pos.assign(C, 0); held.assign(x.world, 0);
    for (int c = 0; c < C; ++c) {
      int robot = 0;
      while (robot + 1 < x.num_robots && x.robot_goff[robot + 1] <= comp[c]) ++robot;
      holder[c] = x.robot_holder[robot];
      pos[c] = held[holder[c]]++;
      if (holder[c] != x.rank) continue;
      lpose[c] = offs[t->id2local.at(robot)] + (int)(comp[c] - x.robot_goff[robot]);
      if (comp[c] != 0) vrow[c] = lpose[c];
      else zero_local = lpose[c];
      mine_pose.push_back(lpose[c]);
    }
    max_held = (size_t)*std::max_element(held.begin(), held.end());
    // ---- allgather E: T of the compact poses, 12 doubles each from its holder, zeros from everyone else
    const HeldRecord rec{12, holder};
    std::vector<double> ge(rec.len(), 0.0), all;
    for (int c = 0; c < C; ++c)
      if (lpose[c] >= 0) std::memcpy(rec.mine(ge, c), T_host + (size_t)12 * lpose[c], sizeof(double) * 12);
    if (x.gather(ge, all)) return 2;
    T_C.resize(12 * (size_t)C);
    for (int c = 0; c < C; ++c) std::memcpy(T_C.data() + 12 * (size_t)c, rec.from(all, c), sizeof(double) * 12);
    return DPGO_OK;
  }

  int rhs(const double *, int N_, double *V, hipStream_t s) override {
    const size_t k = K(), n = 6 * k;
    if (N_ != N) { set_err("linear_update_across: the covariance path's poses are not the call's"); return DPGO_ERR; }
    if (d_cand.upload(cand, s) || d_TC.upload(T_C, s) || d_vrow.upload(vrow, s) || d_mp.upload(mine_pose, s) ||
        d_cpairs.upload(cpairs, s) || d_send.alloc((size_t)6 * mine_pose.size() * n) || d_BC.alloc((size_t)6 * C * n) || d_UC.alloc((size_t)6 * C * n) ||
        d_U.alloc((size_t)6 * N * n) || d_M.alloc(n * n) || d_W.alloc(n * n) || d_G.alloc(n * n) || d_work.alloc(n + 4) ||
        d_out.alloc(out_doubles()) || d_pb.alloc(36 * (size_t)std::max(npairs, 1)) || ev.create()) {
      set_err("linear_update_across: device allocation failed");
      return DPGO_ERR;
    }
    HIPC(hipMemsetAsync(V, 0, sizeof(double) * 6 * (size_t)N * n, s));
    HIPC(hipEventRecord(ev[0], s));
    k_upd_rhs_across<<<(unsigned)std::min<size_t>((k + 255) / 256, 2048), 256, 0, s>>>(d_TC.p, d_cand.p, d_vrow.p, C, (int)k, (size_t)6 * N, V);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    return DPGO_OK;
  }

  // this participant's rows of B_loc at the compact poses it holds, in compact order (6 held x 6 K, column-major): its part of
  // allgather F, padded to the largest part
  int taken(int N_, hipStream_t s) override {
    const size_t n = 6 * K(), mine = (size_t)6 * mine_pose.size() * n;
    if (N_ != N || !X) { set_err("linear_update_across: the covariance path formed no X"); return DPGO_ERR; }
    stream = s;
    launch_apply_gather(s, X, (size_t)6 * N, d_mp.p, (int)mine_pose.size(), (int)n, d_send.p);
    HIPC(hipGetLastError());
    h_send.assign(1 + 6 * max_held * n, 0.0);
    if (mine) HIPC(hipMemcpyAsync(h_send.data() + 1, d_send.p, sizeof(double) * mine, hipMemcpyDeviceToHost, s));
    took = true;  // (the path drains the stream behind taken())
    return DPGO_OK;
  }

  // everything behind B_C and B_loc: queued on s, drained here
  int device_part(hipStream_t s) {
    const size_t k = K(), np = (size_t)npairs;
    const int n = (int)(6 * k);
    double *oT = d_out.p, *odx = oT + (size_t)12 * N, *odiag = odx + (size_t)6 * N, *opairs = odiag + (size_t)36 * N;
    double *oxi = opairs + 36 * np, *otail = oxi + 6 * k, *z = d_work.p, *ldet = z + 6 * k;
    HIPC(hipMemcpyAsync(d_BC.p, h_BC.data(), sizeof(double) * h_BC.size(), hipMemcpyHostToDevice, s));
    if (np) HIPC(hipMemcpyAsync(d_pb.p, view.blocks_h + (size_t)36 * N, sizeof(double) * 36 * np, hipMemcpyHostToDevice, s));
    k_upd_m<<<(unsigned)std::min<size_t>((k * k + 255) / 256, 2048), 256, 0, s>>>(d_TC.p, d_cand.p, (int)k, C, d_BC.p, d_M.p, oxi);
    HIPC(hipGetLastError());
    const int fail = dense_spd_inverse(s, d_M.p, d_W.p, d_G.p, n);  // (synchronises the stream; the factor stays in d_M)
    HIPC(hipGetLastError());
    if (fail < 0) { set_err("linear_update_across: scratch allocation of the inverse failed"); return DPGO_ERR; }
    if (fail > 0) {
      pivot = "non-positive pivot at row " + std::to_string(fail - 1) + " of M (pivot block " + std::to_string((fail - 1) / 6) +
              ", the block of closure " + std::to_string((fail - 1) / 6) + "): M = A Sigma A^T + R is not positive definite at this T";
      return DPGO_OK;
    }
    if (launch_cov_logdet(s, d_M.p, n, ldet)) return DPGO_ERR;
    k_lin_u<<<dim3((unsigned)((6 * (size_t)C + 63) / 64), (unsigned)((n + 63) / 64), 1), 256, 0, s>>>(d_BC.p, d_G.p, d_UC.p, 6 * C, n);
    k_lin_u<<<dim3((unsigned)((6 * (size_t)N + 63) / 64), (unsigned)((n + 63) / 64), 1), 256, 0, s>>>(X, d_G.p, d_U.p, 6 * N, n);
    HIPC(hipGetLastError());
    k_upd_z<<<(unsigned)std::min<size_t>((n + 255) / 256, 2048), 256, 0, s>>>(d_G.p, oxi, d_cand.p, n, z, otail);
    k_upd_scalars<<<1, 64, 0, s>>>(oxi, z, d_cand.p, (int)k, ldet, otail + n);
    HIPC(hipGetLastError());
    k_lin_finish<false><<<(unsigned)(((size_t)N + 3) / 4), 256, 0, s>>>(view.Td, view.diag, nullptr, nullptr, N, (int)k, 0, X, d_U.p, z, oT, odx,
                                                                      odiag, opairs);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[2], s));
    if (np) k_upd_pairs_across<<<(unsigned)((np + 3) / 4), 256, 0, s>>>(d_pb.p, d_cpairs.p, (int)np, (int)k, (size_t)6 * C, d_BC.p, d_UC.p, opairs);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[3], s));
    h_out.resize(out_doubles());
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    // (pose 0 is fixed: its dx is +0, not the -0 that the negated sum of zeros leaves)
    if (zero_local >= 0) std::fill(h_out.begin() + (size_t)12 * N + (size_t)6 * zero_local, h_out.begin() + (size_t)12 * N + (size_t)6 * zero_local + 6, 0.0);
    ran = true;
    return DPGO_OK;
  }

  int exchange(Across &x, hipStream_t s) override {
    const size_t n = 6 * K(), len = 6 * max_held * n, ldc = (size_t)6 * C;
    // ---- allgather F: every participant's six rows of B (6 x 6 K) per compact pose it holds, padded to the largest part
    if (!took || x.bad) h_send.assign(1 + len, 0.0);
    std::vector<double> all;
    if (x.gather(h_send, all)) return DPGO_ERR;
    h_BC.resize(ldc * n);
    for (size_t col = 0; col < n; ++col)
      for (int c = 0; c < C; ++c) {
        const size_t q = (size_t)holder[c], ldq = (size_t)6 * held[q];
        std::memcpy(h_BC.data() + col * ldc + (size_t)6 * c, all.data() + q * (1 + len) + 1 + col * ldq + (size_t)6 * pos[c], 48);
      }
    if (!x.bad && device_part(s)) x.fail_local(g_err);
    return DPGO_OK;
  }
};
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

extern "C" int dpgo_team_linear_update_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, const double *T,
                                              int num, const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new,
                                              double *delta, double *cov_diag, double *cov_pairs, double *xi, double *xi_post,
                                              double *scalars, dpgo_covariance_t *res) {
  const ClosureCall &A = UPDATE_ACROSS;
  const auto t_begin = std::chrono::steady_clock::now();
  if (res) std::memset(res, 0, sizeof *res);
  if (!t || !tr) return A.refuse("null argument");  // (nobody to tell)
  UpdateAcross app;
  app.name = A.name;
  app.op = 8;  // (the step's own record: the number of records, the hash of records and pairs, num_pairs)
  app.t = t;
  app.T_host = T;
  app.meas = closures;
  app.pairs_in = pairs;
  app.num = num;
  app.npairs = num_pairs;
  int N = 0;
  for (auto &a : t->ag) N += a->n;
  // ---- the refusals of the call itself, in the single team's order and words: decided here before any device work, told to
  // everyone by the agreement record (a participant that returned now would leave the others waiting)
  auto refusal = [&]() -> int {
    if (!owner_rank_of_robot || !T || !res || !T_new || !delta || !cov_diag || !xi || !xi_post || !scalars) return A.refuse("null argument");
    if (num <= 0) return A.refuse("num must be positive, not " + std::to_string(num));
    if (!closures) return A.refuse("null argument");
    if (num_pairs < 0) return A.refuse("num_pairs must not be negative, not " + std::to_string(num_pairs));
    if (num_pairs > 0 && (!pairs || !cov_pairs)) return A.refuse("null argument");
    {
      // V, X (the kept B_loc) and U_loc, the three matrices of order 6 K and the compact tables B_C, U_C and the image sent,
      // at most 2 K + 2 P poses: decided before a record is read and before V is written; the path accounts for the rest
      const double K = num, P = num_pairs, Cmax = 2.0 * K + 2.0 * P;
      const double vxu = 3.0 * 288.0 * (double)N * K, mat = 288.0 * K * K, tabs = 3.0 * 288.0 * Cmax * K + 108.0 * Cmax;
      const double need = vxu + 3.0 * mat + tabs + 8.0 * (54.0 * N + 36.0 * P + 18.0 * K + 8.0) + 128.0 * K + 8.0 * P + 288.0 * P;
      double avail = 0.0;
      if (hipSetDevice(t->device) != hipSuccess || A.device_avail(t, &avail)) return A.refuse("hipMemGetInfo failed");
      if (need > avail || 36.0 * K * K > (double)((size_t)1 << 40) || 6.0 * Cmax > (double)(INT32_MAX / 2)) {
        char buf[480];
        std::snprintf(buf, sizeof buf,
                      "%d closures on %d poses here: V, X and U (6 N x 6 K each), the three matrices of order %.0f and the compact tables of "
                      "at most %.0f poses need %.0f bytes (3 x %.0f + 3 x %.0f + %.0f and the working arrays), %.0f are available on the device",
                      num, N, 6.0 * K, Cmax, need, vxu / 3.0, mat, tabs, avail);
        return A.refuse(buf);
      }
    }
    for (int k = 0; k < num; ++k) {
      const dpgo_measurement_t &m = closures[k];
      if (m.r1 == m.r2 && m.p1 == m.p2) return A.refuse(A.item(k) + " joins a pose to itself");
      if (A.check(k, m)) return DPGO_ERR;
    }
    return DPGO_OK;
  };
  if (refusal()) app.argerr = A.refused();
  else {
    RecordHash h;
    for (int k = 0; k < num; ++k) {
      const dpgo_measurement_t &m = closures[k];
      double v[GATE_MEAS];
      h.add(m.r1); h.add(m.p1); h.add(m.r2); h.add(m.p2);
      pack_measurement(m, v);
      h.add(v, sizeof(double) * 14);
    }
    for (int k = 0; k < 2 * num_pairs; ++k) h.add(pairs[k]);
    app.agree_num = num;
    app.agree_hash = h.value();
    app.agree_int = num_pairs;
  }
  SchurAcrossArgs path(t, tr, owner_rank_of_robot, T);
  if (app.argerr.empty()) { path.num_pairs = num_pairs; path.pairs = pairs; }
  path.cov_pairs = cov_pairs;
  path.res = res;
  path.step = &app;
  if (const int rc = covariance_schur_across(path)) return rc;  // (res is then all zero)
  if (!app.pivot.empty() || !app.ran) {  // (every participant formed the same M from the same bytes: the same words everywhere)
    std::memset(res, 0, sizeof *res);
    return A.refuse(app.pivot.empty() ? "the covariance path staged no blocks" : app.pivot);
  }
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr,
                 "linear_update_across: rank %d of %d, %d closures and %d pairs on %d compact poses, %d poses here, k_upd_rhs_across %.3f ms, "
                 "k_upd_pairs_across %.3f ms, allgather E %zu bytes, allgather F %zu bytes per participant, the apply's products %.3f ms, the "
                 "whole call %.3f ms\n",
                 tr->rank, tr->world, num, num_pairs, app.C, N, app.ev.ms(0, 1), app.ev.ms(2, 3), 8 * (1 + 12 * (size_t)app.C),
                 8 * (1 + 36 * app.max_held * (size_t)num), app.ms_products,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  const LinearArgs a{t, T, DPGO_GATE_SCHUR, 0, num, closures, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, res};
  const double *hp = a.copy_head(app.h_out, N);
  std::memcpy(xi_post, hp, sizeof(double) * 6 * (size_t)num);
  std::memcpy(scalars, hp + 6 * (size_t)num, sizeof(double) * 3);
  return DPGO_OK;
}

extern "C" int dpgo_team_linear_update_solved(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                              const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new,
                                              double *delta, double *cov_diag, double *cov_pairs, double *xi, double *xi_post,
                                              double *scalars, dpgo_covariance_t *res) {
  return linear_update_call({t, T, method, max_block, num, closures, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, res}, xi_post,
                            scalars, true);
}

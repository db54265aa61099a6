// gate_joint.hip -- a set of candidate measurements gated jointly, each given those already accepted.
//
// T, Sigma, the perturbation, R_ij, t_ij, J_i, J_j, xi and Sigma_meas are the gate's (gate.hip, gate_block.h).  K candidates,
// candidate k joining the team poses i_k != j_k; A the 6 K x 6 N matrix whose row block k holds J_i^k at pose i_k and J_j^k at
// pose j_k; R the block diagonal of the Sigma_meas,k.
//   joint covariance   M = A Sigma A^T + R of order 6 K, bitwise symmetric; M_kk is the gate's S
//   conditional test   given the accepted set A: xi_k|A = xi_k - M_kA M_AA^-1 xi_A,  S_k|A = M_kk - M_kA M_AA^-1 M_Ak,
//                      d2_k|A = xi_k|A^T S_k|A^-1 xi_k|A; a non-positive pivot gives +inf, which is never accepted
//   greedy             at every step the open candidate of smallest d2_k|A, the lower index on ties: accepted when
//                      d2 <= thr^2, else the call stops and everything left is rejected
//   given              k = 0 .. K - 1 in turn: accepted when d2_k|A <= thr^2, else skipped with A as it is
//   joint figures      d2_joint = the sum of d2_cond over A in the order of acceptance (= xi_A^T M_AA^-1 xi_A),
//                      logdet_joint = log det M_AA
// The covariance path is asked for every unordered pair of the distinct endpoint poses, sorted, so that a pair's block
// follows from the two ranks by arithmetic (gate_joint_block.h).  k_joint_blocks forms xi, the marginal d2 and M behind the
// staged blocks; k_joint_step is one step of a left-looking block-pivoted Cholesky of M in the order the pivots are taken,
// one launch per step and the stream order the only synchronisation; k_joint_finish gathers.  Only the outputs go to the host.
#include <algorithm>
#include <chrono>

#include "certify_internal.h"
#include "covariance_frame.h"
#include "gate_joint_block.h"

namespace dpgo {

// one candidate on the device: team poses i != j, their ranks among the sorted distinct endpoints, and the measurement
struct JointCand {
  int i, j, ri, rj;
  double m[14];  // R~ row-major, t~, kappa, tau
};
static_assert(sizeof(JointCand) == 8 * JOINT_REC, "JointCand is read in 16-byte loads");

// the control words of the elimination
enum { JC_STOP = 0, JC_PARITY = 1, JC_NACC = 2, JC_WORDS = 4 };

__device__ __forceinline__ void joint_ends(const double *T, const JointCand *c, JointEnds &e, double Rij[3][3], double tij[3]) {
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  const v4i_t ids = *(const __attribute__((address_space(1))) v4i_t *)c;
  e.i = ids.x; e.j = ids.y; e.ri = ids.z; e.rj = ids.w;
  double Ri[3][3], Rj[3][3], ti[3], tj[3];
  joint_load_pose(T, e.i, Ri, ti);
  joint_load_pose(T, e.j, Rj, tj);
  joint_jacobians(Ri, ti, Rj, tj, Rij, tij, e.Ji, e.Jj);
}

// One lane per block (k, l) with k <= l of M, K^2 lanes of which the lower triangle rests.  fp64 in registers, no LDS, no
// atomics: the lane writes the block and its transpose, so M is bitwise symmetric.  The lanes of the diagonal also form xi and
// the marginal d2 and open the state of the elimination: D_k = M_kk, xi_k|{} = xi_k, d2c[0] = d2, state[0] = open, rank = -1.
__global__ __launch_bounds__(256) void k_joint_blocks(const double *__restrict__ T, const double *__restrict__ diag,
                                                      const double *__restrict__ pairs, const JointCand *__restrict__ cand, int K, int m,
                                                      double *__restrict__ M, double *__restrict__ D, double *__restrict__ xi,
                                                      double *__restrict__ d2, double *__restrict__ xic, double *__restrict__ d2c,
                                                      int *__restrict__ state, int *__restrict__ rank) {
  const size_t total = (size_t)K * K, ld = (size_t)6 * K;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int k = (int)(t / K), l = (int)(t % K);
    if (l < k) continue;
    // (the block of two candidates is formed from the side their endpoints name: joint_orientation)
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const v2i_t pk = *(const __attribute__((address_space(1))) v2i_t *)(cand + k), pl = *(const __attribute__((address_space(1))) v2i_t *)(cand + l);
    const int way = joint_orientation(pk.x, pk.y, pl.x, pl.y);
    const int kk = way < 0 ? l : k, ll = way < 0 ? k : l;
    JointEnds ek, el;
    double Rij[3][3], tij[3], Rl[3][3], tl[3], G[6][6];
    joint_ends(T, cand + ll, el, Rl, tl);
    joint_ends(T, cand + kk, ek, Rij, tij);
    joint_block(diag, pairs, m, ek, el, G);
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
    const double *rec = (const double *)(cand + k);
    double v[14], S[6][6], x[6];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const double2 w = ld2(rec + 2 + 2 * q);
      v[2 * q] = w.x;
      v[2 * q + 1] = w.y;
    }
    joint_diagonal(G, v[12], v[13], S);
    joint_innovation(Rij, tij, v, x);
    const double dd = joint_distance(S, x);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        gp(M)[((size_t)6 * k + a) * ld + (size_t)6 * k + b] = S[a][b];
        gp(D)[(size_t)36 * k + 6 * a + b] = S[a][b];
      }
      gp(xi)[(size_t)6 * k + a] = x[a];
      gp(xic)[(size_t)6 * k + a] = x[a];
    }
    gp(d2)[k] = dd;
    gp(d2c)[k] = dd;
    gp(state)[k] = 0;
    gp(rank)[k] = -1;
  }
}

// One step of the elimination: workgroups of one wave, one lane per candidate (row block).  Step s reads d2c and state at
// parity s & 1 and writes them at the other parity, every lane its own row, so that no workgroup reads what another writes in
// the same launch; D, xi_cond and the factor are written by a row's own lane and read by others only in later launches.
// Every workgroup finds the same pivot by the same rule from the same words (GREEDY), or takes k = s.  W: the factor, column
// a (the a-th accepted pivot) at W + 36 (a K + r) for row r.  state: 0 open, 1 accepted, 2 rejected (given order).
// nacc[s]: how many were accepted before step s.  A greedy step that finds nothing acceptable raises JC_STOP and returns:
// the steps behind it return at once, and the other workgroups of the same launch, which may or may not have seen the word
// yet, reach the same verdict and write nothing either.
template <bool GREEDY>
__global__ __launch_bounds__(64) void k_joint_step(int s, int K, double thr2, const double *__restrict__ M, double *__restrict__ W,
                                                   double *__restrict__ D, double *__restrict__ xic, double *__restrict__ d2c,
                                                   int *__restrict__ state, int *__restrict__ rank, double *__restrict__ stepv,
                                                   int *__restrict__ nacc, int *__restrict__ ctl) {
  if (GREEDY && gp(ctl)[JC_STOP]) return;
  const int cur = s & 1, lane = threadIdx.x;
  const double *d2r = d2c + (size_t)cur * K;
  double *d2w = d2c + (size_t)(1 - cur) * K;
  const int *str = state + (size_t)cur * K;
  int *stw = state + (size_t)(1 - cur) * K;
  const int r = blockIdx.x * 64 + lane;
  const bool first = blockIdx.x == 0 && lane == 0;
  const int a = gp(nacc)[s];  // accepted so far: the column of the factor this step would write
  int p;
  double dp;
  if constexpr (GREEDY) {
    dp = INFINITY;
    p = -1;
    for (int k = lane; k < K; k += 64)
      if (gp(str)[k] == 0) joint_better(gp(d2r)[k], k, dp, p);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const double od = __shfl_xor(dp, off);
      const int ok = __shfl_xor(p, off);
      joint_better(od, ok, dp, p);
    }
  } else {
    p = s;
    dp = gp(d2r)[s];
  }
  const bool take = p >= 0 && dp <= thr2;
  if (!take) {
    if constexpr (GREEDY) {
      if (first) gp(ctl)[JC_STOP] = 1;
    } else {  // skipped: the set stays as it is, every word goes over to the other parity
      if (r < K) {
        gp(stw)[r] = r == p ? 2 : gp(str)[r];
        gp(d2w)[r] = gp(d2r)[r];
      }
      if (first) { gp(nacc)[s + 1] = a; gp(ctl)[JC_PARITY] = 1 - cur; }
    }
    return;
  }
  if (first) { gp(nacc)[s + 1] = a + 1; gp(ctl)[JC_PARITY] = 1 - cur; gp(ctl)[JC_NACC] = a + 1; }
  if (r >= K) return;
  const int st = gp(str)[r];
  if (r == p || st != 0) {
    gp(stw)[r] = r == p ? 1 : st;
    gp(d2w)[r] = gp(d2r)[r];
    if (r != p) return;
  }
  // the pivot's factor and whitened innovation: every open lane forms them from the same words
  double L[6][6], y[6], xp[6];
  bool ok;
#pragma unroll
  for (int x = 0; x < 6; ++x) {
#pragma unroll
    for (int z = 0; z < 6; ++z) L[x][z] = gp(D)[(size_t)36 * p + 6 * x + z];
    xp[x] = gp(xic)[(size_t)6 * p + x];
  }
  joint_cholesky(L, ok);
  (void)joint_forward(L, xp, y);
  if (r == p) {
    gp(rank)[p] = a;
    gp(stepv)[a] = dp;
    gp(stepv)[(size_t)K + a] = joint_logdet(L);
    return;
  }
  const size_t ld = (size_t)6 * K;
  double G[6][6], Dr[6][6], xr[6];
#pragma unroll
  for (int x = 0; x < 6; ++x) {
#pragma unroll
    for (int z = 0; z < 6; ++z) {
      G[x][z] = gp(M)[((size_t)6 * r + x) * ld + (size_t)6 * p + z];
      Dr[x][z] = gp(D)[(size_t)36 * r + 6 * x + z];
    }
    xr[x] = gp(xic)[(size_t)6 * r + x];
  }
  for (int q = 0; q < a; ++q) joint_subtract_product(W + 36 * ((size_t)q * K + r), W + 36 * ((size_t)q * K + p), G);
  const double dd = joint_row_update(G, L, y, Dr, xr);
  double *w = W + 36 * ((size_t)a * K + r);
#pragma unroll
  for (int x = 0; x < 6; ++x) {
#pragma unroll
    for (int z = 0; z < 6; ++z) {
      gp(w)[6 * x + z] = G[x][z];
      gp(D)[(size_t)36 * r + 6 * x + z] = Dr[x][z];
    }
    gp(xic)[(size_t)6 * r + x] = xr[x];
  }
  gp(d2w)[r] = dd;
  gp(stw)[r] = 0;
}

// d2_cond out of the parity the last step wrote, and the joint figures summed in the order of acceptance by one lane
__global__ __launch_bounds__(256) void k_joint_finish(int K, const double *__restrict__ d2c, const double *__restrict__ stepv,
                                                      const int *__restrict__ ctl, double *__restrict__ d2_cond, double *__restrict__ scal) {
  const int par = gp(ctl)[JC_PARITY], n = gp(ctl)[JC_NACC];
  for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) gp(d2_cond)[k] = gp(d2c)[(size_t)par * K + k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double dj = 0.0, lj = 0.0;
    for (int q = 0; q < n; ++q) {
      dj += gp(stepv)[q];
      lj += gp(stepv)[(size_t)K + q];
    }
    gp(scal)[0] = dj;
    gp(scal)[1] = lj;
  }
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

// the step behind a covariance path's staged blocks: upload the records, form M, eliminate, queue the copies of the outputs
struct JointEpilogue : CovEpilogue {
  std::vector<JointCand> cand;
  int m = 0;  // distinct endpoint poses
  bool greedy = true;
  double thr2 = 0.0;
  double *M_out = nullptr;
  DevBuf<JointCand> d_cand;
  DevBuf<double> d_M, d_W, d_work;
  DevBuf<int> d_int;
  std::vector<double> h_out;  // xi[6 K], d2[K], xi_cond[6 K], d2_cond[K], d2_joint, logdet_joint
  std::vector<int> h_int;     // rank[K], the control words
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ran = false;
  ~JointEpilogue() override {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  // doubles of d_work: xi, d2, xi_cond, d2_cond, the two figures | D, both parities of d2c, the steps' (d2, logdet)
  static size_t out_doubles(size_t K) { return 14 * K + 2; }
  static size_t work_doubles(size_t K) { return out_doubles(K) + 36 * K + 2 * K + 2 * K; }
  // ints of d_int: rank, the control words | both parities of the state, nacc
  static size_t out_ints(size_t K) { return K + JC_WORDS; }
  static size_t work_ints(size_t K) { return out_ints(K) + 2 * K + K + 1; }
  static double bytes(size_t K) {
    return 2.0 * 288.0 * (double)K * (double)K + 8.0 * (double)work_doubles(K) + 4.0 * (double)work_ints(K) + 128.0 * (double)K;
  }
  int alloc() {
    const size_t K = cand.size();
    if (d_cand.alloc(K) || d_M.alloc(36 * K * K) || d_W.alloc(36 * K * K) || d_work.alloc(work_doubles(K)) || d_int.alloc(work_ints(K))) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "gate_candidates_jointly: device allocation failed (%.0f bytes for %zu candidates)", bytes(K), K);
      set_err(buf);
      return DPGO_ERR;
    }
    for (auto &e : ev) HIPC(hipEventCreate(&e));
    return DPGO_OK;
  }
  int run(const CovStage &st) override {
    const size_t K = cand.size();
    if (st.num_pairs != (int)((size_t)m * (m - 1) / 2)) {
      set_err("gate_candidates_jointly: the staged blocks are not the pairs of the endpoints");
      return DPGO_ERR;
    }
    for (const JointCand &c : cand)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.ri < 0 || c.ri >= m || c.rj < 0 || c.rj >= m || c.ri == c.rj) {
        set_err("gate_candidates_jointly: a candidate lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(JointCand) * K, hipMemcpyHostToDevice, s));
    double *xi = d_work.p, *d2 = xi + 6 * K, *xic = d2 + K, *d2o = xic + 6 * K, *scal = d2o + K;
    double *D = scal + 2, *d2c = D + 36 * K, *stepv = d2c + 2 * K;
    int *rank = d_int.p, *ctl = rank + K, *state = ctl + JC_WORDS, *nacc = state + 2 * K;
    HIPC(hipMemsetAsync(ctl, 0, sizeof(int) * JC_WORDS, s));
    HIPC(hipMemsetAsync(nacc, 0, sizeof(int) * (K + 1), s));
    HIPC(hipEventRecord(ev[0], s));
    // at most eight workgroups per CU of an MI355X: the lanes beyond stride over the rest
    k_joint_blocks<<<(unsigned)std::min<size_t>((K * K + 255) / 256, 2048), 256, 0, s>>>(st.Td, st.diag, st.pairs, d_cand.p, (int)K, m, d_M.p, D,
                                                                                         xi, d2, xic, d2c, state, rank);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    // K steps queued without a word from the device in between: those behind a greedy stop return at once
    const unsigned wgs = (unsigned)((K + 63) / 64);
    for (int step = 0; step < (int)K; ++step) {
      if (greedy) k_joint_step<true><<<wgs, 64, 0, s>>>(step, (int)K, thr2, d_M.p, d_W.p, D, xic, d2c, state, rank, stepv, nacc, ctl);
      else k_joint_step<false><<<wgs, 64, 0, s>>>(step, (int)K, thr2, d_M.p, d_W.p, D, xic, d2c, state, rank, stepv, nacc, ctl);
    }
    k_joint_finish<<<(unsigned)std::min<size_t>((K + 255) / 256, 256), 256, 0, s>>>((int)K, d2c, stepv, ctl, d2o, scal);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[2], s));
    h_out.resize(out_doubles(K));
    h_int.resize(out_ints(K));
    HIPC(hipMemcpyAsync(h_out.data(), d_work.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h_int.data(), d_int.p, sizeof(int) * h_int.size(), hipMemcpyDeviceToHost, s));
    if (M_out) HIPC(hipMemcpyAsync(M_out, d_M.p, sizeof(double) * 36 * K * K, hipMemcpyDeviceToHost, s));
    ran = true;
    return DPGO_OK;
  }
};

int joint_refuse(const std::string &msg) {
  set_err("gate_candidates_jointly: " + msg);
  return DPGO_ERR;
}

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_gate_candidates_jointly(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                                 const dpgo_measurement_t *cand, int order, double quantile, double *xi, double *d2,
                                                 double *xi_cond, double *d2_cond, int *accept, int *rank, int *num_accepted,
                                                 double *d2_joint, double *logdet_joint, double *M, dpgo_covariance_t *res) {
  const auto t_begin = std::chrono::steady_clock::now();
  // ---- the refusals of the call itself: on the host, before any device work, no output touched
  if (!t || !T || !res || !xi || !d2 || !xi_cond || !d2_cond || !accept || !rank || !num_accepted || !d2_joint || !logdet_joint)
    return joint_refuse("null argument");
  if (num <= 0) return joint_refuse("num must be positive, not " + std::to_string(num));
  if (!cand) return joint_refuse("null argument");
  if (method != DPGO_GATE_DENSE && method != DPGO_GATE_SCHUR && method != DPGO_GATE_NESTED)
    return joint_refuse("method must be DPGO_GATE_DENSE, DPGO_GATE_SCHUR or DPGO_GATE_NESTED, not " + std::to_string(method));
  if (order != DPGO_JOINT_GREEDY && order != DPGO_JOINT_GIVEN)
    return joint_refuse("order must be DPGO_JOINT_GREEDY or DPGO_JOINT_GIVEN, not " + std::to_string(order));
  if (!(quantile > 0.0 && quantile < 1.0)) {
    char buf[120];
    std::snprintf(buf, sizeof buf, "quantile must lie in (0, 1), not %.6g", quantile);
    return joint_refuse(buf);
  }
  if (check_team_local(t, "gate_candidates_jointly")) return DPGO_ERR;
  const int na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  for (int k = 0; k < na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  JointEpilogue epi;
  epi.greedy = order == DPGO_JOINT_GREEDY;
  const double thr = dpgo_error_threshold_at_quantile(quantile, 6);
  epi.thr2 = thr * thr;
  epi.M_out = M;
  epi.cand.resize(num);
  std::vector<int> poses;  // the endpoints, then sorted and distinct
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &c = cand[k];
    int g[2];
    for (int e = 0; e < 2; ++e) {
      const int r = e ? c.r2 : c.r1, p = e ? c.p2 : c.p1;
      const auto l = t->id2local.find(r);
      if (l == t->id2local.end()) return joint_refuse("candidate " + std::to_string(k) + " names robot " + std::to_string(r) + ", which is not in the team");
      if (p < 0 || p >= t->ag[l->second]->n)
        return joint_refuse("candidate " + std::to_string(k) + " names pose " + std::to_string(p) + " of robot " + std::to_string(r) +
                            ", outside [0, " + std::to_string(t->ag[l->second]->n) + ")");
      g[e] = offs[l->second] + p;
    }
    if (g[0] == g[1]) return joint_refuse("candidate " + std::to_string(k) + " joins a pose to itself");
    if (!(c.kappa > 0.0) || !(c.tau > 0.0) || !std::isfinite(c.kappa) || !std::isfinite(c.tau)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "candidate %d has kappa = %.6g, tau = %.6g: both must be positive", k, c.kappa, c.tau);
      return joint_refuse(buf);
    }
    // R~ in SO(3) by the rule of T (covariance_host_checks); row-major here, which changes neither figure
    const double *R = c.R;
    double orth = 0.0;
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) {
        const double d = R[3 * p] * R[3 * q] + R[3 * p + 1] * R[3 * q + 1] + R[3 * p + 2] * R[3 * q + 2] - (p == q ? 1.0 : 0.0);
        orth = std::max(orth, std::fabs(d));
      }
    const double det = R[0] * (R[4] * R[8] - R[7] * R[5]) - R[3] * (R[1] * R[8] - R[7] * R[2]) + R[6] * (R[1] * R[5] - R[4] * R[2]);
    bool finite = true;
    for (int q = 0; q < 9; ++q) finite = finite && std::isfinite(R[q]);
    for (int q = 0; q < 3; ++q) finite = finite && std::isfinite(c.t[q]);
    if (!finite || !(orth <= 1e-8) || !(std::fabs(det - 1.0) <= 1e-8)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "the measurement of candidate %d is not in SE(3) (|R R^T - I| = %.3g, det R = %.12g)", k, orth, det);
      return joint_refuse(buf);
    }
    JointCand &jc = epi.cand[k];
    std::memset(&jc, 0, sizeof jc);
    jc.i = g[0]; jc.j = g[1];
    std::memcpy(jc.m, c.R, sizeof c.R);
    std::memcpy(jc.m + 9, c.t, sizeof c.t);
    jc.m[12] = c.kappa; jc.m[13] = c.tau;
    poses.push_back(g[0]);
    poses.push_back(g[1]);
  }
  std::sort(poses.begin(), poses.end());
  poses.erase(std::unique(poses.begin(), poses.end()), poses.end());
  const int m = (int)poses.size();
  epi.m = m;
  for (JointCand &jc : epi.cand) {
    jc.ri = (int)(std::lower_bound(poses.begin(), poses.end(), jc.i) - poses.begin());
    jc.rj = (int)(std::lower_bound(poses.begin(), poses.end(), jc.j) - poses.begin());
  }
  const size_t K = (size_t)num, np = (size_t)m * (m - 1) / 2;
  HIPC(hipSetDevice(t->device));
  {
    // the pair blocks the path stages for this call, M and the factor: the rest is the path's own accounting
    const double blocks = 288.0 * (double)np, mat = 288.0 * (double)K * (double)K, need = blocks + JointEpilogue::bytes(K);
    double avail = 0.0;
    if (!cov_device_avail(t, &avail)) return joint_refuse("hipMemGetInfo failed");
    if (need > avail || np > (size_t)INT32_MAX || 36 * K * K > (size_t)1 << 40) {
      char buf[400];
      std::snprintf(buf, sizeof buf,
                    "%d candidates on %d poses: the %zu pair blocks, M of order %zu and the factor need %.0f bytes (%.0f + %.0f + %.0f "
                    "and the working arrays), %.0f are available on the device",
                    num, m, np, 6 * K, need, blocks, mat, mat, avail);
      return joint_refuse(buf);
    }
  }
  std::vector<int> pairs;
  pairs.reserve(2 * np);
  for (int a = 0; a < m; ++a)
    for (int b = a + 1; b < m; ++b) { pairs.push_back(poses[a]); pairs.push_back(poses[b]); }
  if (epi.alloc()) return DPGO_ERR;
  // ---- the covariance path, with its own refusals and messages; its blocks stay on the device for the epilogue
  const int rc = method == DPGO_GATE_NESTED ? marginal_covariances_nested_call(t, T, max_block, (int)np, pairs.data(), nullptr, nullptr, res, &epi)
                                            : marginal_covariances_call(t, T, method == DPGO_GATE_SCHUR ? DPGO_COV_SCHUR : 0, (int)np, pairs.data(),
                                                                        nullptr, nullptr, res, &epi);
  if (rc != DPGO_OK) return rc;
  if (!epi.ran) {  // (a team of the anchor alone has no two poses to join: the endpoint checks have refused already)
    std::memset(res, 0, sizeof *res);
    return joint_refuse("the covariance path staged no blocks");
  }
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  const int *hi = epi.h_int.data();
  const int nacc = hi[K + JC_NACC];
  if (timing) {
    float mb = 0.f, me = 0.f;
    HIPC(hipEventElapsedTime(&mb, epi.ev[0], epi.ev[1]));
    HIPC(hipEventElapsedTime(&me, epi.ev[1], epi.ev[2]));
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "gate_candidates_jointly: %d candidates on %d poses (%zu pair blocks), k_joint_blocks %.3f ms, elimination %.3f ms "
                         "(%d launches, %d accepted), the whole call %.3f ms\n", num, m, np, mb, me, num, nacc, whole);
  }
  const double *h = epi.h_out.data();
  std::memcpy(xi, h, sizeof(double) * 6 * K);
  std::memcpy(d2, h + 6 * K, sizeof(double) * K);
  std::memcpy(xi_cond, h + 7 * K, sizeof(double) * 6 * K);
  std::memcpy(d2_cond, h + 13 * K, sizeof(double) * K);
  *d2_joint = h[14 * K];
  *logdet_joint = h[14 * K + 1];
  std::memcpy(rank, hi, sizeof(int) * K);
  for (size_t k = 0; k < K; ++k) accept[k] = hi[k] >= 0;
  *num_accepted = nacc;
  return DPGO_OK;
}

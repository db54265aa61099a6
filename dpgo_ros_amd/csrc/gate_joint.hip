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

#include "closure_frame.h"
#include "gate_joint_block.h"

namespace dpgo {

// the control words of the elimination
enum { JC_STOP = 0, JC_PARITY = 1, JC_NACC = 2, JC_WORDS = 4 };

// M by joint_assemble from the staged blocks (joint_block).  The lanes of the diagonal also write the marginal d2 and open the
// state of the elimination: D_k = M_kk, xi_k|{} = xi_k, d2c[0] = d2, state[0] = open, rank = -1.
__global__ __launch_bounds__(256) void k_joint_blocks(const double *__restrict__ T, const double *__restrict__ diag,
                                                      const double *__restrict__ pairs, const GateRec *__restrict__ cand, int K, int m,
                                                      double *__restrict__ M, double *__restrict__ D, double *__restrict__ xi,
                                                      double *__restrict__ d2, double *__restrict__ xic, double *__restrict__ d2c,
                                                      int *__restrict__ state, int *__restrict__ rank) {
  joint_assemble(
      T, cand, K, M, xi,
      [=](const JointEnds &ek, int ll, double G[6][6]) __attribute__((always_inline)) {
        JointEnds el;
        double Rl[3][3], tl[3];
        joint_ends(T, cand + ll, el, Rl, tl);
        joint_block(diag, pairs, m, ek, el, G);
      },
      [=](int k, const double S[6][6], const double x[6]) __attribute__((always_inline)) {
        const double dd = gate_distance(S, x);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
          for (int b = 0; b < 6; ++b) gp(D)[(size_t)36 * k + 6 * a + b] = S[a][b];
          gp(xic)[(size_t)6 * k + a] = x[a];
        }
        gp(d2)[k] = dd;
        gp(d2c)[k] = dd;
        gp(state)[k] = 0;
        gp(rank)[k] = -1;
      });
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
  gate_cholesky(L, ok);
  (void)gate_forward(L, xp, y);
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

const ClosureCall JOINT = {"gate_candidates_jointly", "candidate"};

// the step behind a covariance path's staged blocks: upload the records, form M, eliminate, queue the copies of the outputs
struct JointEpilogue : ClosureEpilogue {
  std::vector<GateRec> cand;  // w0, w1: the ranks of i and j among the endpoints
  int m = 0;  // distinct endpoint poses
  bool greedy = true;
  double thr2 = 0.0;
  double *M_out = nullptr;
  DevBuf<GateRec> d_cand;
  DevBuf<double> d_M, d_W, d_work;
  DevBuf<int> d_int;
  std::vector<double> h_out;  // xi[6 K], d2[K], xi_cond[6 K], d2_cond[K], d2_joint, logdet_joint
  std::vector<int> h_int;     // rank[K], the control words
  JointEpilogue() : ClosureEpilogue(3) {}
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
    return ev.create();
  }
  int run(const CovStage &st) override {
    const size_t K = cand.size();
    if (st.num_pairs != (int)((size_t)m * (m - 1) / 2)) {
      set_err("gate_candidates_jointly: the staged blocks are not the pairs of the endpoints");
      return DPGO_ERR;
    }
    for (const GateRec &c : cand)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.w0 < 0 || c.w0 >= m || c.w1 < 0 || c.w1 >= m || c.w0 == c.w1) {
        set_err("gate_candidates_jointly: a candidate lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateRec) * K, hipMemcpyHostToDevice, s));
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
    return JOINT.refuse("null argument");
  if (num <= 0) return JOINT.refuse("num must be positive, not " + std::to_string(num));
  if (!cand) return JOINT.refuse("null argument");
  if (JOINT.check_method(method)) return DPGO_ERR;
  if (order != DPGO_JOINT_GREEDY && order != DPGO_JOINT_GIVEN)
    return JOINT.refuse("order must be DPGO_JOINT_GREEDY or DPGO_JOINT_GIVEN, not " + std::to_string(order));
  if (!(quantile > 0.0 && quantile < 1.0)) {
    char buf[120];
    std::snprintf(buf, sizeof buf, "quantile must lie in (0, 1), not %.6g", quantile);
    return JOINT.refuse(buf);
  }
  if (check_team_local(t, JOINT.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  JointEpilogue epi;
  epi.greedy = order == DPGO_JOINT_GREEDY;
  const double thr = dpgo_error_threshold_at_quantile(quantile, 6);
  epi.thr2 = thr * thr;
  epi.M_out = M;
  epi.cand.resize(num);
  for (int k = 0; k < num; ++k) {
    int g[2];
    if (JOINT.endpoints(t, offs, k, cand[k], g) || JOINT.check(k, cand[k])) return DPGO_ERR;
    GateRec &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    pack_measurement(cand[k], c.m);
  }
  const std::vector<int> poses = rank_endpoints(epi.cand);
  const int m = epi.m = (int)poses.size();
  const size_t K = (size_t)num, np = (size_t)m * (m - 1) / 2;
  HIPC(hipSetDevice(t->device));
  {
    // the pair blocks the path stages for this call, M and the factor: the rest is the path's own accounting
    const double blocks = 288.0 * (double)np, mat = 288.0 * (double)K * (double)K, need = blocks + JointEpilogue::bytes(K);
    double avail = 0.0;
    if (JOINT.device_avail(t, &avail)) return DPGO_ERR;
    if (need > avail || np > (size_t)INT32_MAX || 36 * K * K > (size_t)1 << 40) {
      char buf[400];
      std::snprintf(buf, sizeof buf,
                    "%d candidates on %d poses: the %zu pair blocks, M of order %zu and the factor need %.0f bytes (%.0f + %.0f + %.0f "
                    "and the working arrays), %.0f are available on the device",
                    num, m, np, 6 * K, need, blocks, mat, mat, avail);
      return JOINT.refuse(buf);
    }
  }
  std::vector<int> pairs;
  pairs.reserve(2 * np);
  for (int a = 0; a < m; ++a)
    for (int b = a + 1; b < m; ++b) { pairs.push_back(poses[a]); pairs.push_back(poses[b]); }
  if (epi.alloc()) return DPGO_ERR;
  if (const int rc = JOINT.path(t, T, method, max_block, (int)np, pairs.data(), res, epi)) return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  const int *hi = epi.h_int.data();
  const int nacc = hi[K + JC_NACC];
  if (timing) {
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "gate_candidates_jointly: %d candidates on %d poses (%zu pair blocks), k_joint_blocks %.3f ms, elimination %.3f ms "
                         "(%d launches, %d accepted), the whole call %.3f ms\n", num, m, np, epi.ev.ms(0, 1), epi.ev.ms(1, 2), num, nacc, whole);
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

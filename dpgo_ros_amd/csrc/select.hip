// select.hip -- the most informative candidate closures under a budget, chosen before any of them is measured.
//
// T, Sigma, the perturbation, J_i, J_j and Sigma_meas are the gate's (gate.hip, gate_block.h); A, R and M = A Sigma A^T + R the
// joint gate's (gate_joint.hip).  The Jacobians depend on T alone, so a candidate is its two endpoints and its expected noise
// (kappa, tau): R~, t~ and the weight of a record are not read.  P candidates, a budget b <= P.
//   conditional block  given the selected set A: S_k|A = M_kk - M_kA M_AA^-1 M_Ak
//   gain               gain_k|A = (log det S_k|A - log det Sigma_meas,k) / 2, the mutual information between measurement k and
//                      the trajectory once A has been measured; gain_k = gain_k|{}; a non-positive pivot gives -inf
//   greedy             at every step the open candidate of largest gain_k|A, the lower index on ties: taken while
//                      gain > min_gain and fewer than b are selected, else the call stops
//   given              k = 0 .. b - 1 in turn under the same test: the price of a caller's own plan
//   figures            gain_total = the sum of the gains at selection in selection order = (log det M_AA - log det R_A) / 2,
//                      logdet_joint = log det M_AA
// The covariance path is asked for every unordered pair of the distinct endpoint poses, sorted (gate_joint_block.h).
// k_select_open forms the diagonal blocks and the marginal gains; k_select_step is one step of a left-looking block-pivoted
// Cholesky that forms the pivot's block column of M on the fly and stops at the budget: b launches, a factor of b x P blocks, M
// never formed; k_select_finish gathers.  Only the outputs go to the host.
#include <algorithm>
#include <chrono>

#include "closure_frame.h"
#include "select_block.h"

namespace dpgo {

// the control words of the selection
enum { SC_STOP = 0, SC_PARITY = 1, SC_NSEL = 2, SC_WORDS = 4 };

// One lane per candidate, grid-stride: D_k = M_kk from the staged blocks, the marginal gain, and the state of the elimination
// opened: gains[0] = gain, state[0] = open, rank = -1.
__global__ __launch_bounds__(256) void k_select_open(const double *__restrict__ T, const double *__restrict__ diag,
                                                     const double *__restrict__ pairs, const GateRec *__restrict__ cand, int P, int m,
                                                     double *__restrict__ D, double *__restrict__ lm, double *__restrict__ gain,
                                                     double *__restrict__ gains, int *__restrict__ state, int *__restrict__ rank) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < P; k += gridDim.x * 256) {
    JointEnds e;
    double Rij[3][3], tij[3], G[6][6], S[6][6];
    joint_ends(T, cand + k, e, Rij, tij);
    joint_block(diag, pairs, m, e, e, G);
    double kappa, tau;
    GATE_LD2(cand[k].m + 12, kappa, tau);
    joint_diagonal(G, kappa, tau, S);
    const double l = select_logdet_meas(kappa, tau), g = select_gain(S, l);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) gp(D)[(size_t)36 * k + 6 * a + b] = S[a][b];
    gp(lm)[k] = l;
    gp(gain)[k] = g;
    gp(gains)[k] = g;
    gp(state)[k] = 0;
    gp(rank)[k] = -1;
  }
}

// One step of the selection: workgroups of one wave, one lane per candidate (row block).  Step s reads gains and state at
// parity s & 1 and writes them at the other parity, every lane its own row, so that no workgroup reads what another writes in
// the same launch; D and the factor are written by a row's own lane and read by others only in later launches.  Every
// workgroup finds the same pivot by the same rule from the same words (GREEDY), or takes k = s.  Every step before s has taken
// a pivot, so s is also the column of the factor this step writes: W_s[r] at W + 36 (s P + r).  state: 0 open, 1 selected.
// A step whose pivot has no gain above min_gain raises SC_STOP and returns: the steps behind it return at once, and the other
// workgroups of the same launch, which may or may not have seen the word yet, reach the same verdict and write nothing either.
template <bool GREEDY>
__global__ __launch_bounds__(64) void k_select_step(int s, int P, int budget, int m, double min_gain, const double *__restrict__ T,
                                                    const double *__restrict__ diag, const double *__restrict__ pairs,
                                                    const GateRec *__restrict__ cand, double *__restrict__ W, double *__restrict__ D,
                                                    const double *__restrict__ lm, double *__restrict__ gains, int *__restrict__ state,
                                                    int *__restrict__ rank, double *__restrict__ stepv, int *__restrict__ ctl) {
  if (gp(ctl)[SC_STOP]) return;
  const int cur = s & 1, lane = threadIdx.x;
  const double *gr = gains + (size_t)cur * P;
  double *gw = gains + (size_t)(1 - cur) * P;
  const int *str = state + (size_t)cur * P;
  int *stw = state + (size_t)(1 - cur) * P;
  const int r = blockIdx.x * 64 + lane;
  const bool first = blockIdx.x == 0 && lane == 0;
  int p;
  double gpv;
  if constexpr (GREEDY) {
    gpv = -INFINITY;
    p = -1;
    for (int k = lane; k < P; k += 64)
      if (gp(str)[k] == 0) select_better(gp(gr)[k], k, gpv, p);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const double og = __shfl_xor(gpv, off);
      const int ok = __shfl_xor(p, off);
      select_better(og, ok, gpv, p);
    }
    p = __builtin_amdgcn_readfirstlane(p);  // (every lane holds the same pivot: the addresses behind it are scalar)
  } else {
    p = s;
    gpv = gp(gr)[s];
  }
  const bool take = p >= 0 && gpv > min_gain;  // (-inf and NaN are above nothing)
  if (!take) {
    if (first) gp(ctl)[SC_STOP] = 1;
    return;
  }
  if (first) { gp(ctl)[SC_PARITY] = 1 - cur; gp(ctl)[SC_NSEL] = s + 1; }
  if (r >= P) return;
  const int st = gp(str)[r];
  if (r == p || st != 0) {
    gp(stw)[r] = r == p ? 1 : st;
    gp(gw)[r] = gp(gr)[r];
    if (r != p) return;
  }
  if (r == p) {  // the pivot's own lane: its rank, its gain and the log-determinant of its conditional block
    double L[6][6];
    bool ok;
    gate_load36(D + (size_t)36 * p, L);
    gate_cholesky(L, ok);
    gp(rank)[p] = s;
    gp(stepv)[s] = gpv;
    gp(stepv)[(size_t)budget + s] = joint_logdet(L);
    return;
  }
  // M_rp on the fly, as k_joint_blocks would have stored it
  typedef int v2i_t __attribute__((ext_vector_type(2)));
  const v2i_t er = *(const __attribute__((address_space(1))) v2i_t *)(cand + r), ep = *(const __attribute__((address_space(1))) v2i_t *)(cand + p);
  int ka, kb;
  bool sym;
  const bool tr = select_cross_order(r, er.x, er.y, p, ep.x, ep.y, ka, kb, sym);
  double G[6][6];
  {
    JointEnds ea, eb;
    double Rij[3][3], tij[3];
    joint_ends(T, cand + ka, ea, Rij, tij);
    joint_ends(T, cand + kb, eb, Rij, tij);
    select_cross(diag, pairs, m, ea, eb, tr, sym, G);
  }
  for (int q = 0; q < s; ++q) joint_subtract_product(W + 36 * ((size_t)q * P + r), W + 36 * ((size_t)q * P + p), G);
  // the pivot's factor: every open lane forms it from the same words
  double L[6][6], Dr[6][6];
  bool ok;
  gate_load36(D + (size_t)36 * p, L);
  gate_cholesky(L, ok);
  gate_load36(D + (size_t)36 * r, Dr);
  const double g = select_row_update(G, L, Dr, gp(lm)[r]);
  double *w = W + 36 * ((size_t)s * P + r);
#pragma unroll
  for (int x = 0; x < 6; ++x)
#pragma unroll
    for (int z = 0; z < 6; ++z) {
      gp(w)[6 * x + z] = G[x][z];
      gp(D)[(size_t)36 * r + 6 * x + z] = Dr[x][z];
    }
  gp(gw)[r] = g;
  gp(stw)[r] = 0;
}

// gain_cond out of the parity the last step wrote, and the two figures summed in selection order by one lane
__global__ __launch_bounds__(256) void k_select_finish(int P, int budget, const double *__restrict__ gains, const double *__restrict__ stepv,
                                                       const int *__restrict__ ctl, double *__restrict__ gain_cond, double *__restrict__ scal) {
  const int par = gp(ctl)[SC_PARITY], n = gp(ctl)[SC_NSEL];
  for (int k = blockIdx.x * 256 + threadIdx.x; k < P; k += gridDim.x * 256) gp(gain_cond)[k] = gp(gains)[(size_t)par * P + k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double gt = 0.0, lj = 0.0;
    for (int q = 0; q < n; ++q) {
      gt += gp(stepv)[q];
      lj += gp(stepv)[(size_t)budget + q];
    }
    gp(scal)[0] = gt;
    gp(scal)[1] = lj;
  }
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall SELECT = {"select_candidates", "candidate"};

// the step behind a covariance path's staged blocks: upload the records, open, eliminate up to the budget, queue the copies of
// the outputs
struct SelectEpilogue : ClosureEpilogue {
  std::vector<GateRec> cand;  // w0, w1: the ranks of i and j among the endpoints
  int m = 0;  // distinct endpoint poses
  int budget = 0;
  bool greedy = true;
  double min_gain = 0.0;
  DevBuf<GateRec> d_cand;
  DevBuf<double> d_W, d_work;
  DevBuf<int> d_int;
  std::vector<double> h_out;  // gain[P], gain_cond[P], gain_total, logdet_joint
  std::vector<int> h_int;     // rank[P], the control words
  SelectEpilogue() : ClosureEpilogue(3) {}
  // doubles of d_work: gain, gain_cond, the two figures | D, log det Sigma_meas, both parities of the gains, the steps' (gain, logdet)
  static size_t out_doubles(size_t P) { return 2 * P + 2; }
  static size_t work_doubles(size_t P, size_t b) { return out_doubles(P) + 36 * P + P + 2 * P + 2 * b; }
  // ints of d_int: rank, the control words | both parities of the state
  static size_t out_ints(size_t P) { return P + SC_WORDS; }
  static size_t work_ints(size_t P) { return out_ints(P) + 2 * P; }
  static double factor_bytes(size_t P, size_t b) { return 288.0 * (double)b * (double)P; }
  static double work_bytes(size_t P, size_t b) { return 8.0 * (double)work_doubles(P, b) + 4.0 * (double)work_ints(P) + 128.0 * (double)P; }
  int alloc() {
    const size_t P = cand.size(), b = (size_t)budget;
    if (d_cand.alloc(P) || d_W.alloc(36 * b * P) || d_work.alloc(work_doubles(P, b)) || d_int.alloc(work_ints(P))) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "select_candidates: device allocation failed (%.0f bytes for %zu candidates, budget %zu)",
                    factor_bytes(P, b) + work_bytes(P, b), P, b);
      set_err(buf);
      return DPGO_ERR;
    }
    return ev.create();
  }
  int run(const CovStage &st) override {
    const size_t P = cand.size();
    if (st.num_pairs != (int)((size_t)m * (m - 1) / 2)) {
      set_err("select_candidates: the staged blocks are not the pairs of the endpoints");
      return DPGO_ERR;
    }
    for (const GateRec &c : cand)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.w0 < 0 || c.w0 >= m || c.w1 < 0 || c.w1 >= m || c.w0 == c.w1) {
        set_err("select_candidates: a candidate lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateRec) * P, hipMemcpyHostToDevice, s));
    double *gain = d_work.p, *gc = gain + P, *scal = gc + P;
    double *D = scal + 2, *lm = D + 36 * P, *gains = lm + P, *stepv = gains + 2 * P;
    int *rank = d_int.p, *ctl = rank + P, *state = ctl + SC_WORDS;
    HIPC(hipMemsetAsync(ctl, 0, sizeof(int) * SC_WORDS, s));
    HIPC(hipEventRecord(ev[0], s));
    k_select_open<<<(unsigned)std::min<size_t>((P + 255) / 256, 2048), 256, 0, s>>>(st.Td, st.diag, st.pairs, d_cand.p, (int)P, m, D, lm, gain, gains,
                                                                                   state, rank);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    // `budget` steps queued without a word from the device in between: those behind a stop return at once
    const unsigned wgs = (unsigned)((P + 63) / 64);
    for (int step = 0; step < budget; ++step) {
      if (greedy)
        k_select_step<true><<<wgs, 64, 0, s>>>(step, (int)P, budget, m, min_gain, st.Td, st.diag, st.pairs, d_cand.p, d_W.p, D, lm, gains, state,
                                               rank, stepv, ctl);
      else
        k_select_step<false><<<wgs, 64, 0, s>>>(step, (int)P, budget, m, min_gain, st.Td, st.diag, st.pairs, d_cand.p, d_W.p, D, lm, gains, state,
                                                rank, stepv, ctl);
    }
    k_select_finish<<<(unsigned)std::min<size_t>((P + 255) / 256, 256), 256, 0, s>>>((int)P, budget, gains, stepv, ctl, gc, scal);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[2], s));
    h_out.resize(out_doubles(P));
    h_int.resize(out_ints(P));
    HIPC(hipMemcpyAsync(h_out.data(), d_work.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h_int.data(), d_int.p, sizeof(int) * h_int.size(), hipMemcpyDeviceToHost, s));
    ran = true;
    return DPGO_OK;
  }
};

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_select_candidates(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                           const dpgo_measurement_t *cand, int order, int budget, double min_gain, double *gain,
                                           double *gain_cond, int *rank, int *num_selected, double *gain_total, double *logdet_joint,
                                           dpgo_covariance_t *res) {
  const auto t_begin = std::chrono::steady_clock::now();
  // ---- the refusals of the call itself: on the host, before any device work, no output touched
  if (!t || !T || !res || !gain || !gain_cond || !rank || !num_selected || !gain_total || !logdet_joint) return SELECT.refuse("null argument");
  if (num <= 0) return SELECT.refuse("num must be positive, not " + std::to_string(num));
  if (!cand) return SELECT.refuse("null argument");
  if (budget < 1 || budget > num) return SELECT.refuse("budget must lie in [1, " + std::to_string(num) + "], not " + std::to_string(budget));
  if (SELECT.check_method(method)) return DPGO_ERR;
  if (order != DPGO_JOINT_GREEDY && order != DPGO_JOINT_GIVEN)
    return SELECT.refuse("order must be DPGO_JOINT_GREEDY or DPGO_JOINT_GIVEN, not " + std::to_string(order));
  if (min_gain != min_gain) return SELECT.refuse("min_gain must not be NaN (-INFINITY: no threshold)");
  if (check_team_local(t, SELECT.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  SelectEpilogue epi;
  epi.greedy = order == DPGO_JOINT_GREEDY;
  epi.budget = budget;
  epi.min_gain = min_gain;
  epi.cand.resize(num);
  for (int k = 0; k < num; ++k) {
    int g[2];
    if (SELECT.endpoints(t, offs, k, cand[k], g)) return DPGO_ERR;
    if (!(cand[k].kappa > 0.0) || !(cand[k].tau > 0.0) || !std::isfinite(cand[k].kappa) || !std::isfinite(cand[k].tau)) {
      char buf[200];  // (R~ and t~ are not read: nothing else of the record is checked)
      std::snprintf(buf, sizeof buf, "candidate %d has kappa = %.6g, tau = %.6g: both must be positive", k, cand[k].kappa, cand[k].tau);
      return SELECT.refuse(buf);
    }
    GateRec &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    c.m[12] = cand[k].kappa;
    c.m[13] = cand[k].tau;
  }
  const std::vector<int> poses = rank_endpoints(epi.cand);
  const int m = epi.m = (int)poses.size();
  const size_t P = (size_t)num, b = (size_t)budget, np = (size_t)m * (m - 1) / 2;
  HIPC(hipSetDevice(t->device));
  {
    // the pair blocks the path stages for this call, the factor and the working arrays: the rest is the path's own accounting
    const double blocks = 288.0 * (double)np, fac = SelectEpilogue::factor_bytes(P, b), work = SelectEpilogue::work_bytes(P, b);
    const double need = blocks + fac + work;
    double avail = 0.0;
    if (SELECT.device_avail(t, &avail)) return DPGO_ERR;
    if (need > avail || np > (size_t)INT32_MAX) {
      char buf[400];
      std::snprintf(buf, sizeof buf,
                    "%d candidates on %d poses, budget %d: the %zu pair blocks, the factor of %d x %d blocks and the working arrays need "
                    "%.0f bytes (%.0f + %.0f + %.0f), %.0f are available on the device",
                    num, m, budget, np, budget, num, need, blocks, fac, work, avail);
      return SELECT.refuse(buf);
    }
  }
  std::vector<int> pairs;
  pairs.reserve(2 * np);
  for (int a = 0; a < m; ++a)
    for (int c = a + 1; c < m; ++c) { pairs.push_back(poses[a]); pairs.push_back(poses[c]); }
  if (epi.alloc()) return DPGO_ERR;
  if (const int rc = SELECT.path(t, T, method, max_block, (int)np, pairs.data(), res, epi)) return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  const int *hi = epi.h_int.data();
  const int nsel = hi[P + SC_NSEL];
  if (timing) {
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "select_candidates: %d candidates on %d poses (%zu pair blocks), budget %d, k_select_open %.3f ms, elimination %.3f ms "
                         "(%d launches, %d selected), the whole call %.3f ms\n", num, m, np, budget, epi.ev.ms(0, 1), epi.ev.ms(1, 2), budget, nsel, whole);
  }
  const double *h = epi.h_out.data();
  std::memcpy(gain, h, sizeof(double) * P);
  std::memcpy(gain_cond, h + P, sizeof(double) * P);
  *gain_total = h[2 * P];
  *logdet_joint = h[2 * P + 1];
  std::memcpy(rank, hi, sizeof(int) * P);
  *num_selected = nsel;
  return DPGO_OK;
}

// gate.hip -- candidate measurements tested against the estimate's own uncertainty.
//
// T = (R_i, t_i) in team order, perturbed as in 5e: R_i <- R_i Exp(phi_i), t_i <- t_i + delta_i, rotation first, pose 0 fixed;
// Sigma the inverse reduced Hessian.  A candidate is a measurement (i -> j, R~, t~, kappa, tau) that is NOT in the graph.
//   relative pose   R_ij = R_i^T R_j,  t_ij = R_i^T (t_j - t_i),  perturbed the same way (delta_ij in frame i)
//   Jacobians       J_i = [[-R_ij^T, 0], [[t_ij]x, -R_i^T]],   J_j = [[I, 0], [0, R_i^T]]
//   Sigma_rel       J_i S_ii J_i^T + J_i S_ij J_j^T + J_j S_ij^T J_i^T + J_j S_jj J_j^T, stored as (A + A^T) / 2
//   innovation      xi = (Log(R~^T R_ij)v, t_ij - t~)
//   noise           Sigma_meas = diag(I / (2 kappa), I / tau): the inverse Hessian of the candidate's own term of the cost
//   distance        d^2 = xi^T (Sigma_rel + Sigma_meas)^-1 xi by a 6 x 6 Cholesky; a non-positive pivot gives +inf
// The blocks S_ii, S_jj, S_ij are those a covariance path has staged on the device (certify_internal.h, CovStage): k_gate is
// the step behind them, and only xi, d^2 and the requested Sigma_rel go to the host.
#include <map>

#include "certify_internal.h"
#include "gate_block.h"

namespace dpgo {

// one candidate on the device: team poses i != j, the staged pair block that holds S_ij, and the measurement (128 bytes)
struct GateCand {
  int i, j, blk, pad;
  double R[9];  // row-major
  double t[3];
  double kappa, tau;
};
static_assert(sizeof(GateCand) == 128, "GateCand is read in 16-byte loads");

// One lane per candidate, grid-stride.  fp64 in registers, no LDS, no atomics; the lane writes its own outputs and nothing
// else, so two calls give the same bits.  INNOV: xi and d2 are formed (else the relative covariance alone, and the
// measurement fields of the record are not read).  sigma_rel may be null.
template <bool INNOV>
__global__ __launch_bounds__(256) void k_gate(const double *__restrict__ T, const double *__restrict__ diag, const double *__restrict__ pairs,
                                              const GateCand *__restrict__ cand, int num, double *__restrict__ xi, double *__restrict__ d2,
                                              double *__restrict__ sigma_rel) {
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < (size_t)num; k += (size_t)gridDim.x * 256) {
    const double *rec = (const double *)(cand + k);
    typedef int v4i_t __attribute__((ext_vector_type(4)));
    const v4i_t ids = *(const __attribute__((address_space(1))) v4i_t *)rec;
    const int i = ids.x, j = ids.y, blk = ids.z;
    double M[3][3], tij[3], S[6][6];  // R_ij, t_ij, Sigma_rel
    gate_relative(T, diag, pairs, i, j, blk, M, tij, S);
    if (sigma_rel) {
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) gp(sigma_rel)[(size_t)36 * k + 6 * a + b] = S[a][b];
    }
    if constexpr (INNOV) {
      double v[14];  // doubles [2, 16) of the record: R~ row-major, t~, kappa, tau
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const double2 w = ld2(rec + 2 + 2 * q);
        v[2 * q] = w.x;
        v[2 * q + 1] = w.y;
      }
      const double *Rm = v, *tm = v + 9;
      const double nr = 1.0 / (2.0 * v[12]), nt = 1.0 / v[13];
      S[0][0] += nr; S[1][1] += nr; S[2][2] += nr;
      S[3][3] += nt; S[4][4] += nt; S[5][5] += nt;
      double E[3][3], x[6];  // E = R~^T R_ij
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) E[a][b] = __builtin_fma(Rm[6 + a], M[2][b], __builtin_fma(Rm[3 + a], M[1][b], Rm[a] * M[0][b]));
      gate_log_so3(E, x);
#pragma unroll
      for (int a = 0; a < 3; ++a) x[3 + a] = tij[a] - tm[a];
      // Cholesky of S in place (lower), forward solve y = L^-1 xi, d2 = |y|^2
      bool ok = true;
      double y[6], dd = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double p = S[c][c];
#pragma unroll
        for (int q = 0; q < c; ++q) p = __builtin_fma(-S[c][q], S[c][q], p);
        ok = ok && p > 0.0;
        const double l = sqrt(p), inv = 1.0 / l;
        S[c][c] = l;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
          double v = S[r][c];
#pragma unroll
          for (int q = 0; q < c; ++q) v = __builtin_fma(-S[r][q], S[c][q], v);
          S[r][c] = v * inv;
        }
        double v = x[c];
#pragma unroll
        for (int q = 0; q < c; ++q) v = __builtin_fma(-S[c][q], y[q], v);
        y[c] = v * inv;
        dd = __builtin_fma(y[c], y[c], dd);
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) gp(xi)[(size_t)6 * k + a] = x[a];
      gp(d2)[k] = ok ? dd : INFINITY;
    }
  }
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

// the step behind a covariance path's staged blocks: upload the records, run k_gate, queue the copies of what was asked for
struct GateEpilogue : CovEpilogue {
  std::vector<GateCand> cand;
  bool innov = false, want_sigma = false;
  DevBuf<GateCand> d_cand;
  DevBuf<double> d_out;  // xi[6 K], d2[K], sigma_rel[36 K], whichever are formed
  std::vector<double> h_xi, h_d2, h_sigma;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool ran = false;
  ~GateEpilogue() override {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int alloc() {
    const size_t K = cand.size();
    if (d_cand.alloc(K) || d_out.alloc((innov ? 7 * K : 0) + (want_sigma ? 36 * K : 0))) {
      set_err("gate_candidates: device allocation failed (" + std::to_string(K * (128 + (innov ? 56 : 0) + (want_sigma ? 288 : 0))) +
              " bytes for " + std::to_string(K) + " candidates)");
      return DPGO_ERR;
    }
    for (auto &e : ev) HIPC(hipEventCreate(&e));
    return DPGO_OK;
  }
  int run(const CovStage &st) override {
    const size_t K = cand.size();
    for (const GateCand &c : cand)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.blk < 0 || c.blk >= st.num_pairs) {
        set_err("gate_candidates: a candidate lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateCand) * K, hipMemcpyHostToDevice, s));
    double *xi = innov ? d_out.p : nullptr, *d2 = innov ? d_out.p + 6 * K : nullptr;
    double *sg = want_sigma ? d_out.p + (innov ? 7 * K : 0) : nullptr;
    // at most one workgroup per CU of an MI355X: the lanes beyond stride over the rest
    const unsigned grid = (unsigned)std::min<size_t>((K + 255) / 256, 256);
    HIPC(hipEventRecord(ev[0], s));
    if (innov) k_gate<true><<<grid, 256, 0, s>>>(st.Td, st.diag, st.pairs, d_cand.p, (int)K, xi, d2, sg);
    else k_gate<false><<<grid, 256, 0, s>>>(st.Td, st.diag, st.pairs, d_cand.p, (int)K, xi, d2, sg);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    if (innov) {
      h_xi.resize(6 * K); h_d2.resize(K);
      HIPC(hipMemcpyAsync(h_xi.data(), xi, sizeof(double) * 6 * K, hipMemcpyDeviceToHost, s));
      HIPC(hipMemcpyAsync(h_d2.data(), d2, sizeof(double) * K, hipMemcpyDeviceToHost, s));
    }
    if (want_sigma) {
      h_sigma.resize(36 * K);
      HIPC(hipMemcpyAsync(h_sigma.data(), sg, sizeof(double) * 36 * K, hipMemcpyDeviceToHost, s));
    }
    ran = true;
    return DPGO_OK;
  }
};

int gate_refuse(const std::string &m) {
  set_err("gate_candidates: " + m);
  return DPGO_ERR;
}

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_gate_candidates(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                         const dpgo_measurement_t *cand, double *xi, double *d2, double *sigma_rel,
                                         dpgo_covariance_t *res) {
  // ---- the refusals of the gate itself: on the host, before any device work, no output touched
  if (!t || !T || !res) return gate_refuse("null argument");
  if (num <= 0) return gate_refuse("num must be positive, not " + std::to_string(num));
  if (!cand) return gate_refuse("null argument");
  if (!xi && !d2 && !sigma_rel) return gate_refuse("no output requested (xi, d2 and sigma_rel are all null)");
  if ((xi == nullptr) != (d2 == nullptr)) return gate_refuse("xi and d2 come together: exactly one of them is null");
  if (method != DPGO_GATE_DENSE && method != DPGO_GATE_SCHUR && method != DPGO_GATE_NESTED)
    return gate_refuse("method must be DPGO_GATE_DENSE, DPGO_GATE_SCHUR or DPGO_GATE_NESTED, not " + std::to_string(method));
  if (check_team_local(t, "gate_candidates")) return DPGO_ERR;
  const int na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  for (int k = 0; k < na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  GateEpilogue epi;
  epi.innov = xi != nullptr;
  epi.want_sigma = sigma_rel != nullptr;
  epi.cand.resize(num);
  std::map<std::pair<int, int>, int> blk_of;  // the pair list handed to the path: each (i, j) once, in order of first use
  std::vector<int> pairs;
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &m = cand[k];
    int g[2];
    for (int e = 0; e < 2; ++e) {
      const int r = e ? m.r2 : m.r1, p = e ? m.p2 : m.p1;
      const auto l = t->id2local.find(r);
      if (l == t->id2local.end()) return gate_refuse("candidate " + std::to_string(k) + " names robot " + std::to_string(r) + ", which is not in the team");
      if (p < 0 || p >= t->ag[l->second]->n)
        return gate_refuse("candidate " + std::to_string(k) + " names pose " + std::to_string(p) + " of robot " + std::to_string(r) +
                           ", outside [0, " + std::to_string(t->ag[l->second]->n) + ")");
      g[e] = offs[l->second] + p;
    }
    if (g[0] == g[1]) return gate_refuse("candidate " + std::to_string(k) + " joins a pose to itself");
    GateCand &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    const auto ins = blk_of.insert({{g[0], g[1]}, (int)blk_of.size()});
    if (ins.second) { pairs.push_back(g[0]); pairs.push_back(g[1]); }
    c.blk = ins.first->second;
    if (!epi.innov) continue;
    if (!(m.kappa > 0.0) || !(m.tau > 0.0) || !std::isfinite(m.kappa) || !std::isfinite(m.tau)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "candidate %d has kappa = %.6g, tau = %.6g: both must be positive", k, m.kappa, m.tau);
      return gate_refuse(buf);
    }
    // R~ in SO(3) by the rule of T (covariance_host_checks); row-major here, which changes neither figure
    const double *R = m.R;
    double orth = 0.0;
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) {
        const double d = R[3 * p] * R[3 * q] + R[3 * p + 1] * R[3 * q + 1] + R[3 * p + 2] * R[3 * q + 2] - (p == q ? 1.0 : 0.0);
        orth = std::max(orth, std::fabs(d));
      }
    const double det = R[0] * (R[4] * R[8] - R[7] * R[5]) - R[3] * (R[1] * R[8] - R[7] * R[2]) + R[6] * (R[1] * R[5] - R[4] * R[2]);
    bool finite = true;
    for (int q = 0; q < 9; ++q) finite = finite && std::isfinite(R[q]);
    for (int q = 0; q < 3; ++q) finite = finite && std::isfinite(m.t[q]);
    if (!finite || !(orth <= 1e-8) || !(std::fabs(det - 1.0) <= 1e-8)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "the measurement of candidate %d is not in SE(3) (|R R^T - I| = %.3g, det R = %.12g)", k, orth, det);
      return gate_refuse(buf);
    }
    std::memcpy(c.R, m.R, sizeof c.R);
    std::memcpy(c.t, m.t, sizeof c.t);
    c.kappa = m.kappa; c.tau = m.tau;
  }
  HIPC(hipSetDevice(t->device));
  if (epi.alloc()) return DPGO_ERR;
  // ---- the covariance path, with its own refusals and messages; its blocks stay on the device for the epilogue
  const int np = (int)pairs.size() / 2;
  const int rc = method == DPGO_GATE_NESTED ? marginal_covariances_nested_call(t, T, max_block, np, pairs.data(), nullptr, nullptr, res, &epi)
                                            : marginal_covariances_call(t, T, method == DPGO_GATE_SCHUR ? DPGO_COV_SCHUR : 0, np, pairs.data(),
                                                                        nullptr, nullptr, res, &epi);
  if (rc != DPGO_OK) return rc;
  if (!epi.ran) {  // (a team of the anchor alone has no two poses to join: the endpoint checks have refused already)
    std::memset(res, 0, sizeof *res);
    return gate_refuse("the covariance path staged no blocks");
  }
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, epi.ev[0], epi.ev[1]));
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "gate_candidates: %d candidates on %d pair blocks, gate kernel %.3f ms\n", num, np, ms);
  const size_t K = (size_t)num;
  if (xi) std::memcpy(xi, epi.h_xi.data(), sizeof(double) * 6 * K);
  if (d2) std::memcpy(d2, epi.h_d2.data(), sizeof(double) * K);
  if (sigma_rel) std::memcpy(sigma_rel, epi.h_sigma.data(), sizeof(double) * 36 * K);
  return DPGO_OK;
}

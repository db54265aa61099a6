// audit.hip -- measurements that are in the graph tested against the rest of it: the leave-one-out audit.
//
// T, Sigma, the perturbation, R_ij, t_ij, J_i, J_j, Sigma_rel, xi and the logarithm are the gate's (gate.hip, gate_block.h).
// Record k is a measurement (i -> j, R~, t~, kappa, tau) that IS in the weighted graph at weight w >= 0 (w = 0: not in the
// Hessian).  Its own information w W0, W0 = diag(2 kappa I, tau I), is in Sigma, so its innovation is not independent of the
// estimate; taking it out again by the Woodbury identity needs the 6 x 6 blocks of the pair alone:
//   s = (sqrt(2 kappa) x 3, sqrt(tau) x 3),  z = s o xi,  C = diag(s) Sigma_rel diag(s),  A = I - w C,  B = I + (1 - w) C
//   rho = 1 - w tr(C) / 6 in [0, 1], the redundancy number;  p_min the smallest Cholesky pivot of A; testable: p_min > min_redundancy
//   d2 = z^T A^-1 B^-1 z: to first order in the residuals what the gate would give for this edge had it been left out of the graph
//   xi_loo = (A^-1 z) / s,  Sigma_loo = diag(1 / s) sym(A^-1 C) diag(1 / s) = (Sigma_rel^-1 - w W0)^-1
//   an untestable record, or a non-positive pivot of B, gives d2 = +inf and xi_loo = 0; untestable also Sigma_loo = 0
// The arithmetic is in audit_block.h.  The blocks are those a covariance path has staged on the device (certify_internal.h,
// CovStage): k_audit is the step behind them, and only the per-record outputs go to the host.
#include <map>

#include "certify_internal.h"
#include "audit_block.h"

namespace dpgo {

// one record on the device: team poses i != j, the staged pair block that holds S_ij, and the measurement with its weight
// (144 bytes: nine 16-byte loads; GateCand has no room for the weight)
struct AuditRec {
  int i, j, blk, pad;
  double m[AUDIT_REC];  // R~ row-major, t~, kappa, tau, w, padding
};
static_assert(sizeof(AuditRec) == 144 && sizeof(AuditRec) % 16 == 0, "AuditRec is read in 16-byte loads");

// One lane per record, grid-stride.  fp64 in registers, no LDS, no atomics, nothing across lanes; the lane writes its own
// outputs and nothing else, so two calls and duplicated records give the same bits.  SIGMA: Sigma_loo is formed and written.
template <bool SIGMA>
__global__ __launch_bounds__(256) void k_audit(const double *__restrict__ T, const double *__restrict__ diag, const double *__restrict__ pairs,
                                               const AuditRec *__restrict__ recs, int num, double min_redundancy, double *__restrict__ xi,
                                               double *__restrict__ xi_loo, double *__restrict__ d2, double *__restrict__ rho,
                                               double *__restrict__ pmin, double *__restrict__ sigma_loo) {
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < (size_t)num; k += (size_t)gridDim.x * 256) {
    const double *rec = (const double *)(recs + k);
    typedef int v4i_t __attribute__((ext_vector_type(4)));
    const v4i_t ids = *(const __attribute__((address_space(1))) v4i_t *)rec;
    double M[3][3], tij[3], S[6][6], SL[6][6];
    gate_relative(T, diag, pairs, ids.x, ids.y, ids.z, M, tij, S);
    AuditOut o;
    audit_record<SIGMA>(M, tij, S, rec + 2, min_redundancy, o, SL);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      gp(xi)[(size_t)6 * k + a] = o.xi[a];
      gp(xi_loo)[(size_t)6 * k + a] = o.xi_loo[a];
    }
    gp(d2)[k] = o.d2;
    gp(rho)[k] = o.rho;
    gp(pmin)[k] = o.pmin;
    if constexpr (SIGMA) {
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) gp(sigma_loo)[(size_t)36 * k + 6 * a + b] = SL[a][b];
    }
  }
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

// the step behind a covariance path's staged blocks: upload the records, run k_audit, queue the copies into staging vectors
struct AuditEpilogue : CovEpilogue {
  std::vector<AuditRec> rec;
  double min_redundancy = 0.0;
  bool want_sigma = false;
  DevBuf<AuditRec> d_rec;
  DevBuf<double> d_out;  // xi[6 K], xi_loo[6 K], d2[K], rho[K], pmin[K], sigma_loo[36 K] when it is formed
  std::vector<double> h_out;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool ran = false;
  ~AuditEpilogue() override {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  size_t doubles() const { return (size_t)(want_sigma ? 51 : 15) * rec.size(); }
  int alloc() {
    const size_t K = rec.size();
    if (d_rec.alloc(K) || d_out.alloc(doubles())) {
      set_err("audit_measurements: device allocation failed (" + std::to_string(K * sizeof(AuditRec) + 8 * doubles()) + " bytes for " +
              std::to_string(K) + " records)");
      return DPGO_ERR;
    }
    for (auto &e : ev) HIPC(hipEventCreate(&e));
    return DPGO_OK;
  }
  int run(const CovStage &st) override {
    const size_t K = rec.size();
    for (const AuditRec &c : rec)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.blk < 0 || c.blk >= st.num_pairs) {
        set_err("audit_measurements: a record lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    HIPC(hipMemcpyAsync(d_rec.p, rec.data(), sizeof(AuditRec) * K, hipMemcpyHostToDevice, s));
    double *xi = d_out.p, *xl = xi + 6 * K, *d2 = xl + 6 * K, *rho = d2 + K, *pm = rho + K, *sg = want_sigma ? pm + K : nullptr;
    // at most one workgroup per CU of an MI355X: the lanes beyond stride over the rest
    const unsigned grid = (unsigned)std::min<size_t>((K + 255) / 256, 256);
    HIPC(hipEventRecord(ev[0], s));
    if (want_sigma) k_audit<true><<<grid, 256, 0, s>>>(st.Td, st.diag, st.pairs, d_rec.p, (int)K, min_redundancy, xi, xl, d2, rho, pm, sg);
    else k_audit<false><<<grid, 256, 0, s>>>(st.Td, st.diag, st.pairs, d_rec.p, (int)K, min_redundancy, xi, xl, d2, rho, pm, sg);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    h_out.resize(doubles());
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * doubles(), hipMemcpyDeviceToHost, s));
    ran = true;
    return DPGO_OK;
  }
};

int audit_refuse(const std::string &m) {
  set_err("audit_measurements: " + m);
  return DPGO_ERR;
}

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_audit_measurements(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                            const dpgo_measurement_t *meas, double min_redundancy, double *xi, double *xi_loo,
                                            double *d2, double *rho, double *pmin, double *sigma_loo, dpgo_covariance_t *res) {
  // ---- the refusals of the audit itself: on the host, before any device work, no output touched
  if (!t || !T || !res || !xi || !xi_loo || !d2 || !rho || !pmin) return audit_refuse("null argument");
  if (num <= 0) return audit_refuse("num must be positive, not " + std::to_string(num));
  if (!meas) return audit_refuse("null argument");
  if (method != DPGO_GATE_DENSE && method != DPGO_GATE_SCHUR && method != DPGO_GATE_NESTED)
    return audit_refuse("method must be DPGO_GATE_DENSE, DPGO_GATE_SCHUR or DPGO_GATE_NESTED, not " + std::to_string(method));
  if (!(min_redundancy > 0.0 && min_redundancy < 1.0)) {
    char buf[120];
    std::snprintf(buf, sizeof buf, "min_redundancy must lie in (0, 1), not %.6g", min_redundancy);
    return audit_refuse(buf);
  }
  if (check_team_local(t, "audit_measurements")) return DPGO_ERR;
  const int na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  for (int k = 0; k < na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  AuditEpilogue epi;
  epi.min_redundancy = min_redundancy;
  epi.want_sigma = sigma_loo != nullptr;
  epi.rec.resize(num);
  std::map<std::pair<int, int>, int> blk_of;  // the pair list handed to the path: each (i, j) once, in order of first use
  std::vector<int> pairs;
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &m = meas[k];
    int g[2];
    for (int e = 0; e < 2; ++e) {
      const int r = e ? m.r2 : m.r1, p = e ? m.p2 : m.p1;
      const auto l = t->id2local.find(r);
      if (l == t->id2local.end()) return audit_refuse("record " + std::to_string(k) + " names robot " + std::to_string(r) + ", which is not in the team");
      if (p < 0 || p >= t->ag[l->second]->n)
        return audit_refuse("record " + std::to_string(k) + " names pose " + std::to_string(p) + " of robot " + std::to_string(r) +
                            ", outside [0, " + std::to_string(t->ag[l->second]->n) + ")");
      g[e] = offs[l->second] + p;
    }
    if (g[0] == g[1]) return audit_refuse("record " + std::to_string(k) + " joins a pose to itself");
    if (!(m.kappa > 0.0) || !(m.tau > 0.0) || !std::isfinite(m.kappa) || !std::isfinite(m.tau)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "record %d has kappa = %.6g, tau = %.6g: both must be positive", k, m.kappa, m.tau);
      return audit_refuse(buf);
    }
    if (!(m.weight >= 0.0) || !std::isfinite(m.weight)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "record %d has weight = %.6g: it must be finite and not negative", k, m.weight);
      return audit_refuse(buf);
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
      std::snprintf(buf, sizeof buf, "the measurement of record %d is not in SE(3) (|R R^T - I| = %.3g, det R = %.12g)", k, orth, det);
      return audit_refuse(buf);
    }
    AuditRec &c = epi.rec[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    const auto ins = blk_of.insert({{g[0], g[1]}, (int)blk_of.size()});
    if (ins.second) { pairs.push_back(g[0]); pairs.push_back(g[1]); }
    c.blk = ins.first->second;
    std::memcpy(c.m, m.R, sizeof m.R);
    std::memcpy(c.m + 9, m.t, sizeof m.t);
    c.m[12] = m.kappa; c.m[13] = m.tau; c.m[14] = m.weight;
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
    return audit_refuse("the covariance path staged no blocks");
  }
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, epi.ev[0], epi.ev[1]));
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "audit_measurements: %d records on %d pair blocks, audit kernel %.3f ms\n", num, np, ms);
  const size_t K = (size_t)num;
  const double *h = epi.h_out.data();
  std::memcpy(xi, h, sizeof(double) * 6 * K);
  std::memcpy(xi_loo, h + 6 * K, sizeof(double) * 6 * K);
  std::memcpy(d2, h + 12 * K, sizeof(double) * K);
  std::memcpy(rho, h + 13 * K, sizeof(double) * K);
  std::memcpy(pmin, h + 14 * K, sizeof(double) * K);
  if (sigma_loo) std::memcpy(sigma_loo, h + 15 * K, sizeof(double) * 36 * K);
  return DPGO_OK;
}

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
// CovStage): k_audit is the step behind them, and only the per-record outputs go to the host.  Across teams
// (dpgo_team_audit_measurements_across) the same kernel runs on every participant on the compact tables of AcrossStage.
#include "closure_frame.h"
#include "audit_block.h"

namespace dpgo {

// one record on the device: the head of GateRec (team poses i != j, the staged pair block that holds S_ij) and the measurement
// with its weight (144 bytes: nine 16-byte loads; GateRec has no room for the weight)
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

const ClosureCall AUDIT = {"audit_measurements", "record"};

// the device side of the audit behind either kind of staged tables: the records uploaded, k_audit, the copy into a staging vector
struct AuditWork {
  double min_redundancy = 0.0;
  bool want_sigma = false;
  DevBuf<AuditRec> d_rec;
  DevBuf<double> d_out;  // xi[6 K], xi_loo[6 K], d2[K], rho[K], pmin[K], sigma_loo[36 K] when it is formed
  std::vector<double> h_out;
  size_t doubles(size_t K) const { return (size_t)(want_sigma ? 51 : 15) * K; }
  int alloc(size_t K, const char *name) {
    if (d_rec.alloc(K) || d_out.alloc(doubles(K))) {
      set_err(std::string(name) + ": device allocation failed (" + std::to_string(K * sizeof(AuditRec) + 8 * doubles(K)) + " bytes for " +
              std::to_string(K) + " records)");
      return DPGO_ERR;
    }
    return DPGO_OK;
  }
  // rec: i, j index T and diag, blk indexes pairs (the caller has checked them against the tables)
  int queue(hipStream_t s, const double *Td, const double *diag, const double *pairs, const std::vector<AuditRec> &rec, const Events &ev) {
    const size_t K = rec.size();
    HIPC(hipMemcpyAsync(d_rec.p, rec.data(), sizeof(AuditRec) * K, hipMemcpyHostToDevice, s));
    double *xi = d_out.p, *xl = xi + 6 * K, *d2 = xl + 6 * K, *rho = d2 + K, *pm = rho + K, *sg = want_sigma ? pm + K : nullptr;
    // at most one workgroup per CU of an MI355X: the lanes beyond stride over the rest
    const unsigned grid = (unsigned)std::min<size_t>((K + 255) / 256, 256);
    HIPC(hipEventRecord(ev[0], s));
    if (want_sigma) k_audit<true><<<grid, 256, 0, s>>>(Td, diag, pairs, d_rec.p, (int)K, min_redundancy, xi, xl, d2, rho, pm, sg);
    else k_audit<false><<<grid, 256, 0, s>>>(Td, diag, pairs, d_rec.p, (int)K, min_redundancy, xi, xl, d2, rho, pm, sg);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    h_out.resize(doubles(K));
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * doubles(K), hipMemcpyDeviceToHost, s));
    return DPGO_OK;
  }
  void copy_out(size_t K, double *xi, double *xi_loo, double *d2, double *rho, double *pmin, double *sigma_loo) const {
    const double *h = h_out.data();
    std::memcpy(xi, h, sizeof(double) * 6 * K);
    std::memcpy(xi_loo, h + 6 * K, sizeof(double) * 6 * K);
    std::memcpy(d2, h + 12 * K, sizeof(double) * K);
    std::memcpy(rho, h + 13 * K, sizeof(double) * K);
    std::memcpy(pmin, h + 14 * K, sizeof(double) * K);
    if (sigma_loo) std::memcpy(sigma_loo, h + 15 * K, sizeof(double) * 36 * K);
  }
};

// the step behind a covariance path's staged blocks
struct AuditEpilogue : ClosureEpilogue, AuditWork {
  std::vector<AuditRec> rec;
  AuditEpilogue() : ClosureEpilogue(2) {}
  int alloc() { return AuditWork::alloc(rec.size(), "audit_measurements") ? DPGO_ERR : ev.create(); }
  int run(const CovStage &st) override {
    for (const AuditRec &c : rec)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.blk < 0 || c.blk >= st.num_pairs) {
        set_err("audit_measurements: a record lies outside the staged blocks");
        return DPGO_ERR;
      }
    if (queue(st.stream, st.Td, st.diag, st.pairs, rec, ev)) return DPGO_ERR;
    ran = true;
    return DPGO_OK;
  }
};

const ClosureCall AUDIT_ACROSS = {"audit_measurements_across", "record"};

// the same step behind the compact tables of the path across teams: every participant runs all K records
struct AuditAcross : RecordsAcross<AuditRec>, AuditWork {
  AuditAcross() : RecordsAcross<AuditRec>(&AUDIT_ACROSS, &AuditRec::blk, 5) {}
  int run(const AcrossStage &st) override {
    if (!inside(st)) { set_err("a record lies outside the staged blocks"); return DPGO_ERR; }
    if (AuditWork::alloc(rec.size(), "audit_measurements_across") || ev.create()) return DPGO_ERR;
    return queue(st.stream, st.Td, st.diag, st.pairs, rec, ev);
  }
};

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_audit_measurements(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                            const dpgo_measurement_t *meas, double min_redundancy, double *xi, double *xi_loo,
                                            double *d2, double *rho, double *pmin, double *sigma_loo, dpgo_covariance_t *res) {
  // ---- the refusals of the audit itself: on the host, before any device work, no output touched
  if (!t || !T || !res || !xi || !xi_loo || !d2 || !rho || !pmin) return AUDIT.refuse("null argument");
  if (num <= 0) return AUDIT.refuse("num must be positive, not " + std::to_string(num));
  if (!meas) return AUDIT.refuse("null argument");
  if (AUDIT.check_method(method)) return DPGO_ERR;
  if (!(min_redundancy > 0.0 && min_redundancy < 1.0)) {
    char buf[120];
    std::snprintf(buf, sizeof buf, "min_redundancy must lie in (0, 1), not %.6g", min_redundancy);
    return AUDIT.refuse(buf);
  }
  if (check_team_local(t, AUDIT.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  AuditEpilogue epi;
  epi.min_redundancy = min_redundancy;
  epi.want_sigma = sigma_loo != nullptr;
  epi.rec.resize(num);
  FirstUsePairs pairs;  // the pair list handed to the path
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &m = meas[k];
    int g[2];
    if (AUDIT.endpoints(t, offs, k, m, g) || AUDIT.check(k, m, true)) return DPGO_ERR;
    AuditRec &c = epi.rec[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    c.blk = pairs.block(g[0], g[1]);
    pack_measurement(m, c.m);
    c.m[14] = m.weight;
  }
  HIPC(hipSetDevice(t->device));
  if (epi.alloc()) return DPGO_ERR;
  const int np = pairs.count();
  if (const int rc = AUDIT.path(t, T, method, max_block, np, pairs.pairs.data(), res, epi)) return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "audit_measurements: %d records on %d pair blocks, audit kernel %.3f ms\n", num, np, epi.ev.ms());
  epi.copy_out((size_t)num, xi, xi_loo, d2, rho, pmin, sigma_loo);
  return DPGO_OK;
}

extern "C" int dpgo_team_audit_measurements_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot,
                                                   const double *T, int num, const dpgo_measurement_t *meas, double min_redundancy,
                                                   double *xi, double *xi_loo, double *d2, double *rho, double *pmin, double *sigma_loo,
                                                   dpgo_covariance_t *res) {
  const ClosureCall &A = AUDIT_ACROSS;
  if (res) std::memset(res, 0, sizeof *res);
  AuditAcross epi;
  epi.min_redundancy = min_redundancy;
  epi.want_sigma = sigma_loo != nullptr;
  // ---- the refusals of the audit itself, in the single team's order and words: decided here, told to everyone by the
  // agreement record (a participant that returned now would leave the others waiting)
  auto refusal = [&]() -> int {
    if (!T || !res || !xi || !xi_loo || !d2 || !rho || !pmin) return A.refuse("null argument");
    if (num <= 0) return A.refuse("num must be positive, not " + std::to_string(num));
    if (!meas) return A.refuse("null argument");
    if (!(min_redundancy > 0.0 && min_redundancy < 1.0)) {
      char buf[120];
      std::snprintf(buf, sizeof buf, "min_redundancy must lie in (0, 1), not %.6g", min_redundancy);
      return A.refuse(buf);
    }
    for (int k = 0; k < num; ++k) {
      const dpgo_measurement_t &m = meas[k];
      if (m.r1 == m.r2 && m.p1 == m.p2) return A.refuse(A.item(k) + " joins a pose to itself");
      if (A.check(k, m, true)) return DPGO_ERR;
    }
    return DPGO_OK;
  };
  if (refusal()) epi.argerr = A.refused();
  else {
    epi.meas = meas;
    epi.rec.resize(num);
    RecordHash h;
    h.add(epi.want_sigma ? 1 : 0);
    h.add(min_redundancy);
    for (int k = 0; k < num; ++k) {
      const dpgo_measurement_t &m = meas[k];
      AuditRec &c = epi.rec[k];
      std::memset(&c, 0, sizeof c);
      pack_measurement(m, c.m);
      c.m[14] = m.weight;
      h.add(m.r1); h.add(m.p1); h.add(m.r2); h.add(m.p2);
      h.add(c.m, sizeof(double) * 15);
    }
    epi.agree_num = num;
    epi.agree_hash = h.value();
  }
  SchurAcrossArgs a(t, tr, owner_rank_of_robot, T);
  a.res = res;
  a.step = &epi;
  if (const int rc = covariance_schur_across(a)) return rc;  // (res is then all zero)
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "audit_measurements_across: %d records on %zu pair blocks and %zu endpoints, audit kernel %.3f ms\n", num,
                 epi.pairs.size() / 2, epi.ends.size(), epi.ev.ms());
  epi.copy_out((size_t)num, xi, xi_loo, d2, rho, pmin, sigma_loo);
  return DPGO_OK;
}

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
// the step behind them, and only xi, d^2 and the requested Sigma_rel go to the host.  Across teams (dpgo_team_gate_candidates_across)
// the same kernel runs on every participant behind covariance_schur_across, on compact tables of the records' endpoints
// (AcrossStage): i, j and the block word index those instead of the team's arrays.
#include "closure_frame.h"

namespace dpgo {

// One lane per candidate, grid-stride.  fp64 in registers, no LDS, no atomics; the lane writes its own outputs and nothing
// else, so two calls give the same bits.  INNOV: xi and d2 are formed (else the relative covariance alone, and the
// measurement fields of the record are not read).  sigma_rel may be null.
template <bool INNOV>
__global__ __launch_bounds__(256) void k_gate(const double *__restrict__ T, const double *__restrict__ diag, const double *__restrict__ pairs,
                                              const GateRec *__restrict__ cand, int num, double *__restrict__ xi, double *__restrict__ d2,
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
      double v[GATE_MEAS], x[6];
      gate_load_meas(rec + 2, v);
      const double nr = 1.0 / (2.0 * v[12]), nt = 1.0 / v[13];
      S[0][0] += nr; S[1][1] += nr; S[2][2] += nr;
      S[3][3] += nt; S[4][4] += nt; S[5][5] += nt;
      gate_innovation(M, tij, v, x);
#pragma unroll
      for (int a = 0; a < 6; ++a) gp(xi)[(size_t)6 * k + a] = x[a];
      gp(d2)[k] = gate_distance(S, x);
    }
  }
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall GATE = {"gate_candidates", "candidate"};

// the device side of the gate behind either kind of staged tables: the records uploaded, k_gate, the copies of what was asked for
struct GateWork {
  bool innov = false, want_sigma = false;
  DevBuf<GateRec> d_cand;
  DevBuf<double> d_out;  // xi[6 K], d2[K], sigma_rel[36 K], whichever are formed
  std::vector<double> h_xi, h_d2, h_sigma;
  int alloc(size_t K, const char *name) {
    if (d_cand.alloc(K) || d_out.alloc((innov ? 7 * K : 0) + (want_sigma ? 36 * K : 0))) {
      set_err(std::string(name) + ": device allocation failed (" + std::to_string(K * (128 + (innov ? 56 : 0) + (want_sigma ? 288 : 0))) +
              " bytes for " + std::to_string(K) + " candidates)");
      return DPGO_ERR;
    }
    return DPGO_OK;
  }
  // cand: i, j index T and diag, w0 indexes pairs (the caller has checked them against the tables)
  int queue(hipStream_t s, const double *Td, const double *diag, const double *pairs, const std::vector<GateRec> &cand, const Events &ev) {
    const size_t K = cand.size();
    HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateRec) * K, hipMemcpyHostToDevice, s));
    double *xi = innov ? d_out.p : nullptr, *d2 = innov ? d_out.p + 6 * K : nullptr;
    double *sg = want_sigma ? d_out.p + (innov ? 7 * K : 0) : nullptr;
    // at most one workgroup per CU of an MI355X: the lanes beyond stride over the rest
    const unsigned grid = (unsigned)std::min<size_t>((K + 255) / 256, 256);
    HIPC(hipEventRecord(ev[0], s));
    if (innov) k_gate<true><<<grid, 256, 0, s>>>(Td, diag, pairs, d_cand.p, (int)K, xi, d2, sg);
    else k_gate<false><<<grid, 256, 0, s>>>(Td, diag, pairs, d_cand.p, (int)K, xi, d2, sg);
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
    return DPGO_OK;
  }
  void copy_out(size_t K, double *xi, double *d2, double *sigma_rel) const {
    if (xi) std::memcpy(xi, h_xi.data(), sizeof(double) * 6 * K);
    if (d2) std::memcpy(d2, h_d2.data(), sizeof(double) * K);
    if (sigma_rel) std::memcpy(sigma_rel, h_sigma.data(), sizeof(double) * 36 * K);
  }
};

// the step behind a covariance path's staged blocks
struct GateEpilogue : ClosureEpilogue, GateWork {
  std::vector<GateRec> cand;  // w0: the staged pair block that holds S_ij
  GateEpilogue() : ClosureEpilogue(2) {}
  int alloc() { return GateWork::alloc(cand.size(), "gate_candidates") ? DPGO_ERR : ev.create(); }
  int run(const CovStage &st) override {
    for (const GateRec &c : cand)
      if (c.i < 0 || c.i >= st.N || c.j < 0 || c.j >= st.N || c.w0 < 0 || c.w0 >= st.num_pairs) {
        set_err("gate_candidates: a candidate lies outside the staged blocks");
        return DPGO_ERR;
      }
    if (queue(st.stream, st.Td, st.diag, st.pairs, cand, ev)) return DPGO_ERR;
    ran = true;
    return DPGO_OK;
  }
};

const ClosureCall GATE_ACROSS = {"gate_candidates_across", "candidate"};

// the same step behind the compact tables of the path across teams: every participant runs all K records
struct GateAcross : RecordsAcross<GateRec>, GateWork {
  GateAcross() : RecordsAcross<GateRec>(&GATE_ACROSS, &GateRec::w0, 4) {}
  int run(const AcrossStage &st) override {
    if (!inside(st)) { set_err("a candidate lies outside the staged blocks"); return DPGO_ERR; }
    if (GateWork::alloc(rec.size(), "gate_candidates_across") || ev.create()) return DPGO_ERR;
    return queue(st.stream, st.Td, st.diag, st.pairs, rec, ev);
  }
};

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_gate_candidates(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                         const dpgo_measurement_t *cand, double *xi, double *d2, double *sigma_rel,
                                         dpgo_covariance_t *res) {
  // ---- the refusals of the gate itself: on the host, before any device work, no output touched
  if (!t || !T || !res) return GATE.refuse("null argument");
  if (num <= 0) return GATE.refuse("num must be positive, not " + std::to_string(num));
  if (!cand) return GATE.refuse("null argument");
  if (!xi && !d2 && !sigma_rel) return GATE.refuse("no output requested (xi, d2 and sigma_rel are all null)");
  if ((xi == nullptr) != (d2 == nullptr)) return GATE.refuse("xi and d2 come together: exactly one of them is null");
  if (GATE.check_method(method)) return DPGO_ERR;
  if (check_team_local(t, GATE.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  GateEpilogue epi;
  epi.innov = xi != nullptr;
  epi.want_sigma = sigma_rel != nullptr;
  epi.cand.resize(num);
  FirstUsePairs pairs;  // the pair list handed to the path
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &m = cand[k];
    int g[2];
    if (GATE.endpoints(t, offs, k, m, g)) return DPGO_ERR;
    GateRec &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    c.w0 = pairs.block(g[0], g[1]);
    if (!epi.innov) continue;  // (the relative covariance alone: the measurement fields are not read)
    if (GATE.check(k, m)) return DPGO_ERR;
    pack_measurement(m, c.m);
  }
  HIPC(hipSetDevice(t->device));
  if (epi.alloc()) return DPGO_ERR;
  const int np = pairs.count();
  if (const int rc = GATE.path(t, T, method, max_block, np, pairs.pairs.data(), res, epi)) return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "gate_candidates: %d candidates on %d pair blocks, gate kernel %.3f ms\n", num, np, epi.ev.ms());
  epi.copy_out((size_t)num, xi, d2, sigma_rel);
  return DPGO_OK;
}

extern "C" int dpgo_team_gate_candidates_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, const double *T,
                                                int num, const dpgo_measurement_t *cand, double *xi, double *d2, double *sigma_rel,
                                                dpgo_covariance_t *res) {
  const ClosureCall &G = GATE_ACROSS;
  if (res) std::memset(res, 0, sizeof *res);
  GateAcross epi;
  epi.innov = xi != nullptr;
  epi.want_sigma = sigma_rel != nullptr;
  // ---- the refusals of the gate itself, in the single team's order and words: decided here, told to everyone by the
  // agreement record (a participant that returned now would leave the others waiting)
  auto refusal = [&]() -> int {
    if (!T || !res) return G.refuse("null argument");
    if (num <= 0) return G.refuse("num must be positive, not " + std::to_string(num));
    if (!cand) return G.refuse("null argument");
    if (!xi && !d2 && !sigma_rel) return G.refuse("no output requested (xi, d2 and sigma_rel are all null)");
    if ((xi == nullptr) != (d2 == nullptr)) return G.refuse("xi and d2 come together: exactly one of them is null");
    for (int k = 0; k < num; ++k) {
      const dpgo_measurement_t &m = cand[k];
      if (m.r1 == m.r2 && m.p1 == m.p2) return G.refuse(G.item(k) + " joins a pose to itself");
      if (epi.innov && G.check(k, m)) return DPGO_ERR;
    }
    return DPGO_OK;
  };
  if (refusal()) epi.argerr = G.refused();
  else {
    epi.meas = cand;
    epi.rec.resize(num);
    RecordHash h;
    h.add((epi.innov ? 1 : 0) | (epi.want_sigma ? 2 : 0));
    for (int k = 0; k < num; ++k) {
      const dpgo_measurement_t &m = cand[k];
      GateRec &c = epi.rec[k];
      std::memset(&c, 0, sizeof c);
      h.add(m.r1); h.add(m.p1); h.add(m.r2); h.add(m.p2);
      if (!epi.innov) continue;  // (the relative covariance alone: the measurement fields are not read)
      pack_measurement(m, c.m);
      h.add(c.m, sizeof c.m);
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
    std::fprintf(stderr, "gate_candidates_across: %d candidates on %zu pair blocks and %zu endpoints, gate kernel %.3f ms\n", num,
                 epi.pairs.size() / 2, epi.ends.size(), epi.ev.ms());
  epi.copy_out((size_t)num, xi, d2, sigma_rel);
  return DPGO_OK;
}

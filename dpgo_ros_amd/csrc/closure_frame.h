// closure_frame.h -- the host-side frame of a call that takes a list of measurements and works behind a covariance path's
// staged blocks: gate_candidates (gate.hip), pairwise_consistency (consistency.hip), audit_measurements
// (audit.hip), gate_candidates_jointly (gate_joint.hip), linear_update (linear_update.hip) and select_candidates
// (select.hip).  One layer above covariance_frame.h: how a call words its refusals, resolves and checks a record, packs it for the device, lists the pairs it
// asks the path for, dispatches to the path, and times its own kernels.  A call keeps its own argument checks, the shape of
// its pair list, its budget and its copy-out; the ORDER of its refusals is the call's own too, and the tests see it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "certify_internal.h"
#include "covariance_frame.h"
#include "gate_block.h"

namespace dpgo_cert {

// timing events on a stream, destroyed with their owner
struct Events {
  std::vector<hipEvent_t> e;
  explicit Events(size_t n) : e(n, nullptr) {}
  Events(const Events &) = delete;
  Events &operator=(const Events &) = delete;
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int create() {
    for (hipEvent_t &x : e) HIPC(hipEventCreate(&x));
    return DPGO_OK;
  }
  hipEvent_t operator[](size_t k) const { return e[k]; }
  // the device time between two of them, on a drained stream; 0 where either was never created
  float ms(size_t from = 0, size_t to = 1) const {
    float v = 0.f;
    if (e[from] && e[to]) (void)hipEventElapsedTime(&v, e[from], e[to]);
    return v;
  }
};

// the step behind a covariance path's staged blocks, as the five calls have it: run() sets `ran` once everything is queued
struct ClosureEpilogue : CovEpilogue {
  bool ran = false;
  Events ev;
  explicit ClosureEpilogue(size_t events) : ev(events) {}
};

// a call by its name and the noun of its records ("candidate", "record", "closure")
struct ClosureCall {
  const char *name, *noun;

  int refuse(const std::string &msg) const {
    set_err(std::string(name) + ": " + msg);
    return DPGO_ERR;
  }
  std::string item(int k) const { return std::string(noun) + " " + std::to_string(k); }

  int check_method(int method) const {
    if (method == DPGO_GATE_DENSE || method == DPGO_GATE_SCHUR || method == DPGO_GATE_NESTED) return DPGO_OK;
    return refuse("method must be DPGO_GATE_DENSE, DPGO_GATE_SCHUR or DPGO_GATE_NESTED, not " + std::to_string(method));
  }

  // the team pose of (robot r, pose p) of record k, or a refusal.  team: the label of t where the call has two ("A")
  int endpoint(dpgo_team_t *t, const std::vector<int> &offs, int k, int r, int p, int *g, const char *team = nullptr) const {
    const auto l = t->id2local.find(r);
    if (l == t->id2local.end())
      return refuse(item(k) + " names robot " + std::to_string(r) + ", which is not in " + (team ? std::string("team ") + team : "the team"));
    if (p < 0 || p >= t->ag[l->second]->n)
      return refuse(item(k) + " names pose " + std::to_string(p) + " of robot " + std::to_string(r) + (team ? std::string(" of team ") + team : "") +
                    ", outside [0, " + std::to_string(t->ag[l->second]->n) + ")");
    *g = offs[l->second] + p;
    return DPGO_OK;
  }
  // both endpoints of record k in one team: two different team poses
  int endpoints(dpgo_team_t *t, const std::vector<int> &offs, int k, const dpgo_measurement_t &m, int g[2]) const {
    if (endpoint(t, offs, k, m.r1, m.p1, &g[0]) || endpoint(t, offs, k, m.r2, m.p2, &g[1])) return DPGO_ERR;
    if (g[0] == g[1]) return refuse(item(k) + " joins a pose to itself");
    return DPGO_OK;
  }

  // across teams: the GLOBAL pose (robots by id, then poses) of (robot r, pose p) of record k, or DPGO_ERR with the refusal in
  // msg -- the same words on every participant, which all hold the same records and the same numbering
  int global_endpoint(const Across &x, int k, int r, int p, int *g, std::string &msg) const {
    if (r < 0 || r >= x.num_robots) {
      msg = item(k) + " names robot " + std::to_string(r) + ", outside the problem's [0, " + std::to_string(x.num_robots) + ")";
      return DPGO_ERR;
    }
    if (p < 0 || p >= x.robot_n[r]) {
      msg = item(k) + " names pose " + std::to_string(p) + " of robot " + std::to_string(r) + ", outside [0, " + std::to_string(x.robot_n[r]) + ")";
      return DPGO_ERR;
    }
    *g = (int)(x.robot_goff[r] + p);
    return DPGO_OK;
  }

  // the fields of record k: kappa and tau positive, with_weight: the weight finite and not negative, and (R~, t~) in SE(3) by
  // the rule of T (covariance_host_checks; R~ is row-major here, which changes neither figure)
  int check(int k, const dpgo_measurement_t &m, bool with_weight = false) const {
    char buf[200];
    if (!(m.kappa > 0.0) || !(m.tau > 0.0) || !std::isfinite(m.kappa) || !std::isfinite(m.tau)) {
      std::snprintf(buf, sizeof buf, "%s %d has kappa = %.6g, tau = %.6g: both must be positive", noun, k, m.kappa, m.tau);
      return refuse(buf);
    }
    if (with_weight && (!(m.weight >= 0.0) || !std::isfinite(m.weight))) {
      std::snprintf(buf, sizeof buf, "%s %d has weight = %.6g: it must be finite and not negative", noun, k, m.weight);
      return refuse(buf);
    }
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
      std::snprintf(buf, sizeof buf, "the measurement of %s %d is not in SE(3) (|R R^T - I| = %.3g, det R = %.12g)", noun, k, orth, det);
      return refuse(buf);
    }
    return DPGO_OK;
  }

  // the words of the refusal just made (refuse, check) without the call's name: what travels as argerr across teams
  std::string refused() const {
    const std::string p = std::string(name) + ": ", e = g_err;
    return e.rfind(p, 0) == 0 ? e.substr(p.size()) : e;
  }

  // free bytes of the team's device for the call's budget (cov_device_avail), or a refusal
  int device_avail(dpgo_team_t *t, double *avail) const { return cov_device_avail(t, avail) ? DPGO_OK : refuse("hipMemGetInfo failed"); }

  // The covariance path by `method`, with its own refusals and messages, for the listed pairs; its blocks stay on the device
  // for the epilogue.  The path's code, or a refusal with res cleared when the path returned without staging anything (a team
  // of the anchor alone has no two poses to join: the endpoint checks refuse that before)
  // app: Sigma applied to vectors beside the blocks (covariance_apply.h), for a call that takes its columns from the solve
  int path(dpgo_team_t *t, const double *T, int method, int max_block, int np, const int *pairs, dpgo_covariance_t *res,
           ClosureEpilogue &epi, CovApply *app = nullptr) const {
    const int rc = method == DPGO_GATE_NESTED
                       ? marginal_covariances_nested_call(t, T, max_block, np, pairs, nullptr, nullptr, res, &epi, app)
                       : marginal_covariances_call(t, T, method == DPGO_GATE_SCHUR ? DPGO_COV_SCHUR : 0, np, pairs, nullptr, nullptr, res, &epi, app);
    if (rc != DPGO_OK) return rc;
    if (!epi.ran) {
      std::memset(res, 0, sizeof *res);
      return refuse("the covariance path staged no blocks");
    }
    return DPGO_OK;
  }
};

// pose offsets of the team's robots, na + 1
inline std::vector<int> pose_offsets(dpgo_team_t *t) {
  std::vector<int> offs(t->ag.size() + 1, 0);
  for (size_t k = 0; k < t->ag.size(); ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  return offs;
}

// the doubles of a device record from a checked measurement: R~ row-major, t~, kappa, tau (GATE_MEAS of them)
inline void pack_measurement(const dpgo_measurement_t &m, double *v) {
  std::memcpy(v, m.R, sizeof m.R);
  std::memcpy(v + 9, m.t, sizeof m.t);
  v[12] = m.kappa;
  v[13] = m.tau;
}

// the pair list of the gate and the audit: each ordered (i, j) once, in order of first use
struct FirstUsePairs {
  std::map<std::pair<int, int>, int> blk_of;
  std::vector<int> pairs;
  int block(int i, int j) {
    const auto ins = blk_of.insert({{i, j}, (int)blk_of.size()});
    if (ins.second) { pairs.push_back(i); pairs.push_back(j); }
    return ins.first->second;
  }
  int count() const { return (int)(pairs.size() / 2); }
};

// the endpoints of the joint gate and the update: the distinct poses (i, j) of the records, sorted, and into w0, w1 of every
// record the ranks of its two among them
inline std::vector<int> rank_endpoints(std::vector<GateRec> &recs) {
  std::vector<int> poses;
  for (const GateRec &c : recs) { poses.push_back(c.i); poses.push_back(c.j); }
  std::sort(poses.begin(), poses.end());
  poses.erase(std::unique(poses.begin(), poses.end()), poses.end());
  for (GateRec &c : recs) {
    c.w0 = (int)(std::lower_bound(poses.begin(), poses.end(), c.i) - poses.begin());
    c.w1 = (int)(std::lower_bound(poses.begin(), poses.end(), c.j) - poses.begin());
  }
  return poses;
}

// ---- across teams (the gate and the audit): the AcrossStep of a call with records

// (RecordHash, the hash of what every participant must pass alike: schur_across_plan.h)

// The frame of a per-record call over a split team: the records as the caller passed them, their device form (Rec: GateRec
// or AuditRec, whose words i, j and *blk the kernel reads as indices into the staged tables), and the hook's resolve().  The
// records' endpoints become global poses, the pair list is FirstUsePairs over them (the single team's rule), and i, j are
// rewritten to the ranks of the two poses among the sorted distinct endpoints: the compact tables of AcrossStage.
template <class Rec>
struct RecordsAcross : AcrossStep {
  const ClosureCall *call;
  int Rec::*blk;
  const dpgo_measurement_t *meas = nullptr;
  std::vector<Rec> rec;
  std::vector<int> ends;  // the records' endpoints: global poses, sorted, distinct
  Events ev;
  RecordsAcross(const ClosureCall *c, int Rec::*b, int op_) : call(c), blk(b), ev(2) { name = c->name; op = op_; }
  const std::vector<int> *endpoints() const override { return &ends; }

  int resolve(Across &x, std::string &msg) override {
    FirstUsePairs fp;
    for (size_t k = 0; k < rec.size(); ++k) {
      const dpgo_measurement_t &m = meas[k];
      int g[2];
      if (call->global_endpoint(x, (int)k, m.r1, m.p1, &g[0], msg) || call->global_endpoint(x, (int)k, m.r2, m.p2, &g[1], msg)) return DPGO_ERR;
      rec[k].i = g[0]; rec[k].j = g[1];
      rec[k].*blk = fp.block(g[0], g[1]);
      ends.push_back(g[0]); ends.push_back(g[1]);
    }
    pairs = fp.pairs;
    std::sort(ends.begin(), ends.end());
    ends.erase(std::unique(ends.begin(), ends.end()), ends.end());
    for (Rec &c : rec) {
      c.i = (int)(std::lower_bound(ends.begin(), ends.end(), c.i) - ends.begin());
      c.j = (int)(std::lower_bound(ends.begin(), ends.end(), c.j) - ends.begin());
    }
    return DPGO_OK;
  }
  // every index of every record inside the stage's tables (checked before the launch: the kernel does not)
  bool inside(const AcrossStage &st) const {
    for (const Rec &c : rec)
      if (c.i < 0 || c.i >= st.E || c.j < 0 || c.j >= st.E || c.*blk < 0 || c.*blk >= st.P) return false;
    return true;
  }
};

}  // namespace dpgo_cert

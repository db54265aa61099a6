// covariance_frame.h -- the host-side frame of a marginal-covariance call, shared by the dense path
// (covariance.hip), the robot-wise Schur path (covariance_schur.hip) and the nested path (covariance_nested.hip): the phase
// marks, the head and the tail of a call (CovFrame), the walk over the stored blocks of the team-wide Q, and the small
// functions every path words its refusals with.  The functions are defined in covariance.hip.
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "certify_internal.h"

namespace dpgo_cert {

// events: a mark per phase boundary; phase of the interval that ENDS at a mark: 0 assembly, 1 interior factorisations (the
// dense path: its one inverse), 2 products, 3 separator inverse, 4 extraction, -1 not counted
struct SchurMarks {
  std::vector<hipEvent_t> ev;
  std::vector<int> phase;
  std::vector<std::string> note;  // products: the shapes, for the DPGO_TIMING report
  std::vector<double> flops;
  ~SchurMarks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  int mark(int ph, hipStream_t s) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) { set_err("marginal_covariances: event failed"); return DPGO_ERR; }
    ev.push_back(e);
    phase.push_back(ph);
    note.emplace_back();
    flops.push_back(0.0);
    if (hipEventRecord(e, s) != hipSuccess) { set_err("marginal_covariances: event failed"); return DPGO_ERR; }
    return 0;
  }
  // milliseconds per phase, on a drained stream
  void sum(double ms[5]) const {
    for (int k = 0; k < 5; ++k) ms[k] = 0.0;
    for (size_t k = 1; k < ev.size(); ++k) {
      float v = 0.f;
      if (phase[k] >= 0 && hipEventElapsedTime(&v, ev[k - 1], ev[k]) == hipSuccess) ms[phase[k]] += v;
    }
  }
};
#define MARK(ph) do { if (marks.mark(ph, s)) return DPGO_ERR; } while (0)

// log det, smallest and largest pivot over the counted factors (stat: 4 doubles per factor, [logdet, min, max, spare]) summed
// in factor order, and the times of the phases (ms of SchurMarks::sum) into res; n = the order of H_red
void cov_fill_result(dpgo_covariance_t *res, long long n, const double *stat, const std::vector<char> &counted, const double ms[5]);

// The head and the tail of a single team's call.  d_small is carved into T, E = T Q, Lambda, the Gershgorin scratch of
// k_cert_lambda, [logdet, min, max, spare] per factor, with_keep: the kept blocks of the C_b, and the output blocks (the N
// diagonal blocks, then the pair blocks, 36 doubles each).
struct CovFrame {
  dpgo_team_t *t;
  hipStream_t s;
  int na = 0, N = 0, max_n = 0, nfactors = 0, num_pairs = 0;
  bool with_keep = false;
  size_t nout = 0;
  std::vector<int> offs;  // pose offsets of the robots, na + 1
  DevBuf<double> d_small;
  DevBuf<int> d_off;
  double *Td = nullptr, *lam = nullptr, *stat = nullptr, *keepd = nullptr, *outd = nullptr;
  SchurMarks marks;
  double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

  explicit CovFrame(dpgo_team_t *team);
  // allocates and carves d_small, uploads the offsets and T, queues Lambda(T), clears the kept and the output blocks (a path
  // without kept blocks writes every output element itself) and sets the first mark: the caller's assembly follows.  DPGO_OK,
  // DPGO_ERR (message set), or 1: the allocation failed (the caller names its bytes)
  int begin(const double *T, int nfactors_, int num_pairs_, bool with_keep_);
  // behind the last extraction launch: the statistics back (and the blocks when there is no epilogue), the epilogue, the drain
  // (also when the epilogue fails), res from the counted factors in order, the blocks into cov_diag / cov_pairs.  ms holds the
  // phase times afterwards: the caller prints its own DPGO_TIMING line
  int finish(CovEpilogue *epi, dpgo_covariance_t *res, double *cov_diag, double *cov_pairs, const std::vector<char> &counted);
};

// every stored block of the team-wide Q -- the entries of each robot's block-CSR, then its shared-edge records -- as
// fn(bi, bj, agent, idx): the block couples team poses bi (column) and bj (row) and lives with `agent` at CSR entry idx, or
// at shared-edge record ~idx.  -1 as soon as a block lies outside [0, N) or fn returns nonzero, else 0
template <class Fn>
int cov_for_each_stored_block(dpgo_team_t *t, const std::vector<int> &offs, Fn fn) {
  const int na = (int)t->ag.size(), N = offs[na];
  auto visit = [&](int bi, int bj, int agent, int idx) { return bi < 0 || bi >= N || bj < 0 || bj >= N || fn(bi, bj, agent, idx) != 0; };
  for (int k = 0; k < na; ++k) {
    const Agent &a = *t->ag[k];
    for (int j = 0; j < a.n; ++j)
      for (int p = a.rowptr[j]; p < a.rowptr[j + 1]; ++p)
        if (visit(offs[k] + a.col[p], offs[k] + j, k, p)) return -1;
    for (size_t e = 0; e < a.se_host.size(); ++e) {
      const SharedEdgeDev &se = a.se_host[e];
      if (se.src_agent_local < 0 || se.src_agent_local >= na || visit(offs[se.src_agent_local] + se.src_frame, offs[k] + se.lpose, k, ~(int)e))
        return -1;
    }
  }
  return 0;
}

// free bytes of the team's device plus the idle pooled buffers, which count as used memory but are one flush away from
// free (the accounting of the preconditioner budget, assembly.hip); false: hipMemGetInfo failed
bool cov_device_avail(dpgo_team_t *t, double *avail);

// the first pose of T (12 doubles each, R column-major in the first 9) that is not in SE(3) with its defect |R^T R - I| and
// det R, or -1
int se3_defect(const double *T, int N, double *orth, double *det);

// "<what>: non-positive pivot at row <row> of <where> (pose <pose>): the Hessian is not positive definite ..."
std::string pivot_message(const std::string &what, long long row, const std::string &where, long long pose);

}  // namespace dpgo_cert

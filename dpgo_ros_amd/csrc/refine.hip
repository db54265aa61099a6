// refine.hip -- a trajectory refined to a critical point of the SE(3) cost by Newton steps on Sigma: the
// kernels, the hook and the epilogue of a covariance path, and the drivers behind dpgo_team_refine and, over a team split across
// participants, dpgo_team_refine_across (at the end of the file).
//
// g(xi) = f(T [+] xi), the perturbation, the layout and pose 0 held fixed are 5e's.  From T_k:
//   E = T_k Q (launch_cert_apply3, Lambda off), g = J^T vec(E) (k_refine_grad, six numbers per pose), f the sum of the
//   measurements' terms (k_refine_cost), |g|_inf; two doubles to the host.  |g|_inf <= grad_tol: done, no path is run.
//   One covariance path with a CovApply of one column and no pair blocks: its rhs() copies g into V on the device (the path
//   has uploaded the same T), X = Sigma g comes back on the device.
//   Behind the path, in its epilogue: k_refine_trials writes the `ladder` trajectories T_k [+] (-2^-l X), k_refine_cost their
//   costs (blockIdx.y over the ladder), k_refine_sums the totals and the decrement g^T X; ladder + 1 doubles to the host.
//   The host takes the first l with f_l <= f - armijo 2^-l g^T X + eps_f; that trajectory becomes T_{k+1}.
// Every sum has a fixed order -- a lane's own term, an xor butterfly over the wave (addition commutes: every lane ends with the
// same bits), the waves of a workgroup and then the workgroups' partials in index order by one lane -- and there are no
// floating-point atomics: two calls give the same bytes.  Nothing here writes a solver vector.
#include <chrono>

#include "closure_frame.h"
#include "covariance_apply.h"
#include "refine_block.h"

namespace dpgo {

// the multiple of u f in eps_f: the additions an edge's term passes through inside refine_edge_cost and the butterfly (16 + 8),
// to which the driver adds the number of workgroup partials, summed one after another
constexpr int REFINE_EPS_CHAIN = 24;

// One lane per pose: the pose of T and of E in registers (16-byte loads), the six rows into g (column-major 6 N: rows 6 p ..
// 6 p + 5, 48 contiguous bytes per lane), the rows of the fixed pose (one team: 0; -1: none here) zero.  pmax[blockIdx.x] = the largest |g| of the workgroup's poses (a
// maximum has no order).  A NaN in g makes the partial NaN: the driver refuses it.
__global__ __launch_bounds__(256) void k_refine_grad(const double *__restrict__ T, const double *__restrict__ E, int N, int fixed,
                                                     double *__restrict__ g, double *__restrict__ pmax) {
  __shared__ double wmax[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double m = 0.0;
  if (p < N) {
    double R[3][3], t[3], Ep[12], gr[6];
    gate_load_pose(T, p, R, t);
    gate_load_pairs<6>(E + (size_t)12 * p, Ep);
    refine_grad_rows(p, fixed, R, Ep, gr);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      gp(g)[(size_t)6 * p + a] = gr[a];
      const double v = fabs(gr[a]);
      m = (v > m || v != v) ? v : m;
    }
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double o = __shfl_xor(m, off);
    m = (o > m || o != o) ? o : m;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = wmax[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) r = (wmax[w] > r || wmax[w] != wmax[w]) ? wmax[w] : r;
    gp(pmax)[blockIdx.x] = r;
  }
}

// One lane per (pose, ladder entry), the pose the faster index, grid-stride: trial l is T [+] (-2^-l X), 12 N doubles each
__global__ __launch_bounds__(256) void k_refine_trials(const double *__restrict__ T, const double *__restrict__ X, int N, int fixed,
                                                       int ladder, double *__restrict__ trials) {
  const size_t total = (size_t)N * ladder;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int l = (int)(e / N), p = (int)(e % N);
    double R[3][3], t[3], x[6], P[12];
    gate_load_pose(T, p, R, t);
    gate_load_pairs<3>(X + (size_t)6 * p, x);
    refine_trial_pose(p, fixed, R, t, x, ldexp(1.0, -l), P);
    double *o = trials + ((size_t)l * N + p) * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) gp(o)[q] = P[q];
  }
}

// One lane per measurement, blockIdx.y over the trajectories (12 N doubles apart): the lane's term, the wave's sum by an xor
// butterfly, the four waves in order; part[blockIdx.y * gridDim.x + blockIdx.x] = the workgroup's sum
__global__ __launch_bounds__(256) void k_refine_cost(const double *__restrict__ T, int N, const GateRec *__restrict__ edges, int num_edges,
                                                     double *__restrict__ part) {
  __shared__ double wsum[4];
  const double *Tl = T + (size_t)blockIdx.y * 12 * N;
  const int e = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (e < num_edges) {
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const v2i_t ij = *(const __attribute__((address_space(1))) v2i_t *)(edges + e);
    double Ri[3][3], ti[3], Rj[3][3], tj[3], v[GATE_MEAS];
    gate_load_pose(Tl, ij.x, Ri, ti);
    gate_load_pose(Tl, ij.y, Rj, tj);
    gate_load_meas(edges[e].m, v);
    s = refine_edge_cost(Ri, ti, Rj, tj, v);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) gp(part)[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ONE workgroup.  out[l] = the nblk partials of trajectory l in index order, l < count (lane l);  out[count] = a^T b over n
// entries: lane t its contiguous run in index order, lane 0 the 256 runs in lane order (a null: 0);  out[count + 1] = the
// largest of the npmax partials of k_refine_grad (pmax null: 0)
__global__ __launch_bounds__(256) void k_refine_sums(const double *__restrict__ part, int count, int nblk, const double *__restrict__ a,
                                                     const double *__restrict__ b, int n, const double *__restrict__ pmax, int npmax,
                                                     double *__restrict__ out) {
  __shared__ double run[256];
  const int t = threadIdx.x;
  if (t < count) {
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += gp(part)[(size_t)t * nblk + k];
    gp(out)[t] = s;
  }
  double d = 0.0;
  if (a) {
    const int per = (n + 255) / 256;
    for (int k = t * per; k < min(n, (t + 1) * per); ++k) d = __builtin_fma(gp(a)[k], gp(b)[k], d);
  }
  run[t] = d;
  __syncthreads();
  if (t != 0) return;
  double s = 0.0;
  for (int k = 0; k < 256; ++k) s += run[k];
  gp(out)[count] = s;
  double m = 0.0;
  for (int k = 0; pmax && k < npmax; ++k) {
    const double v = gp(pmax)[k];
    m = (v > m || v != v) ? v : m;
  }
  gp(out)[count + 1] = m;
}

// ---- across teams ("Across teams"): every sum belongs to ONE robot and depends on nothing but the robot.
//
// k_refine_cost over the robots held here: blockIdx.z = the robot (team order), blockIdx.y = the trajectory (12 Nall doubles
// apart, Nall = the participant's poses and their halo), blockIdx.x = a workgroup of 256 of the robot's OWN measurements, in the
// order of the robot's own list (eoff: na + 1 offsets into edges).  The grid covers the largest robot; a workgroup beyond its
// robot's last leaves at once.  The lane's term, the butterfly and the wave order are k_refine_cost's.
// part[(robot * gridDim.y + trajectory) * gridDim.x + workgroup]
__global__ __launch_bounds__(256) void k_refine_cost_robots(const double *__restrict__ T, int Nall, const GateRec *__restrict__ edges,
                                                            const int *__restrict__ eoff, double *__restrict__ part) {
  __shared__ double wsum[4];
  const int a = blockIdx.z;
  const int e0 = eoff[a], ne = eoff[a + 1] - e0;
  if ((int)blockIdx.x * 256 >= ne) return;
  const double *Tl = T + (size_t)blockIdx.y * 12 * Nall;
  const int e = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (e < ne) {
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const GateRec *rec = edges + e0 + e;
    const v2i_t ij = *(const __attribute__((address_space(1))) v2i_t *)rec;
    double Ri[3][3], ti[3], Rj[3][3], tj[3], v[GATE_MEAS];
    gate_load_pose(Tl, ij.x, Ri, ti);
    gate_load_pose(Tl, ij.y, Rj, tj);
    gate_load_meas(rec->m, v);
    s = refine_edge_cost(Ri, ti, Rj, tj, v);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    gp(part)[((size_t)a * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ONE workgroup per robot held here (blockIdx.x, team order).  out[robot * (count + 1) + l] = the robot's ceil(E_a / 256)
// partials of trajectory l in index order (lane l; maxblk: the partials' stride);  out[robot * (count + 1) + count] = a^T b over
// the robot's own 6 n_a rows (poff: na + 1 pose offsets) by k_refine_sums' rule -- lane t its contiguous run in index order, lane
// 0 the 256 runs in lane order (a null: 0);  the first workgroup also out[na * (count + 1)] = the largest of the npmax partials of
// k_refine_grad (pmax null: 0).  No total depends on which participant holds the robot, or on the robots beside it
__global__ __launch_bounds__(256) void k_refine_sums_robots(const double *__restrict__ part, int count, int maxblk, const int *__restrict__ eoff,
                                                            const int *__restrict__ poff, const double *__restrict__ a,
                                                            const double *__restrict__ b, const double *__restrict__ pmax, int npmax,
                                                            double *__restrict__ out) {
  __shared__ double run[256];
  const int t = threadIdx.x, r = blockIdx.x;
  double *o = out + (size_t)r * (count + 1);
  if (t < count) {
    const int nblk = (eoff[r + 1] - eoff[r] + 255) / 256;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += gp(part)[((size_t)r * count + t) * maxblk + k];
    gp(o)[t] = s;
  }
  double d = 0.0;
  if (a) {
    const int r0 = 6 * poff[r], n = 6 * (poff[r + 1] - poff[r]);
    const int per = (n + 255) / 256;
    for (int k = t * per; k < min(n, (t + 1) * per); ++k) d = __builtin_fma(gp(a)[r0 + k], gp(b)[r0 + k], d);
  }
  run[t] = d;
  __syncthreads();
  if (t != 0) return;
  double s = 0.0;
  for (int k = 0; k < 256; ++k) s += run[k];
  gp(o)[count] = s;
  if (r != 0) return;
  double m = 0.0;
  for (int k = 0; pmax && k < npmax; ++k) {
    const double v = gp(pmax)[k];
    m = (v > m || v != v) ? v : m;
  }
  gp(out)[(size_t)gridDim.x * (count + 1)] = m;
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall REFINE = {"refine", "iterate"};

// whether the last error is a covariance path's refusal of a pivot: it then ends with what pivot_message (covariance_frame.h)
// puts behind the pivot's place, taken from pivot_message itself so that a rewording there is followed here
bool pivot_refused() {
  static const std::string tail = [] {
    const std::string m = pivot_message("", 0, "", 0);
    const size_t at = m.rfind("): ");
    return at == std::string::npos ? m : m.substr(at + 3);
  }();
  return g_err.size() >= tail.size() && g_err.compare(g_err.size() - tail.size(), tail.size(), tail) == 0;
}

// what the driver keeps on the device for the whole call
struct RefineWs {
  dpgo_team_t *t = nullptr;
  int N = 0, na = 0, max_n = 0, ladder = 0, num_edges = 0, nblk_e = 0, nblk_p = 0;
  DevBuf<double> d_T, d_E, d_g, d_trials, d_part, d_pmax, d_out;
  DevBuf<int> d_off;
  DevBuf<GateRec> d_edges;
  std::vector<double> h_out;  // ladder + 2

  int alloc(hipStream_t s, const std::vector<int> &offs, const std::vector<GateRec> &edges) {
    num_edges = (int)edges.size();
    nblk_e = std::max(1, (num_edges + 255) / 256);
    nblk_p = (N + 255) / 256;
    h_out.assign((size_t)ladder + 2, 0.0);
    if (d_T.alloc((size_t)12 * N) || d_E.alloc((size_t)12 * N) || d_g.alloc((size_t)6 * N) || d_trials.alloc((size_t)12 * N * ladder) ||
        d_part.alloc((size_t)nblk_e * ladder) || d_pmax.alloc((size_t)nblk_p) || d_out.alloc((size_t)ladder + 2) || d_off.upload(offs, s) ||
        d_edges.upload(edges, s))
      return REFINE.refuse("device allocation failed (" + std::to_string(8 * ((size_t)12 * N * (ladder + 2) + 6 * (size_t)N) + 128 * edges.size()) +
                           " bytes for " + std::to_string(ladder) + " trial trajectories of " + std::to_string(N) + " poses)");
    return DPGO_OK;
  }
  // g = J^T vec(T Q) of the trajectory at Td into out (6 N), the workgroups' maxima into d_pmax
  int gradient(hipStream_t s, const double *Td, double *out) {
    launch_cert_apply3(s, t->d_agents.p, d_off.p, na, max_n, Td, d_E.p, nullptr);
    k_refine_grad<<<nblk_p, 256, 0, s>>>(Td, d_E.p, N, 0, out, d_pmax.p);
    HIPC(hipGetLastError());
    return DPGO_OK;
  }
  // the costs of `count` trajectories at Td (12 N doubles apart) into d_out[0 .. count), a^T b and the gradient's maximum behind
  int costs(hipStream_t s, const double *Td, int count, const double *a, const double *b, bool with_max) {
    k_refine_cost<<<dim3(nblk_e, count), 256, 0, s>>>(Td, N, d_edges.p, num_edges, d_part.p);
    k_refine_sums<<<1, 256, 0, s>>>(d_part.p, count, nblk_e, a, b, 6 * N, with_max ? d_pmax.p : nullptr, nblk_p, d_out.p);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * ((size_t)count + 2), hipMemcpyDeviceToHost, s));
    return DPGO_OK;
  }
};

// the hook of the step: the gradient the driver has just formed at this very T, device to device into V
struct RefineRhs : CovApply {
  RefineWs *ws = nullptr;
  int rhs(const double *, int N, double *V, hipStream_t s) override {
    if (N != ws->N) return REFINE.refuse("the covariance path's poses are not the call's");
    HIPC(hipMemcpyAsync(V, ws->d_g.p, sizeof(double) * 6 * (size_t)N, hipMemcpyDeviceToDevice, s));
    return DPGO_OK;
  }
};

// the step behind the path: the trial trajectories, their costs and the decrement
struct RefineTrials : ClosureEpilogue {
  RefineWs *ws = nullptr;
  RefineRhs *app = nullptr;
  RefineTrials() : ClosureEpilogue(3) {}
  int run(const CovStage &st) override {
    if (!app->X) return REFINE.refuse("the covariance path formed no X");
    if (st.N != ws->N) return REFINE.refuse("the covariance path's poses are not the call's");
    hipStream_t s = st.stream;
    HIPC(hipEventRecord(ev[0], s));
    k_refine_trials<<<(unsigned)std::min<size_t>(((size_t)ws->N * ws->ladder + 255) / 256, 2048), 256, 0, s>>>(st.Td, app->X, ws->N, 0, ws->ladder,
                                                                                                               ws->d_trials.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    // (d_g is what the hook copied into V)
    if (ws->costs(s, ws->d_trials.p, ws->ladder, ws->d_g.p, app->X, false)) return DPGO_ERR;
    HIPC(hipEventRecord(ev[2], s));
    ran = true;
    return DPGO_OK;
  }
};

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_refine(dpgo_team_t *t, const double *T, int method, int max_block, int max_iters, double grad_tol, double armijo,
                                int ladder, double *T_out, double *history, dpgo_refine_t *out, dpgo_covariance_t *res) {
  const auto t_begin = std::chrono::steady_clock::now();
  if (res) std::memset(res, 0, sizeof *res);
  if (out) std::memset(out, 0, sizeof *out);
  // ---- the refusals of the call itself: on the host, before any device work, T_out untouched
  if (!t || !T || !T_out || !history || !out || !res) return REFINE.refuse("null argument");
  if (max_iters < 0) return REFINE.refuse("max_iters must not be negative, not " + std::to_string(max_iters));
  if (ladder < 1 || ladder > 32) return REFINE.refuse("ladder must lie in [1, 32], not " + std::to_string(ladder));
  if (!(grad_tol > 0.0) || !std::isfinite(grad_tol)) return REFINE.refuse("grad_tol must be positive and finite");
  if (!(armijo > 0.0) || !(armijo < 1.0)) return REFINE.refuse("armijo must lie in (0, 1)");
  if (REFINE.check_method(method)) return DPGO_ERR;
  if (method == DPGO_GATE_SCHUR)
    return REFINE.refuse("there is no apply on the robot-wise Schur path: DPGO_GATE_NESTED (method=\"nested\") with no robot split has the "
                         "Schur path's sets");
  if (check_team_local(t, REFINE.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  const int N = offs.back();
  {
    double orth = 0.0, det = 0.0;
    const int g = se3_defect(T, N, &orth, &det);
    if (g >= 0) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "pose %d of T is not in SE(3) (|R^T R - I| = %.3g, det R = %.12g)", g, orth, det);
      return REFINE.refuse(buf);
    }
  }
  // the measurements with their weights folded into kappa and tau, in team numbering
  std::vector<GateRec> edges;
  {
    std::vector<dpgo_measurement_t> mm;
    if (team_measurements(t, offs, REFINE.name, mm)) return DPGO_ERR;
    edges.resize(mm.size());
    for (size_t k = 0; k < mm.size(); ++k) {
      GateRec &c = edges[k];
      std::memset(&c, 0, sizeof c);
      c.i = mm[k].p1; c.j = mm[k].p2;
      if (c.i < 0 || c.i >= N || c.j < 0 || c.j >= N) return REFINE.refuse("a measurement names a pose outside the team");
      pack_measurement(mm[k], c.m);
      c.m[12] *= mm[k].weight;
      c.m[13] *= mm[k].weight;
    }
  }
  std::vector<double> hist((size_t)5 * (max_iters + 1), std::nan(""));
  auto finish = [&](int status, int iters, const std::vector<double> &Tk) {
    out->status = status;
    out->iterations = iters;
    out->f0 = hist[0]; out->grad_inf0 = hist[1];
    out->f = hist[(size_t)5 * iters]; out->grad_inf = hist[(size_t)5 * iters + 1];
    std::memcpy(history, hist.data(), sizeof(double) * hist.size());
    std::memcpy(T_out, Tk.data(), sizeof(double) * 12 * (size_t)N);
    return DPGO_OK;
  };
  std::vector<double> Tk(T, T + (size_t)12 * N);
  HIPC(hipSetDevice(t->device));
  if (check_team(t, REFINE.name)) return DPGO_ERR;
  hipStream_t s = t->stream;
  RefineWs ws;
  ws.t = t; ws.N = N; ws.na = (int)t->ag.size(); ws.ladder = ladder;
  for (const auto &a : t->ag) ws.max_n = std::max(ws.max_n, a->n);
  if (ws.alloc(s, offs, edges)) return DPGO_ERR;
  HIPC(hipMemcpyAsync(ws.d_T.p, Tk.data(), sizeof(double) * 12 * (size_t)N, hipMemcpyHostToDevice, s));
  const double eps_mult = (double)(REFINE_EPS_CHAIN + ws.nblk_e) * 0x1p-53;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  double ms_grad = 0.0, ms_path = 0.0, ms_trials = 0.0, ms_costs = 0.0;
  dpgo_covariance_t last;
  std::memset(&last, 0, sizeof last);
  RefineRhs hook;
  hook.ws = &ws;
  hook.num_cols = 1;
  RefineTrials epi;
  epi.ws = &ws;
  epi.app = &hook;
  if (epi.ev.create()) return DPGO_ERR;
  int k = 0, status = DPGO_REFINE_MAX_ITERS;
  for (;;) {
    // ---- gradient and cost of T_k: two doubles to the host
    const auto t0 = std::chrono::steady_clock::now();
    if (ws.gradient(s, ws.d_T.p, ws.d_g.p) || ws.costs(s, ws.d_T.p, 1, nullptr, nullptr, true)) return DPGO_ERR;
    HIPC(hipStreamSynchronize(s));
    ms_grad += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const double f = ws.h_out[0], ginf = ws.h_out[2];
    hist[(size_t)5 * k] = f;
    hist[(size_t)5 * k + 1] = ginf;
    if (!std::isfinite(f) || !std::isfinite(ginf)) return REFINE.refuse("the cost or the gradient is not finite at iterate " + std::to_string(k));
    if (ginf <= grad_tol) { status = DPGO_REFINE_CONVERGED; break; }
    if (k == max_iters) { status = DPGO_REFINE_MAX_ITERS; break; }
    // ---- the step: X = Sigma g on the factors of one covariance path, the trials behind it
    hook.X = nullptr;
    epi.ran = false;
    dpgo_covariance_t cur;
    const auto t1 = std::chrono::steady_clock::now();
    const int rc = REFINE.path(t, Tk.data(), method, max_block, 0, nullptr, &cur, epi, &hook);
    if (rc != DPGO_OK) {
      // a pivot that is not positive: at the input the call is refused in the path's words, later it stops at the last good T
      if (!pivot_refused()) return rc;
      if (k == 0) { set_err("refine: " + g_err); return DPGO_ERR; }
      status = DPGO_REFINE_INDEFINITE;
      break;
    }
    last = cur;
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    ms_trials += epi.ev.ms(0, 1);
    ms_costs += epi.ev.ms(1, 2);
    ms_path += whole - epi.ev.ms(0, 2);
    const double dec = ws.h_out[ladder];
    hist[(size_t)5 * k + 3] = dec;
    hist[(size_t)5 * k + 4] = cur.min_pivot;
    // ---- acceptance: the first entry of the ladder with sufficient decrease, up to the rounding of the cost's sum
    int took = -1;
    for (int l = 0; l < ladder && took < 0; ++l)
      if (ws.h_out[l] <= f - armijo * std::ldexp(1.0, -l) * dec + eps_mult * std::fabs(f)) took = l;
    if (took < 0) { status = DPGO_REFINE_NO_DESCENT; break; }
    hist[(size_t)5 * k + 2] = std::ldexp(1.0, -took);
    const double *Tn = ws.d_trials.p + (size_t)took * 12 * N;
    HIPC(hipMemcpyAsync(ws.d_T.p, Tn, sizeof(double) * 12 * (size_t)N, hipMemcpyDeviceToDevice, s));
    // (the covariance path checks and uploads a host T: the accepted trajectory comes back as well)
    HIPC(hipMemcpyAsync(Tk.data(), Tn, sizeof(double) * 12 * (size_t)N, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    ++k;
  }
  *res = last;
  if (timing)
    std::fprintf(stderr, "refine: %d poses, %d measurements, %d iterations, status %d: gradient and cost %.3f ms, covariance paths %.3f ms, "
                         "k_refine_trials %.3f ms, k_refine_cost and sums %.3f ms, the whole call %.3f ms\n",
                 N, ws.num_edges, k, status, ms_grad, ms_path, ms_trials, ms_costs,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  return finish(status, k, Tk);
}

// ---- the same iteration over a team split across participants ("Across teams"; the conventions of
// certify_across.hip).  Transport calls, the same on every participant: the two allgathers of the driver's own
// Across::begin; per evaluated iterate one exchange (the T halo) and one allgather (per robot its cost and the number of
// measurements it owns, per participant its |g|_inf); per step the calls of covariance_schur_across with no pairs and one
// allgather (per robot the ladder's costs and its share of g^T X); the closing status word.  Every host decision is taken on the
// robots' totals added in robot order from 0, the same bits on every participant.
namespace dpgo_cert {

namespace {

const ClosureCall REFINE_ACROSS = {"refine_across", "iterate"};

struct RefineAcrossWs {
  dpgo_team_t *t = nullptr;
  Across *x = nullptr;
  int N = 0, na = 0, max_n = 0, halo = 0, Nall = 0, ladder = 0, fixed = -1, maxblk = 1, nblk_p = 0;
  DevBuf<double> d_T, d_E, d_g, d_X, d_trials, d_part, d_pmax, d_out, d_xa;
  DevBuf<int> d_off, d_eoff, d_xi, d_map;
  DevBuf<GateRec> d_edges;
  std::vector<int> offs, eoff, h_map;
  std::vector<GateRec> edges;
  std::vector<double> h_out;  // na (ladder + 1) + 1

  // this participant's robots' own measurements, robot after robot in the order of the robot's list: a private one is its
  // robot's, a shared one the lower robot's (team_measurements' rule).  An endpoint on a robot held elsewhere is its halo slot
  // behind the N poses here
  int measurements() {
    eoff.assign(na + 1, 0);
    std::vector<dpgo_measurement_t> ma;
    for (int k = 0; k < na; ++k) {
      const Agent &A = *t->ag[k];
      const int cntm = dpgo_agent_get_measurements(t, A.id, nullptr);
      if (cntm < 0) return DPGO_ERR;
      ma.resize(cntm);
      if (cntm > 0 && dpgo_agent_get_measurements(t, A.id, ma.data()) != cntm) return DPGO_ERR;
      for (const auto &m : ma) {
        if (m.r1 != m.r2 && std::min(m.r1, m.r2) != A.id) continue;
        int g[2];
        const int rr[2] = {m.r1, m.r2}, pp[2] = {m.p1, m.p2};
        for (int e = 0; e < 2; ++e) {
          const auto l = t->id2local.find(rr[e]);
          if (l != t->id2local.end()) {
            if (pp[e] < 0 || pp[e] >= t->ag[l->second]->n) return REFINE_ACROSS.refuse("a measurement names a pose outside its robot");
            g[e] = offs[l->second] + pp[e];
          } else {
            const auto key = std::make_pair(rr[e], pp[e]);
            const auto it = std::lower_bound(A.np.begin(), A.np.end(), key);
            if (it == A.np.end() || *it != key) return REFINE_ACROSS.refuse("a shared measurement names a pose its robot does not list");
            g[e] = N + x->hoffs[k] + (int)(it - A.np.begin());
          }
        }
        GateRec c;
        std::memset(&c, 0, sizeof c);
        c.i = g[0]; c.j = g[1];
        pack_measurement(m, c.m);
        c.m[12] *= m.weight;
        c.m[13] *= m.weight;
        edges.push_back(c);
      }
      eoff[k + 1] = (int)edges.size();
      maxblk = std::max(maxblk, (eoff[k + 1] - eoff[k] + 255) / 256);
    }
    return DPGO_OK;
  }

  int alloc(hipStream_t s) {
    nblk_p = (N + 255) / 256;
    h_out.assign((size_t)na * (ladder + 1) + 1, 0.0);
    if (d_T.alloc((size_t)12 * Nall) || d_E.alloc((size_t)12 * N) || d_g.alloc((size_t)6 * N) || d_X.alloc((size_t)6 * Nall) ||
        d_trials.alloc((size_t)12 * Nall * ladder) || d_part.alloc((size_t)na * ladder * maxblk) || d_pmax.alloc((size_t)nblk_p) ||
        d_out.alloc(h_out.size()) || d_xa.alloc(x->dev_doubles()) || d_xi.alloc(x->dev_ints()) || d_map.alloc((size_t)2 * halo) ||
        d_off.upload(offs, s) || d_eoff.upload(eoff, s) || d_edges.upload(edges, s))
      return REFINE_ACROSS.refuse("device allocation failed (" +
                                  std::to_string(8 * ((size_t)12 * Nall * (ladder + 1) + 12 * (size_t)N + 6 * (size_t)(N + Nall)) + 128 * edges.size()) +
                                  " bytes for " + std::to_string(ladder) + " trial trajectories of " + std::to_string(Nall) + " poses)");
    return DPGO_OK;
  }

  // the costs of `count` trajectories at Td (12 Nall doubles apart), robot by robot, with every robot's a^T b and the largest of
  // the gradient's partials behind them: into h_out once the stream has drained
  void costs(hipStream_t s, const double *Td, int count, const double *a, const double *b, bool with_max) {
    k_refine_cost_robots<<<dim3(maxblk, count, na), 256, 0, s>>>(Td, Nall, d_edges.p, d_eoff.p, d_part.p);
    k_refine_sums_robots<<<na, 256, 0, s>>>(d_part.p, count, maxblk, d_eoff.p, d_off.p, a, b, with_max ? d_pmax.p : nullptr, nblk_p, d_out.p);
    x->note(hipGetLastError(), __LINE__);
    x->note(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * ((size_t)na * (count + 1) + 1), hipMemcpyDeviceToHost, s), __LINE__);
  }

  // gradient, cost and |g|_inf of the trajectory in d_T: one exchange; h_out is valid when the stream has drained
  void evaluate(hipStream_t s) {
    Cert c;
    c.t = t;
    c.x = x;
    const double *hl = x->halo_of(c, 3, d_T.p, 3);
    if (x->bad || x->dead) return;
    if (halo > 0) x->note(hipMemcpyAsync(d_T.p + (size_t)12 * N, hl, sizeof(double) * 12 * (size_t)halo, hipMemcpyDeviceToDevice, s), __LINE__);
    launch_cert_apply3(s, t->d_agents.p, d_off.p, na, max_n, d_T.p, d_E.p, nullptr, hl, x->d_hoff);
    k_refine_grad<<<nblk_p, 256, 0, s>>>(d_T.p, d_E.p, N, fixed, d_g.p, d_pmax.p);
    costs(s, d_T.p, 1, nullptr, nullptr, true);
  }
};

// the hook of the step across teams: g into V, and behind X the halo rows of X out of x_S, the trial trajectories over this
// participant's poses and their halo, and the robots' sums
struct RefineAcrossStep : ApplyStep {
  RefineAcrossWs *ws = nullptr;
  Events ev{3};
  bool ran = false;
  RefineAcrossStep() : ApplyStep(1) {}
  int rhs(const double *, int N, double *V, hipStream_t s) override {
    if (N != ws->N) return REFINE_ACROSS.refuse("the covariance path's poses are not the call's");
    HIPC(hipMemcpyAsync(V, ws->d_g.p, sizeof(double) * 6 * (size_t)N, hipMemcpyDeviceToDevice, s));
    return DPGO_OK;
  }
  int taken(int N, hipStream_t s) override {
    RefineAcrossWs &w = *ws;
    if (N != w.N || view.N != w.N || view.halo_slots != w.halo || (int)view.halo_sep.size() != w.halo || !view.Td || !X)
      return REFINE_ACROSS.refuse("the covariance path's poses are not the call's");
    HIPC(hipEventRecord(ev[0], s));
    HIPC(hipMemcpyAsync(w.d_X.p, X, sizeof(double) * 6 * (size_t)N, hipMemcpyDeviceToDevice, s));
    if (w.halo > 0) {
      // the rows of X of the poses behind this participant's own: out of x_S, which is whole here; zero for the fixed pose
      HIPC(hipMemsetAsync(w.d_X.p + (size_t)6 * N, 0, sizeof(double) * 6 * (size_t)w.halo, s));
      std::vector<int> src, dst;
      for (int q = 0; q < w.halo; ++q) {
        const int sp = view.halo_sep[q];
        if (sp < 0) continue;
        if (6 * sp + 6 > view.nS || !view.xS) return REFINE_ACROSS.refuse("a halo pose lies outside the separator");
        src.push_back(sp);
        dst.push_back(N + q);
      }
      w.h_map = src;
      w.h_map.insert(w.h_map.end(), dst.begin(), dst.end());
      if (!src.empty()) {
        HIPC(hipMemcpyAsync(w.d_map.p, w.h_map.data(), sizeof(int) * w.h_map.size(), hipMemcpyHostToDevice, s));
        launch_apply_rows_sub(s, view.xS, (size_t)view.nS, w.d_map.p, nullptr, w.d_X.p, (size_t)6 * w.Nall, w.d_map.p + src.size(),
                              6 * (int)src.size(), 1);
      }
    }
    k_refine_trials<<<(unsigned)std::min<size_t>(((size_t)w.Nall * w.ladder + 255) / 256, 2048), 256, 0, s>>>(view.Td, w.d_X.p, w.Nall, w.fixed,
                                                                                                             w.ladder, w.d_trials.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    w.costs(s, w.d_trials.p, w.ladder, w.d_g.p, w.d_X.p, false);
    HIPC(hipEventRecord(ev[2], s));
    ran = true;
    return DPGO_OK;
  }
};

}  // namespace

}  // namespace dpgo_cert

extern "C" int dpgo_team_refine_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, const double *T,
                                       int max_iters, double grad_tol, double armijo, int ladder, double *T_out, double *history,
                                       dpgo_refine_t *out, dpgo_covariance_t *res) {
  const ClosureCall &A = REFINE_ACROSS;
  const auto t_begin = std::chrono::steady_clock::now();
  if (res) std::memset(res, 0, sizeof *res);
  if (out) std::memset(out, 0, sizeof *out);
  if (!t || !tr) return A.refuse("null argument");  // (nobody to tell)
  const std::vector<int> offs = pose_offsets(t);
  const int N = offs.back(), na = (int)t->ag.size();
  // ---- the refusals of the call itself, those of dpgo_team_refine that still apply: decided here, told to everyone by the
  // agreement record (a participant that returned now would leave the others waiting)
  auto refusal = [&]() -> int {
    if (!owner_rank_of_robot || !T || !T_out || !history || !out || !res) return A.refuse("null argument");
    if (max_iters < 0) return A.refuse("max_iters must not be negative, not " + std::to_string(max_iters));
    if (ladder < 1 || ladder > 32) return A.refuse("ladder must lie in [1, 32], not " + std::to_string(ladder));
    if (!(grad_tol > 0.0) || !std::isfinite(grad_tol)) return A.refuse("grad_tol must be positive and finite");
    if (!(armijo > 0.0) || !(armijo < 1.0)) return A.refuse("armijo must lie in (0, 1)");
    double orth = 0.0, det = 0.0;
    const int g = se3_defect(T, N, &orth, &det);
    if (g >= 0) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "pose %d of T (team order) is not in SE(3) (|R^T R - I| = %.3g, det R = %.12g)", g, orth, det);
      return A.refuse(buf);
    }
    return DPGO_OK;
  };
  std::string argerr;
  if (refusal()) argerr = A.refused();
  Across x;
  // (op 7: flags carries the ladder, the two real fields grad_tol and armijo)
  if (x.begin(t, tr, owner_rank_of_robot, A.name, 7, 3, ladder, grad_tol, armijo, max_iters, argerr.empty() ? nullptr : argerr.c_str())) {
    if (!argerr.empty()) set_err(std::string(A.name) + ": " + argerr);
    return DPGO_ERR;
  }
  const int nr = x.num_robots;
  x.note(hipSetDevice(t->device), __LINE__);
  hipStream_t s = t->stream;
  RefineAcrossWs ws;
  ws.t = t; ws.x = &x; ws.N = N; ws.na = na; ws.ladder = ladder; ws.offs = offs;
  ws.halo = x.halo_slots; ws.Nall = N + x.halo_slots;
  for (const auto &a : t->ag) ws.max_n = std::max(ws.max_n, a->n);
  if (t->id2local.count(0)) ws.fixed = offs[t->id2local.at(0)];
  RefineAcrossStep hook;
  hook.ws = &ws;
  if (ws.measurements() || ws.alloc(s) || hook.ev.create()) x.fail_local(g_err);
  // (the driver's halo tables in buffers of its own: every path inside carves its own out of the team's workspace)
  if (!x.bad) x.place(ws.d_xa.p, ws.d_xi.p, s);
  std::vector<double> Tk(T, T + (size_t)12 * N), hist((size_t)5 * (max_iters + 1), std::nan(""));
  if (!x.bad) x.note(hipMemcpyAsync(ws.d_T.p, Tk.data(), sizeof(double) * 12 * (size_t)N, hipMemcpyHostToDevice, s), __LINE__);
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  double ms_grad = 0.0, ms_path = 0.0, ms_trials = 0.0, ms_costs = 0.0, eps_mult = 0.0;
  size_t bytes_eval = 0, bytes_ladder = 0;
  dpgo_covariance_t last;
  std::memset(&last, 0, sizeof last);
  std::vector<double> rec, all;
  // the robots' totals of entry o of their records (m per robot), added in robot order from 0: Across::reduce_agents' rule
  auto total = [&](size_t m, size_t o) {
    const size_t n = 2 + m * (size_t)nr;
    double v = 0.0;
    for (int i = 0; i < nr; ++i) v += all[(size_t)x.robot_holder[i] * n + 2 + (size_t)i * m + o];
    return v;
  };
  const double ms_setup = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  double ms_accept = 0.0, ms_ladder = 0.0, ms_queue = 0.0;
  int k = 0, status = DPGO_REFINE_MAX_ITERS;
  for (;;) {
    // ---- gradient and cost of T_k: per robot (its cost, the measurements it owns), per participant |g|_inf
    const auto t0 = std::chrono::steady_clock::now();
    ws.evaluate(s);
    if (!x.bad && !x.dead) x.note(hipStreamSynchronize(s), __LINE__);
    rec.assign(2 + 2 * (size_t)nr, 0.0);
    if (!x.bad) {
      rec[1] = ws.h_out[(size_t)na * 2];
      for (int a = 0; a < na; ++a) {
        rec[2 + 2 * (size_t)t->ag[a]->id] = ws.h_out[(size_t)2 * a];
        rec[3 + 2 * (size_t)t->ag[a]->id] = (double)(ws.eoff[a + 1] - ws.eoff[a]);
      }
    }
    bytes_eval = sizeof(double) * rec.size();
    if (x.gather(rec, all)) return x.fail();
    ms_grad += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const double f = total(2, 0);
    double ginf = 0.0;
    for (int q = 0; q < x.world; ++q) {
      const double v = all[(size_t)q * rec.size() + 1];
      ginf = (v > ginf || v != v) ? v : ginf;  // (a NaN wins)
    }
    if (k == 0) {
      // eps_f: the chain of a measurement's term, the workgroup partials of the largest robot, the robots' totals
      int blk = 0;
      for (int i = 0; i < nr; ++i) blk = std::max(blk, ((int)all[(size_t)x.robot_holder[i] * rec.size() + 3 + 2 * (size_t)i] + 255) / 256);
      eps_mult = (double)(REFINE_EPS_CHAIN + blk + nr) * 0x1p-53;
    }
    hist[(size_t)5 * k] = f;
    hist[(size_t)5 * k + 1] = ginf;
    if (!std::isfinite(f) || !std::isfinite(ginf))  // (the same on every participant)
      return A.refuse("the cost or the gradient is not finite at iterate " + std::to_string(k));
    if (ginf <= grad_tol) { status = DPGO_REFINE_CONVERGED; break; }
    if (k == max_iters) { status = DPGO_REFINE_MAX_ITERS; break; }
    // ---- the step: X = Sigma g on the Schur path across, the trials behind it in the hook
    hook.X = nullptr;
    hook.ran = false;
    dpgo_covariance_t cur;
    const auto t1 = std::chrono::steady_clock::now();
    SchurAcrossArgs step(t, tr, owner_rank_of_robot, Tk.data());
    step.res = &cur;
    step.step = &hook;
    const int rc = covariance_schur_across(step);
    if (rc != DPGO_OK) {
      // a pivot that is not positive (the same words on every participant): at the input the call is refused in the path's
      // words, later it stops at the last good T
      if (!pivot_refused()) return rc;
      if (k == 0) { set_err("refine: " + g_err); return DPGO_ERR; }
      status = DPGO_REFINE_INDEFINITE;
      break;
    }
    if (!hook.ran) return A.refuse("the covariance path formed no X");  // (a problem of the anchor alone: everywhere)
    last = cur;
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    ms_trials += hook.ev.ms(0, 1);
    ms_costs += hook.ev.ms(1, 2);
    ms_path += whole - hook.ev.ms(0, 2);
    // ---- the ladder's record: per robot its costs of the trials and its share of g^T X
    const auto t2 = std::chrono::steady_clock::now();
    const size_t m = (size_t)ladder + 1;
    rec.assign(2 + m * (size_t)nr, 0.0);
    for (int a = 0; a < na; ++a) std::copy(ws.h_out.begin() + (size_t)a * m, ws.h_out.begin() + (size_t)(a + 1) * m, rec.begin() + 2 + (size_t)t->ag[a]->id * m);
    bytes_ladder = sizeof(double) * rec.size();
    if (x.gather(rec, all)) return x.fail();
    ms_ladder += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    const double dec = total(m, (size_t)ladder);
    hist[(size_t)5 * k + 3] = dec;
    hist[(size_t)5 * k + 4] = cur.min_pivot;
    // ---- acceptance, on every participant from the same bits
    int took = -1;
    for (int l = 0; l < ladder && took < 0; ++l)
      if (total(m, (size_t)l) <= f - armijo * std::ldexp(1.0, -l) * dec + eps_mult * std::fabs(f)) took = l;
    if (took < 0) { status = DPGO_REFINE_NO_DESCENT; break; }
    hist[(size_t)5 * k + 2] = std::ldexp(1.0, -took);
    const double *Tn = ws.d_trials.p + (size_t)took * 12 * ws.Nall;
    const auto t3 = std::chrono::steady_clock::now();
    x.note(hipMemcpyAsync(ws.d_T.p, Tn, sizeof(double) * 12 * (size_t)N, hipMemcpyDeviceToDevice, s), __LINE__);
    // (the path checks and uploads a host T: the accepted local trajectory comes back as well)
    x.note(hipMemcpyAsync(Tk.data(), Tn, sizeof(double) * 12 * (size_t)N, hipMemcpyDeviceToHost, s), __LINE__);
    ms_queue += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t3).count();
    x.note(hipStreamSynchronize(s), __LINE__);
    ms_accept += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    ++k;
  }
  if (x.finish()) return DPGO_ERR;
  if (timing)
    std::fprintf(stderr, "refine_across: rank %d of %d, %d poses and %d halo poses here, %d measurements owned here, %d iterations, status %d: "
                         "agreement, measurements and buffers %.3f ms, gradient and cost %.3f ms, covariance paths %.3f ms, k_refine_trials and the halo rows %.3f ms, k_refine_cost_robots and "
                         "sums %.3f ms, the ladder's allgather %.3f ms, with the accepted T %.3f ms (its copies queued in %.3f ms), %zu bytes per evaluation allgather, %zu per ladder allgather, %lld allgathers and %lld exchanges of the "
                         "driver, the whole call %.3f ms\n",
                 x.rank, x.world, N, ws.halo, (int)ws.edges.size(), k, status, ms_setup, ms_grad, ms_path, ms_trials, ms_costs, ms_ladder, ms_accept, ms_queue, bytes_eval, bytes_ladder,
                 x.n_allgather, x.n_exchange, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  std::memset(out, 0, sizeof *out);
  *res = last;
  out->status = status;
  out->iterations = k;
  out->f0 = hist[0]; out->grad_inf0 = hist[1];
  out->f = hist[(size_t)5 * k]; out->grad_inf = hist[(size_t)5 * k + 1];
  std::memcpy(history, hist.data(), sizeof(double) * hist.size());
  std::memcpy(T_out, Tk.data(), sizeof(double) * 12 * (size_t)N);
  return DPGO_OK;
}

// refine.hip -- a trajectory refined to a critical point of the SE(3) cost by Newton steps on Sigma: the
// kernels, the hook and the epilogue of a covariance path, and the driver behind dpgo_team_refine.
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
#include "refine_block.h"

namespace dpgo {

// the multiple of u f in eps_f: the additions an edge's term passes through inside refine_edge_cost and the butterfly (16 + 8),
// to which the driver adds the number of workgroup partials, summed one after another
constexpr int REFINE_EPS_CHAIN = 24;

// One lane per pose: the pose of T and of E in registers (16-byte loads), the six rows into g (column-major 6 N: rows 6 p ..
// 6 p + 5, 48 contiguous bytes per lane), pose 0's rows zero.  pmax[blockIdx.x] = the largest |g| of the workgroup's poses (a
// maximum has no order).  A NaN in g makes the partial NaN: the driver refuses it.
__global__ __launch_bounds__(256) void k_refine_grad(const double *__restrict__ T, const double *__restrict__ E, int N, double *__restrict__ g,
                                                     double *__restrict__ pmax) {
  __shared__ double wmax[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double m = 0.0;
  if (p < N) {
    double R[3][3], t[3], Ep[12], gr[6];
    gate_load_pose(T, p, R, t);
    gate_load_pairs<6>(E + (size_t)12 * p, Ep);
    refine_grad_rows(p, R, Ep, gr);
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
__global__ __launch_bounds__(256) void k_refine_trials(const double *__restrict__ T, const double *__restrict__ X, int N, int ladder,
                                                       double *__restrict__ trials) {
  const size_t total = (size_t)N * ladder;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int l = (int)(e / N), p = (int)(e % N);
    double R[3][3], t[3], x[6], P[12];
    gate_load_pose(T, p, R, t);
    gate_load_pairs<3>(X + (size_t)6 * p, x);
    refine_trial_pose(p, R, t, x, ldexp(1.0, -l), P);
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
    k_refine_grad<<<nblk_p, 256, 0, s>>>(Td, d_E.p, N, out, d_pmax.p);
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
    k_refine_trials<<<(unsigned)std::min<size_t>(((size_t)ws->N * ws->ladder + 255) / 256, 2048), 256, 0, s>>>(st.Td, app->X, ws->N, ws->ladder,
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

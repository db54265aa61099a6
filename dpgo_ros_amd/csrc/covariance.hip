// covariance.hip -- marginal pose covariances of a trajectory T in SE(3)^N.
//
// Pose i is perturbed by xi_i = (phi_i, delta_i): R_i <- R_i Exp(phi_i), t_i <- t_i + delta_i.  With S = Q - Lambda(T), the
// certificate's operator at rank 3 (certify.hip), and J the map xi -> Tdot (rotation columns of pose i: R_i [phi_i]x,
// translation column: delta_i) the Hessian of the cost 1/2 <T, T Q> in these coordinates is
//     H = J^T (S (x) I_3) J,      H_ij = sum_{cp, c} S_ij[cp, c] (A_i^cp)^T A_j^c,
// A_i^cp = the 3 x 6 matrix that takes xi_i to column cp of Tdot_i: [-R_i [e_cp]x, 0] for cp < 3, [0, I] for cp = 3.
// Column a of -R_i [e_cp]x is R_i (e_a x e_cp) = eps(a, cp, k) R_i[:, k], so with M = R_i^T R_j
//     rotation-rotation     [a][b] = sum_{cp != a, c != b} S[cp][c] eps(a, cp, k) eps(b, c, l) M[k][l]
//     rotation-translation  [a][b] = sum_{cp != a} S[cp][3] eps(a, cp, k) R_i[b][k]
//     translation-rotation  [a][b] = sum_{c != b} S[3][c] eps(b, c, l) R_j[a][l]
//     translation-translation      = S[3][3] I.
// Pose 0 is held fixed: H_red = H without its first 6 rows and columns, n = 6 (N - 1), dense column-major.  Sigma = H_red^-1
// through dense_spd_inverse (dense_inverse.hip: blocked Cholesky, triangular inverse, W^T W on the fp64 matrix cores).
//
// Layouts: T is a K = 3 block of the certificate's iterate layout, T[(4 g + c) * 3 + b], g in team order.  A stored 4 x 4
// block of the team-wide Q -- entry p of row j of an agent's block-CSR (column i), or a shared-edge record of pose j whose
// neighbour is pose i -- holds Q_ij[cp][c] at [cp + 4 c] (the record: its negative).
// Nothing here writes a solver vector: the buffers come from the device pool and go back to it.
//
// This file also holds what the three methods share on the host (covariance_frame.h): the frame of a call (CovFrame), the
// refusals decided before any device work, and the public entry points of the dense and the Schur method
// (covariance_schur.hip, covariance_nested.hip have the other two device parts).
#include "covariance_apply.h"
#include "covariance_block.h"
#include "covariance_frame.h"

namespace dpgo {

// One work item per thread.  Both blocks of a symmetric pair are formed by the same arithmetic: the thread always forms
// H_lo,hi (lo = min(bi, bj)) from S_lo,hi and the two rotations and stores it or its transpose, so H is bitwise symmetric
// wherever the stored blocks of Q are; a diagonal block is formed in its upper triangle and mirrored.  Items are sorted by
// (block column, block row): the 64 items of a wave store into a few neighbouring columns of H, each thread six runs of
// 48 contiguous bytes.  Every block has one writer: no atomics, the buffer was cleared on the same stream.
__global__ __launch_bounds__(256) void k_cov_assemble(const AgentDev *__restrict__ agents, const CovItem *__restrict__ items,
                                                      const CovSrc *__restrict__ src, int nitems, const double *__restrict__ T,
                                                      const double *__restrict__ lam, double *__restrict__ H, int n) {
  const int it = blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  const v4i_t wi = *(const __attribute__((address_space(1))) v4i_t *)(items + it);
  const CovItem w{wi.x, wi.y, wi.z, wi.w};
  double Hc[6][6];  // H_lo,hi
  cov_form_block(agents, src, w, T, lam, Hc, w.bi > w.bj);
  // H_bi,bj[a][b] at H[(6 (bj - 1) + b) n + 6 (bi - 1) + a]: 48 contiguous, 16-byte aligned bytes per column
  cov_store_block(H + (size_t)6 * (w.bj - 1) * n + (size_t)6 * (w.bi - 1), (size_t)n, Hc, w.bi > w.bj);
}

// out[0] = 2 sum_k log L_kk, out[1] / out[2] = the smallest / largest L_kk^2, L the Cholesky factor left in A (n x n
// column-major).  ONE workgroup: thread t sums its contiguous run of the diagonal in index order, thread 0 the 256 runs
// in thread order -- a fixed order, the same bits in every call.
__global__ __launch_bounds__(256) void k_cov_logdet(const double *__restrict__ A, int n, double *__restrict__ out) {
  __shared__ double sum[256], lo[256], hi[256];
  const int t = threadIdx.x, per = (n + 255) / 256;
  double s = 0.0, mn = INFINITY, mx = 0.0;
  for (int k = t * per; k < min(n, (t + 1) * per); ++k) {
    const double l = gp(A)[(size_t)k * n + k];
    s += log(l);
    mn = fmin(mn, l * l);
    mx = fmax(mx, l * l);
  }
  sum[t] = s; lo[t] = mn; hi[t] = mx;
  __syncthreads();
  if (t == 0) {
    double a = 0.0, b = INFINITY, c = 0.0;
    for (int k = 0; k < 256; ++k) { a += sum[k]; b = fmin(b, lo[k]); c = fmax(c, hi[k]); }
    out[0] = 2.0 * a; out[1] = b; out[2] = c;
  }
}

// The blocks of Sigma = M (n x n column-major) the caller asked for, 36 doubles each, row-major; one thread per element.
// Blocks [0, N): the diagonal block of pose g, symmetrised as (B + B^T) / 2 (both operands of an element and of its mirror
// are the same two numbers: bitwise symmetric).  Blocks [N, N + num_pairs): Sigma_ab of pair (a, b).  A block that names
// pose 0 is zero.
__global__ __launch_bounds__(256) void k_cov_extract(const double *__restrict__ M, int n, int N, const int *__restrict__ pairs,
                                                     int num_pairs, double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)36 * (N + num_pairs)) return;
  const int blk = (int)(e / 36), q = (int)(e - (size_t)36 * blk), a = q / 6, b = q - 6 * a;
  double v = 0.0;
  if (blk < N) {
    if (blk > 0) {
      const size_t o = (size_t)6 * (blk - 1);
      v = 0.5 * (gp(M)[(o + b) * n + o + a] + gp(M)[(o + a) * n + o + b]);
    }
  } else {
    const int pa = gp(pairs)[2 * (blk - N)], pb = gp(pairs)[2 * (blk - N) + 1];
    if (pa > 0 && pb > 0) v = gp(M)[((size_t)6 * (pb - 1) + b) * n + (size_t)6 * (pa - 1) + a];
  }
  gp(out)[e] = v;
}

}  // namespace dpgo

namespace dpgo_cert {

int launch_cov_logdet(hipStream_t s, const double *A, int n, double *out) {
  k_cov_logdet<<<1, 256, 0, s>>>(A, n, out);
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// ---- what the methods share on the host (covariance_frame.h)

void cov_fill_result(dpgo_covariance_t *res, long long n, const double *stat, const std::vector<char> &counted, const double ms[5]) {
  double logdet = 0.0, mn = INFINITY, mx = 0.0;
  for (size_t k = 0; k < counted.size(); ++k) {
    if (!counted[k]) continue;
    logdet += stat[4 * k];
    mn = std::fmin(mn, stat[4 * k + 1]);
    mx = std::fmax(mx, stat[4 * k + 2]);
  }
  res->n = (int)n;
  res->logdet = logdet;
  res->min_pivot = mn;
  res->max_pivot = mx;
  res->seconds_assemble = 1e-3 * ms[0];
  res->seconds_invert = 1e-3 * (ms[1] + ms[2] + ms[3]);
}

CovFrame::CovFrame(dpgo_team_t *team) : t(team), s(team->stream), na((int)team->ag.size()), offs(team->ag.size() + 1, 0) {
  for (int k = 0; k < na; ++k) {
    offs[k + 1] = offs[k] + t->ag[k]->n;
    max_n = std::max(max_n, t->ag[k]->n);
  }
  N = offs[na];
}

int CovFrame::begin(const double *T, int nfactors_, int num_pairs_, bool with_keep_) {
  nfactors = nfactors_; num_pairs = num_pairs_; with_keep = with_keep_;
  nout = (size_t)36 * (N + num_pairs);
  const size_t L3 = (size_t)12 * N, gmax_n = (size_t)na * ((max_n + 255) / 256);
  if (d_small.alloc(2 * L3 + (size_t)9 * N + gmax_n + 4 * (size_t)nfactors + (with_keep ? 2 : 1) * nout) || d_off.alloc((size_t)na + 1)) return 1;
  double *E = d_small.p + L3, *gmax = E + L3 + (size_t)9 * N;
  Td = d_small.p; lam = E + L3; stat = gmax + gmax_n; keepd = stat + 4 * (size_t)nfactors; outd = keepd + (with_keep ? nout : 0);
  HIPC(hipMemcpyAsync(d_off.p, offs.data(), sizeof(int) * (na + 1), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(Td, T, sizeof(double) * L3, hipMemcpyHostToDevice, s));
  if (with_keep) HIPC(hipMemsetAsync(keepd, 0, sizeof(double) * 2 * nout, s));
  MARK(-1);
  launch_cert_apply3(s, t->d_agents.p, d_off.p, na, max_n, Td, E, nullptr);
  launch_cert_lambda3(s, t->d_agents.p, d_off.p, na, max_n, Td, E, lam, gmax);
  return DPGO_OK;
}

int CovFrame::finish(CovEpilogue *epi, dpgo_covariance_t *res, double *cov_diag, double *cov_pairs, const std::vector<char> &counted) {
  // with an epilogue the blocks stay on the device: the statistics alone come back, the epilogue queues its own copies
  std::vector<double> host(4 * (size_t)nfactors + (epi ? 0 : (size_t)(outd - keepd) + nout));
  HIPC(hipMemcpyAsync(host.data(), stat, sizeof(double) * host.size(), hipMemcpyDeviceToHost, s));
  if (epi && epi->run({Td, outd, outd + (size_t)36 * N, N, num_pairs, s})) {
    (void)hipStreamSynchronize(s);  // (copies into this frame and into the epilogue may be queued)
    return DPGO_ERR;
  }
  HIPC(hipStreamSynchronize(s));
  marks.sum(ms);
  cov_fill_result(res, 6 * ((long long)N - 1), host.data(), counted, ms);
  if (epi) return DPGO_OK;
  const double *o = host.data() + (outd - stat);
  std::memcpy(cov_diag, o, sizeof(double) * 36 * (size_t)N);
  if (num_pairs > 0) std::memcpy(cov_pairs, o + (size_t)36 * N, sizeof(double) * 36 * (size_t)num_pairs);
  return DPGO_OK;
}

bool cov_device_avail(dpgo_team_t *t, double *avail) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  *avail = (double)free_b + (double)pool_held(t->device);
  return true;
}

int se3_defect(const double *T, int N, double *orth_out, double *det_out) {
  for (int g = 0; g < N; ++g) {
    const double *R = T + (size_t)12 * g;
    double orth = 0.0;
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) {
        const double d = R[3 * p] * R[3 * q] + R[3 * p + 1] * R[3 * q + 1] + R[3 * p + 2] * R[3 * q + 2] - (p == q ? 1.0 : 0.0);
        orth = std::max(orth, std::fabs(d));
      }
    const double det = R[0] * (R[4] * R[8] - R[7] * R[5]) - R[3] * (R[1] * R[8] - R[7] * R[2]) + R[6] * (R[1] * R[5] - R[4] * R[2]);
    bool finite = true;
    for (int k = 0; k < 12; ++k) finite = finite && std::isfinite(R[k]);
    if (!finite || !(orth <= 1e-8) || !(std::fabs(det - 1.0) <= 1e-8)) {
      *orth_out = orth; *det_out = det;
      return g;
    }
  }
  return -1;
}

std::string pivot_message(const std::string &what, long long row, const std::string &where, long long pose) {
  return what + ": non-positive pivot at row " + std::to_string(row) + " of " + where + " (pose " + std::to_string(pose) +
         "): the Hessian is not positive definite at this T: not a minimum";
}

// The device part of dpgo_team_marginal_covariances by the dense inverse (marginal_covariances_call below has made every
// refusal): descriptors synchronised, T on the device, Lambda, H_red, its inverse, the requested blocks.  The outputs are
// written only when the factorisation succeeded.  Returns DPGO_OK, DPGO_ERR (message set), or k + 1 > 0: the pivot of row k of
// H_red was not positive.
int covariance_device(dpgo_team_t *t, const double *T, int num_pairs, const int *pairs, double *cov_diag, double *cov_pairs,
                      dpgo_covariance_t *res, CovEpilogue *epi, CovApply *app) {
  if (check_team(t, "marginal_covariances")) return DPGO_ERR;
  CovFrame F(t);
  const int N = F.N, n = 6 * (N - 1);
  // the work list: every stored block of the team-wide Q outside pose 0's row and column, by (block column, block row);
  // blocks of the same position (parallel shared edges) become one item
  struct Raw { int bi, bj, agent, idx; };
  std::vector<Raw> raw;
  if (cov_for_each_stored_block(t, F.offs, [&](int bi, int bj, int agent, int idx) {
        if (bi != 0 && bj != 0) raw.push_back({bi, bj, agent, idx});
        return 0;
      })) {
    set_err("marginal_covariances: a stored block lies outside the team");
    return DPGO_ERR;
  }
  std::stable_sort(raw.begin(), raw.end(), [](const Raw &x, const Raw &y) { return x.bj != y.bj ? x.bj < y.bj : x.bi < y.bi; });
  std::vector<CovItem> items;
  std::vector<CovSrc> srcs;
  for (const Raw &q : raw) {
    if (!items.empty() && items.back().bi == q.bi && items.back().bj == q.bj) ++items.back().count;
    else items.push_back({q.bi, q.bj, (int)srcs.size(), 1});
    srcs.push_back({q.agent, q.idx});
  }
  const size_t nn = (size_t)n * n;
  DevBuf<double> d_A, d_W, d_M, d_V, d_X;
  DevBuf<int> d_pairs;
  DevBuf<CovItem> d_items;
  DevBuf<CovSrc> d_src;
  DevBuf<ApplyItem> d_app;
  hipStream_t s = t->stream;
  // Sigma applied to vectors (covariance_apply.h): V and X of 6 N x num_cols beside the three matrices
  const size_t vx = app ? (size_t)6 * N * app->num_cols : 0;
  auto nomem = [&]() {
    set_err("marginal_covariances: device allocation failed (" + std::to_string((3 * nn + 2 * vx) * 8) + " bytes for three matrices of order " +
            std::to_string(n) + (app ? ", V and X" : "") + ")");
    return DPGO_ERR;
  };
  if (d_A.alloc(nn) || d_W.alloc(nn) || d_M.alloc(nn) || d_pairs.alloc(2 * (size_t)num_pairs) || d_items.upload(items, s) || d_src.upload(srcs, s))
    return nomem();
  if (app && (d_V.alloc(vx) || d_X.alloc(vx) || d_app.alloc(1))) return nomem();
  // (queued before the frame's first mark: outside the time of the assembly)
  if (num_pairs > 0) HIPC(hipMemcpyAsync(d_pairs.p, pairs, sizeof(int) * 2 * (size_t)num_pairs, hipMemcpyHostToDevice, s));
  if (const int rc = F.begin(T, 1, num_pairs, false)) return rc > 0 ? nomem() : DPGO_ERR;
  SchurMarks &marks = F.marks;
  if (app) {
    HIPC(hipMemsetAsync(d_X.p, 0, sizeof(double) * vx, s));
    if (app->rhs(F.Td, N, d_V.p, s)) return DPGO_ERR;
    MARK(-1);
  }
  HIPC(hipMemsetAsync(d_A.p, 0, sizeof(double) * nn, s));
  if (!items.empty())
    k_cov_assemble<<<(unsigned)((items.size() + 255) / 256), 256, 0, s>>>(t->d_agents.p, d_items.p, d_src.p, (int)items.size(), F.Td,
                                                                           F.lam, d_A.p, n);
  HIPC(hipGetLastError());
  MARK(0);
  const int fail = dense_spd_inverse(s, d_A.p, d_W.p, d_M.p, n);  // (synchronises the stream)
  HIPC(hipGetLastError());
  if (fail < 0) { set_err("marginal_covariances: scratch allocation of the inverse failed"); return DPGO_ERR; }
  if (fail > 0) return fail;
  // the inverse: its launches lie between the mark before it and the synchronisation inside dense_spd_inverse; this mark is
  // recorded on a drained stream, so the interval is the inverse (and the copy of its failure word) alone
  MARK(1);
  k_cov_logdet<<<1, 256, 0, s>>>(d_A.p, n, F.stat);
  k_cov_extract<<<(unsigned)((F.nout + 255) / 256), 256, 0, s>>>(d_M.p, n, N, d_pairs.p, num_pairs, F.outd);
  HIPC(hipGetLastError());
  MARK(4);
  size_t app_mark = 0;
  if (app) {
    // X_red = G V_red: one product with the explicit inverse, past pose 0's rows of V and of X
    const ApplyItem it{d_M.p, d_V.p + 6, d_X.p + 6, nullptr, nullptr, n, 6 * N, 6 * N, n, app->num_cols, n};
    HIPC(hipMemcpyAsync(d_app.p, &it, sizeof it, hipMemcpyHostToDevice, s));
    launch_apply_gemm(s, false, d_app.p, &it, 1, false);
    HIPC(hipGetLastError());
    MARK(-1);
    app_mark = marks.ev.size() - 1;
    app->flops = apply_flops(&it, 1);
    app->X = d_X.p;
  }
  if (F.finish(epi, res, cov_diag, cov_pairs, {1})) return DPGO_ERR;
  if (app) {
    float v = 0.f;
    if (hipEventElapsedTime(&v, marks.ev[app_mark - 1], marks.ev[app_mark]) == hipSuccess) app->ms_products = v;
  }
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "marginal_covariances: n %d, %zu blocks, assemble %.3f ms, invert %.3f ms, extract %.3f ms\n", n, items.size(),
                 F.ms[0], F.ms[1], F.ms[4]);
  return DPGO_OK;
}

// ---- the entry points.  Every refusal that can be decided on the host comes first.  The three methods share them: DPGO_OK to
// go on (the device is selected), 1 when the team holds the anchor alone and the outputs are already written, DPGO_ERR with a
// message that `what` prefixes.  flags_error: what is wrong with the caller's flags (or null)
int covariance_host_checks(dpgo_team_t *t, const double *T, const char *flags_error, int num_pairs, const int *pairs, double *cov_diag,
                           double *cov_pairs, dpgo_covariance_t *res, const char *what, int *num_poses, bool staged) {
  if (res) std::memset(res, 0, sizeof *res);
  // staged: the blocks stay on the device for an epilogue (certify_internal.h) and the two outputs are not used
  if (!t || !T || (!staged && !cov_diag) || !res || num_pairs < 0 || (num_pairs > 0 && (!pairs || (!staged && !cov_pairs)))) {
    set_err(std::string(what) + ": null argument");
    return DPGO_ERR;
  }
  if (flags_error) { set_err(std::string(what) + ": " + flags_error); return DPGO_ERR; }
  if (check_team_local(t, what)) return DPGO_ERR;
  const int na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  for (int k = 0; k < na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  const int N = offs[na];
  double orth = 0.0, det = 0.0;
  const int g = se3_defect(T, N, &orth, &det);
  if (g >= 0) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "%s: pose %d of T is not in SE(3) (|R^T R - I| = %.3g, det R = %.12g)", what, g, orth, det);
    set_err(buf);
    return DPGO_ERR;
  }
  for (int k = 0; k < 2 * num_pairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= N) {
      set_err(std::string(what) + ": pair " + std::to_string(k / 2) + " names pose " + std::to_string(pairs[k]) +
              ", outside [0, " + std::to_string(N) + ")");
      return DPGO_ERR;
    }
  {
    std::vector<dpgo_measurement_t> mm;
    if (team_measurements(t, offs, what, mm)) return DPGO_ERR;
    if (check_joined_to_pose0(mm.data(), (int)mm.size(), N, what)) return DPGO_ERR;
  }
  *num_poses = N;
  if (N < 2) {  // the anchor alone: nothing is free
    if (!staged) {
      std::memset(cov_diag, 0, sizeof(double) * 36 * (size_t)N);
      if (num_pairs > 0) std::memset(cov_pairs, 0, sizeof(double) * 36 * (size_t)num_pairs);
    }
    return 1;
  }
  HIPC(hipSetDevice(t->device));
  return DPGO_OK;
}

int marginal_covariances_call(dpgo_team_t *t, const double *T, int flags, int num_pairs, const int *pairs, double *cov_diag,
                              double *cov_pairs, dpgo_covariance_t *res, CovEpilogue *epi, CovApply *app) {
  const char *what = "marginal_covariances";
  int N = 0;
  const int pre = covariance_host_checks(t, T, flags != 0 && flags != DPGO_COV_SCHUR ? "flags must be 0 or DPGO_COV_SCHUR" : nullptr, num_pairs,
                                         pairs, cov_diag, cov_pairs, res, what, &N, epi != nullptr);
  if (pre != DPGO_OK) return pre > 0 ? DPGO_OK : pre;
  if (flags == DPGO_COV_SCHUR) {
    // by robot-wise Schur complement (covariance_schur.hip): its own memory accounting, from the partition
    int fail[3] = {0, 0, 0};
    const int rc = covariance_schur_device(t, T, num_pairs, pairs, cov_diag, cov_pairs, res, fail, epi);
    if (rc != DPGO_OK) std::memset(res, 0, sizeof *res);
    if (rc > 0) {
      set_err(pivot_message(what, fail[2], fail[0] < 0 ? "the Schur complement on the public poses"
                                                        : "the interior Hessian of robot " + std::to_string(t->ag[fail[0]]->id), fail[1]));
      return DPGO_ERR;
    }
    return rc;
  }
  {
    // three dense matrices of order 6 (N - 1)
    const double n = 6.0 * (N - 1), vx = app ? 2.0 * 8.0 * 6.0 * N * (double)app->num_cols : 0.0, need = 3.0 * n * n * 8.0 + vx;
    double avail = 0.0;
    if (!cov_device_avail(t, &avail)) { set_err(std::string(what) + ": hipMemGetInfo failed"); return DPGO_ERR; }
    if (need > avail && app) {
      char buf[400];
      std::snprintf(buf, sizeof buf,
                    "%s: the dense Hessian of order %.0f, its inverse and V and X of %d columns need %.0f bytes (3 x 8 n^2 + 2 x 8 x 6 N x "
                    "num_cols), %.0f are available on the device",
                    what, n, app->num_cols, need, avail);
      set_err(buf);
      return DPGO_ERR;
    }
    if (need > avail) {
      char buf[400];
      std::snprintf(buf, sizeof buf,
                    "%s: the dense Hessian of order %.0f and its inverse need %.0f bytes, %.0f are available on the device.  "
                    "flags = DPGO_COV_SCHUR (method=\"schur\") eliminates one robot's interior at a time and needs far less",
                    what, n, need, avail);
      set_err(buf);
      return DPGO_ERR;
    }
  }
  const int rc = covariance_device(t, T, num_pairs, pairs, cov_diag, cov_pairs, res, epi, app);
  if (rc != DPGO_OK) std::memset(res, 0, sizeof *res);
  if (rc > 0) {
    set_err(pivot_message(what, rc - 1, "the reduced Hessian", (rc - 1) / 6 + 1));
    return DPGO_ERR;
  }
  return rc;
}

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_marginal_covariances(dpgo_team_t *t, const double *T, int flags, int num_pairs, const int *pairs,
                                              double *cov_diag, double *cov_pairs, dpgo_covariance_t *res) {
  return marginal_covariances_call(t, T, flags, num_pairs, pairs, cov_diag, cov_pairs, res, nullptr);
}

// the same call over a split team (covariance_schur.hip): the Schur path is its only method
extern "C" int dpgo_team_marginal_covariances_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot,
                                                     const double *T, int flags, int num_pairs, const int *pairs, double *cov_diag,
                                                     double *cov_pairs, dpgo_covariance_t *res) {
  SchurAcrossArgs a(t, tr, owner_rank_of_robot, T);
  a.flags = flags;
  a.num_pairs = num_pairs; a.pairs = pairs; a.cov_diag = cov_diag; a.cov_pairs = cov_pairs; a.res = res;
  return covariance_schur_across(a);
}

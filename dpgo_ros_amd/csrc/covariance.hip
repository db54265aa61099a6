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
#include "certify_internal.h"
#include "covariance_block.h"

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

// The device part of dpgo_team_marginal_covariances (capi.hip has made every host-side refusal): descriptors synchronised,
// T on the device, Lambda, H_red, its inverse, the requested blocks.  The outputs are written only when the factorisation
// succeeded.  Returns DPGO_OK, DPGO_ERR (message set), or k + 1 > 0: the pivot of row k of H_red was not positive.
int covariance_device(dpgo_team_t *t, const double *T, int num_pairs, const int *pairs, double *cov_diag, double *cov_pairs,
                      dpgo_covariance_t *res, CovEpilogue *epi) {
  if (check_team(t, "marginal_covariances")) return DPGO_ERR;
  const int na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  int max_n = 0;
  for (int k = 0; k < na; ++k) {
    offs[k + 1] = offs[k] + t->ag[k]->n;
    max_n = std::max(max_n, t->ag[k]->n);
  }
  const int N = offs[na], n = 6 * (N - 1);
  // the work list: every stored block of the team-wide Q outside pose 0's row and column, by (block column, block row);
  // blocks of the same position (parallel shared edges) become one item
  struct Raw { int bi, bj, agent, idx; };
  std::vector<Raw> raw;
  for (int k = 0; k < na; ++k) {
    const Agent &a = *t->ag[k];
    for (int j = 0; j < a.n; ++j)
      for (int p = a.rowptr[j]; p < a.rowptr[j + 1]; ++p) raw.push_back({offs[k] + a.col[p], offs[k] + j, k, p});
    for (size_t e = 0; e < a.se_host.size(); ++e) {
      const SharedEdgeDev &se = a.se_host[e];
      raw.push_back({offs[se.src_agent_local] + se.src_frame, offs[k] + se.lpose, k, ~(int)e});
    }
  }
  std::stable_sort(raw.begin(), raw.end(), [](const Raw &x, const Raw &y) { return x.bj != y.bj ? x.bj < y.bj : x.bi < y.bi; });
  std::vector<CovItem> items;
  std::vector<CovSrc> srcs;
  for (const Raw &q : raw) {
    if (q.bi == 0 || q.bj == 0) continue;
    if (q.bi < 0 || q.bi >= N || q.bj >= N) { set_err("marginal_covariances: a stored block lies outside the team"); return DPGO_ERR; }
    if (!items.empty() && items.back().bi == q.bi && items.back().bj == q.bj) ++items.back().count;
    else items.push_back({q.bi, q.bj, (int)srcs.size(), 1});
    srcs.push_back({q.agent, q.idx});
  }
  const size_t nn = (size_t)n * n, L3 = (size_t)12 * N, nout = (size_t)36 * (N + num_pairs);
  DevBuf<double> d_A, d_W, d_M, d_small;
  DevBuf<int> d_int;
  DevBuf<CovItem> d_items;
  DevBuf<CovSrc> d_src;
  const int gstride = (max_n + 255) / 256;
  // d_small: T, E = T Q, Lambda, the Gershgorin scratch of k_cert_lambda, [logdet, min, max], the output blocks
  const size_t small = 2 * L3 + (size_t)9 * N + (size_t)na * gstride + 4 + nout;
  if (d_A.alloc(nn) || d_W.alloc(nn) || d_M.alloc(nn) || d_small.alloc(small) || d_int.alloc(na + 1 + 2 * (size_t)num_pairs) ||
      d_items.upload(items, t->stream) || d_src.upload(srcs, t->stream)) {
    set_err("marginal_covariances: device allocation failed (" + std::to_string(3 * nn * 8) + " bytes for three matrices of order " +
            std::to_string(n) + ")");
    return DPGO_ERR;
  }
  double *Td = d_small.p, *E = Td + L3, *lam = E + L3, *gmax = lam + (size_t)9 * N, *stat = gmax + (size_t)na * gstride,
         *outd = stat + 4;
  int *off = d_int.p, *pairs_d = off + na + 1;
  hipStream_t s = t->stream;
  hipEvent_t ev[4];
  for (auto &e : ev) HIPC(hipEventCreate(&e));
  struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 4; ++k) (void)hipEventDestroy(e[k]); } } guard{ev};
  HIPC(hipMemcpyAsync(off, offs.data(), sizeof(int) * (na + 1), hipMemcpyHostToDevice, s));
  if (num_pairs > 0) HIPC(hipMemcpyAsync(pairs_d, pairs, sizeof(int) * 2 * (size_t)num_pairs, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(Td, T, sizeof(double) * L3, hipMemcpyHostToDevice, s));
  HIPC(hipEventRecord(ev[0], s));
  launch_cert_apply3(s, t->d_agents.p, off, na, max_n, Td, E, nullptr);
  launch_cert_lambda3(s, t->d_agents.p, off, na, max_n, Td, E, lam, gmax);
  HIPC(hipMemsetAsync(d_A.p, 0, sizeof(double) * nn, s));
  if (!items.empty())
    k_cov_assemble<<<(unsigned)((items.size() + 255) / 256), 256, 0, s>>>(t->d_agents.p, d_items.p, d_src.p, (int)items.size(), Td,
                                                                           lam, d_A.p, n);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[1], s));
  const int fail = dense_spd_inverse(s, d_A.p, d_W.p, d_M.p, n);  // (synchronises the stream)
  HIPC(hipGetLastError());
  if (fail < 0) { set_err("marginal_covariances: scratch allocation of the inverse failed"); return DPGO_ERR; }
  if (fail > 0) return fail;
  HIPC(hipEventRecord(ev[2], s));
  k_cov_logdet<<<1, 256, 0, s>>>(d_A.p, n, stat);
  k_cov_extract<<<(unsigned)((nout + 255) / 256), 256, 0, s>>>(d_M.p, n, N, pairs_d, num_pairs, outd);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev[3], s));
  // with an epilogue the blocks stay on the device: the statistics alone come back, the epilogue queues its own copies
  std::vector<double> host(4 + (epi ? 0 : nout));
  HIPC(hipMemcpyAsync(host.data(), stat, sizeof(double) * host.size(), hipMemcpyDeviceToHost, s));
  if (epi && epi->run({Td, outd, outd + (size_t)36 * N, N, num_pairs, s})) {
    (void)hipStreamSynchronize(s);  // (copies into this frame and into the epilogue may be queued)
    return DPGO_ERR;
  }
  HIPC(hipStreamSynchronize(s));
  float ms_a = 0.f, ms_x = 0.f;
  HIPC(hipEventElapsedTime(&ms_a, ev[0], ev[1]));
  HIPC(hipEventElapsedTime(&ms_x, ev[2], ev[3]));
  // the inverse: its launches lie between ev[1] and the synchronisation inside dense_spd_inverse; ev[2] was recorded on a
  // drained stream, so ev[1] .. ev[2] is the inverse (and the copy of its failure word) alone
  float ms_i = 0.f;
  HIPC(hipEventElapsedTime(&ms_i, ev[1], ev[2]));
  res->n = n;
  res->logdet = host[0];
  res->min_pivot = host[1];
  res->max_pivot = host[2];
  res->seconds_assemble = 1e-3 * ms_a;
  res->seconds_invert = 1e-3 * ms_i;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "marginal_covariances: n %d, %zu blocks, assemble %.3f ms, invert %.3f ms, extract %.3f ms\n", n, items.size(),
                 ms_a, ms_i, ms_x);
  if (epi) return DPGO_OK;
  std::memcpy(cov_diag, host.data() + 4, sizeof(double) * 36 * (size_t)N);
  if (num_pairs > 0) std::memcpy(cov_pairs, host.data() + 4 + (size_t)36 * N, sizeof(double) * 36 * (size_t)num_pairs);
  return DPGO_OK;
}

}  // namespace dpgo_cert

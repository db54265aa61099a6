// covariance_schur.hip -- the marginal pose covariances of covariance.hip by robot-wise Schur complement.
//
// A pose that no shared-edge record names (an INTERIOR pose) couples only to poses of its own robot.  Ordered as
// [interior of robot 0 | ... | interior of robot A-1 | all PUBLIC poses (the separator S, team order)], H_red is block
// arrowhead:
//     H_II,a   the interior block of robot a (order 6 |I_a|),   B_a = H_IS,a  (6 |I_a| x 6 s_a: an interior pose touches only
//     the s_a public poses of its own robot),   H_SS (order 6 |S|).
// Per robot, one after another:  C_a = H_II,a^-1 (dense_spd_inverse),  W_a = C_a B_a,  H_SS[s_a, s_a] -= B_a^T W_a.  The
// contribution lands inside the robot's own diagonal block of the separator: nothing is summed across robots.  Then
// Sigma_SS = S_c^-1 and
//     Sigma_ii = C_a[ii] + (Z_a W_a^T)[ii],  Z_a = W_a Sigma_SS[s_a, s_a]                 (i interior of a)
//     Sigma_ij = C_a[ij] + Z_a[i,:] W_a[j,:]^T                                           (i, j interior of a)
//     Sigma_ij = W_a[i,:] Sigma_SS[s_a, s_b] W_b[j,:]^T                                  (interior of a, interior of b != a)
//     Sigma_is = -W_a[i,:] Sigma_SS[s_a, s]                                              (interior, public)
//     Sigma_st = the block of Sigma_SS                                                   (public, public)
//     log det H_red = sum_a log det H_II,a + log det S_c      (summed on the host in robot order, the separator last).
// Kept per robot: W_a, the diagonal blocks of C_a and its blocks of requested pairs, log det and pivots; C_a is dropped.
// The blocks are read out by the extraction kernels of covariance_extract.h, the ones the nested path launches: a robot is a
// set of their table whose separator indices are a window of one array 0, 1, 2, ... (iota), because a robot's part of the
// separator is one contiguous range.  The head and the tail of the call are CovFrame's (covariance_frame.h).
//
// THE ROW-OWNER RULE.  A symmetric target (H_II,a, H_SS) is filled from the stored blocks S_ij with i <= j (team order)
// alone: the thread forms H_ij and writes it and its transpose.  A stored block S_ij lives with the robot that holds pose
// j -- entry (row j, column i) of its block-CSR, or a shared-edge record of its pose j.  So the lower-triangle block (row
// pose j, column pose i, j > i) of H_SS between two robots is formed from the record of the robot that holds ROW j, and a
// participant that holds only some robots can form the block rows of its own robots from what it stores.
//
// The products run on the fp64 matrix cores (k_dgemm below), one workgroup per 64 x 64 tile of the result with the K
// loop in one fixed order: no split-K, no atomics, the same bits in every call.
#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>

#include "covariance_apply.h"
#include "covariance_extract.h"

namespace dpgo {

// k_cov_assemble's work item, written where the host's list says instead of at the global position.  The same per-block
// arithmetic (cov_form_block), the same merged parallel edges, one writer per block.  bi, bj: rows of T (and of lam)
__global__ __launch_bounds__(256) void k_cov_assemble_map(const AgentDev *__restrict__ agents, const CovItem *__restrict__ items,
                                                          const CovSrc *__restrict__ src, const CovDst *__restrict__ dst, int nitems,
                                                          const double *__restrict__ T, const double *__restrict__ lam,
                                                          double *__restrict__ H, int ld) {
  const int it = blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  const v4i_t wi = *(const __attribute__((address_space(1))) v4i_t *)(items + it);
  const v4i_t di = *(const __attribute__((address_space(1))) v4i_t *)(dst + it);
  const CovItem w{wi.x, wi.y, wi.z, wi.w};
  double Hc[6][6];  // H_lo,hi
  cov_form_block(agents, src, w, T, lam, Hc, (di.z & CD_FLIP) != 0);
  const size_t r = (size_t)6 * di.x, c = (size_t)6 * di.y;
  const bool tr = (di.z & CD_TRANS) != 0;
  cov_store_block(H + c * ld + r, (size_t)ld, Hc, tr);
  if ((di.z & CD_MIRROR) && di.x != di.y) cov_store_block(H + r * ld + c, (size_t)ld, Hc, !tr);
}

// C = op(A) B (sub: C -= op(A) B): one workgroup per 64 x 64 tile (dgemm_tile, covariance_schur.h)
template <bool TA>
__global__ __launch_bounds__(256) void k_dgemm(const double *__restrict__ A, int lda, const double *__restrict__ B, int ldb,
                                               double *__restrict__ C, int ldc, int m, int n, int k, int sub) {
  dgemm_tile<TA>(A, lda, B, ldb, C, ldc, m, n, k, sub, 64 * blockIdx.x, 64 * blockIdx.y);
}

// the upper triangle of the n x n column-major A from its lower one (the Schur complement B^T W is symmetric to round-off
// only; the factorisation is handed a bitwise symmetric matrix)
__global__ __launch_bounds__(256) void k_schur_mirror(double *__restrict__ A, int n) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * n) return;
  const int i = (int)(e % n), j = (int)(e / n);
  if (i > j) gp(A)[(size_t)i * n + j] = gp(A)[e];
}

}  // namespace dpgo

namespace dpgo_cert {

// C = op(A) B or C -= op(A) B on stream s (k_dgemm); nothing to do when a dimension is 0
static void launch_dgemm(hipStream_t s, bool ta, const double *A, int lda, const double *B, int ldb, double *C, int ldc, int m, int n,
                         int k, bool sub) {
  if (m <= 0 || n <= 0 || k <= 0) return;
  const dim3 grid((m + 63) / 64, (n + 63) / 64, 1);
  if (ta) hipLaunchKernelGGL(k_dgemm<true>, grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, m, n, k, sub ? 1 : 0);
  else hipLaunchKernelGGL(k_dgemm<false>, grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, m, n, k, sub ? 1 : 0);
}

void launch_cov_assemble_map(hipStream_t s, const AgentDev *agents, const CovItem *items, const CovSrc *src, const CovDst *dst, int count,
                             const double *T, const double *lam, double *H, int ld) {
  if (count > 0) k_cov_assemble_map<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(agents, items, src, dst, count, T, lam, H, ld);
}

void launch_schur_mirror(hipStream_t s, double *A, int n) {
  if (n > 0) k_schur_mirror<<<(unsigned)(((size_t)n * n + 255) / 256), 256, 0, s>>>(A, n);
}

void schur_partition(dpgo_team_t *t, int zero, SchurPartition &P) {
  P.na = (int)t->ag.size();
  P.offs.assign(P.na + 1, 0);
  for (int k = 0; k < P.na; ++k) P.offs[k + 1] = P.offs[k] + t->ag[k]->n;
  P.N = P.offs[P.na];
  P.robot_of.assign(P.N, 0);
  P.pub.assign(P.N, 0);
  P.pos.assign(P.N, 0);
  for (int k = 0; k < P.na; ++k) {
    for (int j = 0; j < t->ag[k]->n; ++j) P.robot_of[P.offs[k] + j] = k;
    // an edge of weight 0 counts: the pattern does not depend on the weights
    for (const SharedEdgeDev &se : t->ag[k]->se_host)
      if (se.lpose >= 0 && se.lpose < t->ag[k]->n) P.pub[P.offs[k] + se.lpose] = 1;
  }
  P.interior.assign(P.na, {});
  P.sep_off.assign(P.na + 1, 0);
  for (int k = 0; k < P.na; ++k) {
    for (int g = P.offs[k]; g < P.offs[k + 1]; ++g) {
      if (g == zero) continue;
      if (P.pub[g]) { P.pos[g] = (int)P.sep.size(); P.sep.push_back(g); }
      else { P.pos[g] = (int)P.interior[k].size(); P.interior[k].push_back(g); }
    }
    P.sep_off[k + 1] = (int)P.sep.size();
    P.max_int = std::max(P.max_int, (int)P.interior[k].size());
  }
  P.nS = (int)P.sep.size();
}

// the device bytes of the call.  The large buffers: three square ones of order M = max(6 max_a |I_a|, 6 |S|),
// the separator, every kept W_a, one more of the largest W_a (B_a, later Z_a).  The small ones: T, T Q, Lambda, the
// Gershgorin scratch, the factors' statistics, the kept and the output blocks (2 x 36 (N + P) doubles, P pairs), the scratch
// of the pairs between two robots' interiors (every pair counted as one), the block and pair lists (a CovBlk per pose and two
// per pair, a CovCross per pair), the work list (40 bytes per stored block of Q), the maps and iota, the table of sets (a
// CovBlock per robot and two per pair: a split team's rows), and the Linv blocks of dense_spd_inverse.  nS: the separator of the WHOLE problem (a split
// team inverts it too); `who` names what sets M
static double schur_bytes(dpgo_team_t *t, const SchurPartition &P, int nS, int kmax, int num_pairs, std::string &who) {
  int big = -1, max_n = 0;
  size_t stored = 0;
  for (int k = 0; k < P.na; ++k) {
    if (big < 0 || P.interior[k].size() > P.interior[big].size()) big = k;
    max_n = std::max(max_n, t->ag[k]->n);
    stored += t->ag[k]->col.size() + t->ag[k]->se_host.size();
  }
  const double mi = 6.0 * P.max_int, ms = 6.0 * nS, M = std::max(mi, ms);
  double w_all = 0.0, w_max = 0.0;
  for (int k = 0; k < P.na; ++k) {
    const double w = 36.0 * (double)P.interior[k].size() * (double)(P.sep_off[k + 1] - P.sep_off[k]);
    w_all += w;
    w_max = std::max(w_max, w);
  }
  who = ms >= mi ? "the separator of " + std::to_string(nS) + " public poses"
                 : "the " + std::to_string(P.max_int) + " interior poses of robot " + std::to_string(t->ag[big]->id);
  const double N = P.N, np = num_pairs, A = P.na;
  const double small = 8.0 * (33.0 * N + A * ((max_n + 255) / 256) + 4.0 * (A + 1.0) + 72.0 * (N + np)) +
                       8.0 * 6.0 * std::max(kmax, 1) * (double)cov_cross_chunk((size_t)num_pairs, kmax) + (double)sizeof(CovBlk) * (N + 2.0 * np) +
                       (double)sizeof(CovCross) * np + 40.0 * (double)stored + 4.0 * (A + 1.0 + 2.0 * N + nS) +
                       (double)sizeof(CovBlock) * (A + 2.0 * np) + 8.0 * 1024.0 * std::ceil(M / 32.0);
  return 8.0 * (3.0 * M * M + ms * ms + w_all + w_max) + small;
}

// the bytes Sigma applied to `cols` vectors adds on a participant ("across teams"): V and X (8 x 6 N_loc cols
// each), r_S and x_S (8 x 6 |S| cols each, the separator of the whole problem), the temporary W_a^T v_a (8 x cols x max_a K_a
// over the robots here), 64 bytes per product record (three per robot and one) and 4 per public pose here (the row maps)
static double schur_apply_bytes(const SchurPartition &P, int nS, int cols) {
  int kloc = 0;
  for (int k = 0; k < P.na; ++k) kloc = std::max(kloc, 6 * (P.sep_off[k + 1] - P.sep_off[k]));
  return 8.0 * (double)cols * (12.0 * P.N + 12.0 * nS + kloc) + (double)sizeof(ApplyItem) * (3.0 * P.na + 1.0) + 4.0 * P.nS;
}

// cols > 0: with Sigma applied to that many vectors
static int schur_fits(dpgo_team_t *t, const SchurPartition &P, int nS, int kmax, int num_pairs, const char *what, std::string &msg,
                      int cols = 0) {
  std::string who;
  const double need = schur_bytes(t, P, nS, kmax, num_pairs, who);
  double avail = 0.0;
  if (!cov_device_avail(t, &avail)) { msg = std::string(what) + ": hipMemGetInfo failed"; return -1; }
  char buf[400];
  if (cols > 0) {
    const double extra = schur_apply_bytes(P, nS, cols);
    if (need + extra <= avail) return 0;
    std::snprintf(buf, sizeof buf,
                  "%s: the Schur path needs %.0f bytes, set by %s, and V, X, r_S, x_S and the temporary of %d columns %.0f more (8 x "
                  "num_cols x (12 N + 12 |S| + max K), N = %d, |S| = %d), %.0f are available on the device",
                  what, need, who.c_str(), cols, extra, P.N, nS, avail);
    msg = buf;
    return -1;
  }
  if (need <= avail) return 0;
  std::snprintf(buf, sizeof buf,
                "%s: the Schur path needs %.0f bytes, set by %s, %.0f are available on the device; a team of more robots has "
                "smaller interiors and needs less",
                what, need, who.c_str(), avail);
  msg = buf;
  return -1;
}

// the device side of one call: what a single team and a participant of a split team share
struct SchurDev {
  hipStream_t s = nullptr;
  const AgentDev *agents = nullptr;
  const double *Td = nullptr, *lam = nullptr;  // T rows (a participant: its halo behind its own poses), Lambda of the own poses
  DevBuf<double> A, Wk, M, B;
  DevBuf<CovItem> items;
  DevBuf<CovSrc> src;
  DevBuf<CovDst> dst;
  DevBuf<CovBlk> blk;    // the list of the launch at hand
  DevBuf<CovBlock> tab;  // the robots as sets of the extraction kernels (a split team: behind them the gathered rows)
  const SchurItems *L = nullptr;
  void assemble(int list, double *H, int ld) const {
    const int cnt = L->count(list);
    if (cnt > 0)
      k_cov_assemble_map<<<(unsigned)((cnt + 255) / 256), 256, 0, s>>>(agents, items.p + L->lbeg[list], src.p, dst.p + L->lbeg[list], cnt, Td,
                                                                        lam, H, ld);
  }
};

// Sigma applied to vectors beside one robot's step ("across teams"): the records of u_a = C_a v_a (into X) and
// t_a = W_a^T v_a (into tmp, K x cols) on the device and on the host, and where r_a = v_{S_a} - t_a goes: the robot's rows of
// r_S (leading dimension ldr), read out of V through `pub`, the team poses of its public poses
struct SchurApply {
  const ApplyItem *u_d, *t_d, *u_h, *t_h;
  const double *V;
  size_t ldv, ldr;
  const int *pub;
  double *tmp, *r;
  int cols;
  double *flops;              // the step's count of the apply's own products
  std::vector<size_t> *ends;  // the marks that END an interval of the apply's own launches
};

// One robot: H_II and B assembled (lists `lii`, `lb`), C = H_II^-1 into D.M, W = C B, Sd -= B^T W (Sd: the
// robot's diagonal block of the separator, leading dimension lds), the statistics of the factor into stat[0 .. 2], the blocks
// of C named by `keep` (its entries name the robot's set of D.tab) into keepd.  DPGO_OK, DPGO_ERR (message set), or row + 1 of a non-positive pivot.  A single team and
// every participant of a split team come through here with the same shapes: the same bits.  ap: behind W = C B, while C is live
// in D.M, also u_a, t_a and r_a of SchurApply; without one the launches are the ones above and no other.
static int schur_robot_step(SchurDev &D, SchurMarks &marks, int robot_id, int lii, int lb, int ni, int K, double *W, double *Sd, int lds,
                            const std::vector<CovBlk> &keep, double *keepd, double *stat, const SchurApply *ap = nullptr) {
  hipStream_t s = D.s;
  HIPC(hipMemsetAsync(D.A.p, 0, sizeof(double) * (size_t)ni * ni, s));
  D.assemble(lii, D.A.p, ni);
  if (K > 0) {
    HIPC(hipMemsetAsync(D.B.p, 0, sizeof(double) * (size_t)ni * K, s));
    D.assemble(lb, D.B.p, ni);
  }
  HIPC(hipGetLastError());
  MARK(0);
  const int f = dense_spd_inverse(s, D.A.p, D.Wk.p, D.M.p, ni);  // (synchronises the stream)
  HIPC(hipGetLastError());
  if (f < 0) { set_err("marginal_covariances: scratch allocation of the inverse failed"); return DPGO_ERR; }
  if (f > 0) return f;
  if (launch_cov_logdet(s, D.A.p, ni, stat)) return DPGO_ERR;
  MARK(1);
  launch_dgemm(s, false, D.M.p, ni, D.B.p, ni, W, ni, ni, K, ni, false);  // W_a = C_a B_a
  launch_dgemm(s, true, D.B.p, ni, W, ni, Sd, lds, K, K, ni, true);       // S[s_a, s_a] -= B_a^T W_a
  HIPC(hipGetLastError());
  MARK(2);
  marks.note.back() = "robot " + std::to_string(robot_id) + ": W = C B (" + std::to_string(ni) + " x " + std::to_string(K) + " x " +
                      std::to_string(ni) + ") and B^T W (" + std::to_string(K) + " x " + std::to_string(K) + " x " + std::to_string(ni) + ")";
  marks.flops.back() = 2.0 * ni * (double)ni * K + 2.0 * K * (double)K * ni;
  if (ap) {
    launch_apply_gemm(s, false, ap->u_d, ap->u_h, 1, false);  // u_a = C_a v_a, into X
    launch_apply_gemm(s, true, ap->t_d, ap->t_h, 1, false);   // t_a = W_a^T v_a
    launch_apply_rows_sub(s, ap->V, ap->ldv, ap->pub, ap->tmp, ap->r, ap->ldr, nullptr, K, ap->cols);  // r_a = v_{S_a} - t_a
    HIPC(hipGetLastError());
    MARK(-1);
    ap->ends->push_back(marks.ev.size() - 1);
    *ap->flops += apply_flops(ap->u_h, 1) + apply_flops(ap->t_h, 1);
  }
  // (keep is never empty: the diagonal blocks)
  HIPC(hipMemcpyAsync(D.blk.p, keep.data(), sizeof(CovBlk) * keep.size(), hipMemcpyHostToDevice, s));
  launch_ext_keep(s, D.tab.p, D.blk.p, (int)keep.size(), keepd);
  HIPC(hipGetLastError());
  MARK(4);
  return DPGO_OK;
}

// The same robot (set `set` of D.tab) once Sigma_SS (order nS) is known: Z = W Sigma_SS[s, s] into D.B, in place on the
// robot's diagonal block Sss of Sigma_SS; the diagonal blocks of its interior poses and its pairs of two interior poses
static int schur_robot_blocks(SchurDev &D, SchurMarks &marks, int robot_id, int set, int ni, int K, const double *W, const double *Sss, int nS,
                              const std::vector<CovBlk> &same, const double *keepd, double *outd) {
  hipStream_t s = D.s;
  launch_dgemm(s, false, W, ni, Sss, nS, D.B.p, ni, ni, K, K, false);
  HIPC(hipGetLastError());
  MARK(2);
  marks.note.back() = "robot " + std::to_string(robot_id) + ": Z = W Sigma_SS[s, s] (" + std::to_string(ni) + " x " + std::to_string(K) + " x " +
                      std::to_string(K) + ")";
  marks.flops.back() = 2.0 * ni * (double)K * K;
  launch_ext_diag(s, D.tab.p, set, 1, ni, keepd, outd);
  if (!same.empty()) {
    HIPC(hipMemcpyAsync(D.blk.p, same.data(), sizeof(CovBlk) * same.size(), hipMemcpyHostToDevice, s));
    launch_ext_pair_same(s, D.tab.p, D.blk.p, (int)same.size(), keepd, outd);
  }
  HIPC(hipGetLastError());  // (D.blk and D.B serve the next robot: its copy and its product are ordered behind these on the stream)
  MARK(4);
  return DPGO_OK;
}

// pairs of interior poses of two robots: list entries name sets of the table, in chunks
static int schur_cross_pairs(hipStream_t s, const CovBlock *tab_d, const double *Sss, int nS, const std::vector<CovCross> &list, CovCross *list_d,
                             int kmax, double *tbuf, size_t chunk, double *outd) {
  if (list.empty()) return DPGO_OK;
  HIPC(hipMemcpyAsync(list_d, list.data(), sizeof(CovCross) * list.size(), hipMemcpyHostToDevice, s));
  launch_ext_cross_pairs<RowRun>(s, tab_d, Sss, nS, list_d, list.size(), kmax, tbuf, chunk, outd);
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// blocks of Sigma_SS (M, order nS) and pairs of an interior with a public pose, behind the separator's inverse
static int schur_listed(SchurDev &D, int nS, const std::vector<CovBlk> &list, CovBlk *list_d, bool pub, double *outd) {
  if (list.empty()) return DPGO_OK;
  HIPC(hipMemcpyAsync(list_d, list.data(), sizeof(CovBlk) * list.size(), hipMemcpyHostToDevice, D.s));
  if (pub) launch_ext_public(D.s, D.M.p, nS, list_d, (int)list.size(), outd);
  else launch_ext_pair_is<RowRun>(D.s, D.tab.p, D.M.p, nS, list_d, (int)list.size(), outd);
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// the products' lines of the DPGO_TIMING report (on a drained stream)
static void schur_report(const SchurMarks &marks) {
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  for (size_t k = 1; timing && k < marks.ev.size(); ++k) {
    float v = 0.f;
    if (marks.flops[k] > 0.0 && hipEventElapsedTime(&v, marks.ev[k - 1], marks.ev[k]) == hipSuccess)
      std::fprintf(stderr, "marginal_covariances (Schur): products, %s: %.3f ms, %.2f TFLOP/s\n", marks.note[k].c_str(), v,
                   marks.flops[k] / (1e9 * v));
  }
}

// The device part of dpgo_team_marginal_covariances with DPGO_COV_SCHUR (capi.hip has made the refusals that need no
// partition).  DPGO_OK, DPGO_ERR (message set), or 1: a pivot was not positive -- fail[0] the robot's local index (-1: the
// separator), fail[1] the team pose, fail[2] the row of that factor.  The outputs are written only when every factorisation
// succeeded.
int covariance_schur_device(dpgo_team_t *t, const double *T, int num_pairs, const int *pairs, double *cov_diag, double *cov_pairs,
                            dpgo_covariance_t *res, int *fail, CovEpilogue *epi) {
  const char *what = "marginal_covariances";
  if (check_team(t, what)) return DPGO_ERR;
  SchurPartition P;
  schur_partition(t, 0, P);
  const int na = P.na, N = P.N, nS = 6 * P.nS;
  int kmax = 0;
  for (int k = 0; k < na; ++k) kmax = std::max(kmax, 6 * (P.sep_off[k + 1] - P.sep_off[k]));
  {
    std::string msg;
    if (schur_fits(t, P, P.nS, kmax, num_pairs, what, msg)) { set_err(msg); return DPGO_ERR; }
  }
  // ---- the work lists.  Every stored block of the team-wide Q outside pose 0's row and column is one of: interior x
  // interior of one robot, interior x public of one robot (B_a, or its mirror, dropped), public x public.  Symmetric
  // targets keep bi <= bj (the row-owner rule above).  Lists: [0, na) H_II,a, [na, 2 na) B_a, 2 na: H_SS.
  SchurItems L;
  auto classify = [&](int bi, int bj, int agent, int idx) -> int {
    if (bi == 0 || bj == 0) return 0;
    const bool pi = P.pub[bi], pj = P.pub[bj];
    if (pi && pj) { if (bi <= bj) L.add(2 * na, bi, bj, agent, idx, P.pos[bi], P.pos[bj], CD_MIRROR); }
    else if (!pi && !pj) {
      if (P.robot_of[bi] != P.robot_of[bj]) return -1;
      if (bi <= bj) L.add(P.robot_of[bi], bi, bj, agent, idx, P.pos[bi], P.pos[bj], CD_MIRROR);
    } else if (!pi && pj) {
      if (P.robot_of[bi] != P.robot_of[bj]) return -1;
      L.add(na + P.robot_of[bi], bi, bj, agent, idx, P.pos[bi], P.pos[bj] - P.sep_off[P.robot_of[bi]], bi > bj ? (CD_FLIP | CD_TRANS) : 0);
    }
    return 0;
  };
  if (cov_for_each_stored_block(t, P.offs, classify)) { set_err(std::string(what) + ": a stored block lies outside the team"); return DPGO_ERR; }
  L.finish(2 * na + 1);
  // ---- the outputs asked for, by case: a robot's interior is a set, the public poses the separator
  CovOutputs O;
  cov_classify_outputs(N, na, pairs, num_pairs, [&](int g) { return P.pub[g] ? -1 : P.robot_of[g]; }, P.pos, O);
  // ---- device storage
  const int M = std::max(6 * P.max_int, nS);
  const size_t MM = (size_t)M * M;
  size_t w_max = 0;
  for (int k = 0; k < na; ++k) w_max = std::max(w_max, (size_t)36 * P.interior[k].size() * (size_t)(P.sep_off[k + 1] - P.sep_off[k]));
  // scratch of the pairs between interiors of two robots: at most 64 MB at a time
  const size_t cross_chunk = cov_cross_chunk(O.cross.size(), kmax);
  CovFrame F(t);
  SchurDev D;
  DevBuf<double> d_S, d_t;
  std::vector<DevBuf<double>> d_W(na);
  DevBuf<int> d_int;
  DevBuf<CovBlk> d_is;
  DevBuf<CovCross> d_cross;
  hipStream_t s = t->stream;
  size_t nblk = O.pub.size();
  for (int k = 0; k < na; ++k) nblk = std::max(nblk, O.keep[k].size() + O.same[k].size());
  // d_int: the team pose of every interior index (robot after robot), then iota = 0, 1, ..., |S| - 1
  std::vector<int> ints, ipose_off(na + 1, 0);
  for (int k = 0; k < na; ++k) {
    ints.insert(ints.end(), P.interior[k].begin(), P.interior[k].end());
    ipose_off[k + 1] = (int)ints.size();
  }
  for (int q = 0; q < P.nS; ++q) ints.push_back(q);
  bool bad = D.A.alloc(MM) || D.Wk.alloc(MM) || D.M.alloc(MM) || d_S.alloc((size_t)nS * nS) || D.B.alloc(w_max) || d_int.upload(ints, s) ||
             D.items.upload(L.items, s) || D.src.upload(L.srcs, s) || D.dst.upload(L.dsts, s) || D.blk.alloc(nblk) || d_is.alloc(O.is.size()) ||
             d_cross.alloc(O.cross.size()) || D.tab.alloc(na) || d_t.alloc(cross_chunk * 6 * std::max(kmax, 1));
  for (int k = 0; k < na && !bad; ++k) bad = d_W[k].alloc((size_t)36 * P.interior[k].size() * (size_t)(P.sep_off[k + 1] - P.sep_off[k])) != 0;
  auto nomem = [&]() {
    std::string who;
    set_err(std::string(what) + ": device allocation failed (the Schur path needs " +
            std::to_string((long long)schur_bytes(t, P, P.nS, kmax, num_pairs, who)) + " bytes)");
    return DPGO_ERR;
  };
  if (bad) return nomem();
  // the robots as sets: M = C_a during the robot's step, Z = Z_a during its extraction, nb a window of iota
  std::vector<CovBlock> rob(na);
  const int *iota_d = d_int.p + ipose_off[na];
  for (int k = 0; k < na; ++k)
    rob[k] = {d_W[k].p, iota_d + P.sep_off[k], d_int.p + ipose_off[k], D.M.p, nullptr, D.B.p, 6 * (int)P.interior[k].size(),
              6 * (P.sep_off[k + 1] - P.sep_off[k])};
  HIPC(hipMemcpyAsync(D.tab.p, rob.data(), sizeof(CovBlock) * na, hipMemcpyHostToDevice, s));
  if (const int rc = F.begin(T, na + 1, num_pairs, true)) return rc > 0 ? nomem() : DPGO_ERR;
  D.s = s; D.agents = t->d_agents.p; D.Td = F.Td; D.lam = F.lam; D.L = &L;
  SchurMarks &marks = F.marks;
  if (nS > 0) {
    HIPC(hipMemsetAsync(d_S.p, 0, sizeof(double) * (size_t)nS * nS, s));
    D.assemble(2 * na, d_S.p, nS);
  }
  HIPC(hipGetLastError());
  MARK(0);
  // ---- the robots, one after another: the three square buffers and B serve each in turn
  std::vector<char> counted(na + 1, 0);
  for (int k = 0; k < na; ++k) {
    const int ni = rob[k].ld;
    if (ni == 0) continue;
    const size_t soff = (size_t)6 * P.sep_off[k];
    const int f = schur_robot_step(D, marks, t->ag[k]->id, k, na + k, ni, rob[k].K, d_W[k].p, d_S.p + soff * nS + soff, nS, O.keep[k], F.keepd,
                                   F.stat + 4 * k);
    if (f < 0) return DPGO_ERR;
    if (f > 0) { fail[0] = k; fail[1] = P.interior[k][(f - 1) / 6]; fail[2] = f - 1; return 1; }
    counted[k] = 1;
  }
  // ---- the separator
  if (nS > 0) {
    launch_schur_mirror(s, d_S.p, nS);
    HIPC(hipGetLastError());
    const int f = dense_spd_inverse(s, d_S.p, D.Wk.p, D.M.p, nS);
    HIPC(hipGetLastError());
    if (f < 0) { set_err(std::string(what) + ": scratch allocation of the inverse failed"); return DPGO_ERR; }
    if (f > 0) { fail[0] = -1; fail[1] = P.sep[(f - 1) / 6]; fail[2] = f - 1; return 1; }
    if (launch_cov_logdet(s, d_S.p, nS, F.stat + 4 * na)) return DPGO_ERR;
    counted[na] = 1;
    MARK(3);
    if (schur_listed(D, nS, O.pub, D.blk.p, true, F.outd)) return DPGO_ERR;
    MARK(4);
  }
  // ---- the interior blocks
  for (int k = 0; k < na; ++k) {
    if (rob[k].ld == 0) continue;
    const size_t soff = (size_t)6 * P.sep_off[k];
    if (schur_robot_blocks(D, marks, t->ag[k]->id, k, rob[k].ld, rob[k].K, d_W[k].p, D.M.p + soff * nS + soff, nS, O.same[k], F.keepd, F.outd))
      return DPGO_ERR;
  }
  if (schur_listed(D, nS, O.is, d_is.p, false, F.outd)) return DPGO_ERR;
  if (schur_cross_pairs(s, D.tab.p, D.M.p, nS, O.cross, d_cross.p, kmax, d_t.p, cross_chunk, F.outd)) return DPGO_ERR;
  MARK(4);
  if (F.finish(epi, res, cov_diag, cov_pairs, counted)) return DPGO_ERR;
  schur_report(marks);
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr,
                 "marginal_covariances (Schur): n %d, separator %d, largest interior %d, %zu blocks, assemble %.3f ms, factorisations %.3f ms, "
                 "products %.3f ms, separator inverse %.3f ms, extract %.3f ms\n",
                 6 * (N - 1), nS, 6 * P.max_int, L.items.size(), F.ms[0], F.ms[1], F.ms[2], F.ms[3], F.ms[4]);
  return DPGO_OK;
}

// ---- the same call over a split team ("across teams"; the conventions of certify_across.hip)
//
// A participant holds some robots.  Poses are numbered globally, robots by id, then poses; pose 0 is robot 0's first pose.
// Transport calls, the same on every participant: the two allgathers and the exchange of Across::begin and Cert::setup,
// the exchange of the T halo, then
//   A  sizes: per robot its public poses, its interior poses and the cross blocks it holds (the payload lengths follow);
//   B  per robot: a failure record, the frames of its public poses, its diagonal block of the Schur complement
//      H_SS[s_a, s_a] - B_a^T W_a, the statistics of its factor, and the blocks of H_SS below the diagonal in the rows it holds
//      (the row-owner rule), padded to the longest;
//   C  the pair blocks a participant owns (two interior poses of one of its robots; an interior pose of one of its robots
//      with a public pose) and, for every pair of interior poses of two robots, the two rows W_a[i,:], W_b[j,:] from their
//      holders;
// with an AcrossStep that has endpoints (the gate and the audit across teams) also
//   D  per endpoint of the step's records, sorted by global pose: T and the diagonal block from the pose's holder, zeros
//      from everyone else -- every participant then runs the step's kernel on compact tables of endpoints and pairs;
// and the closing status word.  Every participant builds the same S_c from B, inverts it itself (deterministic: no
// broadcast) and forms the pairs of two robots itself from the rows of C.  No sum crosses a robot boundary except the
// host's log det in robot order, so every block, log det and pivot is bitwise the single team's.
// The layout of every record is SchurAcrossPlan's (schur_across_plan.h, host only); what a public call adds is its AcrossStep
// (certify_internal.h).  SchurAcross below is one call: run() is the list above.
namespace {

enum { XF_OK = 0, XF_PIVOT = 1, XF_MEMORY = 2, XF_LOCAL = 3 };

struct SchurAcross {
  const SchurAcrossArgs &a;
  AcrossStep &st;
  const bool plain;  // no step of the caller's: the blocks go to cov_diag and cov_pairs
  dpgo_team_t *const t;
  const char *const what;
  const int *pairs;
  int num_pairs;
  const int cols;    // the columns Sigma is applied to (0: none)
  int rc = DPGO_ERR;  // what the call returns when a step ends it
  Across x;
  Cert c;
  hipStream_t s = nullptr;
  SchurPartition P;
  SchurAcrossPlan pl;
  SchurItems L;
  SchurMarks marks;
  int nr = 0, na = 0, N = 0, nS = 0;
  size_t nout = 0;  // the doubles of the N diagonal and the num_pairs pair blocks
  std::vector<double> gall;
  // a block of H_SS between two robots in a row this participant holds.  row: local robot and index among its public poses;
  // column: robot id, frame
  struct CrossBlk { int lrobot, lrow, crobot, cframe; };
  std::vector<CrossBlk> xb;
  std::vector<int> ncross, byid;  // cross blocks per local robot; the local robots in id order
  // this participant's failure, told in allgather B
  int fcode = XF_OK, frobot = 0, fpose = 0, frow = 0, sfail = 0;
  std::string fmsg;
  // device storage (as the single team's, the separator that of the whole problem)
  SchurDev D;
  DevBuf<double> d_S, d_small, d_t, d_T, d_D, d_X, d_rows, d_tab;
  std::vector<DevBuf<double>> d_W;
  DevBuf<int> d_int;
  DevBuf<CovBlk> d_is;
  DevBuf<CovCross> d_cross;
  size_t cross_chunk = 0;
  std::vector<size_t> doff;          // a robot's diagonal block of the separator in d_D
  std::vector<int> ipose_off, soff;  // a robot's interior poses in d_int; its first row of the global separator
  const int *iota_d = nullptr;
  double *stat = nullptr, *keepd = nullptr, *outd = nullptr;
  std::vector<CovBlock> rob;
  std::vector<double> hD, hX, hstat, hS, hout, hrows, sstat = std::vector<double>(4, 0.0);
  // Sigma applied to vectors ("across teams").  d_aV, d_aX: 6 N x cols; d_rS, d_xS: r_S and x_S of the whole
  // problem, 6 |S| x cols; d_tmp: W_a^T v_a of the robot at hand; d_pub: the team poses of this participant's public poses
  // (P.sep), a robot's row map a window of it.  Records: [0, na) u_a = C_a v_a, [na, 2 na) t_a = W_a^T v_a, [2 na, 3 na)
  // x_a -= W_a x_S[S_a], 3 na: x_S = Sigma_SS r_S
  DevBuf<double> d_aV, d_aX, d_rS, d_xS, d_tmp;
  DevBuf<int> d_pub;
  DevBuf<ApplyItem> d_app;
  std::vector<ApplyItem> aitem;
  std::vector<size_t> app_marks, roff;  // roff: a robot's r_a (K_a x cols) in h_ra, id order
  std::vector<double> h_ra;             // the r_a of the robots here, back from the device

  SchurAcross(const SchurAcrossArgs &args, AcrossStep &step, bool plain_)
      : a(args), st(step), plain(plain_), t(args.t), what(step.name), pairs(args.pairs), num_pairs(args.num_pairs), cols(step.num_cols()) {}

  // a step that returns true has ended the call with rc; a participant that failed locally (x.bad) launches nothing more but
  // makes every transport call of the sequence
  int run() {
    if (agree()) return rc;
    if (lambda_of_T()) return rc;
    work_lists();
    if (gather_sizes()) return rc;
    if (!x.bad && fcode == XF_OK && (storage() || phase1())) { fcode = XF_LOCAL; fmsg = g_err; }
    if (gather_b()) return rc;
    pl.classify(P, pairs, num_pairs, cols);
    if (!x.bad && phase2()) x.fail_local(g_err);
    if (gather_c()) return rc;
    if (!x.bad && phase3()) x.fail_local(g_err);
    if (cols > 0 && !x.bad && apply()) x.fail_local(g_err);
    if (st.exchange(x, s)) return x.fail();
    if (st.endpoints() && gather_d()) return rc;
    return close();
  }

  // ---- the agreement record, the step's resolve(), the partition; a problem of the fixed pose alone ends here
  bool agree() {
    std::string argerr = st.argerr;
    if (!argerr.empty()) {}
    else if (!a.T || !a.res || (plain && !a.cov_diag) || num_pairs < 0 || (num_pairs > 0 && (!pairs || !a.cov_pairs))) argerr = "null argument";
    else if (a.flags != DPGO_COV_SCHUR) argerr = "flags must be DPGO_COV_SCHUR";
    else if (t) {
      int n = 0;
      for (auto &ag : t->ag) n += ag->n;
      double orth = 0.0, det = 0.0;
      const int g = se3_defect(a.T, n, &orth, &det);
      if (g >= 0) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "pose %d of T (team order) is not in SE(3) (|R^T R - I| = %.3g, det R = %.12g)", g, orth, det);
        argerr = buf;
      }
    }
    if (plain) {  // (op 3: the number of pairs and their hash)
      st.agree_num = num_pairs;
      RecordHash h;
      for (int k = 0; argerr.empty() && k < 2 * num_pairs; ++k) h.add(pairs[k]);
      st.agree_hash = h.value();
    }
    if (x.begin(t, a.tr, a.owner, what, st.op, 3, a.flags, st.agree_num, argerr.empty() ? st.agree_hash : 0.0, st.agree_int,
                argerr.empty() ? nullptr : argerr.c_str())) {
      // (a participant whose own records were refused says why in the words of the single team's call)
      if (!st.argerr.empty()) set_err(std::string(what) + ": " + st.argerr);
      return true;
    }
    // (from here on the participants agree on the owner table, the robots' sizes and the pair list)
    nr = x.num_robots; na = (int)t->ag.size();
    {  // the step's records in the global numbering: a refusal is the same on every participant
      std::string msg;
      const int r = st.resolve(x, msg);
      if (r == 2) { rc = x.fail(); return true; }
      if (r) { set_err(std::string(what) + ": " + msg); return true; }
      if (st.endpoints()) { pairs = st.pairs.data(); num_pairs = (int)(st.pairs.size() / 2); }
    }
    for (int k = 0; k < 2 * num_pairs; ++k)
      if (pairs[k] < 0 || pairs[k] >= x.nglob) {  // (the same on every participant: nobody goes on)
        set_err(std::string(what) + ": pair " + std::to_string(k / 2) + " names pose " + std::to_string(pairs[k]) + ", outside [0, " +
                std::to_string(x.nglob) + ")");
        return true;
      }
    int z = -1;  // team pose of the fixed pose, robot 0's first, when robot 0 lives here
    if (t->id2local.count(0)) {
      z = 0;
      for (int k = 0; k < t->id2local.at(0); ++k) z += t->ag[k]->n;
    }
    schur_partition(t, z, P);
    N = P.N;
    nout = (size_t)36 * (N + num_pairs);
    if (x.nglob < 2 && !st.endpoints()) {  // (with records never: a record joins two different poses of the problem)
      if (plain) {  // (nothing is free; with a step the caller's own outputs are zero)
        std::memset(a.cov_diag, 0, sizeof(double) * 36 * (size_t)N);
        if (num_pairs > 0) std::memset(a.cov_pairs, 0, sizeof(double) * 36 * (size_t)num_pairs);
      }
      rc = x.finish() ? DPGO_ERR : DPGO_OK;
      return true;
    }
    std::vector<int> local_of(nr, -1);
    for (int i = 0; i < nr; ++i)
      if (x.robot_holder[i] == x.rank) { local_of[i] = t->id2local.at(i); byid.push_back(local_of[i]); }
    pl.init(x.rank, x.world, x.robot_holder, x.robot_n, local_of);
    return false;
  }

  // ---- Lambda of T from the across operator at K = 3; the T halo stays on the device
  bool lambda_of_T() {
    x.note(hipSetDevice(t->device), __LINE__);
    s = t->stream;
    c.t = t;
    c.x = &x;
    c.setup(3);
    if (!c.halted()) x.note(hipMemcpyAsync(c.T, a.T, sizeof(double) * 12 * (size_t)N, hipMemcpyHostToDevice, s), __LINE__);
    c.apply(3, c.T, 3, c.T2, 3, false);
    if (!c.halted()) launch_cert_lambda3(s, t->d_agents.p, c.off, na, c.max_n, c.T, c.T2, c.lam, c.gmax);
    if (!c.halted()) x.note(hipGetLastError(), __LINE__);
    if (x.dead) { rc = x.fail(); return true; }
    return false;
  }

  // ---- the work lists of this participant.  Lists: [0, na) H_II,a, [na, 2 na) B_a, [2 na, 3 na) the diagonal block of H_SS of
  // robot a, 3 na: the blocks of H_SS between two robots in the rows this participant holds, one 6 x 6 slot each
  void work_lists() {
    bool outside = false;
    ncross.assign(na, 0);
    std::map<std::tuple<int, int, int>, int> slot_of;  // (team pose of the row, column robot, column frame) -> slot
    for (int k = 0; k < na; ++k) {
      const Agent &ag = *t->ag[k];
      const int so = P.sep_off[k];
      for (int j = 0; j < ag.n; ++j)
        for (int p = ag.rowptr[j]; p < ag.rowptr[j + 1]; ++p) {
          const int bi = P.offs[k] + ag.col[p], bj = P.offs[k] + j;
          if (ag.col[p] < 0 || ag.col[p] >= ag.n) { outside = true; continue; }
          if (ag.id == 0 && (ag.col[p] == 0 || j == 0)) continue;  // the fixed pose
          const bool pi = P.pub[bi], pj = P.pub[bj];
          if (pi && pj) { if (bi <= bj) L.add(2 * na + k, bi, bj, k, p, P.pos[bi] - so, P.pos[bj] - so, CD_MIRROR); }
          else if (!pi && !pj) { if (bi <= bj) L.add(k, bi, bj, k, p, P.pos[bi], P.pos[bj], CD_MIRROR); }
          else if (!pi && pj) L.add(na + k, bi, bj, k, p, P.pos[bi], P.pos[bj] - so, bi > bj ? (CD_FLIP | CD_TRANS) : 0);
        }
      for (size_t e = 0; e < ag.se_host.size(); ++e) {
        const SharedEdgeDev &se = ag.se_host[e];
        const int cr = se.src_robot, cf = se.src_frame;
        if (cr < 0 || cr >= nr || cf < 0 || cf >= x.robot_n[cr] || se.lpose < 0 || se.lpose >= ag.n) { outside = true; continue; }
        if (cr >= ag.id) continue;            // the row-owner rule: the block (row own pose, column the LOWER robot's pose)
        if (cr == 0 && cf == 0) continue;     // the fixed pose
        if (ag.id == 0 && se.lpose == 0) continue;
        const int bj = P.offs[k] + se.lpose;
        // the column pose's row of T: its own when the neighbour lives here, else its halo slot behind this team's poses
        const int bi = se.src_agent_local >= 0 ? P.offs[se.src_agent_local] + cf : N + x.hoffs[k] + se.slot;
        const auto key = std::make_tuple(bj, cr, cf);
        auto it = slot_of.find(key);
        if (it == slot_of.end()) {
          it = slot_of.emplace(key, (int)xb.size()).first;
          xb.push_back({k, P.pos[bj] - so, cr, cf});
          ++ncross[k];
        }
        L.add(3 * na, bi, bj, k, ~(int)e, 0, it->second, CD_TRANS);
      }
    }
    L.finish(3 * na + 1);
    if (outside) x.fail_local("a stored block lies outside the problem");
  }

  // ---- allgather A: the sizes.  Behind it every participant knows the separator of the whole problem, and this one its
  // pairs of two interior poses of one robot (their blocks of C_a are kept in the robot's step) and whether it fits its device
  bool gather_sizes() {
    std::vector<double> ga(pl.a_len(), 0.0);
    for (int k = 0; k < na; ++k) pl.a_put(ga, t->ag[k]->id, P.sep_off[k + 1] - P.sep_off[k], (int)P.interior[k].size(), ncross[k]);
    if (x.gather(ga, gall)) { rc = x.fail(); return true; }
    pl.a_take(gall);
    nS = pl.nS;
    pl.same_robot_pairs(P, pairs, num_pairs);
    // (V and X alone beyond the device: the caller has decided it without reading V, and says so in its own words)
    if (!x.bad && !st.memerr.empty()) { fcode = XF_MEMORY; fmsg = std::string(what) + ": " + st.memerr; }
    else if (!x.bad && schur_fits(t, P, pl.nSp, pl.kmax, num_pairs, what, fmsg, cols)) { fcode = XF_MEMORY; }
    return false;
  }

  // ---- device storage, the robots as sets, the records of the apply.  DPGO_ERR: a local failure (message set)
  int storage() {
    const int M = std::max(6 * P.max_int, nS);
    const size_t MM = (size_t)M * M, ncrosspairs = pl.two_robot_pairs(pairs, num_pairs);
    size_t w_max = 0, rlen = 0;
    doff.assign(na + 1, 0);
    for (int k = 0; k < na; ++k) {
      const size_t sk = (size_t)(P.sep_off[k + 1] - P.sep_off[k]);
      w_max = std::max(w_max, (size_t)36 * P.interior[k].size() * sk);
      doff[k + 1] = doff[k] + 36 * sk * sk;
    }
    const size_t d_all = doff[na], small = 4 * (size_t)(na + 1) + 2 * nout;
    cross_chunk = cov_cross_chunk(ncrosspairs, pl.kmax);
    roff.assign(na, 0);
    for (int k : byid) { roff[k] = rlen; rlen += (size_t)6 * pl.gs[t->ag[k]->id] * cols; }
    h_ra.resize(rlen);
    // d_int: the team pose of every interior index (robot after robot), then iota = 0, 1, ..., |S| - 1 over the GLOBAL separator
    std::vector<int> ints;
    ipose_off.assign(na + 1, 0); soff.assign(na, 0);
    for (int k = 0; k < na; ++k) {
      ints.insert(ints.end(), P.interior[k].begin(), P.interior[k].end());
      ipose_off[k + 1] = (int)ints.size();
      soff[k] = 6 * pl.gsoff[t->ag[k]->id];
    }
    for (int q = 0; q < pl.nSp; ++q) ints.push_back(q);
    d_W.resize(na);
    aitem.resize(cols > 0 ? 3 * (size_t)na + 1 : 0);
    bool bad = D.A.alloc(MM) || D.Wk.alloc(MM) || D.M.alloc(MM) || d_S.alloc((size_t)nS * nS) || D.B.alloc(w_max) || d_small.alloc(small) ||
               d_int.upload(ints, s) || D.items.upload(L.items, s) || D.src.upload(L.srcs, s) || D.dst.upload(L.dsts, s) ||
               D.blk.alloc((size_t)N + num_pairs) || d_is.alloc((size_t)num_pairs) || d_cross.alloc(ncrosspairs) ||
               D.tab.alloc((size_t)na + 2 * ncrosspairs) || d_t.alloc(cross_chunk * 6 * std::max(pl.kmax, 1)) ||
               d_T.alloc((size_t)12 * (N + x.halo_slots)) || d_D.alloc(d_all) || d_X.alloc(36 * xb.size());
    if (cols > 0 && !bad) {
      int kloc = 0;
      for (int k = 0; k < na; ++k) kloc = std::max(kloc, 6 * (P.sep_off[k + 1] - P.sep_off[k]));
      const size_t vx = (size_t)6 * N * cols, sx = (size_t)nS * cols;
      bad = d_aV.alloc(vx) || d_aX.alloc(vx) || d_rS.alloc(sx) || d_xS.alloc(sx) || d_tmp.alloc((size_t)kloc * cols) || d_pub.upload(P.sep, s) ||
            d_app.alloc(aitem.size());
    }
    for (int k = 0; k < na && !bad; ++k) bad = d_W[k].alloc((size_t)36 * P.interior[k].size() * (size_t)(P.sep_off[k + 1] - P.sep_off[k])) != 0;
    if (bad) { set_err("device allocation failed"); return DPGO_ERR; }
    stat = d_small.p; keepd = stat + 4 * (size_t)(na + 1); outd = keepd + nout;
    HIPC(hipMemcpyAsync(d_T.p, c.T, sizeof(double) * 12 * (size_t)N, hipMemcpyDeviceToDevice, s));
    if (x.halo_slots > 0)
      HIPC(hipMemcpyAsync(d_T.p + (size_t)12 * N, x.d_halo, sizeof(double) * 12 * (size_t)x.halo_slots, hipMemcpyDeviceToDevice, s));
    D.s = s; D.agents = t->d_agents.p; D.Td = d_T.p; D.lam = c.lam; D.L = &L;
    // the robots as sets (the table is on the device before the first keep launch): nb a window of iota at the robot's place
    // in the global separator
    iota_d = d_int.p + ipose_off[na];
    rob.resize(na);
    for (int k = 0; k < na; ++k)
      rob[k] = {d_W[k].p, iota_d + pl.gsoff[t->ag[k]->id], d_int.p + ipose_off[k], D.M.p, nullptr, D.B.p, 6 * (int)P.interior[k].size(),
                6 * (P.sep_off[k + 1] - P.sep_off[k])};
    HIPC(hipMemcpyAsync(D.tab.p, rob.data(), sizeof(CovBlock) * na, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(stat, 0, sizeof(double) * small, s));
    if (d_all) HIPC(hipMemsetAsync(d_D.p, 0, sizeof(double) * d_all, s));
    if (cols > 0) {
      for (int k = 0; k < na; ++k) {
        const int *poses = d_int.p + ipose_off[k];
        const int ni = rob[k].ld, K = rob[k].K;
        aitem[k] = {D.M.p, d_aV.p, d_aX.p, poses, poses, ni, 6 * N, 6 * N, ni, cols, ni};
        aitem[na + k] = {d_W[k].p, d_aV.p, d_tmp.p, poses, nullptr, ni, 6 * N, K, K, cols, ni};
        aitem[2 * na + k] = {d_W[k].p, d_xS.p + soff[k], d_aX.p, nullptr, poses, ni, nS, 6 * N, ni, cols, K};
      }
      aitem[3 * na] = {D.M.p, d_rS.p, d_xS.p, nullptr, nullptr, nS, nS, nS, nS, cols, nS};
      HIPC(hipMemcpyAsync(d_app.p, aitem.data(), sizeof(ApplyItem) * aitem.size(), hipMemcpyHostToDevice, s));
      HIPC(hipMemsetAsync(d_aX.p, 0, sizeof(double) * 6 * (size_t)N * cols, s));
      if (st.rhs(d_T.p, N, d_aV.p, s)) return DPGO_ERR;
    }
    MARK(-1);
    return DPGO_OK;
  }

  // ---- phase 1 on the device: this participant's robots, one after another.  A pivot that is not positive is this
  // participant's failure record (fcode), not an error of the phase
  int phase1() {
    for (int k = 0; k < na; ++k) D.assemble(2 * na + k, d_D.p + doff[k], rob[k].K);
    D.assemble(3 * na, d_X.p, 6);
    HIPC(hipGetLastError());
    MARK(0);
    for (int k : byid) {
      const int ni = rob[k].ld;
      const int *pub = cols > 0 ? d_pub.p + P.sep_off[k] : nullptr;
      if (ni == 0) {  // (a robot with no interior pose: r_a = v_{S_a})
        if (cols > 0) launch_apply_rows_sub(s, d_aV.p, (size_t)6 * N, pub, nullptr, d_rS.p + soff[k], (size_t)nS, nullptr, rob[k].K, cols);
        continue;
      }
      const SchurApply ap{d_app.p + k, d_app.p + na + k, aitem.data() + k, aitem.data() + na + k, d_aV.p, (size_t)6 * N, (size_t)nS, pub,
                          d_tmp.p, d_rS.p + soff[k], cols, &st.flops, &app_marks};
      const int f = schur_robot_step(D, marks, t->ag[k]->id, k, na + k, ni, rob[k].K, d_W[k].p, d_D.p + doff[k], rob[k].K, pl.keep_list[k], keepd,
                                     stat + 4 * k, cols > 0 ? &ap : nullptr);
      if (f < 0) return DPGO_ERR;
      if (f > 0) {
        fcode = XF_PIVOT; frobot = t->ag[k]->id; frow = f - 1;
        const int g = P.interior[k][(f - 1) / 6];
        fpose = (int)(x.robot_goff[frobot] + (g - P.offs[k]));
        return DPGO_OK;
      }
    }
    hD.resize(doff[na]); hX.resize(36 * xb.size()); hstat.resize(4 * (size_t)(na + 1));
    if (!hD.empty()) HIPC(hipMemcpyAsync(hD.data(), d_D.p, sizeof(double) * hD.size(), hipMemcpyDeviceToHost, s));
    if (!xb.empty()) HIPC(hipMemcpyAsync(hX.data(), d_X.p, sizeof(double) * hX.size(), hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(hstat.data(), stat, sizeof(double) * hstat.size(), hipMemcpyDeviceToHost, s));
    if (cols > 0) {  // the r_a of the robots here, K_a x cols each, in id order: this participant's part of allgather C
      HIPC(hipGetLastError());
      for (int k : byid)
        if (rob[k].K > 0)
          HIPC(hipMemcpy2DAsync(h_ra.data() + roff[k], sizeof(double) * rob[k].K, d_rS.p + soff[k], sizeof(double) * nS, sizeof(double) * rob[k].K,
                                cols, hipMemcpyDeviceToHost, s));
    }
    HIPC(hipStreamSynchronize(s));
    return DPGO_OK;
  }

  // ---- allgather B, the failure of any participant told by all in the same words, and S_c of the whole problem
  bool gather_b() {
    std::vector<double> gb(pl.pmax, 0.0);
    gb[pl.B_CODE] = fcode; gb[pl.B_ROBOT] = frobot; gb[pl.B_POSE] = fpose; gb[pl.B_ROW] = frow;
    for (int k : byid) {
      if (fcode != XF_OK || x.bad) break;
      const double rstat[4] = {hstat[4 * k], hstat[4 * k + 1], hstat[4 * k + 2], rob[k].ld > 0 ? 1.0 : 0.0};
      std::vector<int> frames;
      for (int q = P.sep_off[k]; q < P.sep_off[k + 1]; ++q) frames.push_back(P.sep[q] - P.offs[k]);
      std::vector<SchurAcrossPlan::BCross> cross;
      for (size_t b = 0; b < xb.size(); ++b)
        if (xb[b].lrobot == k) cross.push_back({xb[b].lrow, xb[b].crobot, xb[b].cframe, hX.data() + 36 * b});
      pl.b_pack(gb, t->ag[k]->id, frames.data(), hD.data() + doff[k], rstat, cross);
    }
    if (x.gather(gb, gall)) { rc = x.fail(); return true; }
    for (int q = 0; q < x.world; ++q) {
      const double *h = pl.b_header(gall, q);
      if (h[pl.B_CODE] == XF_OK) continue;
      std::string m = std::string(what) + ": rank " + std::to_string(q) + ": ";
      if (h[pl.B_CODE] == XF_PIVOT)
        m = pivot_message(std::string(what) + ": rank " + std::to_string(q), (long long)h[pl.B_ROW],
                          "the interior Hessian of robot " + std::to_string((long long)h[pl.B_ROBOT]), (long long)h[pl.B_POSE]);
      else if (h[pl.B_CODE] == XF_MEMORY) m += "the Schur path does not fit its device (its own error names the bytes)";
      else m += "local failure (its own error names the cause)";
      if (q == x.rank && !fmsg.empty() && h[pl.B_CODE] != XF_PIVOT) m += " [" + fmsg + "]";
      set_err(m);
      return true;
    }
    if (!pl.assemble(gall, hS)) {  // (the same on every participant)
      set_err(std::string(what) + ": a shared edge names a pose its robot does not list as public (the measurement sets differ)");
      return true;
    }
    return false;
  }

  // ---- phase 2 on the device: the separator's inverse and this participant's blocks.  A pivot of the separator that is not
  // positive is sfail, the same on every participant
  int phase2() {
    if (nS > 0) {
      HIPC(hipMemcpyAsync(d_S.p, hS.data(), sizeof(double) * hS.size(), hipMemcpyHostToDevice, s));
      launch_schur_mirror(s, d_S.p, nS);
      HIPC(hipGetLastError());
      const int f = dense_spd_inverse(s, d_S.p, D.Wk.p, D.M.p, nS);
      HIPC(hipGetLastError());
      if (f < 0) { set_err("scratch allocation of the inverse failed"); return DPGO_ERR; }
      if (f > 0) { sfail = f; return DPGO_OK; }
      if (launch_cov_logdet(s, d_S.p, nS, stat + 4 * na)) return DPGO_ERR;
      MARK(3);
      if (schur_listed(D, nS, pl.pub_list, D.blk.p, true, outd)) return DPGO_ERR;
      MARK(4);
    }
    for (int k : byid) {
      if (rob[k].ld == 0) continue;
      if (schur_robot_blocks(D, marks, t->ag[k]->id, k, rob[k].ld, rob[k].K, d_W[k].p, D.M.p + (size_t)soff[k] * nS + soff[k], nS, pl.same_list[k],
                             keepd, outd))
        return DPGO_ERR;
    }
    if (schur_listed(D, nS, pl.is_list, d_is.p, false, outd)) return DPGO_ERR;
    hout.resize(nout);
    HIPC(hipMemcpyAsync(hout.data(), outd, sizeof(double) * nout, hipMemcpyDeviceToHost, s));
    if (nS > 0) HIPC(hipMemcpyAsync(sstat.data(), stat + 4 * na, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
    // the rows W_a[i,:] this participant holds, 6 x 6 s_a column-major each, at their places in the record
    hrows.assign(pl.rows_max, 0.0);
    for (size_t r = 0; r < pl.rows.size(); ++r) {
      if (x.robot_holder[pl.rows[r].robot] != x.rank) continue;
      const int lk = t->id2local.at(pl.rows[r].robot);
      if (rob[lk].K > 0)
        HIPC(hipMemcpy2DAsync(hrows.data() + pl.rowoff[r], 48, d_W[lk].p + (size_t)6 * pl.rows[r].li, sizeof(double) * rob[lk].ld, 48, rob[lk].K,
                              hipMemcpyDeviceToHost, s));
    }
    HIPC(hipStreamSynchronize(s));
    return DPGO_OK;
  }

  // ---- allgather C: the owned pair blocks, the rows and the r_a; behind it the separator's pivot, and everyone's pair blocks
  bool gather_c() {
    std::vector<double> gcv(pl.cmax, 0.0);
    if (!x.bad && sfail == 0) {
      pl.c_pack(gcv, hout.data() + (size_t)36 * N, hrows);
      for (int k : byid)
        if (cols > 0) pl.c_pack_ra(gcv, t->ag[k]->id, h_ra.data() + roff[k], cols);
    }
    if (x.gather(gcv, gall)) { rc = x.fail(); return true; }
    if (sfail > 0) {  // (deterministic: the same on every participant, and behind the allgather that would have told of a failure)
      const int sp = (sfail - 1) / 6;
      int robot = 0;
      while (robot + 1 < nr && pl.gsoff[robot + 1] <= sp) ++robot;
      const long long pose = x.robot_goff[robot] + pl.pubf[robot][sp - pl.gsoff[robot]];
      set_err(pivot_message(what, sfail - 1, "the Schur complement on the public poses", pose));
      return true;
    }
    pl.c_unpack_pairs(gall, hout.data() + (size_t)36 * N);
    return false;
  }

  // ---- phase 3: the pairs of two robots' interiors, from the gathered rows: each row a robot of its own in the table
  int phase3() {
    const size_t nrows = pl.rows.size();
    if (nrows == 0) return DPGO_OK;
    size_t total = 0;
    std::vector<size_t> ro(nrows);
    for (size_t r = 0; r < nrows; ++r) { ro[r] = total; total += pl.row_len(r); }
    if (d_rows.alloc(total)) { set_err("device allocation failed"); return DPGO_ERR; }
    std::vector<double> hr(total);
    std::vector<CovBlock> prob(nrows);  // a row as a robot of one pose
    std::vector<CovCross> cross_list;
    for (size_t r = 0; r < nrows; ++r) {
      std::memcpy(hr.data() + ro[r], pl.c_row(gall, r), sizeof(double) * pl.row_len(r));
      prob[r] = {d_rows.p + ro[r], iota_d + pl.gsoff[pl.rows[r].robot], nullptr, nullptr, nullptr, nullptr, 6, 6 * pl.gs[pl.rows[r].robot]};
    }
    for (size_t r = 0; r + 1 < nrows; r += 2) cross_list.push_back({N + pl.rows[r].pair, na + (int)r, 0, na + (int)r + 1, 0, 0});
    HIPC(hipMemcpyAsync(d_rows.p, hr.data(), sizeof(double) * total, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(D.tab.p + na, prob.data(), sizeof(CovBlock) * prob.size(), hipMemcpyHostToDevice, s));
    if (schur_cross_pairs(s, D.tab.p, D.M.p, nS, cross_list, d_cross.p, pl.kmax, d_t.p, cross_chunk, outd)) return DPGO_ERR;
    std::vector<double> hc(36 * (size_t)num_pairs);
    HIPC(hipMemcpyAsync(hc.data(), outd + 36 * (size_t)N, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (const CovCross &e : cross_list) std::memcpy(hout.data() + 36 * (size_t)e.blk, hc.data() + 36 * (size_t)(e.blk - N), sizeof(double) * 36);
    return DPGO_OK;
  }

  // ---- Sigma applied to vectors, behind the separator's inverse (D.M = Sigma_SS).  r_S from the gathered r_a, the same bytes
  // on every participant; x_S = Sigma_SS r_S, the whole of it, here; x_a = u_a - W_a x_S[S_a] and X[S_a] = x_S[S_a] for the
  // robots here.  Then the step's view and its taken()
  int apply() {
    if (nS > 0) {
      std::vector<double> hrS;
      pl.c_unpack_rs(gall, cols, hrS);
      HIPC(hipMemcpyAsync(d_rS.p, hrS.data(), sizeof(double) * hrS.size(), hipMemcpyHostToDevice, s));
      MARK(-1);
      launch_apply_gemm(s, false, d_app.p + 3 * na, aitem.data() + 3 * na, 1, false);
      for (int k : byid) {
        launch_apply_gemm(s, false, d_app.p + 2 * na + k, aitem.data() + 2 * na + k, 1, true);
        launch_apply_rows_sub(s, d_xS.p + soff[k], (size_t)nS, nullptr, nullptr, d_aX.p, (size_t)6 * N, d_pub.p + P.sep_off[k], rob[k].K, cols);
        st.flops += apply_flops(aitem.data() + 2 * na + k, 1);
      }
      HIPC(hipGetLastError());
      MARK(-1);
      app_marks.push_back(marks.ev.size() - 1);
      st.flops += apply_flops(aitem.data() + 3 * na, 1);
      HIPC(hipStreamSynchronize(s));  // (hrS has been read)
    }
    st.X = d_aX.p;
    // what a step along X needs of the poses behind this participant's own (CovAcrossView): host tables, no launch
    CovAcrossView &v = st.view;
    v.Td = d_T.p; v.N = N; v.halo_slots = x.halo_slots; v.xS = nS > 0 ? d_xS.p : nullptr; v.nS = nS;
    v.diag = outd; v.blocks_h = hout.data(); v.num_pairs = num_pairs;
    v.halo_sep.assign(x.halo_slots, -1);
    for (int k = 0; k < na; ++k)
      for (size_t q = 0; q < t->ag[k]->np.size(); ++q) {
        const int b = t->ag[k]->np[q].first, f = t->ag[k]->np[q].second;
        if (b >= 0 && b < nr && !t->id2local.count(b)) v.halo_sep[x.hoffs[k] + q] = pl.sep_index(b, f);
      }
    if (st.taken(N, s)) return DPGO_ERR;
    HIPC(hipStreamSynchronize(s));
    for (size_t k : app_marks) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, marks.ev[k - 1], marks.ev[k]) == hipSuccess) st.ms_products += ms;
    }
    return DPGO_OK;
  }

  // ---- the step behind the blocks (the gate, the audit).  Allgather D: per endpoint of the records, sorted by global pose,
  // 12 doubles of T and the 36 of its diagonal block from the participant that holds it, zeros from everyone else (pose 0's
  // block is zero with its holder too).  Then every participant holds the compact tables and runs all records itself
  bool gather_d() {
    const std::vector<int> &ends = *st.endpoints();
    const int E = (int)ends.size();
    HeldRecord rec{48, std::vector<int>(E)};
    for (int e = 0; e < E; ++e) rec.holder[e] = x.robot_holder[pl.grobot[ends[e]]];
    std::vector<double> gd(rec.len(), 0.0);
    for (int e = 0; e < E && !x.bad; ++e) {
      if (rec.holder[e] != x.rank) continue;
      const int lp = P.offs[t->id2local.at(pl.grobot[ends[e]])] + pl.gframe[ends[e]];
      std::memcpy(rec.mine(gd, e), a.T + (size_t)12 * lp, sizeof(double) * 12);
      std::memcpy(rec.mine(gd, e) + 12, hout.data() + (size_t)36 * lp, sizeof(double) * 36);
    }
    if (x.gather(gd, gall)) { rc = x.fail(); return true; }
    // T of the E endpoints, their diagonal blocks, the pair blocks
    std::vector<double> tab((size_t)48 * E + (size_t)36 * num_pairs);
    for (int e = 0; e < E; ++e) {
      std::memcpy(tab.data() + (size_t)12 * e, rec.from(gall, e), sizeof(double) * 12);
      std::memcpy(tab.data() + (size_t)12 * E + (size_t)36 * e, rec.from(gall, e) + 12, sizeof(double) * 36);
    }
    std::memcpy(tab.data() + (size_t)48 * E, hout.data() + (size_t)36 * N, sizeof(double) * 36 * (size_t)num_pairs);
    if (run_records(tab, E)) x.fail_local(g_err);
    return false;
  }
  int run_records(const std::vector<double> &tab, int E) {
    if (d_tab.alloc(tab.size())) { set_err("device allocation failed"); return DPGO_ERR; }
    HIPC(hipMemcpyAsync(d_tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s));
    const AcrossStage stage{d_tab.p, d_tab.p + (size_t)12 * E, d_tab.p + (size_t)48 * E, E, num_pairs, s};
    if (st.run(stage)) return DPGO_ERR;
    HIPC(hipStreamSynchronize(s));
    return DPGO_OK;
  }

  // ---- the closing status word and the results: log det and pivots in robot order, the separator last
  int close() {
    if (x.finish()) return DPGO_ERR;
    std::vector<char> counted(nr + 1, 0);
    for (int i = 0; i < nr; ++i) counted[i] = pl.rstat[4 * i + 3] != 0.0;
    counted[nr] = nS > 0;
    std::vector<double> rstat = pl.rstat;
    rstat.insert(rstat.end(), sstat.begin(), sstat.end());
    double ms[5];
    marks.sum(ms);
    cov_fill_result(a.res, 6 * (x.nglob - 1), rstat.data(), counted, ms);
    schur_report(marks);
    static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
    if (timing)
      std::fprintf(stderr,
                   "%s: rank %d of %d, n %lld, separator %d, largest interior here %d, assemble %.3f ms, factorisations "
                   "%.3f ms, products %.3f ms, separator inverse %.3f ms, extract %.3f ms, %lld allgathers, %lld exchanges\n",
                   what, x.rank, x.world, 6 * (x.nglob - 1), nS, 6 * P.max_int, ms[0], ms[1], ms[2], ms[3], ms[4], x.n_allgather, x.n_exchange);
    if (!plain) return DPGO_OK;  // (the blocks stay here: the step's outputs are the call's)
    std::memcpy(a.cov_diag, hout.data(), sizeof(double) * 36 * (size_t)N);
    if (num_pairs > 0) std::memcpy(a.cov_pairs, hout.data() + (size_t)36 * N, sizeof(double) * 36 * (size_t)num_pairs);
    return DPGO_OK;
  }
};

}  // namespace

int covariance_schur_across(const SchurAcrossArgs &a) {
  if (a.res) std::memset(a.res, 0, sizeof *a.res);
  AcrossStep plain_step;
  SchurAcross call(a, a.step ? *a.step : plain_step, !a.step);
  return call.run();
}
#undef MARK


}  // namespace dpgo_cert

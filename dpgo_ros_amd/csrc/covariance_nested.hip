// covariance_nested.hip -- the marginal pose covariances of covariance.hip by nested dissection inside each robot
// ("nested").
//
// The robot-wise Schur path (covariance_schur.hip) takes its sets from the team alone: a robot's interior is one block, however
// large.  Here a robot whose interior holds more than max_block poses has the interior's own graph dissected by
// tl_make_plan (twolevel_plan.cpp): the subdomains become BLOCKS of that robot, the dissection's separator poses are
// PROMOTED into the robot's part of the global separator S (team order: a robot's part stays one contiguous range).  A
// robot whose interior fits is one block.  Blocks are ordered by robot, then by first pose.  N_b: the separator poses
// coupled to block b, ascending; they lie in the block's own robot's range.  Per block
//     C_b = H_bb^-1,   B_b = H[b, N_b]  (6 |I_b| x 6 |N_b|: the coupled columns alone),   W_b = C_b B_b,
//     S_c = H_SS - sum_b B_b^T W_b  scattered through N_b, one block after another in block order,   Sigma_SS = S_c^-1,
//     Sigma_ij = C_b[ij] + Z_b[i,:] W_b[j,:]^T,  Z_b = W_b Sigma_SS[N_b, N_b]                 (i, j in block b)
//     Sigma_ij = W_b[i,:] Sigma_SS[N_b, N_c] W_c[j,:]^T                                        (i in b, j in c != b)
//     Sigma_is = -W_b[i,:] Sigma_SS[N_b, s],   Sigma_st = the block of Sigma_SS,   pose 0: zeros,
//     log det H_red = sum_b log det H_bb + log det S_c   (summed on the host in block order, the separator last).
// The blocks are assembled, factored (dense_spd_inverse_batched) and multiplied (k_dgemm_batched) a BATCH at a time: batches
// are filled in block order while their matrices fit the workspace.  A block's arithmetic does not depend on the batch it
// rides in (one workgroup per 64 x 64 tile and K in index order, dgemm_tile; the factorisation's kernels serve a matrix by
// blockIdx.z), so neither do the bits of the result.  No atomics, fp64 throughout, outputs staged on the device.
// The blocks are the sets of the extraction kernels of covariance_extract.h, which the Schur path launches too; the head and
// the tail of the call are CovFrame's (covariance_frame.h).
// With a CovApply (certify_internal.h, covariance_apply.h) the path also forms X = Sigma V from the same factors,
// without a block of Sigma: u_b = C_b v_b and W_b^T v_b while C_b is live in its batch, r_S = v_S - sum_b scatter(W_b^T v_b) one
// launch per block in block order, x_S = Sigma_SS r_S, x_b = u_b - W_b x_S[N_b].  Without one it queues what it queued before.
// Loads of matrices, lists and index arrays go through gp(); the one exception is the record of a table (GemmItem,
// NestTarget, CovBlock: one per workgroup or per thread, a few dozen bytes), copied as a struct -- where the index is
// uniform (blockIdx) the compiler reads it through the scalar cache.
#include <cmath>
#include <cstdlib>

#include "covariance_apply.h"
#include "covariance_extract.h"

namespace dpgo {

// a target of the batched assembly: H_bb (row 2 b of the table) or B_b (row 2 b + 1), column-major
struct NestTarget {
  double *H;
  int ld, pad_;
};
static_assert(sizeof(NestTarget) == 16, "the byte formula of include/dpgo_hip.h counts 16 bytes");

// k_cov_assemble_map with the target taken from a table (CovDst::tgt): H_bb and B_b of every block of a batch in one launch
__global__ __launch_bounds__(256) void k_nest_assemble(const AgentDev *__restrict__ agents, const CovItem *__restrict__ items,
                                                       const CovSrc *__restrict__ src, const CovDst *__restrict__ dst, int nitems,
                                                       const double *__restrict__ T, const double *__restrict__ lam,
                                                       const NestTarget *__restrict__ targets) {
  const int it = blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  const v4i_t wi = *(const __attribute__((address_space(1))) v4i_t *)(items + it);
  const v4i_t di = *(const __attribute__((address_space(1))) v4i_t *)(dst + it);
  const CovItem w{wi.x, wi.y, wi.z, wi.w};
  const NestTarget tg = targets[di.w];
  double Hc[6][6];  // H_lo,hi
  cov_form_block(agents, src, w, T, lam, Hc, (di.z & CD_FLIP) != 0);
  const size_t r = (size_t)6 * di.x, c = (size_t)6 * di.y, ld = (size_t)tg.ld;
  const bool tr = (di.z & CD_TRANS) != 0;
  cov_store_block(tg.H + c * ld + r, ld, Hc, tr);
  if ((di.z & CD_MIRROR) && di.x != di.y) cov_store_block(tg.H + r * ld + c, ld, Hc, !tr);
}

// one product of a batch: C = op(A) B with its own pointers, shapes and leading dimensions
struct GemmItem {
  const double *A, *B;
  double *C;
  int lda, ldb, ldc, m, n, k;
};
static_assert(sizeof(GemmItem) == 48, "the byte formula of include/dpgo_hip.h counts 48 bytes");

// k_dgemm for many products at once: the item rides on blockIdx.z, the grid covers the largest item and a tile outside
// its own item leaves at once.  The tile is dgemm_tile: an item's bits are those of k_dgemm on the same operands
template <bool TA>
__global__ __launch_bounds__(256) void k_dgemm_batched(const GemmItem *__restrict__ items, int sub) {
  const GemmItem g = items[blockIdx.z];
  const int i0 = 64 * blockIdx.x, j0 = 64 * blockIdx.y;
  if (i0 >= g.m || j0 >= g.n || g.k <= 0) return;
  dgemm_tile<TA>(g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.m, g.n, g.k, sub, i0, j0);
}

// S[N_b, N_b] -= P (K x K, column-major, ld K), S of order n.  One launch per block, in block order on one stream: two blocks
// that meet in an element of S subtract from it in that order
__global__ __launch_bounds__(256) void k_nest_scatter_sub(double *__restrict__ S, int n, const double *__restrict__ P, int K,
                                                          const int *__restrict__ nb) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * K) return;
  const int i = (int)(e % K), j = (int)(e / K);
  double *s = S + cov_row(nb, j) * n + cov_row(nb, i);
  gp(s)[0] = gp(s)[0] - gp(P)[e];
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

// the sets of a call ("nested"), from the team's poses in team order, who is public among them and the
// pattern of the blocks that join two poses of one robot
struct NestPlan {
  int N = 0, na = 0, nS = 0, promoted = 0;
  bool split = false;                       // some robot's interior was dissected
  std::vector<int> offs, robot_of;
  std::vector<int> block_of;                // block index, -1 a separator pose, -2 pose 0
  std::vector<int> pos;                     // index inside the pose's own set (its block, or the separator)
  std::vector<int> sep;                     // team pose of separator index
  struct Block {
    int robot;
    std::vector<int> poses, nb;             // team poses in order; separator indices of N_b, ascending
  };
  std::vector<Block> blocks;
  int largest_block() const { size_t m = 0; for (const Block &b : blocks) m = std::max(m, b.poses.size()); return (int)m; }
  int largest_nb() const { size_t m = 0; for (const Block &b : blocks) m = std::max(m, b.nb.size()); return (int)m; }
  long long sum_nb() const { long long s = 0; for (const Block &b : blocks) s += (long long)b.nb.size(); return s; }
  void info(int *out) const {
    out[0] = (int)blocks.size(); out[1] = nS; out[2] = promoted; out[3] = largest_block(); out[4] = largest_nb(); out[5] = (int)sum_nb();
  }
};

// offs: na + 1 pose offsets; pub: public by the team's rule; rowptr / col: a pattern over the N poses in which only entries
// between two poses of one robot are looked at.  Host arithmetic only, index order throughout: deterministic
void nest_build(int na, const std::vector<int> &offs, const std::vector<char> &pub, const std::vector<int> &rowptr,
                const std::vector<int> &col, int max_block, NestPlan &P) {
  const int N = offs[na];
  P.N = N; P.na = na; P.offs = offs;
  P.robot_of.assign(N, 0);
  P.block_of.assign(N, -1);
  P.pos.assign(N, 0);
  if (N > 0) P.block_of[0] = -2;
  std::vector<int> loc(N, -1);
  for (int k = 0; k < na; ++k) {
    std::vector<int> I;
    for (int g = offs[k]; g < offs[k + 1]; ++g) {
      P.robot_of[g] = k;
      if (g != 0 && !pub[g]) I.push_back(g);
    }
    if (I.empty()) continue;
    if ((int)I.size() <= max_block) {
      for (int g : I) P.block_of[g] = (int)P.blocks.size();
      P.blocks.push_back({k, I, {}});
      continue;
    }
    P.split = true;
    // the pattern of the robot's block-CSR restricted to its interior poses
    for (size_t v = 0; v < I.size(); ++v) loc[I[v]] = (int)v;
    std::vector<int> rp(I.size() + 1, 0), cl;
    for (size_t v = 0; v < I.size(); ++v) {
      for (int p = rowptr[I[v]]; p < rowptr[I[v] + 1]; ++p) {
        const int u = col[p];
        if (u >= offs[k] && u < offs[k + 1] && loc[u] >= 0) cl.push_back(loc[u]);
      }
      rp[v + 1] = (int)cl.size();
    }
    const dpgo_host::TLPlan pl = dpgo_host::tl_make_plan((int)I.size(), rp, cl, max_block);
    for (const std::vector<int> &sub : pl.sub) {  // (in order of their first pose)
      NestPlan::Block b{k, {}, {}};
      for (int v : sub) { b.poses.push_back(I[v]); P.block_of[I[v]] = (int)P.blocks.size(); }
      P.blocks.push_back(std::move(b));
    }
    P.promoted += pl.ns;  // (block_of stays -1: a separator pose)
  }
  for (int g = 1; g < N; ++g)
    if (P.block_of[g] == -1) { P.pos[g] = (int)P.sep.size(); P.sep.push_back(g); }
  P.nS = (int)P.sep.size();
  for (NestPlan::Block &b : P.blocks) {
    for (size_t v = 0; v < b.poses.size(); ++v) {
      const int g = b.poses[v];
      P.pos[g] = (int)v;
      for (int p = rowptr[g]; p < rowptr[g + 1]; ++p) {
        const int u = col[p];
        if (u >= offs[b.robot] && u < offs[b.robot + 1] && P.block_of[u] == -1) b.nb.push_back(P.pos[u]);
      }
    }
    std::sort(b.nb.begin(), b.nb.end());
    b.nb.erase(std::unique(b.nb.begin(), b.nb.end()), b.nb.end());
  }
}

// the plan of a team: public poses by the rule of schur_partition (a pose that a shared-edge record names, whatever the
// weight), the pattern from the robots' block-CSR
void nest_plan_team(dpgo_team_t *t, int max_block, NestPlan &P) {
  SchurPartition sp;
  schur_partition(t, 0, sp);
  std::vector<int> rowptr(1, 0), col;
  for (int k = 0; k < sp.na; ++k) {
    const Agent &a = *t->ag[k];
    for (int j = 0; j < a.n; ++j) {
      for (int p = a.rowptr[j]; p < a.rowptr[j + 1]; ++p) col.push_back(sp.offs[k] + a.col[p]);
      rowptr.push_back((int)col.size());
    }
  }
  nest_build(sp.na, sp.offs, sp.pub, rowptr, col, max_block, P);
}

// ---- memory ("nested"; include/dpgo_hip.h has the formula).  Doubles of workspace block b needs while its
// batch is eliminated: H_bb, the inverse's work matrix and C_b (3 n_b^2), B_b (n_b K_b), B_b^T W_b (K_b^2); n_b = 6 |I_b|,
// K_b = 6 |N_b|.  (The extraction puts Z_b where B_b was and Sigma_SS[N_b, N_b] where B_b^T W_b was.)  With Sigma applied to
// `cols` vectors (covariance_apply.h) the temporary W_b^T v_b (K_b cols) rides in the same workspace.
double nest_block_ws(const NestPlan::Block &b, int cols = 0) {
  const double n = 6.0 * b.poses.size(), K = 6.0 * b.nb.size();
  return 3.0 * n * n + n * K + K * K + K * cols;
}

struct NestBytes {
  double large = 0, small = 0, ws_min = 0, w_all = 0, sep = 0, apply = 0;
  int ws_block = -1;
};

// large = 8 (3 (6 |S|)^2 + sum_b 36 |I_b| |N_b| + max_b ws_b); small: T, T Q, Lambda (33 N doubles), the Gershgorin scratch,
// 4 statistics per factor, the kept and the output blocks (72 (N + P) doubles), the scratch of pairs across blocks, the lists
// (24 bytes per kept or requested block), the work list (40 bytes per stored block of Q), the tables of the blocks
// (56 + 3 x 48 + 2 x 16 bytes each: a CovBlock, three GemmItem, two NestTarget), the index lists (4 bytes per interior pose
// and per entry of an N_b), the Linv blocks of dense_spd_inverse (8 KiB per 32 rows of every factor)
// With Sigma applied to `cols` vectors: apply = V and X (8 x 6 N cols each), r_S (8 x 6 |S| cols; x_S is written straight into
// X), one ApplyItem per block for each of the three products and one for the separator's (64 bytes each), the team poses of
// the separator and of every N_b (4 bytes each); the temporaries are in the batch workspace (nest_block_ws)
NestBytes nest_bytes(dpgo_team_t *t, const NestPlan &P, int num_pairs, int cols = 0) {
  NestBytes r;
  int max_n = 0, kmax = 0;
  size_t stored = 0;
  for (int k = 0; k < P.na; ++k) {
    max_n = std::max(max_n, t->ag[k]->n);
    stored += t->ag[k]->col.size() + t->ag[k]->se_host.size();
  }
  double linv = std::ceil(6.0 * P.nS / 32.0);
  for (size_t b = 0; b < P.blocks.size(); ++b) {
    const double ws = nest_block_ws(P.blocks[b], cols);
    if (ws > r.ws_min) { r.ws_min = ws; r.ws_block = (int)b; }
    r.w_all += 36.0 * (double)P.blocks[b].poses.size() * (double)P.blocks[b].nb.size();
    kmax = std::max(kmax, 6 * (int)P.blocks[b].nb.size());
    linv += std::ceil(6.0 * P.blocks[b].poses.size() / 32.0);
  }
  r.sep = 3.0 * 36.0 * (double)P.nS * (double)P.nS;
  r.large = 8.0 * (r.sep + r.w_all + r.ws_min);
  const double N = P.N, np = num_pairs, A = P.na, nb = (double)P.blocks.size();
  r.small = 8.0 * (33.0 * N + A * ((max_n + 255) / 256) + 4.0 * (nb + 1.0) + 72.0 * (N + np)) +
            8.0 * 6.0 * std::max(kmax, 1) * (double)cov_cross_chunk((size_t)num_pairs, kmax) + 24.0 * (2.0 * N + 3.0 * np) +
            40.0 * (double)stored + (double)(sizeof(CovBlock) + 3 * sizeof(GemmItem) + 2 * sizeof(NestTarget)) * nb +
            4.0 * (N + (double)P.sum_nb() + A + 1.0) + 8.0 * 1024.0 * linv;
  if (cols > 0)
    r.apply = 8.0 * (double)cols * (12.0 * N + 6.0 * P.nS) + (double)sizeof(ApplyItem) * (3.0 * nb + 1.0) + 4.0 * ((double)P.sum_nb() + P.nS);
  return r;
}

// the batches: blocks [beg[q], beg[q + 1]) in block order, each batch's workspace within ws_cap doubles (a single block may
// exceed it: it then rides alone)
std::vector<int> nest_batches(const NestPlan &P, double ws_cap, int cols = 0) {
  std::vector<int> beg(1, 0);
  double used = 0.0;
  for (size_t b = 0; b < P.blocks.size(); ++b) {
    const double ws = nest_block_ws(P.blocks[b], cols);
    if (b > (size_t)beg.back() && (used + ws > ws_cap || b - beg.back() >= 65535)) { beg.push_back((int)b); used = 0.0; }
    used += ws;
  }
  beg.push_back((int)P.blocks.size());
  return beg;
}

void launch_dgemm_batched(hipStream_t s, bool ta, const GemmItem *items_d, const GemmItem *items_h, int count, bool sub) {
  int mm = 0, mn = 0, mk = 0;
  for (int q = 0; q < count; ++q) { mm = std::max(mm, items_h[q].m); mn = std::max(mn, items_h[q].n); mk = std::max(mk, items_h[q].k); }
  if (count <= 0 || mm <= 0 || mn <= 0 || mk <= 0) return;
  const dim3 grid((mm + 63) / 64, (mn + 63) / 64, count);
  if (ta) hipLaunchKernelGGL(k_dgemm_batched<true>, grid, dim3(256), 0, s, items_d, sub ? 1 : 0);
  else hipLaunchKernelGGL(k_dgemm_batched<false>, grid, dim3(256), 0, s, items_d, sub ? 1 : 0);
}

double gemm_flops(const GemmItem *it, int count) {
  double f = 0.0;
  for (int q = 0; q < count; ++q) f += 2.0 * it[q].m * (double)it[q].n * it[q].k;
  return f;
}

// The device part of dpgo_team_marginal_covariances_nested for a plan in which some robot is split.  DPGO_OK, DPGO_ERR
// (message set), or 1: a pivot was not positive -- fail[0] the block (-1: the separator), fail[1] the team pose, fail[2] the
// row of that factor.  The outputs are written only when every factorisation succeeded.
// app: Sigma applied to vectors beside the blocks (covariance_apply.h); with one, any plan is valid -- an unsplit one, whose
// blocks are the robots' interiors, and one block with an empty separator included.  Without one the launches are the same.
int covariance_nested_device(dpgo_team_t *t, const NestPlan &P, const double *T, int num_pairs, const int *pairs, double *cov_diag,
                             double *cov_pairs, dpgo_covariance_t *res, int *fail, CovEpilogue *epi, CovApply *app) {
  const int cols = app ? app->num_cols : 0;
  const char *what = "marginal_covariances_nested";
  const int N = P.N, nS = 6 * P.nS, nblk = (int)P.blocks.size();
  int kmax = 0;
  for (const NestPlan::Block &b : P.blocks) kmax = std::max(kmax, 6 * (int)b.nb.size());
  // ---- memory: refused before any device work
  const NestBytes nbytes = nest_bytes(t, P, num_pairs, cols);
  double avail = 0.0;
  {
    if (!cov_device_avail(t, &avail)) { set_err(std::string(what) + ": hipMemGetInfo failed"); return DPGO_ERR; }
    if (app && nbytes.large + nbytes.small + nbytes.apply > avail) {
      char buf[600];
      std::snprintf(buf, sizeof buf,
                    "%s: the nested path needs %.0f bytes for its large buffers (the temporaries of %d columns among them), %.0f for "
                    "the small ones and %.0f for V, X and r_S (8 x (12 N + 6 |S|) x num_cols, N = %d, |S| = %d), %.0f are available on "
                    "the device",
                    what, nbytes.large, cols, nbytes.small, nbytes.apply, N, P.nS, avail);
      set_err(buf);
      return DPGO_ERR;
    }
    if (nbytes.large + nbytes.small > avail) {
      const bool by_sep = nbytes.sep >= nbytes.ws_min;
      const NestPlan::Block &wb = P.blocks[nbytes.ws_block];
      char who[200], buf[600];
      if (by_sep) std::snprintf(who, sizeof who, "the separator of %d poses", P.nS);
      else
        std::snprintf(who, sizeof who, "the batch workspace of block %d (%zu poses of robot %d, coupled to %zu separator poses)",
                      nbytes.ws_block, wb.poses.size(), t->ag[wb.robot]->id, wb.nb.size());
      std::snprintf(buf, sizeof buf,
                    "%s: the nested path needs %.0f bytes for its large buffers and %.0f for the small ones, set by %s, %.0f are "
                    "available on the device; another max_block changes the figure (a smaller one shrinks the blocks and grows the "
                    "separator, a larger one the reverse)",
                    what, nbytes.large, nbytes.small, who, avail);
      set_err(buf);
      return DPGO_ERR;
    }
  }
  // the workspace of a batch: what is left beside everything else, at most 2 GiB, at least the largest block
  const double ws_cap = std::max(nbytes.ws_min, std::min((double)((size_t)1 << 28), 0.5 * (avail - nbytes.large - nbytes.small - nbytes.apply) / 8.0 + nbytes.ws_min));
  const std::vector<int> bbeg = nest_batches(P, ws_cap, cols);
  const int nbatch = (int)bbeg.size() - 1;
  // ---- the work lists.  Every stored block of the team-wide Q outside pose 0's row and column is one of: two poses of one
  // block (H_bb), a block's pose and a separator pose of its N_b (B_b, or its mirror, dropped), two separator poses.  Symmetric
  // targets keep bi <= bj (the row-owner rule of covariance_schur.hip).  Lists: [0, nblk) the blocks, nblk: H_SS.
  SchurItems L;
  auto classify = [&](int bi, int bj, int agent, int idx) -> int {
    if (bi == 0 || bj == 0) return 0;
    const int ci = P.block_of[bi], cj = P.block_of[bj];
    if (ci < 0 && cj < 0) { if (bi <= bj) L.add(nblk, bi, bj, agent, idx, P.pos[bi], P.pos[bj], CD_MIRROR); }
    else if (ci >= 0 && cj >= 0) {
      if (ci != cj) return -1;
      if (bi <= bj) L.add(ci, bi, bj, agent, idx, P.pos[bi], P.pos[bj], CD_MIRROR, 2 * ci);
    } else if (ci >= 0) {
      const std::vector<int> &nb = P.blocks[ci].nb;
      const auto at = std::lower_bound(nb.begin(), nb.end(), P.pos[bj]);
      if (at == nb.end() || *at != P.pos[bj]) return -1;
      L.add(ci, bi, bj, agent, idx, P.pos[bi], (int)(at - nb.begin()), bi > bj ? (CD_FLIP | CD_TRANS) : 0, 2 * ci + 1);
    }
    return 0;
  };
  if (cov_for_each_stored_block(t, P.offs, classify)) { set_err(std::string(what) + ": a stored block lies outside the plan's sets"); return DPGO_ERR; }
  L.finish(nblk + 1);
  // ---- the outputs asked for, by case.  Block numbers: [0, N) the diagonal blocks, N + k pair k.  keep and same are in
  // block order (the blocks of a batch are one range of either list)
  CovOutputs O;
  cov_classify_outputs(N, nblk, pairs, num_pairs, [&](int g) { return P.block_of[g]; }, P.pos, O);
  std::vector<CovBlk> keep_list, same_list;
  std::vector<int> keep_beg(nblk + 1, 0), same_beg(nblk + 1, 0);
  for (int b = 0; b < nblk; ++b) {
    keep_list.insert(keep_list.end(), O.keep[b].begin(), O.keep[b].end());
    same_list.insert(same_list.end(), O.same[b].begin(), O.same[b].end());
    keep_beg[b + 1] = (int)keep_list.size();
    same_beg[b + 1] = (int)same_list.size();
  }
  // ---- device storage
  const size_t SS = (size_t)nS * nS;
  const size_t cross_chunk = cov_cross_chunk(O.cross.size(), kmax);
  // the batch workspace: the largest batch as the batches were cut
  double ws_need = 0.0;
  for (int q = 0; q < nbatch; ++q) {
    double u = 0.0;
    for (int b = bbeg[q]; b < bbeg[q + 1]; ++b) u += nest_block_ws(P.blocks[b], cols);
    ws_need = std::max(ws_need, u);
  }
  CovFrame F(t);
  DevBuf<double> d_S, d_Wk, d_M, d_W, d_ws, d_t;
  DevBuf<int> d_int;
  DevBuf<CovItem> d_items;
  DevBuf<CovSrc> d_src;
  DevBuf<CovDst> d_dst;
  DevBuf<NestTarget> d_tgt;
  DevBuf<GemmItem> d_gemm;
  DevBuf<CovBlock> d_tab;
  DevBuf<CovBlk> d_keep, d_same, d_pub, d_is;
  DevBuf<CovCross> d_cross;
  DevBuf<double> d_V, d_X, d_rS;
  DevBuf<int> d_aint;
  DevBuf<ApplyItem> d_app;
  // d_int: the team pose of every interior index (block after block), the N_b
  std::vector<int> ints;
  std::vector<size_t> ipose_at(nblk), nb_at(nblk), w_at(nblk + 1, 0);
  for (int b = 0; b < nblk; ++b) {
    ipose_at[b] = ints.size();
    ints.insert(ints.end(), P.blocks[b].poses.begin(), P.blocks[b].poses.end());
    nb_at[b] = ints.size();
    ints.insert(ints.end(), P.blocks[b].nb.begin(), P.blocks[b].nb.end());
    w_at[b + 1] = w_at[b] + (size_t)36 * P.blocks[b].poses.size() * P.blocks[b].nb.size();
  }
  hipStream_t s = t->stream;
  const bool bad = d_S.alloc(SS) || d_Wk.alloc(SS) || d_M.alloc(SS) || d_W.alloc(w_at[nblk]) || d_ws.alloc((size_t)ws_need) ||
                   d_t.alloc(cross_chunk * 6 * std::max(kmax, 1)) || d_int.upload(ints, s) ||
                   d_items.upload(L.items, s) || d_src.upload(L.srcs, s) || d_dst.upload(L.dsts, s) || d_tgt.alloc((size_t)2 * nblk) ||
                   d_gemm.alloc((size_t)3 * nblk) || d_tab.alloc(nblk) || d_keep.upload(keep_list, s) || d_same.upload(same_list, s) ||
                   d_pub.upload(O.pub, s) || d_is.upload(O.is, s) || d_cross.upload(O.cross, s);
  auto nomem = [&]() {
    set_err(std::string(what) + ": device allocation failed (the nested path needs " + std::to_string((long long)(nbytes.large + nbytes.small)) +
            " bytes)");
    return DPGO_ERR;
  };
  if (bad) return nomem();
  // Sigma applied to vectors.  d_aint: the team poses of the separator, then of every N_b (the row maps of the tile)
  std::vector<int> aints;
  std::vector<size_t> nbp_at(nblk, 0);
  const size_t vx = (size_t)6 * N * cols;
  if (app) {
    aints = P.sep;
    for (int b = 0; b < nblk; ++b) {
      nbp_at[b] = aints.size();
      for (int k : P.blocks[b].nb) aints.push_back(P.sep[k]);
    }
    if (d_V.alloc(vx) || d_X.alloc(vx) || d_rS.alloc((size_t)nS * cols) || d_aint.upload(aints, s) || d_app.alloc((size_t)3 * nblk + 1))
      return nomem();
  }
  // the tables of the blocks.  Workspace of block b inside its batch: A | Wk | M | B (later Z) | P (later G) | W_b^T v_b (app)
  std::vector<NestTarget> tgt(2 * (size_t)nblk);
  std::vector<GemmItem> gemm(3 * (size_t)nblk);  // [0, nblk) W = C B, [nblk, 2 nblk) P = B^T W, [2 nblk, 3 nblk) Z = W G
  std::vector<CovBlock> tab(nblk);
  std::vector<double *> pA(nblk), pWk(nblk), pM(nblk), pP(nblk), pEnd(nblk);
  // [0, nblk) u_b = C_b v_b, [nblk, 2 nblk) t_b = W_b^T v_b, [2 nblk, 3 nblk) x_b -= W_b x_S[N_b], 3 nblk: x_S = Sigma_SS r_S
  std::vector<ApplyItem> aitem(app ? 3 * (size_t)nblk + 1 : 0);
  std::vector<int> order(nblk);
  for (int q = 0; q < nbatch; ++q) {
    double *w = d_ws.p;
    for (int b = bbeg[q]; b < bbeg[q + 1]; ++b) {
      const int n = 6 * (int)P.blocks[b].poses.size(), K = 6 * (int)P.blocks[b].nb.size();
      const size_t nn = (size_t)n * n, nK = (size_t)n * K;
      double *A = w, *Wk = A + nn, *M = Wk + nn, *B = M + nn, *Pm = B + nK;
      double *Tm = Pm + (size_t)K * K;
      w = Tm + (size_t)K * cols;
      pEnd[b] = w;
      double *W = d_W.p + w_at[b];
      pA[b] = A; pWk[b] = Wk; pM[b] = M; pP[b] = Pm; order[b] = n;
      tgt[2 * b] = {A, n, 0};
      tgt[2 * b + 1] = {B, n, 0};
      gemm[b] = {M, B, W, n, n, n, n, K, n};
      gemm[nblk + b] = {B, W, Pm, n, n, K, K, K, n};
      gemm[2 * nblk + b] = {W, Pm, B, n, K, n, n, K, K};
      tab[b] = {W, d_int.p + nb_at[b], d_int.p + ipose_at[b], M, Pm, B, n, K};
      if (app) {
        const int *poses = d_int.p + ipose_at[b], *nbp = d_aint.p + nbp_at[b];
        aitem[b] = {M, d_V.p, d_X.p, poses, poses, n, 6 * N, 6 * N, n, cols, n};
        aitem[nblk + b] = {W, d_V.p, Tm, poses, nullptr, n, 6 * N, K, K, cols, n};
        aitem[2 * nblk + b] = {W, d_X.p, d_X.p, nbp, poses, n, 6 * N, 6 * N, n, cols, K};
      }
    }
  }
  if (app) {
    aitem[3 * nblk] = {d_M.p, d_rS.p, d_X.p, nullptr, d_aint.p, nS, nS, 6 * N, nS, cols, nS};
    HIPC(hipMemcpyAsync(d_app.p, aitem.data(), sizeof(ApplyItem) * aitem.size(), hipMemcpyHostToDevice, s));
  }
  HIPC(hipMemcpyAsync(d_tgt.p, tgt.data(), sizeof(NestTarget) * tgt.size(), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_gemm.p, gemm.data(), sizeof(GemmItem) * gemm.size(), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_tab.p, tab.data(), sizeof(CovBlock) * tab.size(), hipMemcpyHostToDevice, s));
  if (const int rc = F.begin(T, nblk + 1, num_pairs, true)) return rc > 0 ? nomem() : DPGO_ERR;
  double *Td = F.Td, *lam = F.lam, *stat = F.stat, *keepd = F.keepd, *outd = F.outd;
  SchurMarks &marks = F.marks;
  std::vector<size_t> app_marks;  // the marks that END an interval of the apply's own launches
  if (app) {
    HIPC(hipMemsetAsync(d_X.p, 0, sizeof(double) * vx, s));
    if (app->rhs(Td, N, d_V.p, s)) return DPGO_ERR;
    launch_apply_gather(s, d_V.p, (size_t)6 * N, d_aint.p, P.nS, cols, d_rS.p);  // r_S = v_S
    HIPC(hipGetLastError());
    MARK(-1);
  }
  if (nS > 0) {
    HIPC(hipMemsetAsync(d_S.p, 0, sizeof(double) * SS, s));
    launch_cov_assemble_map(s, t->d_agents.p, d_items.p + L.lbeg[nblk], d_src.p, d_dst.p + L.lbeg[nblk], L.count(nblk), Td, lam, d_S.p, nS);
  }
  HIPC(hipGetLastError());
  MARK(0);
  // ---- the blocks, a batch at a time
  double flops_fact = 0.0, flops_prod = 0.0;
  for (int q = 0; q < nbatch; ++q) {
    const int b0 = bbeg[q], b1 = bbeg[q + 1], cnt = b1 - b0;
    const size_t used = (size_t)(pEnd[b1 - 1] - d_ws.p);
    HIPC(hipMemsetAsync(d_ws.p, 0, sizeof(double) * used, s));
    const int i0 = L.lbeg[b0], ni = L.lbeg[b1] - i0;
    if (ni > 0)
      k_nest_assemble<<<(unsigned)((ni + 255) / 256), 256, 0, s>>>(t->d_agents.p, d_items.p + i0, d_src.p, d_dst.p + i0, ni, Td, lam, d_tgt.p);
    HIPC(hipGetLastError());
    MARK(0);
    // (the failing matrix comes back through fail_at: a batch holds more blocks than the return code has room for)
    int fail_at = 0;
    const int f = dense_spd_inverse_batched(s, cnt, pA.data() + b0, pWk.data() + b0, pM.data() + b0, order.data() + b0, true,
                                            &fail_at);  // (synchronises)
    HIPC(hipGetLastError());
    if (f < 0) { set_err(std::string(what) + ": scratch allocation of the inverse failed"); return DPGO_ERR; }
    if (f > 0) {
      const int b = b0 + fail_at, row = f - 1;
      if (fail_at < 0 || fail_at >= cnt || row >= order[b]) {
        set_err(std::string(what) + ": the inverse reported a pivot outside its batch");
        return DPGO_ERR;
      }
      fail[0] = b; fail[1] = P.blocks[b].poses[row / 6]; fail[2] = row;
      return 1;
    }
    for (int b = b0; b < b1; ++b) {
      if (launch_cov_logdet(s, pA[b], order[b], stat + 4 * b)) return DPGO_ERR;
      flops_fact += (double)order[b] * order[b] * order[b];
    }
    MARK(1);
    launch_dgemm_batched(s, false, d_gemm.p + b0, gemm.data() + b0, cnt, false);               // W_b = C_b B_b
    launch_dgemm_batched(s, true, d_gemm.p + nblk + b0, gemm.data() + nblk + b0, cnt, false);  // P_b = B_b^T W_b
    for (int b = b0; b < b1; ++b) {                                                           // S_c[N_b, N_b] -= P_b, in block order
      const size_t kk = (size_t)tab[b].K * tab[b].K;
      if (kk > 0) k_nest_scatter_sub<<<(unsigned)((kk + 255) / 256), 256, 0, s>>>(d_S.p, nS, pP[b], tab[b].K, tab[b].nb);
    }
    HIPC(hipGetLastError());
    MARK(2);
    flops_prod += gemm_flops(gemm.data() + b0, cnt) + gemm_flops(gemm.data() + nblk + b0, cnt);
    if (app) {
      launch_apply_gemm(s, false, d_app.p + b0, aitem.data() + b0, cnt, false);               // u_b = C_b v_b, into X
      launch_apply_gemm(s, true, d_app.p + nblk + b0, aitem.data() + nblk + b0, cnt, false);  // t_b = W_b^T v_b
      for (int b = b0; b < b1; ++b)                                                           // r_S[N_b] -= t_b, in block order
        launch_apply_scatter_sub(s, d_rS.p, (size_t)nS, aitem[nblk + b].C, tab[b].K, cols, tab[b].nb);
      HIPC(hipGetLastError());
      MARK(-1);
      app_marks.push_back(marks.ev.size() - 1);
      app->flops += apply_flops(aitem.data() + b0, cnt) + apply_flops(aitem.data() + nblk + b0, cnt);
    }
    const int k0 = keep_beg[b0], nk = keep_beg[b1] - k0;  // (never empty: the diagonal blocks)
    launch_ext_keep(s, d_tab.p, d_keep.p + k0, nk, keepd);
    HIPC(hipGetLastError());
    MARK(4);
  }
  // ---- the separator
  if (nS > 0) {
    launch_schur_mirror(s, d_S.p, nS);
    HIPC(hipGetLastError());
    const int f = dense_spd_inverse(s, d_S.p, d_Wk.p, d_M.p, nS);
    HIPC(hipGetLastError());
    if (f < 0) { set_err(std::string(what) + ": scratch allocation of the inverse failed"); return DPGO_ERR; }
    if (f > 0) { fail[0] = -1; fail[1] = P.sep[(f - 1) / 6]; fail[2] = f - 1; return 1; }
    if (launch_cov_logdet(s, d_S.p, nS, stat + 4 * nblk)) return DPGO_ERR;
    MARK(3);
    launch_ext_public(s, d_M.p, nS, d_pub.p, (int)O.pub.size(), outd);
    HIPC(hipGetLastError());
    MARK(4);
    if (app) {
      launch_apply_gemm(s, false, d_app.p + 3 * nblk, aitem.data() + 3 * nblk, 1, false);  // x_S = Sigma_SS r_S, into X
      for (int q = 0; q < nbatch; ++q)                                                     // x_b = u_b - W_b x_S[N_b]
        launch_apply_gemm(s, false, d_app.p + 2 * nblk + bbeg[q], aitem.data() + 2 * nblk + bbeg[q], bbeg[q + 1] - bbeg[q], true);
      HIPC(hipGetLastError());
      MARK(-1);
      app_marks.push_back(marks.ev.size() - 1);
      app->flops += apply_flops(aitem.data() + 2 * nblk, nblk + 1);
    }
  }
  // ---- the interior blocks, by the same batches: Sigma_SS[N_b, N_b], Z_b = W_b Sigma_SS[N_b, N_b], the diagonal blocks and the
  // pairs inside a block
  for (int q = 0; q < nbatch; ++q) {
    const int b0 = bbeg[q], b1 = bbeg[q + 1], cnt = b1 - b0;
    int mk = 0, mld = 0;
    for (int b = b0; b < b1; ++b) { mk = std::max(mk, tab[b].K); mld = std::max(mld, tab[b].ld); }
    launch_ext_gather(s, d_tab.p, b0, cnt, mk, d_M.p, nS);
    launch_dgemm_batched(s, false, d_gemm.p + 2 * nblk + b0, gemm.data() + 2 * nblk + b0, cnt, false);
    HIPC(hipGetLastError());
    MARK(2);
    flops_prod += gemm_flops(gemm.data() + 2 * nblk + b0, cnt);
    launch_ext_diag(s, d_tab.p, b0, cnt, mld, keepd, outd);
    const int s0 = same_beg[b0];
    launch_ext_pair_same(s, d_tab.p, d_same.p + s0, same_beg[b1] - s0, keepd, outd);
    HIPC(hipGetLastError());  // (the workspace serves the next batch: its launches are ordered behind these on the stream)
    MARK(4);
  }
  launch_ext_pair_is<RowList>(s, d_tab.p, d_M.p, nS, d_is.p, (int)O.is.size(), outd);
  launch_ext_cross_pairs<RowList>(s, d_tab.p, d_M.p, nS, d_cross.p, O.cross.size(), kmax, d_t.p, cross_chunk, outd);
  HIPC(hipGetLastError());
  MARK(4);
  // log det and pivots: the blocks in order, the separator last
  std::vector<char> counted(nblk + 1, 1);
  counted[nblk] = nS > 0;
  if (app) app->X = d_X.p;
  if (F.finish(epi, res, cov_diag, cov_pairs, counted)) return DPGO_ERR;
  for (size_t k : app_marks) {
    float v = 0.f;
    if (hipEventElapsedTime(&v, marks.ev[k - 1], marks.ev[k]) == hipSuccess) app->ms_products += v;
  }
  const double *ms = F.ms;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr,
                 "marginal_covariances (nested): n %d, %d blocks (largest %d) in %d batches, separator %d (%d promoted poses), largest "
                 "N_b %d, %.0f bytes; assemble %.3f ms, factorisations %.3f ms (%.2f TFLOP/s), products %.3f ms (%.2f TFLOP/s), separator "
                 "inverse %.3f ms, extract %.3f ms\n",
                 6 * (N - 1), nblk, 6 * P.largest_block(), nbatch, nS, P.promoted, 6 * P.largest_nb(),
                 nbytes.large + nbytes.small + nbytes.apply + 8.0 * (ws_need - nbytes.ws_min), ms[0], ms[1], flops_fact / (1e9 * std::max(ms[1], 1e-9)), ms[2],
                 flops_prod / (1e9 * std::max(ms[2], 1e-9)), ms[3], ms[4]);
  return DPGO_OK;
}

int nest_max_block(int max_block) { return max_block > 0 ? max_block : DPGO_COV_NESTED_DEFAULT_BLOCK; }

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_covariance_nested_plan(int num_poses, const int *robot_of, const int *rowptr, const int *col, int max_block,
                                           int *block_of, int *info) {
  const char *what = "covariance_nested_plan";
  if (num_poses < 1 || !robot_of || !rowptr || !col) { set_err(std::string(what) + ": num_poses >= 1, robot_of, rowptr and col required"); return DPGO_ERR; }
  if (rowptr[0] != 0) { set_err(std::string(what) + ": rowptr[0] must be 0"); return DPGO_ERR; }
  for (int i = 0; i < num_poses; ++i)
    if (rowptr[i + 1] < rowptr[i]) { set_err(std::string(what) + ": rowptr must be non-decreasing"); return DPGO_ERR; }
  for (int p = 0; p < rowptr[num_poses]; ++p)
    if (col[p] < 0 || col[p] >= num_poses) { set_err(std::string(what) + ": column index out of range"); return DPGO_ERR; }
  // team order: robots 0, 1, ... each one contiguous range
  if (robot_of[0] != 0) { set_err(std::string(what) + ": robot_of[0] must be 0 (team order)"); return DPGO_ERR; }
  std::vector<int> offs(1, 0);
  for (int i = 1; i < num_poses; ++i) {
    if (robot_of[i] == robot_of[i - 1]) continue;
    if (robot_of[i] != robot_of[i - 1] + 1) { set_err(std::string(what) + ": robot_of must be non-decreasing without gaps (team order)"); return DPGO_ERR; }
    offs.push_back(i);
  }
  offs.push_back(num_poses);
  const int na = (int)offs.size() - 1;
  // public: a pose joined to a pose of another robot, either way round
  std::vector<char> pub(num_poses, 0);
  for (int i = 0; i < num_poses; ++i)
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p)
      if (robot_of[col[p]] != robot_of[i]) pub[i] = pub[col[p]] = 1;
  NestPlan P;
  nest_build(na, offs, pub, std::vector<int>(rowptr, rowptr + num_poses + 1), std::vector<int>(col, col + rowptr[num_poses]),
             nest_max_block(max_block), P);
  if (block_of) for (int i = 0; i < num_poses; ++i) block_of[i] = P.block_of[i];
  if (info) P.info(info);
  return DPGO_OK;
}

extern "C" int dpgo_team_covariance_nested_plan(dpgo_team_t *t, int max_block, int *block_of, int *info) {
  const char *what = "covariance_nested_plan";
  if (!t) { set_err(std::string(what) + ": null argument"); return DPGO_ERR; }
  if (check_team_local(t, what)) return DPGO_ERR;
  HIPC(hipSetDevice(t->device));
  if (check_team(t, what)) return DPGO_ERR;
  NestPlan P;
  nest_plan_team(t, nest_max_block(max_block), P);
  if (block_of) for (int i = 0; i < P.N; ++i) block_of[i] = P.block_of[i];
  if (info) P.info(info);
  return DPGO_OK;
}

extern "C" int dpgo_team_marginal_covariances_nested(dpgo_team_t *t, const double *T, int max_block, int num_pairs, const int *pairs,
                                                     double *cov_diag, double *cov_pairs, dpgo_covariance_t *res) {
  return marginal_covariances_nested_call(t, T, max_block, num_pairs, pairs, cov_diag, cov_pairs, res, nullptr);
}

int dpgo_cert::marginal_covariances_nested_call(dpgo_team_t *t, const double *T, int max_block, int num_pairs, const int *pairs,
                                                double *cov_diag, double *cov_pairs, dpgo_covariance_t *res, CovEpilogue *epi,
                                                CovApply *app) {
  const char *what = "marginal_covariances_nested";
  int N = 0;
  const int pre = covariance_host_checks(t, T, nullptr, num_pairs, pairs, cov_diag, cov_pairs, res, what, &N, epi != nullptr);
  if (pre != DPGO_OK) return pre > 0 ? DPGO_OK : pre;
  if (check_team(t, what)) return DPGO_ERR;
  NestPlan P;
  nest_plan_team(t, nest_max_block(max_block), P);
  // no robot is split: the sets are those of the robot-wise Schur path, and so is the call
  if (!P.split && !app) return marginal_covariances_call(t, T, DPGO_COV_SCHUR, num_pairs, pairs, cov_diag, cov_pairs, res, epi);
  int fail[3] = {0, 0, 0};
  const int rc = covariance_nested_device(t, P, T, num_pairs, pairs, cov_diag, cov_pairs, res, fail, epi, app);
  if (rc != DPGO_OK) std::memset(res, 0, sizeof *res);
  if (rc > 0) {
    set_err(pivot_message(what, fail[2], fail[0] < 0 ? "the Schur complement on the separator"
                                                     : "block " + std::to_string(fail[0]) + " of robot " + std::to_string(t->ag[P.blocks[fail[0]].robot]->id),
                          fail[1]));
    return DPGO_ERR;
  }
  return rc;
}

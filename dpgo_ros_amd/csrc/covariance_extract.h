// covariance_extract.h -- the extraction kernels of the marginal covariances: ONE text for the robot-wise Schur
// path (covariance_schur.hip, a set = a robot's interior) and for the nested path (covariance_nested.hip, a set = a block).
// Both hand the kernels a table of sets (CovBlock) and lists of output blocks (CovBlk, CovCross).  Column k of a set's W
// belongs to row 6 nb[k / 6] + k mod 6 of the separator's matrices.  A robot's part of the separator is a contiguous range,
// so the Schur path's nb is a window of one array 0, 1, 2, ... (`iota`), and 6 (off + k / 6) + k mod 6 = 6 off + k.  The two
// kernels whose threads walk a K loop through that map (k_ext_pair_is, k_ext_cross_t) are templates on it, RowList or RowRun.
// Every row product goes through schur_row_dot or a __builtin_fma loop in index order: the project's bitwise equalities
// (across == single team, nested unsplit == Schur, diagonal block == pair (i, i)) hold because there is one text.
// Loads of matrices, lists and index arrays go through gp(); the one exception is the record of a table (one per workgroup or
// per thread, 56 bytes), copied as a struct -- where the index is uniform (blockIdx) the compiler reads it through the scalar
// cache.  The kernels and their launch helpers are static: each file that includes this header compiles its own copy.
#pragma once
#include "covariance_schur.h"

namespace dpgo {

// set b on the device.  W: the kept W_b (ld x K, ld = 6 |I_b|, K = 6 |N_b|); nb: the |N_b| separator indices; ipose: the
// team pose of interior index li; M: C_b while the set is being eliminated; Z: Z_b (ld x K) while it is being extracted;
// G: Sigma_SS[N_b, N_b] (K x K) for k_ext_gather (the Schur path multiplies in place and leaves it null).  M, G and Z are
// work buffers that sets share in turn
struct CovBlock {
  const double *W;
  const int *nb, *ipose;
  double *M, *G, *Z;
  int ld, K;
};
static_assert(sizeof(CovBlock) == 56, "the byte formulas of include/dpgo_hip.h count 56 bytes");

// (the list entries of the extraction, CovBlk and CovCross, are plain host structs: schur_across_plan.h)

// row r of the separator's matrices for column k of a set's W: pose nb[k / 6], component k mod 6
__device__ __forceinline__ size_t cov_row(const int *__restrict__ nb, int k) { return (size_t)6 * gp(nb)[k / 6] + (size_t)(k % 6); }

// The row map of a set inside a K loop, the one parameter the kernels with such a loop are instantiated on.  RowList: any
// ascending index list, read at every k (the nested path).  RowRun: the list is a run of consecutive integers (a robot's part
// of the separator, a window of iota), read once: 6 (nb[0] + k / 6) + k mod 6 = 6 nb[0] + k -- the same row, so the same bits,
// without a dependent load in front of every term of a sum that a single thread runs through
struct RowList {
  const int *nb;
  __device__ __forceinline__ RowList(const int *__restrict__ p, int) : nb(p) {}
  __device__ __forceinline__ size_t operator()(int k) const { return cov_row(nb, k); }
};
struct RowRun {
  size_t r0;
  __device__ __forceinline__ RowRun(const int *__restrict__ p, int K) : r0(K > 0 ? (size_t)6 * gp(p)[0] : 0) {}
  __device__ __forceinline__ size_t operator()(int k) const { return r0 + (size_t)k; }
};

// keep[36 blk + 6 a + c] = C_b[6 i + a, 6 j + c], one thread per element
static __global__ __launch_bounds__(256) void k_ext_keep(const CovBlock *__restrict__ tab, const CovBlk *__restrict__ list, int count,
                                                         double *__restrict__ keep) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)36 * count) return;
  const int q = (int)(e % 36), a = q / 6, c = q - 6 * a;
  const int *lp = (const int *)(list + e / 36);
  const int blk = gp(lp)[0], b = gp(lp)[1], i = gp(lp)[2], j = gp(lp)[3];
  const CovBlock B = tab[b];
  gp(keep)[(size_t)36 * blk + q] = gp(B.M)[((size_t)6 * j + c) * B.ld + (size_t)6 * i + a];
}

// G_b = Sigma_SS[N_b, N_b] for the sets b0 + blockIdx.y (Sg: Sigma_SS, order n)
static __global__ __launch_bounds__(256) void k_ext_gather(const CovBlock *__restrict__ tab, int b0, const double *__restrict__ Sg, int n) {
  const CovBlock B = tab[b0 + blockIdx.y];
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)B.K * B.K) return;
  const int i = (int)(e % B.K), j = (int)(e / B.K);
  gp(B.G)[e] = gp(Sg)[cov_row(B.nb, j) * n + cov_row(B.nb, i)];
}

// the diagonal blocks of the interior poses of the sets b0 + blockIdx.y: X = C_ii + Z[i,:] W[i,:]^T, out = (X + X^T) / 2 (both
// operands of an element and of its mirror are the same two numbers: bitwise symmetric).  Thread e: row r = e mod ld of Z
// (pose r / 6, a = r mod 6: consecutive threads read consecutive rows), c = e / ld
static __global__ __launch_bounds__(256) void k_ext_diag(const CovBlock *__restrict__ tab, int b0, const double *__restrict__ keep,
                                                         double *__restrict__ out) {
  const CovBlock B = tab[b0 + blockIdx.y];
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)6 * B.ld) return;
  const int r = (int)(e % B.ld), c = (int)(e / B.ld), li = r / 6, a = r - 6 * li;
  const double sac = schur_row_dot(B.Z, B.ld, r, B.W, B.ld, 6 * li + c, B.K), sca = schur_row_dot(B.Z, B.ld, 6 * li + c, B.W, B.ld, r, B.K);
  const size_t o = (size_t)36 * gp(B.ipose)[li];
  gp(out)[o + 6 * a + c] = 0.5 * ((gp(keep)[o + 6 * a + c] + sac) + (gp(keep)[o + 6 * c + a] + sca));
}

// pairs of two interior poses of one set: out = C_ij + Z[i,:] W[j,:]^T
static __global__ __launch_bounds__(256) void k_ext_pair_same(const CovBlock *__restrict__ tab, const CovBlk *__restrict__ list, int count,
                                                              const double *__restrict__ keep, double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)36 * count) return;
  const int q = (int)(e % 36), a = q / 6, c = q - 6 * a;
  const int *lp = (const int *)(list + e / 36);
  const int blk = gp(lp)[0], b = gp(lp)[1], i = gp(lp)[2], j = gp(lp)[3];
  const CovBlock B = tab[b];
  const size_t o = (size_t)36 * blk + q;
  gp(out)[o] = gp(keep)[o] + schur_row_dot(B.Z, B.ld, 6 * i + a, B.W, B.ld, 6 * j + c, B.K);
}

// blocks of Sigma_SS (Sg, order n): f = 1 a diagonal block, symmetrised as k_cov_extract does; f = 0 the block (i, j)
static __global__ __launch_bounds__(256) void k_ext_public(const double *__restrict__ Sg, int n, const CovBlk *__restrict__ list, int count,
                                                           double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)36 * count) return;
  const int q = (int)(e % 36), a = q / 6, c = q - 6 * a;
  const int *lp = (const int *)(list + e / 36);
  const int blk = gp(lp)[0], i = gp(lp)[2], j = gp(lp)[3], f = gp(lp)[4];
  const size_t oi = (size_t)6 * i, oj = (size_t)6 * j;
  double v = gp(Sg)[(oj + c) * n + oi + a];
  if (f) v = 0.5 * (v + gp(Sg)[(oi + a) * n + oi + c]);
  gp(out)[(size_t)36 * blk + q] = v;
}

// interior pose i of set b with separator pose j: -W_b[i,:] Sigma_SS[N_b, j], k in index order (f: its transpose, the pair
// was (separator, interior))
template <class Row>
static __global__ __launch_bounds__(256) void k_ext_pair_is(const CovBlock *__restrict__ tab, const double *__restrict__ Sg, int n,
                                                            const CovBlk *__restrict__ list, int count, double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)36 * count) return;
  const int q = (int)(e % 36), a = q / 6, c = q - 6 * a;
  const int *lp = (const int *)(list + e / 36);
  const int blk = gp(lp)[0], b = gp(lp)[1], li = gp(lp)[2], sj = gp(lp)[3], f = gp(lp)[4];
  const CovBlock B = tab[b];
  const double *col = Sg + ((size_t)6 * sj + c) * n;
  const Row row(B.nb, B.K);
  double acc = 0.0;
  for (int k = 0; k < B.K; ++k) acc = __builtin_fma(gp(B.W)[(size_t)k * B.ld + 6 * li + a], gp(col)[row(k)], acc);
  gp(out)[(size_t)36 * blk + (f ? 6 * c + a : 6 * a + c)] = -acc;
}

// interior poses of two sets, first half: t[p][c][a] = sum_k W_a[6 li + a, k] Sigma_SS[N_a[k], N_b[c]] for the K_b columns
// c.  blockIdx.y: the pair of this chunk; a thread per column, the six rows at once (Sigma_SS is bitwise symmetric: the
// element is read at [N_b[c], N_a[k]], consecutive threads near-consecutive addresses)
template <class Row>
static __global__ __launch_bounds__(256) void k_ext_cross_t(const CovBlock *__restrict__ tab, const double *__restrict__ Sg, int n,
                                                            const CovCross *__restrict__ list, int kmax, double *__restrict__ tbuf) {
  const int *lp = (const int *)(list + blockIdx.y);
  const int ba = gp(lp)[1], li = gp(lp)[2], bb = gp(lp)[3];
  const CovBlock A = tab[ba], B = tab[bb];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= B.K) return;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double *w = A.W + 6 * li, *sg = Sg + cov_row(B.nb, c);
  const Row row(A.nb, A.K);
  for (int k = 0; k < A.K; ++k) {
    const double sv = gp(sg)[row(k) * n];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] = __builtin_fma(gp(w)[(size_t)k * A.ld + a], sv, acc[a]);
  }
  double *o = tbuf + ((size_t)blockIdx.y * kmax + c) * 6;
#pragma unroll
  for (int a = 0; a < 6; ++a) gp(o)[a] = acc[a];
}

// second half: out[a][c] = sum_l t[p][l][a] W_b[6 lj + c, l], l in index order
static __global__ __launch_bounds__(256) void k_ext_cross_out(const CovBlock *__restrict__ tab, const CovCross *__restrict__ list, int count,
                                                              int kmax, const double *__restrict__ tbuf, double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)36 * count) return;
  const int p = (int)(e / 36), q = (int)(e % 36), a = q / 6, c = q - 6 * a;
  const int *lp = (const int *)(list + p);
  const int blk = gp(lp)[0], bb = gp(lp)[3], lj = gp(lp)[4];
  const CovBlock B = tab[bb];
  const double *t = tbuf + (size_t)p * kmax * 6 + a;
  double acc = 0.0;
  for (int l = 0; l < B.K; ++l) acc = __builtin_fma(gp(t)[(size_t)6 * l], gp(B.W)[(size_t)l * B.ld + 6 * lj + c], acc);
  gp(out)[(size_t)36 * blk + q] = acc;
}

}  // namespace dpgo

namespace dpgo_cert {

// ---- one launch helper per kernel.  An empty grid is never launched: a list without entries, a range of sets whose largest
// interior (max_ld) or largest N_b (max_K) is empty is a skipped launch.  Errors are left to the caller's hipGetLastError.
static inline unsigned ext_grid(size_t threads) { return (unsigned)((threads + 255) / 256); }

static inline void launch_ext_keep(hipStream_t s, const CovBlock *tab, const CovBlk *list, int count, double *keep) {
  if (count > 0) k_ext_keep<<<ext_grid((size_t)36 * count), 256, 0, s>>>(tab, list, count, keep);
}
static inline void launch_ext_gather(hipStream_t s, const CovBlock *tab, int b0, int nsets, int max_K, const double *Sg, int n) {
  if (nsets > 0 && max_K > 0) k_ext_gather<<<dim3(ext_grid((size_t)max_K * max_K), nsets, 1), 256, 0, s>>>(tab, b0, Sg, n);
}
static inline void launch_ext_diag(hipStream_t s, const CovBlock *tab, int b0, int nsets, int max_ld, const double *keep, double *out) {
  if (nsets > 0 && max_ld > 0) k_ext_diag<<<dim3(ext_grid((size_t)6 * max_ld), nsets, 1), 256, 0, s>>>(tab, b0, keep, out);
}
static inline void launch_ext_pair_same(hipStream_t s, const CovBlock *tab, const CovBlk *list, int count, const double *keep, double *out) {
  if (count > 0) k_ext_pair_same<<<ext_grid((size_t)36 * count), 256, 0, s>>>(tab, list, count, keep, out);
}
static inline void launch_ext_public(hipStream_t s, const double *Sg, int n, const CovBlk *list, int count, double *out) {
  if (count > 0) k_ext_public<<<ext_grid((size_t)36 * count), 256, 0, s>>>(Sg, n, list, count, out);
}
template <class Row>
static inline void launch_ext_pair_is(hipStream_t s, const CovBlock *tab, const double *Sg, int n, const CovBlk *list, int count,
                                      double *out) {
  if (count > 0) k_ext_pair_is<Row><<<ext_grid((size_t)36 * count), 256, 0, s>>>(tab, Sg, n, list, count, out);
}
// (kmax = 0: no set is coupled to the separator, the blocks across two of them are the zeros already there)
template <class Row>
static inline void launch_ext_cross_t(hipStream_t s, const CovBlock *tab, const double *Sg, int n, const CovCross *list, int count, int kmax,
                                      double *tbuf) {
  if (count > 0 && kmax > 0) k_ext_cross_t<Row><<<dim3((kmax + 255) / 256, count, 1), 256, 0, s>>>(tab, Sg, n, list, kmax, tbuf);
}
static inline void launch_ext_cross_out(hipStream_t s, const CovBlock *tab, const CovCross *list, int count, int kmax, const double *tbuf,
                                        double *out) {
  if (count > 0 && kmax > 0) k_ext_cross_out<<<ext_grid((size_t)36 * count), 256, 0, s>>>(tab, list, count, kmax, tbuf, out);
}

// ---- the outputs asked for, by case.  Block numbers: [0, N) the diagonal blocks, N + k pair k.  keep[b]: the blocks of C_b
// to keep (the diagonal blocks of its poses and its pairs), same[b]: its pairs; pub: blocks of Sigma_SS; is: an interior
// and a separator pose; cross: interior poses of two sets
struct CovOutputs {
  std::vector<std::vector<CovBlk>> keep, same;
  std::vector<CovBlk> pub, is;
  std::vector<CovCross> cross;
};
// set_of(g): the set of team pose g (the robot for the Schur path, the block for the nested one), negative for a separator
// pose; pos[g]: its index inside its set (or the separator).  Pose 0 and every pair that names it stay the zeros
template <class SetOf>
void cov_classify_outputs(int N, int nsets, const int *pairs, int num_pairs, SetOf set_of, const std::vector<int> &pos, CovOutputs &o) {
  o.keep.assign(nsets, {});
  o.same.assign(nsets, {});
  for (int g = 1; g < N; ++g) {
    const int b = set_of(g);
    if (b < 0) o.pub.push_back({g, -1, pos[g], pos[g], 1, 0});
    else o.keep[b].push_back({g, b, pos[g], pos[g], 0, 0});
  }
  for (int k = 0; k < num_pairs; ++k) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1], blk = N + k;
    if (a == 0 || b == 0) continue;  // zeros
    const int ca = set_of(a), cb = set_of(b);
    if (ca < 0 && cb < 0) o.pub.push_back({blk, -1, pos[a], pos[b], 0, 0});
    else if (ca >= 0 && cb >= 0) {
      if (ca == cb) { o.keep[ca].push_back({blk, ca, pos[a], pos[b], 0, 0}); o.same[ca].push_back({blk, ca, pos[a], pos[b], 0, 0}); }
      else o.cross.push_back({blk, ca, pos[a], cb, pos[b], 0});
    } else if (ca >= 0) o.is.push_back({blk, ca, pos[a], pos[b], 0, 0});
    else o.is.push_back({blk, cb, pos[b], pos[a], 1, 0});
  }
}

// pairs between interiors of two sets handled by one launch pair: the scratch t (6 kmax doubles each) stays within 64 MB
// and the pair index, which rides on gridDim.y, within its limit of 65 535
static inline size_t cov_cross_chunk(size_t pairs, int kmax) {
  if (pairs == 0) return 0;
  return std::max<size_t>(1, std::min<size_t>({pairs, (size_t)65535, ((size_t)8 << 20) / ((size_t)6 * std::max(kmax, 1))}));
}

// the pairs of interior poses of two sets (list_d: the uploaded list of `count` entries), a chunk at a time
template <class Row>
static inline void launch_ext_cross_pairs(hipStream_t s, const CovBlock *tab, const double *Sg, int n, const CovCross *list_d, size_t count,
                                          int kmax, double *tbuf, size_t chunk, double *out) {
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const int cnt = (int)std::min<size_t>(chunk, count - c0);
    launch_ext_cross_t<Row>(s, tab, Sg, n, list_d + c0, cnt, kmax, tbuf);
    launch_ext_cross_out(s, tab, list_d + c0, cnt, kmax, tbuf, out);
  }
}

}  // namespace dpgo_cert

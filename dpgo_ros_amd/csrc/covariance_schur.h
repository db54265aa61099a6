// covariance_schur.h -- what the robot-wise Schur path (covariance_schur.hip) shares with the nested path
// (covariance_nested.hip): the destination record of the assembly through a pose map, the tile of the fp64 product, the
// partition into public and interior poses and the work lists.  The extraction kernels both paths launch are in
// covariance_extract.h, the frame of a call (marks, head, tail) in covariance_frame.h.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "certify_internal.h"
#include "covariance_block.h"
#include "covariance_frame.h"

namespace dpgo {

// where an item's block goes: block (r, c) of the launch's column-major target (leading dimension ld).  Hc = H_lo,hi is
// formed with bi as lo, or bj when CD_FLIP is set; the target receives Hc, or its transpose with CD_TRANS; with CD_MIRROR
// the other one goes to block (c, r) as well (symmetric targets list every pair of poses once).  tgt: the target's row in
// the table of a launch that fills several matrices (k_nest_assemble; k_cov_assemble_map has one target and ignores it)
struct CovDst {
  int r, c, f, tgt;
};
constexpr int CD_FLIP = 1, CD_TRANS = 2, CD_MIRROR = 4;

// ---- C = op(A) B (sub: C -= op(A) B), column-major, op(A) m x k (TA: A is k x m and transposed), B k x n, any m, n, k >= 1
// and leading dimensions.  One workgroup of 256 threads = 4 waves per 64 x 64 tile of C (the tile at rows i0, columns j0);
// a K slab of 32 is staged in LDS (zero padded past the edges), the next slab's loads are in flight under the products.
// v_mfma_f64_16x16x4_f64: operands A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], result
// D[row = (lane >> 4) + 4 reg][col = lane & 15] (the f64 map, not the f32 one).  As in dense_inverse.hip the instruction's
// ROW index carries the matrix COLUMN j and its column index the matrix row i, so the 16 lanes that share a result register
// store 16 consecutive rows of one column.  Wave w owns the quadrant rows 32 (w & 1), columns 32 (w >> 1) as 2 x 2 blocks of
// 16 x 16.  An element's sum runs over k in index order whatever tile it lies in -- and whatever launch the tile rides in:
// the single product (k_dgemm) and the batched one (k_dgemm_batched) both come through here.
constexpr int GK = 32;
typedef double v4f64_t __attribute__((ext_vector_type(4)));

template <bool TA>
__device__ __forceinline__ void dgemm_tile(const double *__restrict__ A, int lda, const double *__restrict__ B, int ldb,
                                           double *__restrict__ C, int ldc, int m, int n, int k, int sub, int i0, int j0) {
  __shared__ double As[GK][65], Bs[GK][65];
  const int tid = threadIdx.x;
  double ra[8], rb[8];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = tid + 256 * q;
      const int kb = t & 31, jb = t >> 5;  // B: consecutive threads run down a column of B
      const double vb = gp(B)[(size_t)min(j0 + jb, n - 1) * ldb + min(k0 + kb, k - 1)];
      rb[q] = (k0 + kb < k && j0 + jb < n) ? vb : 0.0;
      if (TA) {
        const double va = gp(A)[(size_t)min(i0 + jb, m - 1) * lda + min(k0 + kb, k - 1)];
        ra[q] = (k0 + kb < k && i0 + jb < m) ? va : 0.0;
      } else {
        const int ia = t & 63, ka = t >> 6;
        const double va = gp(A)[(size_t)min(k0 + ka, k - 1) * lda + min(i0 + ia, m - 1)];
        ra[q] = (k0 + ka < k && i0 + ia < m) ? va : 0.0;
      }
    }
  };
  v4f64_t acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = v4f64_t{0.0, 0.0, 0.0, 0.0};
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int ib = 32 * (wave & 1), jbase = 32 * (wave >> 1);
  load(0);
  for (int k0 = 0; k0 < k; k0 += GK) {
    __syncthreads();  // (the products of the slab before this one have read LDS)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = tid + 256 * q;
      Bs[t & 31][t >> 5] = rb[q];
      if (TA) As[t & 31][t >> 5] = ra[q];
      else As[t >> 6][t & 63] = ra[q];
    }
    __syncthreads();
    if (k0 + GK < k) load(k0 + GK);
#pragma unroll
    for (int kk = 0; kk < GK; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) { a[u] = Bs[kk + lk][jbase + 16 * u + li]; b[u] = As[kk + lk][ib + 16 * u + li]; }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[v], b[u], acc[u][v], 0, 0, 0);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + ib + 16 * u + li, j = j0 + jbase + 16 * v + lk + 4 * q;
        if (i < m && j < n) {
          double *c = C + (size_t)j * ldc + i;
          gp(c)[0] = sub ? gp(c)[0] - acc[u][v][q] : acc[u][v][q];
        }
      }
}

// sum_k Z[rz, k] W[rw, k], k in index order, one fused multiply-add per term: EVERY row product of the extraction goes
// through here, so a diagonal block and the pair (i, i) agree bitwise
__device__ __forceinline__ double schur_row_dot(const double *__restrict__ Z, size_t ldz, int rz, const double *__restrict__ W,
                                                size_t ldw, int rw, int K) {
  double s = 0.0;
  for (int k = 0; k < K; ++k) s = __builtin_fma(gp(Z)[(size_t)k * ldz + rz], gp(W)[(size_t)k * ldw + rw], s);
  return s;
}

}  // namespace dpgo

namespace dpgo_cert {

// k_cov_assemble_map over `count` items into the one target H (leading dimension ld); nothing to do when count is 0
void launch_cov_assemble_map(hipStream_t s, const AgentDev *agents, const CovItem *items, const CovSrc *src, const CovDst *dst, int count,
                             const double *T, const double *lam, double *H, int ld);
// the upper triangle of the n x n column-major A from its lower one (k_schur_mirror)
void launch_schur_mirror(hipStream_t s, double *A, int n);

// who is public, who is interior among a team's poses (SchurPartition, schur_across_plan.h)
void schur_partition(dpgo_team_t *t, int zero, SchurPartition &P);

// the work lists of the assembly: raw stored blocks, sorted by (list, block column, block row) and merged where they name
// the same pose pair (parallel edges, in record order)
struct SchurItems {
  struct Raw { int bi, bj, agent, idx, list; CovDst d; };
  std::vector<Raw> raw;
  std::vector<CovItem> items;
  std::vector<CovSrc> srcs;
  std::vector<CovDst> dsts;
  std::vector<int> lbeg;
  void add(int list, int bi, int bj, int agent, int idx, int r, int c, int f, int tgt = 0) {
    raw.push_back({bi, bj, agent, idx, list, {r, c, f, tgt}});
  }
  void finish(int nlists) {
    std::stable_sort(raw.begin(), raw.end(), [](const Raw &x, const Raw &y) {
      return x.list != y.list ? x.list < y.list : x.bj != y.bj ? x.bj < y.bj : x.bi < y.bi;
    });
    lbeg.assign(nlists + 1, 0);
    int cur = -1;
    for (const Raw &q : raw) {
      if (q.list == cur && items.back().bi == q.bi && items.back().bj == q.bj) ++items.back().count;
      else {
        while (cur < q.list) lbeg[++cur] = (int)items.size();
        items.push_back({q.bi, q.bj, (int)srcs.size(), 1});
        dsts.push_back(q.d);
      }
      srcs.push_back({q.agent, q.idx});
    }
    while (cur < nlists) lbeg[++cur] = (int)items.size();
  }
  int count(int list) const { return lbeg[list + 1] - lbeg[list]; }
};

}  // namespace dpgo_cert

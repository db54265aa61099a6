// covariance_apply.h -- Sigma applied to vectors on the factors a covariance path already holds: the product
// tile with row maps, the table record of a batched launch, and the launch helpers the paths call (covariance_apply.hip has
// the kernels and the public entry).
//
// X = Sigma V is the solve H_red X_red = V_red.  V and X are 6 N x m, column-major with leading dimension 6 N; rows
// 6 p .. 6 p + 5 belong to team pose p (rotation first, body frame; translation, world frame; pose 0 fixed: its rows of V are
// not read, its rows of X are zero bits).  On the nested path, with v_b the rows of block b and v_S those of the separator,
//     u_b = C_b v_b                                   (while C_b is live in its batch)
//     r_S = v_S - sum_b scatter_{N_b}(W_b^T v_b)      (one block after another in block order)
//     x_S = Sigma_SS r_S
//     x_b = u_b - W_b x_S[N_b]
// and on the dense path X_red = G V_red with the explicit inverse.  No block of Sigma is formed.
//
// The tile is dgemm_tile (covariance_schur.h) -- one workgroup of 256 threads per 64 x 64 tile of C, a K slab of 32 staged in
// LDS with the next slab's loads in flight under the products, v_mfma_f64_16x16x4_f64 with the operand map described there,
// an element's sum over k in index order whatever tile or launch it rides in -- with a ROW MAP on the B operand and on C: row r
// of a mapped operand is row 6 pose[r / 6] + r mod 6 of a 6 N-row matrix, the pose list being a block's `poses`, its N_b as
// team poses, the separator's poses, or none (the identity).  So the products read v_b straight out of V and write straight
// into X: no gathered copy of 6 N x m is made.  Loads go through gp(); no atomics.
#pragma once
#include "covariance_schur.h"

namespace dpgo {

// one product of a batch: C = op(A) B (sub: C -= op(A) B); bmap / cmap: the pose list of B's / C's rows, or null
struct ApplyItem {
  const double *A, *B;
  double *C;
  const int *bmap, *cmap;
  int lda, ldb, ldc, m, n, k;
};
static_assert(sizeof(ApplyItem) == 64, "the byte formula of include/dpgo_hip.h counts 64 bytes");

#if defined(__HIPCC__)

// row r of an operand through a pose list (null: the identity)
__device__ __forceinline__ size_t apply_row(const int *__restrict__ map, int r) {
  return map ? (size_t)6 * gp(map)[r / 6] + (size_t)(r % 6) : (size_t)r;
}

template <bool TA>
__device__ __forceinline__ void apply_tile(const double *__restrict__ A, int lda, const double *__restrict__ B, int ldb,
                                           const int *__restrict__ bmap, double *__restrict__ C, int ldc, const int *__restrict__ cmap,
                                           int m, int n, int k, int sub, int i0, int j0) {
  __shared__ double As[GK][65], Bs[GK][65];
  const int tid = threadIdx.x;
  double ra[8], rb[8];
  // a thread's row of B inside a slab is the same for its eight loads (t & 31 does not depend on q): one map lookup per slab
  const int kb = tid & 31;
  auto load = [&](int k0) {
    const size_t brow = apply_row(bmap, min(k0 + kb, k - 1));
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = tid + 256 * q;
      const int jb = t >> 5;  // B: consecutive threads run down a column of B
      const double vb = gp(B)[(size_t)min(j0 + jb, n - 1) * ldb + brow];
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
  for (int u = 0; u < 2; ++u) {
    const int i = i0 + ib + 16 * u + li;
    if (i >= m) continue;
    const size_t crow = apply_row(cmap, i);
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = j0 + jbase + 16 * v + lk + 4 * q;
        if (j < n) {
          double *c = C + (size_t)j * ldc + crow;
          gp(c)[0] = sub ? gp(c)[0] - acc[u][v][q] : acc[u][v][q];
        }
      }
  }
}

#endif  // __HIPCC__

}  // namespace dpgo

namespace dpgo_cert {

// k_apply_gemm over `count` items (items_h: their host copies, for the grid): the item rides on blockIdx.z, at most 65535
void launch_apply_gemm(hipStream_t s, bool ta, const dpgo::ApplyItem *items_d, const dpgo::ApplyItem *items_h, int count, bool sub);
// R[r, c] = V[6 pose[r / 6] + r mod 6, c]: the rows of `count` poses out of V (leading dimension ldv) into R (6 count x cols)
void launch_apply_gather(hipStream_t s, const double *V, size_t ldv, const int *pose, int count, int cols, double *R);
// R[6 nb[i / 6] + i mod 6, c] -= P[i, c], P K x cols with leading dimension K, R with leading dimension ldr.  One launch per
// block, in block order on one stream: two blocks that meet in a row of R subtract from it in that order
void launch_apply_scatter_sub(hipStream_t s, double *R, size_t ldr, const double *P, int K, int cols, const int *nb);
// D[drow(i), c] = S[srow(i), c] - P[i, c] over K rows and `cols` columns: S and D with leading dimensions lds and ldd and rows
// through the pose lists smap and dmap (null: the identity), P K x cols with leading dimension K (null: nothing is subtracted).
// Across teams: r_a = v_{S_a} - W_a^T v_a out of V into the robot's rows of r_S, and X[S_a] = x_S[S_a]
void launch_apply_rows_sub(hipStream_t s, const double *S, size_t lds, const int *smap, const double *P, double *D, size_t ldd,
                           const int *dmap, int K, int cols);
// the flops of a list of items
double apply_flops(const dpgo::ApplyItem *it, int count);

}  // namespace dpgo_cert

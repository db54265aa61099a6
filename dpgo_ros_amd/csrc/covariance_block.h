// covariance_block.h -- one 6 x 6 block of the Hessian H = J^T (S (x) I_3) J (covariance.hip has the derivation), shared by
// the dense assembly (k_cov_assemble, covariance.hip) and the assembly through a pose map (k_cov_assemble_map,
// covariance_schur.hip): both form a block by exactly these statements.
#pragma once
#include "kernel_common.h"

namespace dpgo {

// one block of H: block row bi, block column bj (team poses, both >= 1); its S block is the sum of `count` stored blocks
// src[first ..] in list order (parallel edges between two robots are separate shared-edge records)
struct CovItem {
  int bi, bj, first, count;
};
// where a stored block lives: idx >= 0 entry idx of the agent's block-CSR, idx < 0 shared-edge record ~idx
struct CovSrc {
  int agent, idx;
};

__device__ __forceinline__ int cov_eps(int a, int b, int c) { return ((a - b) * (b - c) * (c - a)) / 2; }

// Hc = H_lo,hi from S_lo,hi, R_lo, R_hi and, on the diagonal, Lambda_lo; a diagonal block is formed in its upper triangle and
// mirrored.  flip says which of bi, bj is lo: false bi (H_bi,bj is Hc), true bj (H_bi,bj is its transpose) -- the dense
// assembly passes bi > bj; bi and bj are rows of T (and, on the diagonal, of lam).
__device__ __forceinline__ void cov_form_block(const AgentDev *__restrict__ agents, const CovSrc *__restrict__ src, const CovItem &w,
                                               const double *__restrict__ T, const double *__restrict__ lam, double (*Hc)[6],
                                               const bool flip) {
  // S_bi,bj[cp][c] at s[cp + 4 c]
  double s[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) s[u] = 0.0;
  for (int k = 0; k < w.count; ++k) {
    const int *qs = (const int *)(src + w.first + k);
    const CovSrc q{gp(qs)[0], gp(qs)[1]};
    const AgentDev &ag = agents[q.agent];
    const double *bp = q.idx >= 0 ? ag.qval + (size_t)16 * q.idx : ag.se[~q.idx].coef;
    const double sg = q.idx >= 0 ? 1.0 : -1.0;
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
      const double2 v = ld2(bp + u);
      s[u] += sg * v.x;
      s[u + 1] += sg * v.y;
    }
  }
  const bool diag = w.bi == w.bj;
  const int lo = flip ? w.bj : w.bi, hi = flip ? w.bi : w.bj;
  // S_lo,hi[cp][c]
  double S[4][4];
#pragma unroll
  for (int cp = 0; cp < 4; ++cp)
#pragma unroll
    for (int c = 0; c < 4; ++c) S[cp][c] = flip ? s[c + 4 * cp] : s[cp + 4 * c];
  if (diag) {
    const double *L = lam + (size_t)9 * lo;
#pragma unroll
    for (int cp = 0; cp < 3; ++cp)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[cp][c] -= gp(L)[3 * cp + c];
  }
  double Rl[3][3], Rh[3][3];  // [b][c]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Rl[b][c] = gp(T)[((size_t)4 * lo + c) * 3 + b];
      Rh[b][c] = gp(T)[((size_t)4 * hi + c) * 3 + b];
    }
  double M[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) M[k][l] = Rl[0][k] * Rh[0][l] + Rl[1][k] * Rh[1][l] + Rl[2][k] * Rh[2][l];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double rr = 0.0, rt = 0.0, tr = 0.0;
#pragma unroll
      for (int cp = 0; cp < 3; ++cp) {
        if (cp == a) continue;
        const int k = 3 - a - cp;
        const double ea = (double)cov_eps(a, cp, k);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c == b) continue;
          const int l = 3 - b - c;
          rr += S[cp][c] * (ea * (double)cov_eps(b, c, l)) * M[k][l];
        }
        rt += S[cp][3] * ea * Rl[b][k];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c == b) continue;
        const int l = 3 - b - c;
        tr += S[3][c] * (double)cov_eps(b, c, l) * Rh[a][l];
      }
      Hc[a][b] = rr;
      Hc[a][3 + b] = rt;
      Hc[3 + a][b] = tr;
      Hc[3 + a][3 + b] = a == b ? S[3][3] : 0.0;
    }
  if (diag) {
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < a; ++b) Hc[a][b] = Hc[b][a];
  }
}

// the 6 x 6 block X (flip: its transpose) into a column-major matrix at `base` with leading dimension ld: six runs of 48
// contiguous, 16-byte aligned bytes (ld and the block offsets are multiples of 6)
__device__ __forceinline__ void cov_store_block(double *base, size_t ld, const double (*X)[6], bool flip) {
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    v2d_t *col = (v2d_t *)(base + (size_t)b * ld);
#pragma unroll
    for (int a = 0; a < 6; a += 2) {
      v2d_t v;
      v.x = flip ? X[b][a] : X[a][b];
      v.y = flip ? X[b][a + 1] : X[a + 1][b];
      gp(col)[a / 2] = v;
    }
  }
}

}  // namespace dpgo

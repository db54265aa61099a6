// certify.hip -- global-optimality certificate of a team's iterate (Rosen et al., SE-Sync; Tian et al., distributed
// certifiably correct PGO) and the staircase step that leaves a saddle.
//
// S(X) = Q - Lambda(X),  Lambda(X) = blockdiag_i [[Sym(Y_i^T (X Q)_i,rot), 0], [0, 0]]  (4 x 4 per pose).
// X is the global optimum of the pose-graph problem when S(X) is positive semidefinite (on the complement of the
// gauge directions).  The smallest eigenvalue of S is found by LOBPCG with the operator, the Gram matrices and the
// block updates on the device and a Rayleigh-Ritz problem of at most 3K x 3K on the host.
//
// Layout: a block of K vectors of R^{4N} is stored like an iterate, K x 4N column-major over the poses of the team in
// team order (local agent after local agent): element (b, column 4 g + c) at [(4 g + c) * ld + b], g = off[agent] + j.
// ld >= K lets one array hold several blocks (the basis [X; W; P] of the eigensolver is one 3K-row array).
//
// Every reduction is a Gram matrix A^T B: fixed column chunks per workgroup, one partial per chunk, summed in chunk
// order by ONE workgroup of a second launch -- two calls on the same inputs give the same bits.  The eigensolver's own
// Grams (gram_agents) chunk inside each agent and add the agents' totals in team order, so that robots split across
// teams (certify_across.hip) give the single team's bits.
// Nothing here writes a solver vector, a slab, a counter or a Nesterov state: the workspace is the team's d_cert.
#include "certify_internal.h"

namespace dpgo {

// OUT = V Q_a + G_a(V) - V Lambda_a  for every pose of every agent (blockIdx.y = agent), one lane per (pose, row b).
// lam == null: the Euclidean gradient product V Q_full alone.  The SpMM is the library's block product (spmm_row); the
// neighbour term reads the neighbour's rows of V itself when it is a local agent (src_agent_local >= 0), else from the
// halo of the calls across teams: halo[(4 (hoff[agent] + slot) + c) K + b] (certify_across.hip; null for one team).
template <int K>
__global__ __launch_bounds__(64) void k_cert_apply(const AgentDev *__restrict__ agents, const int *__restrict__ off,
                                                   const double *__restrict__ V, int ldv, double *__restrict__ out, int ldo,
                                                   const double *__restrict__ lam, const double *__restrict__ halo,
                                                   const int *__restrict__ hoff) {
  const int ai = blockIdx.y;
  const AgentDev &ag = agents[ai];
  constexpr int PPB = 64 / K;
  const int lane = threadIdx.x, lp = lane / K, b = lane - lp * K;
  const int j = blockIdx.x * PPB + lp;
  if (lp >= PPB || j >= ag.n) return;
  const int o = off[ai];
  double acc[1][4] = {{0.0, 0.0, 0.0, 0.0}};
  spmm_row<K, 1>(ag, j, [&](int i, double(*x)[4]) {
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) x[0][cp] = V[((size_t)4 * (o + i) + cp) * ldv + b];
  }, acc);
  const int e0 = ag.pose_eptr[j], e1 = ag.pose_eptr[j + 1];
  for (int e = e0; e < e1; ++e) {
    const SharedEdgeDev &se = ag.se[e];
    double x[4];
    if (se.src_agent_local >= 0) {
      const size_t nc = (size_t)4 * (off[se.src_agent_local] + se.src_frame);
#pragma unroll
      for (int cp = 0; cp < 4; ++cp) x[cp] = V[(nc + cp) * ldv + b];
    } else {
      const size_t hc = (size_t)4 * (hoff[ai] + se.slot);
#pragma unroll
      for (int cp = 0; cp < 4; ++cp) x[cp] = halo[(hc + cp) * K + b];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int cp = 0; cp < 4; ++cp) acc[0][c] -= x[cp] * se.coef[cp + 4 * c];
  }
  const size_t g = (size_t)(o + j);
  if (lam) {
    const double *L = lam + 9 * g;
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = V[(4 * g + c) * ldv + b];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int cp = 0; cp < 3; ++cp) acc[0][c] -= v[cp] * L[3 * cp + c];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) out[(4 * g + c) * ldo + b] = acc[0][c];
}

// Lambda_g = Sym(Y_g^T E_g,rot) from X and its Euclidean gradient E (both r rows, ld r), and the Gershgorin row sums of
// S (Q blocks, shared-edge blocks, Lambda): the largest of each workgroup's poses into gmax[agent * gstride + block]
template <int R>
__global__ __launch_bounds__(256) void k_cert_lambda(const AgentDev *__restrict__ agents, const int *__restrict__ off,
                                                     const double *__restrict__ X, const double *__restrict__ E,
                                                     double *__restrict__ lam, double *__restrict__ gmax, int gstride) {
  __shared__ double red[256];
  const int ai = blockIdx.y;
  const AgentDev &ag = agents[ai];
  const int j = blockIdx.x * 256 + threadIdx.x;
  double rmax = 0.0;
  if (j < ag.n) {
    const size_t g = (size_t)(off[ai] + j);
    double S[3][3];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < R; ++a) s += X[(4 * g + p) * R + a] * E[(4 * g + q) * R + a];
        S[p][q] = s;
      }
    double rs[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double l = 0.5 * (S[p][q] + S[q][p]);
        lam[9 * g + 3 * p + q] = l;
        rs[p] += fabs(l);
      }
    for (int p = ag.rowptr[j]; p < ag.rowptr[j + 1]; ++p) {
      const double *val = ag.qval + (size_t)16 * p;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) rs[c] += fabs(val[cp + 4 * c]);
    }
    for (int e = ag.pose_eptr[j]; e < ag.pose_eptr[j + 1]; ++e) {
      const double *cf = ag.se[e].coef;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) rs[c] += fabs(cf[cp + 4 * c]);
    }
    rmax = fmax(fmax(rs[0], rs[1]), fmax(rs[2], rs[3]));
  }
  red[threadIdx.x] = rmax;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) gmax[(size_t)ai * gstride + blockIdx.x] = red[0];
}

// partial Gram matrices: part[k][p * kb + q] = sum over chunk k's columns of A[p] B[q].  Chunk k covers the columns
// [c0s[k], cends[k]) -- at most CG_CH of them --, or without a table [k CG_CH, min((k + 1) CG_CH, ncols))
__global__ __launch_bounds__(256) void k_cert_gram(const double *__restrict__ A, int lda, int ka, const double *__restrict__ B,
                                                   int ldb, int kb, int ncols, const int *__restrict__ c0s,
                                                   const int *__restrict__ cends, double *__restrict__ part) {
  __shared__ double As[CG_CH * CG_MAXK], Bs[CG_CH * CG_MAXK];
  const int c0 = c0s ? c0s[blockIdx.x] : blockIdx.x * CG_CH, cend = c0s ? cends[blockIdx.x] : ncols, tid = threadIdx.x;
  for (int i = tid; i < CG_CH * ka; i += 256) {
    const int c = i / ka, p = i - c * ka;
    As[i] = (c0 + c < cend) ? A[(size_t)(c0 + c) * lda + p] : 0.0;
  }
  for (int i = tid; i < CG_CH * kb; i += 256) {
    const int c = i / kb, q = i - c * kb;
    Bs[i] = (c0 + c < cend) ? B[(size_t)(c0 + c) * ldb + q] : 0.0;
  }
  __syncthreads();
  const int m = ka * kb;
  for (int o = tid; o < m; o += 256) {
    const int p = o / kb, q = o - p * kb;
    double s = 0.0;
    for (int c = 0; c < CG_CH; ++c) s += As[c * ka + p] * Bs[c * kb + q];
    part[(size_t)blockIdx.x * m + o] = s;
  }
}

// ONE workgroup: group a's partials [gptr[a], gptr[a + 1]) in order into its total (kept in tot[a * m + o] when tot is
// given: what a participant across teams sends for its robots), then the groups' totals in order, from 0, into out[o].
// Without a table there is one group, the partials [0, ng): their plain sum in order.  With the agents as groups the
// order of additions does not depend on how the robots are split across teams
__global__ __launch_bounds__(256) void k_cert_gram_sum(const double *__restrict__ part, const int *__restrict__ gptr, int ng, int m,
                                                       double *__restrict__ tot, double *__restrict__ out) {
  const int groups = gptr ? ng : 1;
  for (int o = threadIdx.x; o < m; o += 256) {
    double s = 0.0;
    for (int a = 0; a < groups; ++a) {
      const int k0 = gptr ? gptr[a] : 0, k1 = gptr ? gptr[a + 1] : ng;
      double sa = 0.0;
      for (int k = k0; k < k1; ++k) sa += part[(size_t)k * m + o];
      if (tot) tot[(size_t)a * m + o] = sa;
      s += sa;
    }
    out[o] = s;
  }
}

// OUT = beta OUT + sum_t s_t A_t C_t (CertTerm: certify_internal.h)
__global__ __launch_bounds__(256) void k_cert_update(double *__restrict__ out, int ldo, int ko, double beta, CertTerms tm, int ncols) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)ncols * ko) return;
  const size_t col = e / ko;
  const int q = (int)(e - col * ko);
  double s = (beta != 0.0) ? beta * out[col * ldo + q] : 0.0;
  for (int u = 0; u < tm.n; ++u) {
    const CertTerm &T = tm.t[u];
    const double *a = T.A + col * T.lda;
    double acc = 0.0;
    if (T.C) {
      for (int p = 0; p < T.ka; ++p) acc += a[p] * T.C[p * ko + q];
    } else {
      acc = a[q];
    }
    s += T.s * acc;
  }
  out[col * ldo + q] = s;
}

// Cholesky G = L L^T of an n x n Gram matrix (one thread) -> C = L^-T (row-major: rows' new block X C^T ... see the host),
// i.e. C[p][q] = (L^-1)[q][p], so that X_new[q] = sum_p X[p] C[p][q] has orthonormal rows.  A pivot that is not positive
// raises *flag and leaves the identity.
__global__ void k_cert_chol(const double *__restrict__ G, int n, double *__restrict__ C, double *__restrict__ flag) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double L[CG_MAXK][CG_MAXK], Li[CG_MAXK][CG_MAXK];
  bool ok = true;
  for (int i = 0; i < n && ok; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = G[i * n + j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(s > 1e-300)) { ok = false; break; }
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  if (!ok) {
    *flag = 1.0;
    for (int p = 0; p < n; ++p)
      for (int q = 0; q < n; ++q) C[p * n + q] = (p == q) ? 1.0 : 0.0;
    return;
  }
  for (int j = 0; j < n; ++j)  // L^-1, column j by forward substitution
    for (int i = 0; i < n; ++i) {
      if (i < j) { Li[i][j] = 0.0; continue; }
      double s = (i == j) ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= L[i][k] * Li[k][j];
      Li[i][j] = s / L[i][i];
    }
  for (int p = 0; p < n; ++p)
    for (int q = 0; q < n; ++q) C[p * n + q] = Li[q][p];
}

// deflation basis Z = [rows of X; e_t] (r + 1 rows): e_t is 1 on every pose's translation coordinate
__global__ __launch_bounds__(256) void k_cert_zbasis(const double *__restrict__ X, int r, double *__restrict__ Z, int ncols) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ncols) return;
  for (int a = 0; a < r; ++a) Z[(size_t)col * (r + 1) + a] = X[(size_t)col * r + a];
  Z[(size_t)col * (r + 1) + r] = ((col & 3) == 3) ? 1.0 : 0.0;
}

// block-Jacobi preconditioner by agent without the tangent projection: OUT_a = V_a (Q_a + shift I)^-1 from the agent's
// dense inverse M, or its inverted 4 x 4 diagonal blocks.  Workgroup = one output column of one agent (blockIdx.y).
template <int K>
__global__ __launch_bounds__(256) void k_cert_precond(const AgentDev *__restrict__ agents, const int *__restrict__ off,
                                                      const double *__restrict__ V, int ldv, double *__restrict__ out, int ldo) {
  __shared__ double red[256 * K];
  const int ai = blockIdx.y;
  const AgentDev &ag = agents[ai];
  const int col = blockIdx.x, tid = threadIdx.x;
  if (col >= ag.N4) return;
  const size_t o4 = (size_t)4 * off[ai];
  double acc[K];
#pragma unroll
  for (int b = 0; b < K; ++b) acc[b] = 0.0;
  if (ag.M) {
    const double *Mc = ag.M + (size_t)col * ag.N4;
    for (int k = tid; k < ag.N4; k += 256) {
      const double m = Mc[k];
#pragma unroll
      for (int b = 0; b < K; ++b) acc[b] += V[(o4 + k) * ldv + b] * m;
    }
  } else if (tid == 0) {
    const int j = col >> 2, c = col & 3;
    const double *D = ag.Dinv + (size_t)16 * j;
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) {
      const double m = D[cp + 4 * c];
#pragma unroll
      for (int b = 0; b < K; ++b) acc[b] += V[(o4 + 4 * j + cp) * ldv + b] * m;
    }
  }
#pragma unroll
  for (int b = 0; b < K; ++b) red[b * 256 + tid] = acc[b];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int b = 0; b < K; ++b) red[b * 256 + tid] += red[b * 256 + tid + s];
    __syncthreads();
  }
  if (tid < K) out[(o4 + col) * ldo + tid] = red[tid * 256];
}

}  // namespace dpgo

// =================================================================================================
// host side
using namespace dpgo;
using namespace dpgo_host;
using namespace dpgo_cert;

namespace dpgo_cert {

void jacobi_eig(int n, std::vector<double> A, std::vector<double> &w, std::vector<double> &V) {
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const double a = A[(size_t)i * n + j] * A[(size_t)i * n + j];
        tot += a;
        if (i != j) off += a;
      }
    if (off <= 1e-32 * tot || off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < n; ++k) {  // A <- J^T A J
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - s * akq;
          A[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - s * aqk;
          A[(size_t)q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = c * vkp - s * vkq;
          V[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  std::vector<int> ord(n);
  for (int i = 0; i < n; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return A[(size_t)a * n + a] < A[(size_t)b * n + b]; });
  std::vector<double> V2((size_t)n * n);
  w.resize(n);
  for (int k = 0; k < n; ++k) {
    w[k] = A[(size_t)ord[k] * n + ord[k]];
    for (int i = 0; i < n; ++i) V2[(size_t)i * n + k] = V[(size_t)i * n + ord[k]];
  }
  V.swap(V2);
}

void launch_cert_apply3(hipStream_t s, const AgentDev *agents, const int *off, int na, int max_n, const double *V, double *out,
                        const double *lam, const double *halo, const int *hoff) {
  k_cert_apply<3><<<dim3(spmm_grid(3, max_n), na), 64, 0, s>>>(agents, off, V, 3, out, 3, lam, halo, hoff);
}

void launch_cert_lambda3(hipStream_t s, const AgentDev *agents, const int *off, int na, int max_n, const double *X,
                         const double *E, double *lam, double *gmax) {
  const int gstride = (max_n + 255) / 256;
  k_cert_lambda<3><<<dim3(gstride, na), 256, 0, s>>>(agents, off, X, E, lam, gmax, gstride);
}

int Cert::setup(int K_) {
  K = K_;
  r = t->prm.r;
  na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  max_n = 0;
  for (int k = 0; k < na; ++k) {
    offs[k + 1] = offs[k] + t->ag[k]->n;
    max_n = std::max(max_n, t->ag[k]->n);
  }
  N = offs[na];
  L = 4 * N;
  nblk = (L + CG_CH - 1) / CG_CH;
  // the chunks of the split-invariant Gram sums: 128 columns at a time inside each agent
  std::vector<int> ach(na + 1, 0), cc0, cce;
  for (int k = 0; k < na; ++k) {
    for (int c = 4 * offs[k]; c < 4 * offs[k + 1]; c += CG_CH) { cc0.push_back(c); cce.push_back(std::min(c + CG_CH, 4 * offs[k + 1])); }
    ach[k + 1] = (int)cc0.size();
  }
  nchunk = (int)cc0.size();
  gstride = (max_n + 255) / 256;
  const size_t Ls = (size_t)L;
  const size_t need = 2 * r * Ls + 9 * (size_t)N + 2 * (r + 1) * Ls + 4 * 3 * (size_t)K * Ls + 2 * (size_t)K * Ls +
                      (size_t)std::max(nblk, nchunk) * SLOT + 8 * (size_t)SLOT + (size_t)na * gstride +
                      8 * (size_t)na * SLOT + (x ? x->dev_doubles() : 0);
  const size_t ints = (size_t)2 * (na + 1) + 2 * (size_t)nchunk;
  if (t->d_cert.alloc(need) || t->d_cert_int.alloc(ints + (x ? x->dev_ints() : 0)) ||
      t->h_cert.alloc(5 * SLOT + (size_t)K * L)) {
    set_err("certificate: workspace allocation failed");
    if (!x) return DPGO_ERR;
    x->fail_local("certificate: workspace allocation failed");
  }
  if (!halted()) {
    double *p = t->d_cert.p;
    auto take = [&](size_t n) { double *q = p; p += n; return q; };
    Xt = take(r * Ls); E = take(r * Ls); lam = take(9 * (size_t)N);
    Zr = take((r + 1) * Ls); Zo = take((r + 1) * Ls);
    for (int b = 0; b < 2; ++b) { U[b] = take(3 * K * Ls); AU[b] = take(3 * K * Ls); }
    T = take(K * Ls); T2 = take(K * Ls);
    part = take((size_t)std::max(nblk, nchunk) * SLOT); G = take(8 * (size_t)SLOT); gmax = take((size_t)na * gstride);
    atot = take(8 * (size_t)na * SLOT);
    off = t->d_cert_int.p;
    achunk = off + na + 1; chunk0 = achunk + na + 1; chunkend = chunk0 + nchunk;
    if (x) x->place(p, off + ints, t->stream);
  }
  CERT_CK(*this, hipMemcpyAsync(off, offs.data(), sizeof(int) * (na + 1), hipMemcpyHostToDevice, t->stream));
  CERT_CK(*this, hipMemcpyAsync(achunk, ach.data(), sizeof(int) * (na + 1), hipMemcpyHostToDevice, t->stream));
  CERT_CK(*this, hipMemcpyAsync(chunk0, cc0.data(), sizeof(int) * nchunk, hipMemcpyHostToDevice, t->stream));
  CERT_CK(*this, hipMemcpyAsync(chunkend, cce.data(), sizeof(int) * nchunk, hipMemcpyHostToDevice, t->stream));
  CERT_CK(*this, hipStreamSynchronize(t->stream));  // (the tables are locals of this function)
  CERT_CK(*this, hipMemsetAsync(G, 0, sizeof(double) * 8 * SLOT, t->stream));
  // the team's iterate, gathered in team order (agent arrays are r x 4n each: ld r)
  for (int k = 0; k < na; ++k)
    CERT_CK(*this, hipMemcpyAsync(Xt + (size_t)4 * offs[k] * r, t->ag[k]->dev.buf[B_X], sizeof(double) * r * 4 * t->ag[k]->n,
                                  hipMemcpyDeviceToDevice, t->stream));
  apply(r, Xt, r, E, r, false);
  if (!halted())
    DPGO_DISPATCH_R(r, (k_cert_lambda<R><<<dim3(gstride, na), 256, 0, t->stream>>>(t->d_agents.p, off, Xt, E, lam, gmax, gstride)));
  CERT_CK(*this, hipGetLastError());
  return 0;
}

bool Cert::halted() const { return x && (x->bad || x->dead); }
bool Cert::dead() const { return x && x->dead; }

void Cert::reduce(std::initializer_list<std::pair<double *, int>> parts) {
  if (x) x->reduce(*this, parts);
}

void Cert::apply(int k, const double *V, int ldv, double *out, int ldo, bool with_lam) {
  const double *halo = nullptr;
  const int *hoff = nullptr;
  if (x) {
    halo = x->halo_of(*this, k, V, ldv);
    hoff = x->d_hoff;
    if (halted()) return;
  }
  const dim3 grid(spmm_grid(k, max_n), na);
  const double *lm = with_lam ? lam : nullptr;
  DPGO_DISPATCH_R(k, (k_cert_apply<R><<<grid, 64, 0, t->stream>>>(t->d_agents.p, off, V, ldv, out, ldo, lm, halo, hoff)));
}

void Cert::gram(const double *A, int lda, int ka, const double *B, int ldb, int kb, double *out) {
  if (halted()) return;
  k_cert_gram<<<nblk, 256, 0, t->stream>>>(A, lda, ka, B, ldb, kb, L, nullptr, nullptr, part);
  k_cert_gram_sum<<<1, 256, 0, t->stream>>>(part, nullptr, nblk, ka * kb, nullptr, out);
}

void Cert::gram_agents(const double *A, int lda, int ka, const double *B, int ldb, int kb, int slot_) {
  if (halted()) return;
  k_cert_gram<<<nchunk, 256, 0, t->stream>>>(A, lda, ka, B, ldb, kb, L, chunk0, chunkend, part);
  k_cert_gram_sum<<<1, 256, 0, t->stream>>>(part, achunk, na, ka * kb, atot + (size_t)slot_ * na * SLOT, slot(slot_));
}

void Cert::reduce_agents(std::initializer_list<std::pair<int, int>> parts) {
  if (x) x->reduce_agents(*this, parts);
}

void Cert::sum_partials(const double *p, int nblk_, int m, double *out) {
  if (halted()) return;
  k_cert_gram_sum<<<1, 256, 0, t->stream>>>(p, nullptr, nblk_, m, nullptr, out);
}

void Cert::update(double *out, int ldo, int ko, double beta, std::initializer_list<CertTerm> terms) {
  if (halted()) return;
  CertTerms tm{};
  for (const CertTerm &x : terms) tm.t[tm.n++] = x;
  const size_t cnt = (size_t)L * ko;
  k_cert_update<<<(unsigned)((cnt + 255) / 256), 256, 0, t->stream>>>(out, ldo, ko, beta, tm, L);
}

void Cert::project(double *V, int ld, int k) {
  if (!deflate) return;
  gram_agents(Zo, nz, nz, V, ld, k, 5);
  reduce_agents({{5, nz * k}});
  update(V, ld, k, 1.0, {CertTerm{Zo, slot(5), nz, nz, -1.0}});
}

void Cert::cholqr(double *V, int ld, int k, double *S) {
  gram_agents(V, ld, k, V, ld, k, 4);
  reduce_agents({{4, k * k}});
  if (!halted()) k_cert_chol<<<1, 64, 0, t->stream>>>(slot(4), k, slot(6), slot(3));
  update(S, k, k, 0.0, {CertTerm{V, slot(6), ld, k, 1.0}});
  update(V, ld, k, 0.0, {CertTerm{S, nullptr, k, k, 1.0}});
}

void Cert::precondition(const double *V, int ldv, double *out, int ldo) {
  if (halted()) return;
  DPGO_DISPATCH_R(K,(k_cert_precond<R><<<dim3(4 * max_n, na), 256, 0, t->stream>>>(t->d_agents.p, off, V, ldv, out, ldo)));
}

int check_team_local(dpgo_team_t *t, const char *what) {
  if ((int)t->ag.size() != t->prm.num_robots) {
    set_err(std::string(what) + ": the team must hold every robot (num_local == num_robots)");
    return DPGO_ERR;
  }
  for (auto &a : t->ag)
    if (a->state != DPGO_INITIALIZED || !a->has_X) {
      set_err(std::string(what) + ": robot " + std::to_string(a->id) + " is not initialized");
      return DPGO_ERR;
    }
  return 0;
}

int check_team(dpgo_team_t *t, const char *what) {
  if (check_team_local(t, what)) return DPGO_ERR;
  if (sync_descs(t)) return DPGO_ERR;
  for (auto &a : t->ag)
    for (const auto &d : a->se_host)
      if (d.src_agent_local < 0) {
        set_err(std::string(what) + ": robot " + std::to_string(a->id) + " has a neighbour outside the team");
        return DPGO_ERR;
      }
  return 0;
}

}  // namespace dpgo_cert

extern "C" {

int dpgo_team_certificate_apply(dpgo_team_t *t, int K, const double *V, double *out) {
  if (!t || !V || !out) { set_err("certificate_apply: null argument"); return DPGO_ERR; }
  if (K < 3 || K > 8) { set_err("certificate_apply: K must lie in 3..8"); return DPGO_ERR; }
  if (check_team(t, "certificate_apply")) return DPGO_ERR;
  Cert c;
  c.t = t;
  if (c.setup(K)) return DPGO_ERR;
  const size_t bytes = sizeof(double) * (size_t)K * c.L;
  HIPC(hipMemcpyAsync(c.T, V, bytes, hipMemcpyHostToDevice, t->stream));
  c.apply(K, c.T, K, c.T2, K, true);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(out, c.T2, bytes, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipStreamSynchronize(t->stream));
  return 0;
}

int dpgo_team_certificate_precondition(dpgo_team_t *t, int K, const double *V, double *out) {
  if (!t || !V || !out) { set_err("certificate_precondition: null argument"); return DPGO_ERR; }
  if (K < 3 || K > 8) { set_err("certificate_precondition: K must lie in 3..8"); return DPGO_ERR; }
  if (check_team(t, "certificate_precondition")) return DPGO_ERR;
  for (auto &a : t->ag)
    if (!a->dev.M && !a->dev.Dinv) {
      set_err("certificate_precondition: robot " + std::to_string(a->id) + " has the two-level form (no raw inverse to apply)");
      return DPGO_ERR;
    }
  Cert c;
  c.t = t;
  if (c.setup(K)) return DPGO_ERR;
  const size_t bytes = sizeof(double) * (size_t)K * c.L;
  HIPC(hipMemcpyAsync(c.T, V, bytes, hipMemcpyHostToDevice, t->stream));
  c.precondition(c.T, K, c.T2, K);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(out, c.T2, bytes, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipStreamSynchronize(t->stream));
  return 0;
}

}  // extern "C"

namespace dpgo_cert {

constexpr double CERT_PC_OFF = 1e-3;  // the preconditioner is left out below -CERT_PC_OFF s (certify_body)

// the state of the starting block's generator s <- 6364136223846793005 s + 1442695040888963407 after n steps, in O(log n)
static unsigned long long lcg_skip(unsigned long long s, unsigned long long n) {
  unsigned long long a = 6364136223846793005ull, c = 1442695040888963407ull, A = 1, C = 0;
  for (; n; n >>= 1) {
    if (n & 1) { A *= a; C = C * a + c; }
    c *= a + 1;
    a *= a;
  }
  return A * s + C;
}

// Across teams (c.x) every Gram matrix is summed over the participants before its first use (Cert::reduce, inside
// project / cholqr), the operator exchanges its halo (Cert::apply), and every host decision is taken right behind an
// allgather on the summed bits: all participants take the same branches and make the same transport calls.
int certify_body(Cert &c, double eta, double tol, int max_iters, int K, int flags, dpgo_certificate_t *out, double *v) {
#define CK(expr) CERT_CK(c, expr)
  dpgo_team_t *t = c.t;
  Across *x = c.x;
  c.deflate = !(flags & DPGO_CERT_NO_DEFLATION);
  c.precond = !(flags & DPGO_CERT_NO_PRECONDITIONER);
  for (auto &a : t->ag)
    if (!a->dev.M && !a->dev.Dinv) c.precond = false;  // (two-level agents: no raw apply of their operator)
  if (x && !x->all_precond) c.precond = false;         // (one decision for every participant)
  if (c.setup(K)) return DPGO_ERR;
  const int r = c.r, L = c.L, K3 = 3 * K;
  const size_t Ls = (size_t)L;

  // deflation basis, orthonormal.  Z may lose rank (an iterate of rank < r -- a lifted one, a rank-deficient optimum --
  // has dependent rows): it is orthonormalised through the eigenvectors of its Gram matrix, directions below 1e-12 of
  // the largest (unit-scaled rows) dropped, then once more by CholQR
  if (c.deflate) {
    const int z = r + 1;
    if (!c.halted()) k_cert_zbasis<<<(L + 255) / 256, 256, 0, t->stream>>>(c.Xt, r, c.Zr, L);
    c.gram_agents(c.Zr, z, z, c.Zr, z, z, 4);
    c.reduce_agents({{4, z * z}});
    if (c.dead()) return x->fail();
    std::vector<double> gz((size_t)z * z);
    CK(hipMemcpyAsync(gz.data(), c.slot(4), sizeof(double) * z * z, hipMemcpyDeviceToHost, t->stream));
    CK(hipStreamSynchronize(t->stream));
    std::vector<double> d(z), B((size_t)z * z), mu, Vz;
    for (int p = 0; p < z; ++p) d[p] = gz[p * z + p] > 0 ? 1.0 / std::sqrt(gz[p * z + p]) : 0.0;
    for (int p = 0; p < z; ++p)
      for (int q = 0; q < z; ++q) B[(size_t)p * z + q] = 0.5 * (gz[p * z + q] + gz[q * z + p]) * d[p] * d[q];
    jacobi_eig(z, B, mu, Vz);
    std::vector<int> keep;
    for (int k = 0; k < z; ++k) if (mu[k] > 1e-12 * mu[z - 1]) keep.push_back(k);
    c.nz = (int)keep.size();
    double *hc = t->h_cert.p + 4 * Cert::SLOT;
    for (int p = 0; p < z; ++p)
      for (int k = 0; k < c.nz; ++k) hc[p * c.nz + k] = d[p] * Vz[(size_t)p * z + keep[k]] / std::sqrt(mu[keep[k]]);
    CK(hipMemcpyAsync(c.slot(7), hc, sizeof(double) * z * c.nz, hipMemcpyHostToDevice, t->stream));
    c.update(c.Zo, c.nz, c.nz, 0.0, {CertTerm{c.Zr, c.slot(7), z, z, 1.0}});
    c.cholqr(c.Zo, c.nz, c.nz, c.Zr);
  }
  // a block of K independent vectors needs K dimensions outside Z: a team of one to three poses may not have them (the
  // projected starting block would be round-off, orthonormalised into vectors that are not in Z-perp at all).  Refused
  // here, on numbers every participant holds alike, before anything is iterated
  {
    const long long Lg = x ? 4ll * x->nglob : (long long)L;
    const long long dim = Lg - (c.deflate ? c.nz : 0);
    if (dim < K) {
      set_err("certify: the team is too small for the block size: 4N - nz = " + std::to_string(dim) + " dimensions (4N = " +
              std::to_string(Lg) + (c.deflate ? ", nz = " + std::to_string(c.nz) + " deflated" : std::string(", no deflation")) +
              ") are fewer than the block size " + std::to_string(K));
      if (x) x->finish();
      return DPGO_ERR;
    }
  }
  // starting block: fixed pseudo-random numbers (the call is a function of the iterate alone).  Across teams each
  // participant draws its own columns of the single team's block: the generator skipped ahead to the global position
  // (robots by id, then poses) of each of its robots
  if (!c.halted()) {
    double *h = t->h_cert.p + 5 * Cert::SLOT;  // (behind the coefficients, whose upload may still be queued)
    if (!x) {
      unsigned long long s = 0x2545F4914F6CDD1Dull;
      for (size_t i = 0; i < (size_t)K * Ls; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        h[i] = (double)(s >> 11) / 9007199254740992.0 - 0.5;
      }
    } else {
      size_t o = 0;
      for (auto &a : t->ag) {
        const size_t cnt = (size_t)K * 4 * a->n;
        unsigned long long s = lcg_skip(0x2545F4914F6CDD1Dull, (unsigned long long)K * 4 * x->robot_goff[a->id]);
        for (size_t i = 0; i < cnt; ++i) {
          s = s * 6364136223846793005ull + 1442695040888963407ull;
          h[o + i] = (double)(s >> 11) / 9007199254740992.0 - 0.5;
        }
        o += cnt;
      }
    }
    CK(hipMemcpyAsync(c.T, h, sizeof(double) * K * Ls, hipMemcpyHostToDevice, t->stream));
    CK(hipStreamSynchronize(t->stream));  // (the pinned image is reused for the read-backs)
  }
  int cur = 0;
  c.update(c.U[cur], K3, K, 0.0, {CertTerm{c.T, nullptr, K, K, 1.0}});
  c.project(c.U[cur], K3, K);
  c.cholqr(c.U[cur], K3, K, c.T);
  c.cholqr(c.U[cur], K3, K, c.T);
  CK(hipGetLastError());
  // Gershgorin bound on |S| (once per call)
  std::vector<double> gm((size_t)c.na * c.gstride);
  CK(hipMemcpyAsync(gm.data(), c.gmax, sizeof(double) * gm.size(), hipMemcpyDeviceToHost, t->stream));
  CK(hipStreamSynchronize(t->stream));
  double s_bound = 0.0;
  for (double g : gm) s_bound = std::max(s_bound, g);
  if (x) {
    std::vector<double> mine{0.0, s_bound};
    if (x->gather(mine, x->hall)) return x->fail();
    for (int q = 0; q < x->world; ++q) s_bound = std::max(s_bound, x->hall[2 * q + 1]);
  }
  const double eta_abs = (flags & DPGO_CERT_ETA_RELATIVE) ? eta * s_bound : eta;
  const double tol_abs = tol * s_bound;

  double *hG = t->h_cert.p;
  int status = -1, it = 0;
  double theta0 = 0.0, res0 = 0.0;
  std::vector<double> y0(K, 0.0);
  for (it = 0; it < max_iters; ++it) {
    if (c.dead()) return x->fail();
    double *U = c.U[cur], *AU = c.AU[cur];
    double *X = U, *W = U + K, *P = U + 2 * K, *AX = AU, *AW = AU + K;
    // AX = P S X;  R = AX - X (X^T AX)
    c.apply(K, X, K3, AX, K3, true);
    c.project(AX, K3, K);
    c.gram_agents(X, K3, K, AX, K3, K, 4);
    c.reduce_agents({{4, K * K}});
    c.update(W, K3, K, 0.0, {CertTerm{AX, nullptr, K3, K, 1.0}, CertTerm{X, c.slot(4), K3, K, -1.0}});
    c.gram_agents(W, K3, K, W, K3, K, 2);
    // T = (Q_a + shift I)^-1 stands for (S - theta I)^-1 near a critical point, where Lambda is small against Q and
    // theta is about 0.  Far from one (a Ritz value below -CERT_PC_OFF s, a thousand times the default eta) it inverts
    // another operator and slows the iteration: seeded random points with lambda_min = -0.3 s did not converge in 753
    // iterations with it, and do in 37 .. 66 without.  The Ritz value is the last iteration's, from summed bits: the
    // same decision on every participant.  Relative to s, so that neither the shift nor round-off about 0 decides it.
    const bool far_from_critical = it > 0 && theta0 < -CERT_PC_OFF * s_bound;
    if (c.precond && !far_from_critical) {
      c.precondition(W, K3, c.T, K);
      c.update(W, K3, K, 0.0, {CertTerm{c.T, nullptr, K, K, 1.0}});
    }
    c.project(W, K3, K);
    c.apply(K, W, K3, AW, K3, true);
    c.project(AW, K3, K);
    const int nb = it == 0 ? 2 * K : K3;
    c.gram_agents(U, K3, nb, AU, K3, nb, 0);
    c.gram_agents(U, K3, nb, U, K3, nb, 1);
    // (across teams: the residual Gram of slot 2 travels with the basis Grams -- the Cholesky word of slot 3 needs no
    // reduction, it comes from summed Grams and is the same on every participant)
    c.reduce_agents({{0, nb * nb}, {1, nb * nb}, {2, K * K}});
    if (c.dead()) return x->fail();
    CK(hipGetLastError());
    CK(hipMemcpyAsync(hG, c.G, sizeof(double) * 4 * Cert::SLOT, hipMemcpyDeviceToHost, t->stream));
    CK(hipStreamSynchronize(t->stream));
    if (hG[3 * Cert::SLOT] != 0.0) {
      set_err("certify: the block lost rank (Cholesky of its Gram matrix failed)");
      if (x) x->finish();  // (the same on every participant: the closing status word keeps the sequence)
      return DPGO_ERR;
    }
    const double *G1 = hG, *G2 = hG + Cert::SLOT, *Grr = hG + 2 * Cert::SLOT;
    // Ritz pairs of X: M = X^T S X (the X block of G1)
    std::vector<double> M((size_t)K * K), th, Y;
    for (int p = 0; p < K; ++p)
      for (int q = 0; q < K; ++q) M[(size_t)p * K + q] = 0.5 * (G1[p * nb + q] + G1[q * nb + p]);
    jacobi_eig(K, M, th, Y);
    theta0 = th[0];
    double rr = 0.0;
    for (int p = 0; p < K; ++p)
      for (int q = 0; q < K; ++q) rr += Y[(size_t)p * K] * Grr[p * K + q] * Y[(size_t)q * K];
    res0 = std::sqrt(std::max(rr, 0.0));
    for (int p = 0; p < K; ++p) y0[p] = Y[(size_t)p * K];
    // a Rayleigh quotient bounds lambda_min from above: below -eta proves there is negative curvature
    if (theta0 < -eta_abs) { status = 0; break; }
    if (res0 <= tol_abs) { status = 1; break; }
    if (it == max_iters - 1) break;
    // Rayleigh-Ritz on [X W P]: the basis scaled to unit columns, orthonormalised through the eigenvectors of its Gram
    // matrix (directions below 1e-10 of the largest dropped), then the small symmetric problem
    std::vector<double> d(nb), B((size_t)nb * nb), mu, Vb;
    for (int p = 0; p < nb; ++p) d[p] = G2[p * nb + p] > 0 ? 1.0 / std::sqrt(G2[p * nb + p]) : 0.0;
    for (int p = 0; p < nb; ++p)
      for (int q = 0; q < nb; ++q) B[(size_t)p * nb + q] = 0.5 * (G2[p * nb + q] + G2[q * nb + p]) * d[p] * d[q];
    jacobi_eig(nb, B, mu, Vb);
    const double mu_max = mu[nb - 1];
    std::vector<int> keep;
    for (int k = 0; k < nb; ++k) if (mu[k] > 1e-10 * mu_max) keep.push_back(k);
    const int nk = (int)keep.size();
    if (nk < K) {
      set_err("certify: the search space collapsed below the block size");
      if (x) x->finish();
      return DPGO_ERR;
    }
    std::vector<double> Tm((size_t)nb * nk);  // basis -> orthonormal coordinates
    for (int p = 0; p < nb; ++p)
      for (int k = 0; k < nk; ++k) Tm[(size_t)p * nk + k] = d[p] * Vb[(size_t)p * nb + keep[k]] / std::sqrt(mu[keep[k]]);
    std::vector<double> A2((size_t)nk * nk, 0.0), w2, Y2;
    for (int k = 0; k < nk; ++k)
      for (int l = 0; l < nk; ++l) {
        double s = 0.0;
        for (int p = 0; p < nb; ++p)
          for (int q = 0; q < nb; ++q) s += Tm[(size_t)p * nk + k] * 0.5 * (G1[p * nb + q] + G1[q * nb + p]) * Tm[(size_t)q * nk + l];
        A2[(size_t)k * nk + l] = s;
      }
    jacobi_eig(nk, A2, w2, Y2);
    double *hc = hG + 4 * Cert::SLOT;  // (pinned; the previous upload has completed behind the last synchronisation)
    for (int p = 0; p < nb; ++p)
      for (int q = 0; q < K; ++q) {
        double s = 0.0;
        for (int k = 0; k < nk; ++k) s += Tm[(size_t)p * nk + k] * Y2[(size_t)k * nk + q];
        hc[p * K + q] = s;
      }
    CK(hipMemcpyAsync(c.slot(7), hc, sizeof(double) * nb * K, hipMemcpyHostToDevice, t->stream));
    const int nxt = 1 - cur;
    double *Un = c.U[nxt], *AUn = c.AU[nxt];
    c.update(Un, K3, K, 0.0, {CertTerm{U, c.slot(7), K3, nb, 1.0}});
    c.update(Un + 2 * K, K3, K, 0.0, {CertTerm{W, c.slot(7) + K * K, K3, nb - K, 1.0}});
    c.update(AUn + 2 * K, K3, K, 0.0, {CertTerm{AW, c.slot(7) + K * K, K3, nb - K, 1.0}});
    cur = nxt;
    c.project(c.U[cur], K3, K);
    c.cholqr(c.U[cur], K3, K, c.T);
    c.cholqr(c.U[cur], K3, K, c.T);
    (void)P;
  }
  out->lambda_min = c.deflate ? std::min(0.0, theta0) : theta0;
  out->residual = res0;
  out->norm_bound = s_bound;
  out->certified = status;
  out->iterations = std::min(it + 1, max_iters);
  out->block = K;
  out->deflated = c.deflate ? 1 : 0;
  if (v && !c.halted()) {
    double *hc = hG + 4 * Cert::SLOT;
    for (int p = 0; p < K; ++p) hc[p] = y0[p];
    CK(hipMemcpyAsync(c.slot(7), hc, sizeof(double) * K, hipMemcpyHostToDevice, t->stream));
    c.update(c.T2, 1, 1, 0.0, {CertTerm{c.U[cur], c.slot(7), K3, K, 1.0}});
    CK(hipGetLastError());
    CK(hipMemcpyAsync(v, c.T2, sizeof(double) * Ls, hipMemcpyDeviceToHost, t->stream));
  }
  CK(hipStreamSynchronize(t->stream));
  if (x && x->finish()) return DPGO_ERR;
  return 0;
#undef CK
}

}  // namespace dpgo_cert

extern "C" {

int dpgo_team_certify(dpgo_team_t *t, double eta, double tol, int max_iters, int block, int flags, dpgo_certificate_t *out,
                      double *v) {
  if (!t || !out) { set_err("certify: null argument"); return DPGO_ERR; }
  const int K = block > 0 ? block : t->prm.r;
  if (K < 3 || K > 8) { set_err("certify: the block size must lie in 3..8"); return DPGO_ERR; }
  if (max_iters < 1 || !(tol > 0) || !(eta >= 0)) { set_err("certify: max_iters >= 1, tol > 0 and eta >= 0 required"); return DPGO_ERR; }
  if (check_team(t, "certify")) return DPGO_ERR;
  Cert c;
  c.t = t;
  return certify_body(c, eta, tol, max_iters, K, flags, out, v);
}


// staircase step, host arithmetic: [X; 0] + alpha [0; v^T], rotation blocks back onto the Stiefel manifold (polar factor)
int dpgo_escape_point(const double *X, int r, int num_poses, const double *v, double alpha, double *X_out) {
  if (!X || !v || !X_out || num_poses < 1) { set_err("escape_point: null argument"); return DPGO_ERR; }
  if (r < 3 || r > 7) { set_err("escape_point: r must lie in 3..7 (no kernel is instantiated above rank 8)"); return DPGO_ERR; }
  const int r1 = r + 1;
  for (int i = 0; i < num_poses; ++i) {
    double A[8][4];
    for (int c = 0; c < 4; ++c) {
      for (int a = 0; a < r; ++a) A[a][c] = X[((size_t)4 * i + c) * r + a];
      A[r][c] = alpha != 0.0 ? alpha * v[(size_t)4 * i + c] : 0.0;  // ([X; 0] exactly: no -0)
    }
    if (alpha != 0.0) {
      // polar factor of the (r+1) x 3 rotation block: A (A^T A)^-1/2
      std::vector<double> S(9), w, Vs;
      for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
          double s = 0.0;
          for (int a = 0; a < r1; ++a) s += A[a][p] * A[a][q];
          S[3 * p + q] = s;
        }
      jacobi_eig(3, S, w, Vs);
      if (!(w[0] > 0.0)) { set_err("escape_point: a rotation block is rank deficient"); return DPGO_ERR; }
      double Sih[3][3];
      for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
          double s = 0.0;
          for (int k = 0; k < 3; ++k) s += Vs[3 * p + k] * Vs[3 * q + k] / std::sqrt(w[k]);
          Sih[p][q] = s;
        }
      double B[8][3];
      for (int a = 0; a < r1; ++a)
        for (int q = 0; q < 3; ++q) B[a][q] = A[a][0] * Sih[0][q] + A[a][1] * Sih[1][q] + A[a][2] * Sih[2][q];
      for (int a = 0; a < r1; ++a)
        for (int q = 0; q < 3; ++q) A[a][q] = B[a][q];
    }
    for (int c = 0; c < 4; ++c)
      for (int a = 0; a < r1; ++a) X_out[((size_t)4 * i + c) * r1 + a] = A[a][c];
  }
  return DPGO_OK;
}

}  // extern "C"

// linear_removal.hip -- measurements that are in the graph removed or down-weighted in the estimate and its covariances, to
// first order and without a re-solve: the counterpart of linear_update.hip for weight taken OUT of the graph.
//
// T, Sigma, the perturbation, J_i, J_j, xi with no Log-Jacobian, and Sigma_meas are 5f's (gate.hip); A is 5i's (gate_joint.hip),
// B = Sigma A^T 5j's.  Record k is in the weighted graph at weight w_k, T a minimum of that graph, and its weight drops to
// w'_k, 0 <= w'_k < w_k (w' = 0 removes the edge).  dw_k = w_k - w'_k, R_k = Sigma_meas,k / dw_k.
//   H' = H - A^T R^-1 A,  N = R - A B (the covariance of the post-fit residuals of the set),  Sigma' = Sigma + B N^-1 B^T,
//   dx = +B N^-1 xi,  T' = T [+] dx,  xi_loo = xi + A dx = R N^-1 xi,  d2_joint = xi^T N^-1 xi,
//   log det H' - log det H = log det N - log det R
// Worked whitened: s_k = (sqrt(2 kappa_k dw_k) x 3, sqrt(tau_k dw_k) x 3), D = diag(s), R = D^-2, B~ = B D, xi~ = D xi,
//   N~ = D N D = I - (D A) B~, whose pivots lie in (0, 1] and whose diagonal block is the audit's I - dw C;  G~ = N~^-1,
//   z~ = G~ xi~,  U~ = B~ G~,  dx_p = B~_p z~,  Sigma'_pq = Sigma_pq + U~_p B~_q^T,  xi_loo = z~ / s,  d2_joint = xi~^T z~,
//   log det N = log det N~ + log det R,  log det R = sum_k -3 log(2 kappa_k) - 3 log tau_k - 6 log dw_k.
// A set whose removal leaves the graph without another way to some relative pose makes N~ singular: the call refuses when a
// record's own diagonal block, the factorisation, or the smallest pivot of the whole factor says so (min_redundancy).
// Every sum runs in index order with __builtin_fma; no floating-point atomics: two calls give the same bytes.
//
// The covariance path is asked for the rectangular set of linear_update.hip, the caller's own pairs behind it.  k_rem_b forms
// B~ (column-major, leading dimension 6 N) behind the staged blocks, k_rem_n forms N~, xi, xi~ and every record's pivot_min,
// dense_spd_inverse inverts N~ in place of a copy (its factor stays for the log det and the smallest pivot), k_rem_u is
// U~ = B~ G~ on the fp64 matrix cores through dgemm_tile, k_rem_z forms z~ and xi_loo, k_rem_scalars the four figures, and
// k_rem_finish, one wave per pose or requested pair, reduces the 6 K columns and writes T', dx and the blocks of Sigma'.
// B~, U~, N~ and G~ stay on the device; only the outputs go to the host.
#include <algorithm>
#include <chrono>

#include "closure_frame.h"
#include "covariance_schur.h"
#include "linear_removal_block.h"

namespace dpgo {

// the six doubles of a RemRec in three 16-byte loads
__device__ __forceinline__ RemRec rem_load(const RemRec *r) {
  RemRec o;
  double v[6];
  gate_load_pairs<3>((const double *)r, v);
  o.kappa = v[0]; o.tau = v[1]; o.w = v[2]; o.dw = v[3]; o.s_rot = v[4]; o.s_trn = v[5];
  o.pad[0] = o.pad[1] = 0.0;
  return o;
}

// One lane per (p, k), p the faster index, grid-stride: the record's Jacobians from T, the two staged blocks Sigma_{p,i_k}
// and Sigma_{p,j_k}, the block B_p,k, its six columns scaled by s_k.  Consecutive lanes read consecutive staged blocks and
// store consecutive runs of 48 bytes of every column of B~.
__global__ __launch_bounds__(256) void k_rem_b(const double *__restrict__ T, const double *__restrict__ blocks,
                                               const GateRec *__restrict__ cand, const RemRec *__restrict__ rec, int N, int K,
                                               double *__restrict__ B) {
  const size_t total = (size_t)N * K, ld = (size_t)6 * N;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int k = (int)(t / N), p = (int)(t % N);
    JointEnds e;
    double Rij[3][3], tij[3], Si[6][6], Sj[6][6], Bk[6][6];
    joint_ends(T, cand + k, e, Rij, tij);
    const RemRec sc = rem_load(rec + k);
    gate_load36(blocks + 36 * upd_block_index(N, e.ri, p), Si);
    gate_load36(blocks + 36 * upd_block_index(N, e.rj, p), Sj);
    upd_b_block(Si, Sj, e.Ji, e.Jj, Bk);
    rem_scale_columns(Bk, sc.s_rot, sc.s_trn);
    double *o = B + (size_t)6 * k * ld + (size_t)6 * p;
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int a = 0; a < 6; ++a) gp(o)[c * ld + a] = Bk[a][c];
  }
}

// N~ from B~ (order 6 K, leading dimension 6 K), xi, xi~ and every record's pivot_min: one lane per block (k, l) with k <= l,
// K^2 lanes of which the lower triangle rests, grid-stride, in the shape of joint_assemble (gate_joint_block.h).  The
// removal has an assembly of its own because joint_assemble averages the block of two records on the same ordered pair of
// poses with its transpose: right for M = A Sigma A^T + R, wrong for N~, whose block s_k o (A Sigma A^T)_kl o s_l is symmetric
// only when the two records' noise is proportional.  Which of (k, l) and (l, k) a lane forms follows from the endpoints
// (joint_orientation; on the same ordered pair: the lower index), and it writes that block and its transpose, so N~ is
// bitwise symmetric.  The lanes of the diagonal store I + (G + G^T) / 2, xi, xi~ and the smallest pivot of their block.
__global__ __launch_bounds__(256) void k_rem_n(const double *__restrict__ T, const GateRec *__restrict__ cand, const RemRec *__restrict__ rec,
                                               int K, int N, const double *__restrict__ B, double *__restrict__ Nt, double *__restrict__ xi,
                                               double *__restrict__ xit, double *__restrict__ pmin) {
  const size_t total = (size_t)K * K, ld = (size_t)6 * K, ldb = (size_t)6 * N;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int k = (int)(t / K), l = (int)(t % K);
    if (l < k) continue;
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    const v2i_t pk = *(const __attribute__((address_space(1))) v2i_t *)(cand + k), pl = *(const __attribute__((address_space(1))) v2i_t *)(cand + l);
    const int way = joint_orientation(pk.x, pk.y, pl.x, pl.y);
    const int kk = way < 0 ? l : k, ll = way < 0 ? k : l;
    JointEnds ek;
    double Rij[3][3], tij[3], G[6][6];
    joint_ends(T, cand + kk, ek, Rij, tij);
    const RemRec sc = rem_load(rec + kk);
    rem_n_block(B, ldb, ek, ll, sc.s_rot, sc.s_trn, G);
    if (k != l) {
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          gp(Nt)[((size_t)6 * kk + a) * ld + (size_t)6 * ll + b] = G[a][b];
          gp(Nt)[((size_t)6 * ll + b) * ld + (size_t)6 * kk + a] = G[a][b];
        }
      continue;
    }
    double v[GATE_MEAS], S[6][6], x[6], xt[6];
    gate_load_meas(cand[k].m, v);
    rem_diagonal(G, S);
    gate_innovation(Rij, tij, v, x);
    rem_whiten(x, sc.s_rot, sc.s_trn, xt);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) gp(Nt)[((size_t)6 * k + a) * ld + (size_t)6 * k + b] = S[a][b];
      gp(xi)[(size_t)6 * k + a] = x[a];
      gp(xit)[(size_t)6 * k + a] = xt[a];
    }
    gp(pmin)[k] = rem_pivot_min(S);
  }
}

// U~ = B~ G~: B~ 6 N x 6 K and U~ column-major with leading dimension 6 N, G~ of order 6 K; one workgroup per 64 x 64 tile
__global__ __launch_bounds__(256) void k_rem_u(const double *__restrict__ B, const double *__restrict__ G, double *__restrict__ U, int m, int n) {
  dgemm_tile<false>(B, m, G, n, U, m, m, n, n, 0, 64 * (int)blockIdx.x, 64 * (int)blockIdx.y);
}

// z~ = G~ xi~, one lane per row, the sum over the columns in index order (G~ is bitwise symmetric: the element (r, c) is read
// at (c, r), consecutive lanes consecutive addresses), and xi_loo = z~ / s beside it
__global__ __launch_bounds__(256) void k_rem_z(const double *__restrict__ G, const double *__restrict__ xit, const RemRec *__restrict__ rec,
                                               int n, double *__restrict__ z, double *__restrict__ xi_loo) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s = __builtin_fma(gp(G)[(size_t)c * n + r], gp(xit)[c], s);
    gp(z)[r] = s;
    const double *p = (const double *)(rec + r / 6);
    gp(xi_loo)[r] = s / (r % 6 < 3 ? gp(p)[4] : gp(p)[5]);
  }
}

// the four figures by one lane: d2_joint = xi~^T z~ and logdet_R in index order; logdet_N = log det N~ + logdet_R and the
// smallest pivot of the factor as k_cov_logdet left them in ld
__global__ __launch_bounds__(64) void k_rem_scalars(const double *__restrict__ xit, const double *__restrict__ z, const RemRec *__restrict__ rec,
                                                    int K, const double *__restrict__ ld, double *__restrict__ scal) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double d = 0.0, lr = 0.0;
  for (int c = 0; c < 6 * K; ++c) d = __builtin_fma(gp(xit)[c], gp(z)[c], d);
  for (int k = 0; k < K; ++k) {
    const double *p = (const double *)(rec + k);
    lr += rem_logdet_r(gp(p)[0], gp(p)[1], gp(p)[3]);
  }
  gp(scal)[0] = d;
  gp(scal)[1] = gp(ld)[0] + lr;
  gp(scal)[2] = lr;
  gp(scal)[3] = gp(ld)[1];
}

// The reduction over the 6 K columns, one wave per pose and, in a second range of waves, per requested pair, as in
// k_upd_finish: lane l takes the columns l, l + 64, ... in index order; a pose's lane keeps the 21 sums of the upper triangle
// of U~_p B~_p^T and the 6 of B~_p z~, a pair's the 36 of U~_p B~_q^T; the lanes' sums meet in an xor butterfly of fixed order,
// and lane 0 ADDS to the staged block, retracts and writes T'_p, dx_p and Sigma'_pp, or Sigma'_pq.  fp64 in registers, no LDS.
__global__ __launch_bounds__(256) void k_rem_finish(const double *__restrict__ T, const double *__restrict__ diag,
                                                    const double *__restrict__ pair_blocks, const int *__restrict__ pairs, int N, int K,
                                                    int num_pairs, const double *__restrict__ B, const double *__restrict__ U,
                                                    const double *__restrict__ z, double *__restrict__ T_new, double *__restrict__ delta,
                                                    double *__restrict__ out_diag, double *__restrict__ out_pairs) {
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), ld = (size_t)6 * N;
  const int lane = threadIdx.x & 63, n = 6 * K;
  if (w >= (size_t)N + (size_t)num_pairs) return;
  if (w < (size_t)N) {
    const int p = (int)w;
    double acc[UPD_SUMS];
#pragma unroll
    for (int q = 0; q < UPD_SUMS; ++q) acc[q] = 0.0;
    for (int c = lane; c < n; c += 64) {
      double u[6], b[6];
      gate_load_pairs<3>(U + (size_t)c * ld + (size_t)6 * p, u);
      gate_load_pairs<3>(B + (size_t)c * ld + (size_t)6 * p, b);
      upd_accumulate(u, b, gp(z)[c], acc);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1)
#pragma unroll
      for (int q = 0; q < UPD_SUMS; ++q) acc[q] += __shfl_xor(acc[q], off);
    if (lane != 0) return;
    double Sn[6][6], dx[6], R[3][3], t[3], Rn[3][3], tn[3], P[12];
    rem_close_pose(diag + (size_t)36 * p, acc, Sn, dx);
    gate_load_pose(T, p, R, t);
    upd_retract(R, t, dx, Rn, tn);
    upd_store_pose(Rn, tn, P);
#pragma unroll
    for (int q = 0; q < 12; ++q) gp(T_new)[(size_t)12 * p + q] = P[q];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      gp(delta)[(size_t)6 * p + a] = dx[a];
#pragma unroll
      for (int c = 0; c < 6; ++c) gp(out_diag)[(size_t)36 * p + 6 * a + c] = Sn[a][c];
    }
    return;
  }
  const size_t e = w - (size_t)N;
  const int p = gp(pairs)[2 * e], q = gp(pairs)[2 * e + 1];
  double acc[36];
#pragma unroll
  for (int x = 0; x < 36; ++x) acc[x] = 0.0;
  for (int c = lane; c < n; c += 64) {
    double u[6], b[6];
    gate_load_pairs<3>(U + (size_t)c * ld + (size_t)6 * p, u);
    gate_load_pairs<3>(B + (size_t)c * ld + (size_t)6 * q, b);
    upd_accumulate_pair(u, b, acc);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1)
#pragma unroll
    for (int x = 0; x < 36; ++x) acc[x] += __shfl_xor(acc[x], off);
  if (lane != 0) return;
#pragma unroll
  for (int x = 0; x < 36; ++x) gp(out_pairs)[36 * e + x] = gp(pair_blocks)[36 * e + x] + acc[x];
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall REMOVAL = {"linear_removal", "record"};

// the step behind a covariance path's staged blocks: upload the records, form B~ and N~, invert, decide the three refusals
// of testability, multiply, reduce, queue the copy of the outputs
struct RemovalEpilogue : ClosureEpilogue {
  std::vector<GateRec> cand;  // w0, w1: the ranks of i and j among the endpoints
  std::vector<RemRec> rec;
  std::vector<int> user_pairs;  // the caller's pairs, behind the N m blocks of the call
  int m = 0, N = 0;
  double min_redundancy = 0.0;
  DevBuf<GateRec> d_cand;
  DevBuf<RemRec> d_rec;
  DevBuf<double> d_B, d_U, d_M, d_W, d_G, d_work, d_out;
  DevBuf<int> d_pairs;
  // T' (12 N), dx (6 N), Sigma' diagonal (36 N), Sigma' pairs (36 P), xi (6 K), xi_loo (6 K), pivot_min (K), 4 figures
  std::vector<double> h_out;
  RemovalEpilogue() : ClosureEpilogue(7) {}
  size_t K() const { return cand.size(); }
  size_t P() const { return user_pairs.size() / 2; }
  size_t out_doubles() const { return (size_t)54 * N + 36 * P() + 13 * K() + 4; }
  static double bytes(double N, double K, double P) {
    return 2.0 * 288.0 * N * K + 3.0 * 288.0 * K * K + 8.0 * (54.0 * N + 36.0 * P + 25.0 * K + 8.0) + 192.0 * K + 8.0 * P;
  }
  int alloc() {
    const size_t k = K();
    if (d_cand.alloc(k) || d_rec.alloc(k) || d_B.alloc((size_t)36 * N * k) || d_U.alloc((size_t)36 * N * k) || d_M.alloc(36 * k * k) ||
        d_W.alloc(36 * k * k) || d_G.alloc(36 * k * k) || d_work.alloc(12 * k + 4) || d_out.alloc(out_doubles()) || d_pairs.alloc(2 * P())) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "linear_removal: device allocation failed (%.0f bytes for %zu records on %d poses)",
                    bytes(N, (double)k, (double)P()), k, N);
      set_err(buf);
      return DPGO_ERR;
    }
    return ev.create();
  }
  int run(const CovStage &st) override {
    const size_t k = K(), np = P();
    if (st.N != N || (size_t)st.num_pairs != (size_t)N * m + np) {
      set_err("linear_removal: the staged blocks are not the rectangular set of the endpoints");
      return DPGO_ERR;
    }
    for (const GateRec &c : cand)
      if (c.i < 0 || c.i >= N || c.j < 0 || c.j >= N || c.w0 < 0 || c.w0 >= m || c.w1 < 0 || c.w1 >= m || c.w0 == c.w1) {
        set_err("linear_removal: a record lies outside the staged blocks");
        return DPGO_ERR;
      }
    for (int p : user_pairs)
      if (p < 0 || p >= N) {
        set_err("linear_removal: a pair lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    const int n = (int)(6 * k);
    HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateRec) * k, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_rec.p, rec.data(), sizeof(RemRec) * k, hipMemcpyHostToDevice, s));
    if (np) HIPC(hipMemcpyAsync(d_pairs.p, user_pairs.data(), sizeof(int) * 2 * np, hipMemcpyHostToDevice, s));
    double *oT = d_out.p, *odx = oT + (size_t)12 * N, *odiag = odx + (size_t)6 * N, *opairs = odiag + (size_t)36 * N;
    double *oxi = opairs + 36 * np, *oloo = oxi + 6 * k, *opiv = oloo + 6 * k, *oscal = opiv + k;
    double *xit = d_work.p, *z = xit + 6 * k, *ldet = z + 6 * k;
    HIPC(hipEventRecord(ev[0], s));
    // at most eight workgroups per CU of an MI355X: the lanes beyond stride over the rest
    k_rem_b<<<(unsigned)std::min<size_t>(((size_t)N * k + 255) / 256, 2048), 256, 0, s>>>(st.Td, st.pairs, d_cand.p, d_rec.p, N, (int)k, d_B.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    k_rem_n<<<(unsigned)std::min<size_t>((k * k + 255) / 256, 2048), 256, 0, s>>>(st.Td, d_cand.p, d_rec.p, (int)k, N, d_B.p, d_M.p, oxi, xit, opiv);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[2], s));
    const int fail = dense_spd_inverse(s, d_M.p, d_W.p, d_G.p, n);  // (synchronises the stream; the factor stays in d_M)
    HIPC(hipGetLastError());
    if (fail < 0) { set_err("linear_removal: scratch allocation of the inverse failed"); return DPGO_ERR; }
    // ---- the three refusals of testability, in their order; nothing has been copied out
    std::vector<double> piv(k);
    HIPC(hipMemcpyAsync(piv.data(), opiv, sizeof(double) * k, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    char buf[400];
    for (size_t q = 0; q < k; ++q)
      if (!(piv[q] > min_redundancy)) {
        std::snprintf(buf, sizeof buf,
                      "linear_removal: record %zu is not testable: the smallest pivot of its block of the whitened N is %.6g, not above "
                      "min_redundancy = %.6g; the graph knows the relative pose of its endpoints by no other way than the weight taken out",
                      q, piv[q], min_redundancy);
        set_err(buf);
        return DPGO_ERR;
      }
    if (fail > 0) {
      set_err("linear_removal: non-positive pivot at row " + std::to_string(fail - 1) + " of N (pivot block " + std::to_string((fail - 1) / 6) +
              ", the block of record " + std::to_string((fail - 1) / 6) +
              "): N = R - A Sigma A^T is not positive definite at this T; the records together leave no redundancy");
      return DPGO_ERR;
    }
    HIPC(hipEventRecord(ev[3], s));
    if (launch_cov_logdet(s, d_M.p, n, ldet)) return DPGO_ERR;
    double lds[3];
    HIPC(hipMemcpyAsync(lds, ldet, sizeof lds, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (!(lds[1] > min_redundancy)) {
      std::snprintf(buf, sizeof buf,
                    "linear_removal: the records together leave no redundancy: the smallest pivot of the whitened N is %.6g, not above "
                    "min_redundancy = %.6g, though every record alone is testable",
                    lds[1], min_redundancy);
      set_err(buf);
      return DPGO_ERR;
    }
    k_rem_u<<<dim3((unsigned)((6 * (size_t)N + 63) / 64), (unsigned)((n + 63) / 64), 1), 256, 0, s>>>(d_B.p, d_G.p, d_U.p, 6 * N, n);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[4], s));
    k_rem_z<<<(unsigned)std::min<size_t>((n + 255) / 256, 2048), 256, 0, s>>>(d_G.p, xit, d_rec.p, n, z, oloo);
    k_rem_scalars<<<1, 64, 0, s>>>(xit, z, d_rec.p, (int)k, ldet, oscal);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[5], s));
    k_rem_finish<<<(unsigned)(((size_t)N + np + 3) / 4), 256, 0, s>>>(st.Td, st.diag, st.pairs + (size_t)36 * N * m, d_pairs.p, N, (int)k, (int)np,
                                                                     d_B.p, d_U.p, z, oT, odx, odiag, opairs);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[6], s));
    h_out.resize(out_doubles());
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, s));
    ran = true;
    return DPGO_OK;
  }
};

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_linear_removal(dpgo_team_t *t, const double *T, int method, int max_block, int num,
                                        const dpgo_measurement_t *records, const double *new_weight, double min_redundancy,
                                        int num_pairs, const int *pairs, double *T_new, double *delta, double *cov_diag,
                                        double *cov_pairs, double *xi, double *xi_loo, double *pivot_min, double *scalars,
                                        dpgo_covariance_t *res) {
  const auto t_begin = std::chrono::steady_clock::now();
  // ---- the refusals of the call itself: on the host, before any device work, no output touched
  if (!t || !T || !res || !T_new || !delta || !cov_diag || !xi || !xi_loo || !pivot_min || !scalars) return REMOVAL.refuse("null argument");
  if (num <= 0) return REMOVAL.refuse("num must be positive, not " + std::to_string(num));
  if (!records) return REMOVAL.refuse("null argument");
  if (num_pairs < 0) return REMOVAL.refuse("num_pairs must not be negative, not " + std::to_string(num_pairs));
  if (num_pairs > 0 && (!pairs || !cov_pairs)) return REMOVAL.refuse("null argument");
  if (REMOVAL.check_method(method)) return DPGO_ERR;
  if (!(min_redundancy > 0.0 && min_redundancy < 1.0)) {
    char buf[120];
    std::snprintf(buf, sizeof buf, "min_redundancy must lie in (0, 1), not %.6g", min_redundancy);
    return REMOVAL.refuse(buf);
  }
  if (check_team_local(t, REMOVAL.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(t);
  const int N = offs.back();
  RemovalEpilogue epi;
  epi.N = N;
  epi.min_redundancy = min_redundancy;
  epi.cand.resize(num);
  epi.rec.resize(num);
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &m = records[k];
    int g[2];
    if (REMOVAL.endpoints(t, offs, k, m, g) || REMOVAL.check(k, m, true)) return DPGO_ERR;
    char buf[200];
    if (!(m.weight > 0.0)) {
      std::snprintf(buf, sizeof buf, "record %d has weight = %.6g: a record must be in the graph at a positive weight", k, m.weight);
      return REMOVAL.refuse(buf);
    }
    const double nw = new_weight ? new_weight[k] : 0.0;
    if (!(nw >= 0.0) || !std::isfinite(nw) || !(nw < m.weight)) {
      std::snprintf(buf, sizeof buf, "record %d has new_weight = %.6g: it must be finite, not negative and below its weight = %.6g", k, nw,
                    m.weight);
      return REMOVAL.refuse(buf);
    }
    GateRec &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    pack_measurement(m, c.m);
    RemRec &r = epi.rec[k];
    std::memset(&r, 0, sizeof r);
    r.kappa = m.kappa; r.tau = m.tau; r.w = m.weight; r.dw = m.weight - nw;
    r.s_rot = std::sqrt(2.0 * m.kappa * r.dw);
    r.s_trn = std::sqrt(m.tau * r.dw);
  }
  for (int k = 0; k < 2 * num_pairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= N)
      return REMOVAL.refuse("pair " + std::to_string(k / 2) + " names pose " + std::to_string(pairs[k]) + ", outside [0, " + std::to_string(N) + ")");
  const std::vector<int> poses = rank_endpoints(epi.cand);
  const int m = epi.m = (int)poses.size();
  const size_t K = (size_t)num, nb = (size_t)N * m, np = nb + (size_t)num_pairs;
  HIPC(hipSetDevice(t->device));
  {
    // the pair blocks the path stages for this call, B~ and U~, N~, the scratch of its inverse and G~: the rest is the path's own
    // accounting
    const double blocks = 288.0 * (double)np, bu = 288.0 * (double)N * (double)K, mat = 288.0 * (double)K * (double)K;
    const double need = blocks + RemovalEpilogue::bytes(N, (double)K, num_pairs);
    double avail = 0.0;
    if (REMOVAL.device_avail(t, &avail)) return DPGO_ERR;
    if (need > avail || np > (size_t)INT32_MAX || 36 * K * K > (size_t)1 << 40 || 6 * K > (size_t)INT32_MAX / 2) {
      char buf[480];
      std::snprintf(buf, sizeof buf,
                    "%d records on %d of %d poses: the %zu pair blocks, B and U (6 N x 6 K each) and the three matrices of order %zu need "
                    "%.0f bytes (%.0f + 2 x %.0f + 3 x %.0f and the working arrays), %.0f are available on the device; the pair blocks must "
                    "number at most %d",
                    num, m, N, np, 6 * K, need, blocks, bu, mat, avail, INT32_MAX);
      return REMOVAL.refuse(buf);
    }
  }
  // the rectangular set of linear_update: block a N + p = Sigma_{p, e_a}; the caller's pairs behind them
  std::vector<int> all;
  all.reserve(2 * np);
  for (int a = 0; a < m; ++a)
    for (int p = 0; p < N; ++p) { all.push_back(p); all.push_back(poses[a]); }
  all.insert(all.end(), pairs, pairs + 2 * (size_t)num_pairs);
  epi.user_pairs.assign(pairs, pairs + 2 * (size_t)num_pairs);
  if (epi.alloc()) return DPGO_ERR;
  if (const int rc = REMOVAL.path(t, T, method, max_block, (int)np, all.data(), res, epi)) {
    std::memset(res, 0, sizeof *res);  // (also when the path went through and the call itself refused behind it)
    return rc;
  }
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing) {
    float ms[6];
    for (int q = 0; q < 6; ++q) ms[q] = epi.ev.ms(q, q + 1);
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "linear_removal: %d records on %d of %d poses (%zu pair blocks), k_rem_b %.3f ms, k_rem_n %.3f ms, inverse %.3f ms, "
                         "log det (with the host's read of it) and k_rem_u %.3f ms, k_rem_z and figures %.3f ms, k_rem_finish %.3f ms, the whole call %.3f ms\n",
                 num, m, N, np, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], whole);
  }
  const double *h = epi.h_out.data();
  std::memcpy(T_new, h, sizeof(double) * 12 * (size_t)N);
  std::memcpy(delta, h + (size_t)12 * N, sizeof(double) * 6 * (size_t)N);
  std::memcpy(cov_diag, h + (size_t)18 * N, sizeof(double) * 36 * (size_t)N);
  const double *hp = h + (size_t)54 * N;
  if (num_pairs > 0) std::memcpy(cov_pairs, hp, sizeof(double) * 36 * (size_t)num_pairs);
  hp += 36 * (size_t)num_pairs;
  std::memcpy(xi, hp, sizeof(double) * 6 * K);
  std::memcpy(xi_loo, hp + 6 * K, sizeof(double) * 6 * K);
  std::memcpy(pivot_min, hp + 12 * K, sizeof(double) * K);
  std::memcpy(scalars, hp + 13 * K, sizeof(double) * 4);
  return DPGO_OK;
}

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
// The covariance path is asked for the rectangular set of linear_update.hip, the caller's own pairs behind it, and the step
// behind it is linear_frame.h's, shared with the update.  k_lin_b<true> forms B~ (column-major, leading dimension 6 N) behind
// the staged blocks, k_rem_n forms N~, xi, xi~ and every record's pivot_min, dense_spd_inverse inverts N~ in place of a copy
// (its factor stays for the log det and the smallest pivot), k_lin_u is U~ = B~ G~ on the fp64 matrix cores through
// dgemm_tile, k_rem_z forms z~ and xi_loo, k_rem_scalars the four figures, and k_lin_finish<true>, one wave per pose or
// requested pair, reduces the 6 K columns, ADDS to the staged block and writes T', dx and the blocks of Sigma'.
// B~, U~, N~ and G~ stay on the device; only the outputs go to the host.
#include "linear_frame.h"

namespace dpgo {

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

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall REMOVAL = {"linear_removal", "record"};

// the removal behind the shared step: N~, xi, xi~ and every pivot_min by k_rem_n, the three refusals of testability, z~,
// xi_loo and the four figures.  d_out behind xi: xi_loo (6 K), pivot_min (K), 4 figures.  d_work: xi~ (6 K), z~ (6 K), the
// log det's 4
struct RemovalEpilogue : LinearEpilogue<true> {
  double min_redundancy = 0.0;
  RemovalEpilogue() : LinearEpilogue<true>(REMOVAL) {}
  size_t tail_doubles() const override { return 7 * K() + 4; }
  size_t work_doubles() const override { return 12 * K() + 4; }
  double bytes(double N, double K, double P) const override {
    return 2.0 * 288.0 * N * K + 3.0 * 288.0 * K * K + 8.0 * (54.0 * N + 36.0 * P + 25.0 * K + 8.0) + 192.0 * K + 8.0 * P;
  }
  double *xit() const { return d_work.p; }
  double *opiv() const { return otail + 6 * K(); }
  void assemble(const CovStage &st, const double *B) override {
    const size_t k = K();
    k_rem_n<<<(unsigned)std::min<size_t>((k * k + 255) / 256, 2048), 256, 0, st.stream>>>(st.Td, d_cand.p, d_rec.p, (int)k, N, B, d_M.p, oxi, xit(),
                                                                                       opiv());
  }
  // ---- the three refusals of testability, in their order; nothing has been copied out
  int after_inverse(hipStream_t s, int fail) override {
    const size_t k = K();
    std::vector<double> piv(k);
    HIPC(hipMemcpyAsync(piv.data(), opiv(), sizeof(double) * k, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    char buf[400];
    for (size_t q = 0; q < k; ++q)
      if (!(piv[q] > min_redundancy)) {
        std::snprintf(buf, sizeof buf,
                      "record %zu is not testable: the smallest pivot of its block of the whitened N is %.6g, not above "
                      "min_redundancy = %.6g; the graph knows the relative pose of its endpoints by no other way than the weight taken out",
                      q, piv[q], min_redundancy);
        return call.refuse(buf);
      }
    if (fail > 0)
      return call.refuse("non-positive pivot at row " + std::to_string(fail - 1) + " of N (pivot block " + std::to_string((fail - 1) / 6) +
                         ", the block of record " + std::to_string((fail - 1) / 6) +
                         "): N = R - A Sigma A^T is not positive definite at this T; the records together leave no redundancy");
    return DPGO_OK;
  }
  int after_logdet(hipStream_t s) override {
    double lds[3];
    HIPC(hipMemcpyAsync(lds, ldet, sizeof lds, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (!(lds[1] > min_redundancy)) {
      char buf[400];
      std::snprintf(buf, sizeof buf,
                    "the records together leave no redundancy: the smallest pivot of the whitened N is %.6g, not above "
                    "min_redundancy = %.6g, though every record alone is testable",
                    lds[1], min_redundancy);
      return call.refuse(buf);
    }
    return DPGO_OK;
  }
  void z_and_figures(hipStream_t s) override {
    const int n = (int)(6 * K());
    k_rem_z<<<(unsigned)std::min<size_t>((n + 255) / 256, 2048), 256, 0, s>>>(d_G.p, xit(), d_rec.p, n, z, otail);
    k_rem_scalars<<<1, 64, 0, s>>>(xit(), z, d_rec.p, (int)K(), ldet, opiv() + K());
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
  const LinearArgs a = {t, T, method, max_block, num, records, num_pairs, pairs, T_new, delta, cov_diag, cov_pairs, xi, res};
  RemovalEpilogue epi;
  epi.min_redundancy = min_redundancy;
  const auto redundancy_in_range = [&]() -> int {
    if (min_redundancy > 0.0 && min_redundancy < 1.0) return DPGO_OK;
    char buf[120];
    std::snprintf(buf, sizeof buf, "min_redundancy must lie in (0, 1), not %.6g", min_redundancy);
    return REMOVAL.refuse(buf);
  };
  // the weight a record is in the graph at and the weight it drops to, and what the device needs of both
  const auto weights = [&](int k, const dpgo_measurement_t &m) -> int {
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
    RemRec &r = epi.rec[k];
    std::memset(&r, 0, sizeof r);
    r.kappa = m.kappa; r.tau = m.tau; r.w = m.weight; r.dw = m.weight - nw;
    r.s_rot = std::sqrt(2.0 * m.kappa * r.dw);
    r.s_trn = std::sqrt(m.tau * r.dw);
    return DPGO_OK;
  };
  if (const int rc = linear_call(a, !xi_loo || !pivot_min || !scalars, epi, nullptr, redundancy_in_range, weights)) return rc;
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing) {  // (the fields keep the names the profiles quote: k_rem_b, k_rem_u and k_rem_finish are linear_frame.h's kernels)
    float ms[6];
    for (int q = 0; q < 6; ++q) ms[q] = epi.ev.ms(q, q + 1);
    const double whole = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    std::fprintf(stderr, "linear_removal: %d records on %d of %d poses (%zu pair blocks), k_rem_b %.3f ms, k_rem_n %.3f ms, inverse %.3f ms, "
                         "log det (with the host's read of it) and k_rem_u %.3f ms, k_rem_z and figures %.3f ms, k_rem_finish %.3f ms, the whole call %.3f ms\n",
                 num, epi.m, epi.N, epi.rect() + (size_t)num_pairs, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], whole);
  }
  const size_t K = (size_t)num;
  const double *hp = a.copy_head(epi.h_out, epi.N);
  std::memcpy(xi_loo, hp, sizeof(double) * 6 * K);
  std::memcpy(pivot_min, hp + 6 * K, sizeof(double) * K);
  std::memcpy(scalars, hp + 7 * K, sizeof(double) * 4);
  return DPGO_OK;
}

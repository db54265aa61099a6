// linear_frame.h -- what the first-order update (linear_update.hip) and the first-order removal
// (linear_removal.hip, 5l) share: the same computation with a sign and a whitening between them.  Each takes B = Sigma A^T
// behind the covariance path's staged blocks, a matrix of order 6 K (M, or the whitened N), its inverse G, U = B G, and one
// wave per pose or requested pair that reduces the 6 K columns, retracts, and writes T', dx and Sigma' = Sigma -/+ U B^T.
//   device   k_lin_b<Scaled> (B, its columns scaled by a RemRec or not), k_lin_u (U = B G), k_lin_finish<Add> (the reduction);
//            static, in the idiom of covariance_extract.h: each of the two files compiles the instantiations it launches
//   host     LinearEpilogue<Removal>, the step behind the staged blocks, and linear_call, the entry point up to the path.
// A call supplies its assembly kernel (k_upd_m, k_rem_n), what it decides behind the inverse and the log det, its z and
// figures kernels, and the sizes of what lies behind xi in the outputs and in front of z in the working array.  One layer
// above closure_frame.h, whose ClosureCall words the refusals: their order and every message are the calls' own, and the
// tests see them.
#pragma once
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
// and Sigma_{p,j_k}, the two products, and the block B_p,k; Scaled: its six columns times s_k of rec[k] (B~ of the removal;
// the unscaled kernel neither loads nor holds a record, rec may be null).  Consecutive lanes read consecutive staged blocks
// and store consecutive runs of 48 bytes of every column of B (column-major, leading dimension 6 N).
template <bool Scaled>
static __global__ __launch_bounds__(256) void k_lin_b(const double *__restrict__ T, const double *__restrict__ blocks,
                                                      const GateRec *__restrict__ cand, const RemRec *__restrict__ rec, int N, int K,
                                                      double *__restrict__ B) {
  const size_t total = (size_t)N * K, ld = (size_t)6 * N;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int k = (int)(t / N), p = (int)(t % N);
    JointEnds e;
    double Rij[3][3], tij[3], Si[6][6], Sj[6][6], Bk[6][6], s_rot = 1.0, s_trn = 1.0;
    joint_ends(T, cand + k, e, Rij, tij);
    if constexpr (Scaled) {
      const RemRec sc = rem_load(rec + k);
      s_rot = sc.s_rot; s_trn = sc.s_trn;
    }
    gate_load36(blocks + 36 * upd_block_index(N, e.ri, p), Si);
    gate_load36(blocks + 36 * upd_block_index(N, e.rj, p), Sj);
    upd_b_block(Si, Sj, e.Ji, e.Jj, Bk);
    if constexpr (Scaled) rem_scale_columns(Bk, s_rot, s_trn);
    double *o = B + (size_t)6 * k * ld + (size_t)6 * p;
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int a = 0; a < 6; ++a) gp(o)[c * ld + a] = Bk[a][c];
  }
}

// U = B G: B 6 N x 6 K and U column-major with leading dimension 6 N, G of order 6 K; one workgroup per 64 x 64 tile of U
static __global__ __launch_bounds__(256) void k_lin_u(const double *__restrict__ B, const double *__restrict__ G, double *__restrict__ U, int m,
                                                      int n) {
  dgemm_tile<false>(B, m, G, n, U, m, m, n, n, 0, 64 * (int)blockIdx.x, 64 * (int)blockIdx.y);
}

// The reduction over the 6 K columns, one wave per pose and, in a second range of waves, per requested pair.  Lane l takes
// the columns l, l + 64, ... in index order: rows 6 p .. 6 p + 5 of column c of U and of B are 48 contiguous bytes each.  A
// pose's lane accumulates the 21 sums of the upper triangle of U_p B_p^T and the 6 of B_p z; a pair's the 36 of U_p B_q^T.
// The lanes' sums meet in an xor butterfly of fixed order (addition commutes: every lane ends with the same bits), and lane 0
// subtracts them from the staged block (the update) or adds them to it (Add, the removal), retracts and writes T'_p, dx_p
// and Sigma'_pp, or Sigma'_pq.  The sign is the instantiation's: a + or a -, no factor.  fp64 in registers, no LDS.
template <bool Add>
static __global__ __launch_bounds__(256) void k_lin_finish(const double *__restrict__ T, const double *__restrict__ diag,
                                                           const double *__restrict__ pair_blocks, const int *__restrict__ pairs, int N,
                                                           int K, int num_pairs, const double *__restrict__ B,
                                                           const double *__restrict__ U, const double *__restrict__ z,
                                                           double *__restrict__ T_new, double *__restrict__ delta,
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
    lin_close_pose<Add>(diag + (size_t)36 * p, acc, Sn, dx);
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
  for (int x = 0; x < 36; ++x) {
    const double S = gp(pair_blocks)[36 * e + x];
    gp(out_pairs)[36 * e + x] = Add ? S + acc[x] : S - acc[x];
  }
}

}  // namespace dpgo

namespace dpgo_cert {

// The step behind a covariance path's staged blocks: upload the records, form B and the matrix of order 6 K, invert,
// multiply, reduce, queue the copy of the outputs.  Removal: B is scaled by rec, and Sigma' = Sigma + U B^T.
// d_out and h_out: T' (12 N), dx (6 N), Sigma' diagonal (36 N), Sigma' pairs (36 P), xi (6 K), then the call's own
// tail_doubles().  d_work: the call's own, then z (6 K) and the four doubles of launch_cov_logdet.
template <bool Removal>
struct LinearEpilogue : ClosureEpilogue {
  const ClosureCall &call;
  std::vector<GateRec> cand;  // w0, w1: the ranks of i and j among the endpoints
  std::vector<RemRec> rec;  // the removal's
  std::vector<int> user_pairs;  // the caller's pairs, behind the N m blocks of the call
  int m = 0, N = 0;
  CovApply *solve = nullptr;  // on the solve: the path's X is B, and the records are already on the device
  DevBuf<GateRec> d_cand;
  DevBuf<RemRec> d_rec;
  DevBuf<double> d_B, d_U, d_M, d_W, d_G, d_work, d_out;
  DevBuf<int> d_pairs;
  std::vector<double> h_out;
  double *oxi = nullptr, *otail = nullptr, *z = nullptr, *ldet = nullptr;  // carved by run()
  explicit LinearEpilogue(const ClosureCall &c) : ClosureEpilogue(7), call(c) {}
  size_t K() const { return cand.size(); }
  size_t P() const { return user_pairs.size() / 2; }
  size_t rect() const { return solve ? 0 : (size_t)N * m; }  // the blocks of the rectangular set, in front of the caller's
  size_t out_doubles() const { return (size_t)54 * N + 36 * P() + 6 * K() + tail_doubles(); }

  // ---- what a call supplies
  virtual size_t tail_doubles() const = 0;
  virtual size_t work_doubles() const = 0;
  virtual double bytes(double N, double K, double P) const = 0;  // of everything alloc() takes
  // the matrix of order 6 K into d_M and xi into oxi, from B
  virtual void assemble(const CovStage &st, const double *B) = 0;
  // behind the inverse (fail > 0: the row of a non-positive pivot, plus one) and behind the log det: DPGO_OK or a refusal
  virtual int after_inverse(hipStream_t s, int fail) = 0;
  virtual int after_logdet(hipStream_t) { return DPGO_OK; }
  // z from d_G and the call's figures
  virtual void z_and_figures(hipStream_t s) = 0;

  int alloc() {
    const size_t k = K();
    if (d_cand.alloc(k) || (Removal && d_rec.alloc(k)) || (!solve && d_B.alloc((size_t)36 * N * k)) || d_U.alloc((size_t)36 * N * k) ||
        d_M.alloc(36 * k * k) || d_W.alloc(36 * k * k) || d_G.alloc(36 * k * k) || d_work.alloc(work_doubles()) ||
        d_out.alloc(out_doubles()) || d_pairs.alloc(2 * P())) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "device allocation failed (%.0f bytes for %zu %ss on %d poses)", bytes(N, (double)k, (double)P()), k,
                    call.noun, N);
      return call.refuse(buf);
    }
    return ev.create();
  }

  int run(const CovStage &st) override {
    const size_t k = K(), np = P(), nrect = rect();
    if (solve && !solve->X) return call.refuse("the covariance path formed no X");
    const double *B = solve ? solve->X : d_B.p;
    if (st.N != N || (size_t)st.num_pairs != nrect + np) return call.refuse("the staged blocks are not the rectangular set of the endpoints");
    for (const GateRec &c : cand)
      if (c.i < 0 || c.i >= N || c.j < 0 || c.j >= N || c.w0 < 0 || c.w0 >= m || c.w1 < 0 || c.w1 >= m || c.w0 == c.w1)
        return call.refuse(std::string("a ") + call.noun + " lies outside the staged blocks");
    for (int p : user_pairs)
      if (p < 0 || p >= N) return call.refuse("a pair lies outside the staged blocks");
    hipStream_t s = st.stream;
    const int n = (int)(6 * k);
    if (!solve) HIPC(hipMemcpyAsync(d_cand.p, cand.data(), sizeof(GateRec) * k, hipMemcpyHostToDevice, s));
    if (Removal) HIPC(hipMemcpyAsync(d_rec.p, rec.data(), sizeof(RemRec) * k, hipMemcpyHostToDevice, s));
    if (np) HIPC(hipMemcpyAsync(d_pairs.p, user_pairs.data(), sizeof(int) * 2 * np, hipMemcpyHostToDevice, s));
    double *oT = d_out.p, *odx = oT + (size_t)12 * N, *odiag = odx + (size_t)6 * N, *opairs = odiag + (size_t)36 * N;
    oxi = opairs + 36 * np;
    otail = oxi + 6 * k;
    z = d_work.p + work_doubles() - 6 * k - 4;
    ldet = z + 6 * k;
    HIPC(hipEventRecord(ev[0], s));
    // at most eight workgroups per CU of an MI355X: the lanes beyond stride over the rest
    if (!solve)
      k_lin_b<Removal><<<(unsigned)std::min<size_t>(((size_t)N * k + 255) / 256, 2048), 256, 0, s>>>(st.Td, st.pairs, d_cand.p, d_rec.p, N, (int)k,
                                                                                                  d_B.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    assemble(st, B);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[2], s));
    const int fail = dense_spd_inverse(s, d_M.p, d_W.p, d_G.p, n);  // (synchronises the stream; the factor stays in d_M)
    HIPC(hipGetLastError());
    if (fail < 0) return call.refuse("scratch allocation of the inverse failed");
    if (after_inverse(s, fail)) return DPGO_ERR;
    HIPC(hipEventRecord(ev[3], s));
    if (launch_cov_logdet(s, d_M.p, n, ldet) || after_logdet(s)) return DPGO_ERR;
    k_lin_u<<<dim3((unsigned)((6 * (size_t)N + 63) / 64), (unsigned)((n + 63) / 64), 1), 256, 0, s>>>(B, d_G.p, d_U.p, 6 * N, n);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[4], s));
    z_and_figures(s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[5], s));
    k_lin_finish<Removal><<<(unsigned)(((size_t)N + np + 3) / 4), 256, 0, s>>>(st.Td, st.diag, st.pairs + 36 * nrect, d_pairs.p, N, (int)k, (int)np,
                                                                             B, d_U.p, z, oT, odx, odiag, opairs);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[6], s));
    h_out.resize(out_doubles());
    HIPC(hipMemcpyAsync(h_out.data(), d_out.p, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, s));
    ran = true;
    return DPGO_OK;
  }
};

// the arguments the two entry points share; cov_pairs may be null without pairs
struct LinearArgs {
  dpgo_team_t *t;
  const double *T;
  int method, max_block, num;
  const dpgo_measurement_t *recs;
  int num_pairs;
  const int *pairs;
  double *T_new, *delta, *cov_diag, *cov_pairs, *xi;
  dpgo_covariance_t *res;

  // the head of the outputs from a drained epilogue; returns what lies behind xi
  const double *copy_head(const std::vector<double> &h_out, int N) const {
    const double *h = h_out.data();
    std::memcpy(T_new, h, sizeof(double) * 12 * (size_t)N);
    std::memcpy(delta, h + (size_t)12 * N, sizeof(double) * 6 * (size_t)N);
    std::memcpy(cov_diag, h + (size_t)18 * N, sizeof(double) * 36 * (size_t)N);
    const double *hp = h + (size_t)54 * N;
    if (num_pairs > 0) std::memcpy(cov_pairs, hp, sizeof(double) * 36 * (size_t)num_pairs);
    hp += 36 * (size_t)num_pairs;
    std::memcpy(xi, hp, sizeof(double) * 6 * (size_t)num);
    return hp + 6 * (size_t)num;
  }
};

// An entry point up to the drained covariance path.  The refusals of the call itself come first, on the host, before any
// device work, with no output touched, in this order: null arguments (tail_null: one of the call's own outputs is), num,
// null records, num_pairs, null pairs, method; after_method() (int: DPGO_OK or a refusal made); check_team_local; per record
// its endpoints, ClosureCall::check (the removal's with the weight) and per_record(k, record); the range of the pairs; the
// budget.  app: the solve route (B is the path's X, the path is asked for the caller's pairs alone).  A refusal of the path or
// behind it leaves res as the path left it for the update and cleared for the removal.
template <bool Removal, class AfterMethod, class PerRecord>
int linear_call(const LinearArgs &a, bool tail_null, LinearEpilogue<Removal> &epi, CovApply *app, AfterMethod after_method,
                PerRecord per_record) {
  const ClosureCall &call = epi.call;
  const int num = a.num, num_pairs = a.num_pairs;
  if (!a.t || !a.T || !a.res || !a.T_new || !a.delta || !a.cov_diag || !a.xi || tail_null) return call.refuse("null argument");
  if (num <= 0) return call.refuse("num must be positive, not " + std::to_string(num));
  if (!a.recs) return call.refuse("null argument");
  if (num_pairs < 0) return call.refuse("num_pairs must not be negative, not " + std::to_string(num_pairs));
  if (num_pairs > 0 && (!a.pairs || !a.cov_pairs)) return call.refuse("null argument");
  if (call.check_method(a.method) || after_method()) return DPGO_ERR;
  if (check_team_local(a.t, call.name)) return DPGO_ERR;
  const std::vector<int> offs = pose_offsets(a.t);
  const int N = epi.N = offs.back();
  epi.cand.resize(num);
  if (Removal) epi.rec.resize(num);
  for (int k = 0; k < num; ++k) {
    int g[2];
    if (call.endpoints(a.t, offs, k, a.recs[k], g) || call.check(k, a.recs[k], Removal) || per_record(k, a.recs[k])) return DPGO_ERR;
    GateRec &c = epi.cand[k];
    std::memset(&c, 0, sizeof c);
    c.i = g[0]; c.j = g[1];
    pack_measurement(a.recs[k], c.m);
  }
  for (int k = 0; k < 2 * num_pairs; ++k)
    if (a.pairs[k] < 0 || a.pairs[k] >= N)
      return call.refuse("pair " + std::to_string(k / 2) + " names pose " + std::to_string(a.pairs[k]) + ", outside [0, " + std::to_string(N) + ")");
  const std::vector<int> poses = rank_endpoints(epi.cand);
  const int m = epi.m = (int)poses.size();
  if (app) {
    app->num_cols = 6 * num;
    epi.solve = app;
  }
  const size_t K = (size_t)num, np = epi.rect() + (size_t)num_pairs;
  HIPC(hipSetDevice(a.t->device));
  {
    // the pair blocks the path stages for this call, B and U, the matrix of order 6 K, the scratch of its inverse and G: the
    // rest is the path's own accounting
    const double blocks = 288.0 * (double)np, bu = 288.0 * (double)N * (double)K, mat = 288.0 * (double)K * (double)K;
    const double need = blocks + epi.bytes(N, (double)K, num_pairs);
    double avail = 0.0;
    if (call.device_avail(a.t, &avail)) return DPGO_ERR;
    char buf[480];
    if (app && (need - bu > avail || 36 * K * K > (size_t)1 << 40 || 6 * K > (size_t)INT32_MAX / 2)) {
      std::snprintf(buf, sizeof buf,
                    "%d %ss on %d of %d poses: the %zu pair blocks, U (6 N x 6 K; V and B are the covariance path's) and the three "
                    "matrices of order %zu need %.0f bytes (%.0f + %.0f + 3 x %.0f and the working arrays), %.0f are available on the device",
                    num, call.noun, m, N, np, 6 * K, need - bu, blocks, bu, mat, avail);
      return call.refuse(buf);
    }
    if (need > avail || np > (size_t)INT32_MAX || 36 * K * K > (size_t)1 << 40 || 6 * K > (size_t)INT32_MAX / 2) {
      std::snprintf(buf, sizeof buf,
                    "%d %ss on %d of %d poses: the %zu pair blocks, B and U (6 N x 6 K each) and the three matrices of order %zu need "
                    "%.0f bytes (%.0f + 2 x %.0f + 3 x %.0f and the working arrays), %.0f are available on the device; "
                    "the pair blocks must number at most %d",
                    num, call.noun, m, N, np, 6 * K, need, blocks, bu, mat, avail, INT32_MAX);
      return call.refuse(buf);
    }
  }
  // the rectangular set: block a N + p = Sigma_{p, e_a} (the paths check a pair for range only: p = e_a and p = 0 pass, the
  // first as the pair (i, i), which agrees with the diagonal block, the second as zeros); the caller's pairs behind them
  std::vector<int> all;
  all.reserve(2 * np);
  for (int e = 0; e < m && !app; ++e)
    for (int p = 0; p < N; ++p) { all.push_back(p); all.push_back(poses[e]); }
  all.insert(all.end(), a.pairs, a.pairs + 2 * (size_t)num_pairs);
  epi.user_pairs.assign(a.pairs, a.pairs + 2 * (size_t)num_pairs);
  if (epi.alloc()) return DPGO_ERR;
  const int rc = call.path(a.t, a.T, a.method, a.max_block, (int)np, all.data(), a.res, epi, app);
  if (rc && Removal) std::memset(a.res, 0, sizeof *a.res);  // (also when the path went through and the call itself refused behind it)
  return rc;
}

}  // namespace dpgo_cert

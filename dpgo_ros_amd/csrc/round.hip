// round.hip -- SE-Sync rounding of a team's iterate (Rosen et al. 2019, Alg. 2) and the suboptimality gap it bounds.
//
// X (r x 4N, team order) -> T (3 x 4N: R_i, t_i):  U = the top-3 left singular vectors of the rotation block Y (r x 3N), the
// eigenvectors of the r x r Gram matrix Y Y^T;  D = diag(1, 1, -1) when more poses have det(U^T Y_i) < 0 than > 0, else I;
// R_i = the nearest rotation to D U^T Y_i,  t_i = D U^T p_i;  then every pose relative to the first:  T_i <- T_0^-1 T_i.
// f_relaxed = 1/2 <X, X Q>, f_rounded = 1/2 <T, T Q> with the certificate's operator (Lambda off) and its fixed-order Gram:
// T in the library's 12-doubles-per-pose layout (R column-major, then t) IS a K = 3 block of the iterate layout.
//
// One lane per pose, no atomics: every sum is a wave reduction in a fixed order into one partial per workgroup, the
// partials summed in workgroup order -- two calls give the same bits.  The workspace is the team's certificate workspace
// (d_cert): nothing here writes a solver vector.
#include "certify_internal.h"
#include "device_math.h"

namespace dpgo {

constexpr int RD_WG = 64;  // poses per workgroup of the rounding kernels (one wave)

// sum over the 64 lanes of the wave in a fixed order; lane 0 holds it
__device__ __forceinline__ double rd_wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  return s;
}

// partial R x R Gram matrices of the rotation columns: part[blk * R * R + p * R + q] = sum over the workgroup's poses of
// sum_c Y_i[p][c] Y_i[q][c]
template <int R>
__global__ __launch_bounds__(RD_WG) void k_round_gram(const double *__restrict__ X, int N, double *__restrict__ part) {
  const int g = blockIdx.x * RD_WG + threadIdx.x;
  double y[3][R];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int a = 0; a < R; ++a) y[c][a] = (g < N) ? X[((size_t)4 * g + c) * R + a] : 0.0;
  double *out = part + (size_t)blockIdx.x * R * R;
#pragma unroll
  for (int p = 0; p < R; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) {
      const double s = rd_wave_sum(y[0][p] * y[0][q] + y[1][p] * y[1][q] + y[2][p] * y[2][q]);
      if (threadIdx.x == 0) {
        out[p * R + q] = s;
        out[q * R + p] = s;
      }
    }
}

// B = U^T [Y_i | p_i] (3 x 4, B[k][c]); U is r x 3 row-major on the device
template <int R>
__device__ __forceinline__ void rd_load_block(const double *__restrict__ X, const double *__restrict__ U, int g, double B[3][4]) {
  double x[4][R];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int a = 0; a < R; ++a) x[c][a] = X[((size_t)4 * g + c) * R + a];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < R; ++a) s += U[3 * a + k] * x[c][a];
      B[k][c] = s;
    }
}

// per workgroup: poses with det(U^T Y_i) < 0 and > 0 -> cnt[2 blk], cnt[2 blk + 1]
template <int R>
__global__ __launch_bounds__(RD_WG) void k_round_det(const double *__restrict__ X, const double *__restrict__ U, int N,
                                                     int *__restrict__ cnt) {
  const int g = blockIdx.x * RD_WG + threadIdx.x;
  double det = 0.0;
  if (g < N) {
    double B[3][4];
    rd_load_block<R>(X, U, g, B);
    det = rd_det3(B);
  }
  const unsigned long long neg = __ballot(det < 0.0), pos = __ballot(det > 0.0);
  if (threadIdx.x == 0) {
    cnt[2 * blockIdx.x] = __popcll(neg);
    cnt[2 * blockIdx.x + 1] = __popcll(pos);
  }
}

// ONE lane: the counts summed in workgroup order; flag[0] = -1 (reflect: D = diag(1, 1, -1)) when the negatives outnumber
// the positives, else +1 (a tie keeps U); flag[1], flag[2] = the counts
__global__ void k_round_sign(const int *__restrict__ cnt, int nblk, double *__restrict__ flag) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long neg = 0, pos = 0;
  for (int k = 0; k < nblk; ++k) {
    neg += cnt[2 * k];
    pos += cnt[2 * k + 1];
  }
  flag[0] = neg > pos ? -1.0 : 1.0;
  flag[1] = (double)neg;
  flag[2] = (double)pos;
}

// per pose: B = D U^T [Y_i | p_i]; T_i = [nearest rotation to B's 3 x 3 block | B's last column] (12 doubles: R column-major,
// then t); degenerate blocks of the workgroup -> deg[blk]
template <int R>
__global__ __launch_bounds__(RD_WG) void k_round_project(const double *__restrict__ X, const double *__restrict__ U,
                                                         const double *__restrict__ flag, int N, double *__restrict__ T,
                                                         int *__restrict__ deg) {
  const int g = blockIdx.x * RD_WG + threadIdx.x;
  bool dg = false;
  if (g < N) {
    double B[3][4];
    rd_load_block<R>(X, U, g, B);
    const double d3 = flag[0];
#pragma unroll
    for (int c = 0; c < 4; ++c) B[2][c] *= d3;
    double Rm[3][3];
    dg = rd_nearest_rotation(B, Rm);
    double *o = T + (size_t)12 * g;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) o[3 * c + k] = Rm[k][c];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[9 + k] = B[k][3];
  }
  const unsigned long long m = __ballot(dg);
  if (threadIdx.x == 0) deg[blockIdx.x] = __popcll(m);
}

// T_i <- T_0^-1 T_i  (R_0^T R_i, R_0^T (t_i - t_0)); the anchor, pose g0 of Tin, becomes exactly (I, 0).  T0: the anchor's
// 12 doubles (Tin + 12 g0 for one team; across teams its owner's, and g0 = -1 where the anchor lives elsewhere)
__global__ __launch_bounds__(RD_WG) void k_round_anchor(const double *__restrict__ Tin, const double *__restrict__ T0, int g0,
                                                        int N, double *__restrict__ Tout) {
  const int g = blockIdx.x * RD_WG + threadIdx.x;
  if (g >= N) return;
  double *o = Tout + (size_t)12 * g;
  if (g == g0) {
#pragma unroll
    for (int e = 0; e < 12; ++e) o[e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
    return;
  }
  double R0[9], t0[3], Ri[9], ti[3];  // column-major
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    R0[e] = T0[e];
    Ri[e] = Tin[(size_t)12 * g + e];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t0[k] = T0[9 + k];
    ti[k] = Tin[(size_t)12 * g + 9 + k] - t0[k];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k)  // (R_0^T R_i)[k][c] = sum_m R_0[m][k] R_i[m][c]
      o[3 * c + k] = R0[3 * k] * Ri[3 * c] + R0[3 * k + 1] * Ri[3 * c + 1] + R0[3 * k + 2] * Ri[3 * c + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) o[9 + k] = R0[3 * k] * ti[0] + R0[3 * k + 1] * ti[1] + R0[3 * k + 2] * ti[2];
}

}  // namespace dpgo

// =================================================================================================
// host side
using namespace dpgo;
using namespace dpgo_host;
using namespace dpgo_cert;

namespace {

// the rounding's workspace inside the certificate's (d_cert, d_cert_int, h_cert)
struct RoundWs {
  Cert c;
  int nbr = 0;  // workgroups of the per-pose kernels
  double *E = nullptr, *Tp = nullptr, *Ta = nullptr, *TE = nullptr, *rpart = nullptr, *Ud = nullptr, *flag = nullptr;
  double *T0 = nullptr;  // across teams: the anchor pose from its owner
  int *cnt = nullptr, *deg = nullptr;
  double *hG = nullptr, *hU = nullptr, *hS = nullptr, *hT = nullptr;
  int *hD = nullptr;
  // slots of c.G: 0 the rotation Gram, 1 X^T (X Q), 2 T^T (T Q)

  int setup(dpgo_team_t *t, Across *x = nullptr) {
    c.t = t;
    c.x = x;
    c.r = t->prm.r;
    c.K = 3;
    c.na = (int)t->ag.size();
    std::vector<int> offs(c.na + 1, 0);
    c.max_n = 0;
    for (int k = 0; k < c.na; ++k) {
      offs[k + 1] = offs[k] + t->ag[k]->n;
      c.max_n = std::max(c.max_n, t->ag[k]->n);
    }
    const int r = c.r, N = c.N = offs[c.na];
    c.L = 4 * N;
    c.nblk = (c.L + CG_CH - 1) / CG_CH;
    nbr = (N + RD_WG - 1) / RD_WG;
    const size_t Ls = (size_t)c.L, S = Cert::SLOT;
    const size_t need = 2 * r * Ls + 3 * 3 * Ls + (size_t)c.nblk * S + (size_t)nbr * r * r + 3 * S + 32 +
                        (x ? 16 + x->dev_doubles() : 0);
    const size_t ineed = (size_t)c.na + 1 + 3 * (size_t)nbr + (x ? x->dev_ints() : 0);
    const size_t hneed = 3 * S + (size_t)nbr + 3 * Ls;
    if (t->d_cert.alloc(need) || t->d_cert_int.alloc(ineed) || t->h_cert.alloc(hneed)) {
      set_err("round: workspace allocation failed");
      if (!x) return DPGO_ERR;
      x->fail_local("round: workspace allocation failed");
    }
    if (!c.halted()) {
      double *p = t->d_cert.p;
      auto take = [&](size_t n) { double *q = p; p += n; return q; };
      c.Xt = take(r * Ls); E = take(r * Ls);
      Tp = take(3 * Ls); Ta = take(3 * Ls); TE = take(3 * Ls);
      c.part = take((size_t)c.nblk * S); rpart = take((size_t)nbr * r * r);
      c.G = take(3 * S); Ud = take(24); flag = take(8);
      c.off = t->d_cert_int.p;
      cnt = c.off + c.na + 1;
      deg = cnt + 2 * nbr;
      hG = t->h_cert.p; hU = hG + S; hS = hU + S;
      hD = (int *)(hS + S);
      hT = hS + S + nbr;
      if (x) {
        T0 = take(16);
        x->place(p, deg + nbr, t->stream);
      }
    }
    CERT_CK(c, hipMemcpyAsync(c.off, offs.data(), sizeof(int) * (c.na + 1), hipMemcpyHostToDevice, t->stream));
    // the team's iterate, gathered in team order (agent arrays are r x 4n each: ld r)
    for (int k = 0; k < c.na; ++k)
      CERT_CK(c, hipMemcpyAsync(c.Xt + (size_t)4 * offs[k] * r, t->ag[k]->dev.buf[B_X], sizeof(double) * r * 4 * t->ag[k]->n,
                                hipMemcpyDeviceToDevice, t->stream));
    return 0;
  }

  // 1/2 <T, T Q> of the trajectory in Ta into slot 2
  void rounded_cost() {
    c.apply(3, Ta, 3, TE, 3, false);
    c.gram(Ta, 3, 3, TE, 3, 3, c.slot(2));
  }
};

}  // namespace

namespace dpgo_cert {

int team_measurements(dpgo_team_t *t, const std::vector<int> &offs, const char *what, std::vector<dpgo_measurement_t> &mm) {
  std::vector<dpgo_measurement_t> ma;
  mm.clear();
  for (size_t k = 0; k < t->ag.size(); ++k) {
    const int id = t->ag[k]->id;
    const int cntm = dpgo_agent_get_measurements(t, id, nullptr);
    if (cntm < 0) return DPGO_ERR;
    ma.resize(cntm);
    if (cntm > 0 && dpgo_agent_get_measurements(t, id, ma.data()) != cntm) return DPGO_ERR;
    for (const auto &m : ma) {
      if (m.r1 != m.r2 && std::min(m.r1, m.r2) != id) continue;
      const auto l1 = t->id2local.find(m.r1), l2 = t->id2local.find(m.r2);
      if (l1 == t->id2local.end() || l2 == t->id2local.end()) {
        set_err(std::string(what) + ": a measurement names a robot outside the team");
        return DPGO_ERR;
      }
      dpgo_measurement_t q = m;
      q.r1 = q.r2 = 0;
      q.p1 = offs[l1->second] + m.p1;
      q.p2 = offs[l2->second] + m.p2;
      mm.push_back(q);
    }
  }
  return 0;
}

}  // namespace dpgo_cert

extern "C" {

int dpgo_team_round(dpgo_team_t *t, int flags, double *T, dpgo_rounding_t *out) {
  if (!t || !T || !out) { set_err("round: null argument"); return DPGO_ERR; }
  if (check_team(t, "round")) return DPGO_ERR;
  RoundWs ws;
  if (ws.setup(t)) return DPGO_ERR;
  Cert &c = ws.c;
  const int r = c.r, N = c.N, nbr = ws.nbr;
  const size_t Ls = (size_t)c.L;
  // Gram matrix of the rotation block; f_relaxed queued behind it (the device runs it while the host solves for U)
  DPGO_DISPATCH_R(r, (k_round_gram<R><<<nbr, RD_WG, 0, t->stream>>>(c.Xt, N, ws.rpart)));
  c.sum_partials(ws.rpart, nbr, r * r, c.slot(0));
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(ws.hG, c.slot(0), sizeof(double) * r * r, hipMemcpyDeviceToHost, t->stream));
  c.apply(r, c.Xt, r, ws.E, r, false);
  c.gram(c.Xt, r, r, ws.E, r, r, c.slot(1));
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(t->stream));
  // U: eigenvectors of the 3 largest eigenvalues, descending (row-major r x 3)
  std::vector<double> A((size_t)r * r), w, V;
  for (int p = 0; p < r; ++p)
    for (int q = 0; q < r; ++q) A[(size_t)p * r + q] = 0.5 * (ws.hG[p * r + q] + ws.hG[q * r + p]);
  jacobi_eig(r, A, w, V);
  for (int a = 0; a < r; ++a)
    for (int k = 0; k < 3; ++k) ws.hU[3 * a + k] = V[(size_t)a * r + (r - 1 - k)];
  for (int k = 0; k < 8; ++k) out->sigma[k] = k < r ? std::sqrt(std::max(w[r - 1 - k], 0.0)) : 0.0;
  HIPC(hipMemcpyAsync(ws.Ud, ws.hU, sizeof(double) * 3 * r, hipMemcpyHostToDevice, t->stream));
  // determinant rule, projection, gauge
  DPGO_DISPATCH_R(r, (k_round_det<R><<<nbr, RD_WG, 0, t->stream>>>(c.Xt, ws.Ud, N, ws.cnt)));
  k_round_sign<<<1, 64, 0, t->stream>>>(ws.cnt, nbr, ws.flag);
  DPGO_DISPATCH_R(r, (k_round_project<R><<<nbr, RD_WG, 0, t->stream>>>(c.Xt, ws.Ud, ws.flag, N, ws.Tp, ws.deg)));
  k_round_anchor<<<nbr, RD_WG, 0, t->stream>>>(ws.Tp, ws.Tp, 0, N, ws.Ta);
  ws.rounded_cost();
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(ws.hT, ws.Ta, sizeof(double) * 3 * Ls, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipMemcpyAsync(ws.hS, c.slot(1), sizeof(double) * r * r, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipMemcpyAsync(ws.hS + 64, c.slot(2), sizeof(double) * 9, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipMemcpyAsync(ws.hS + 80, ws.flag, sizeof(double) * 3, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipMemcpyAsync(ws.hD, ws.deg, sizeof(int) * nbr, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipStreamSynchronize(t->stream));
  double fx = 0.0;
  for (int a = 0; a < r; ++a) fx += ws.hS[a * r + a];
  out->f_relaxed = 0.5 * fx;
  out->f_rounded = 0.5 * (ws.hS[64] + ws.hS[68] + ws.hS[72]);
  out->r = r;
  out->reflected = ws.hS[80] < 0.0 ? 1 : 0;
  out->refined = 0;
  int nd = 0;
  for (int k = 0; k < nbr; ++k) nd += ws.hD[k];
  out->num_degenerate = nd;
  std::memcpy(T, ws.hT, sizeof(double) * 3 * Ls);
  if (!(flags & DPGO_ROUND_REFINE_TRANSLATIONS)) return DPGO_OK;

  // translations given the rounded rotations: the team's measurements with their current weights in team-order numbering,
  // each shared edge once (the copy of the lower robot, which owns its weight)
  std::vector<int> offs(c.na + 1, 0);
  for (int k = 0; k < c.na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  std::vector<dpgo_measurement_t> mm;
  if (team_measurements(t, offs, "round", mm)) return DPGO_ERR;
  if (dpgo_translations_given_rotations(t->device, mm.data(), (int)mm.size(), N, T)) {
    set_err(std::string("round: ") + dpgo_last_error());
    return DPGO_ERR;
  }
  HIPC(hipSetDevice(t->device));
  std::memcpy(ws.hT, T, sizeof(double) * 3 * Ls);
  HIPC(hipMemcpyAsync(ws.Ta, ws.hT, sizeof(double) * 3 * Ls, hipMemcpyHostToDevice, t->stream));
  ws.rounded_cost();
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(ws.hS + 64, c.slot(2), sizeof(double) * 9, hipMemcpyDeviceToHost, t->stream));
  HIPC(hipStreamSynchronize(t->stream));
  out->f_rounded = 0.5 * (ws.hS[64] + ws.hS[68] + ws.hS[72]);
  out->refined = 1;
  return DPGO_OK;
}

}  // extern "C"

// ---- across teams (certify_across.hip): the same steps with the Grams, the determinant counts and the cost
// sums reduced over the participants in rank order, the anchor pose allgathered from its owner; projection, nearest rotation
// and determinant rule stay per pose and local
namespace {

constexpr int RD_REC = 21;  // doubles of one measurement in the refinement's allgather

void pack_measurement(const dpgo_measurement_t &m, double *o) {
  o[0] = m.r1; o[1] = m.p1; o[2] = m.r2; o[3] = m.p2;
  for (int k = 0; k < 9; ++k) o[4 + k] = m.R[k];
  for (int k = 0; k < 3; ++k) o[13 + k] = m.t[k];
  o[16] = m.kappa; o[17] = m.tau; o[18] = m.weight; o[19] = m.fixed_weight; o[20] = m.is_known_inlier;
}

dpgo_measurement_t unpack_measurement(const double *o) {
  dpgo_measurement_t m{};
  m.r1 = (int)o[0]; m.p1 = (int)o[1]; m.r2 = (int)o[2]; m.p2 = (int)o[3];
  for (int k = 0; k < 9; ++k) m.R[k] = o[4 + k];
  for (int k = 0; k < 3; ++k) m.t[k] = o[13 + k];
  m.kappa = o[16]; m.tau = o[17]; m.weight = o[18]; m.fixed_weight = (int)o[19]; m.is_known_inlier = (int)o[20];
  return m;
}

}  // namespace

extern "C" {

int dpgo_team_round_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, int flags, double *T,
                           dpgo_rounding_t *out) {
  Across x;
  if (x.begin(t, tr, owner_rank_of_robot, "round_across", 2, 3, flags, 0.0, 0.0, 0, (!T || !out) ? "null argument" : nullptr))
    return DPGO_ERR;
  RoundWs ws;
  if (ws.setup(t, &x)) return DPGO_ERR;
  Cert &c = ws.c;
  const int r = c.r, N = c.N, nbr = ws.nbr, na = c.na;
  const size_t Ls = (size_t)c.L;
  std::vector<int> offs(na + 1, 0);
  for (int k = 0; k < na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  // the rotation block's Gram matrix and X^T (X Q), one allgather
  if (!c.halted()) DPGO_DISPATCH_R(r, (k_round_gram<R><<<nbr, RD_WG, 0, t->stream>>>(c.Xt, N, ws.rpart)));
  c.sum_partials(ws.rpart, nbr, r * r, c.slot(0));
  c.apply(r, c.Xt, r, ws.E, r, false);
  c.gram(c.Xt, r, r, ws.E, r, r, c.slot(1));
  c.reduce({{c.slot(0), r * r}, {c.slot(1), r * r}});
  if (c.dead()) return x.fail();
  const double *red = x.reduced();
  std::vector<double> A((size_t)r * r), w, V, hU(3 * (size_t)r);
  for (int p = 0; p < r; ++p)
    for (int q = 0; q < r; ++q) A[(size_t)p * r + q] = 0.5 * (red[p * r + q] + red[q * r + p]);
  double fx = 0.0;
  for (int a = 0; a < r; ++a) fx += red[r * r + a * r + a];
  jacobi_eig(r, A, w, V);
  for (int a = 0; a < r; ++a)
    for (int k = 0; k < 3; ++k) hU[3 * a + k] = V[(size_t)a * r + (r - 1 - k)];
  for (int k = 0; k < 8; ++k) out->sigma[k] = k < r ? std::sqrt(std::max(w[r - 1 - k], 0.0)) : 0.0;
  CERT_CK(c, hipMemcpyAsync(ws.Ud, hU.data(), sizeof(double) * 3 * r, hipMemcpyHostToDevice, t->stream));
  // determinant rule: this team's counts (flag[1], flag[2]) summed over the participants, the sign on the host
  if (!c.halted()) {
    DPGO_DISPATCH_R(r, (k_round_det<R><<<nbr, RD_WG, 0, t->stream>>>(c.Xt, ws.Ud, N, ws.cnt)));
    k_round_sign<<<1, 64, 0, t->stream>>>(ws.cnt, nbr, ws.flag);
  }
  c.reduce({{ws.flag + 1, 2}});
  if (c.dead()) return x.fail();
  const double neg = x.reduced()[0], pos = x.reduced()[1];
  const std::vector<double> hflag{neg > pos ? -1.0 : 1.0, neg, pos};
  CERT_CK(c, hipMemcpyAsync(ws.flag, hflag.data(), sizeof(double) * 3, hipMemcpyHostToDevice, t->stream));
  if (!c.halted())
    DPGO_DISPATCH_R(r, (k_round_project<R><<<nbr, RD_WG, 0, t->stream>>>(c.Xt, ws.Ud, ws.flag, N, ws.Tp, ws.deg)));
  // the anchor (robot 0's first pose) from its owner, with the degenerate counts
  const auto l0 = t->id2local.find(0);
  const int g0 = l0 == t->id2local.end() ? -1 : offs[l0->second];
  std::vector<double> an(14, 0.0);
  std::vector<int> hdeg(nbr, 0);
  if (g0 >= 0) CERT_CK(c, hipMemcpyAsync(an.data() + 1, ws.Tp + (size_t)12 * g0, sizeof(double) * 12, hipMemcpyDeviceToHost, t->stream));
  CERT_CK(c, hipMemcpyAsync(hdeg.data(), ws.deg, sizeof(int) * nbr, hipMemcpyDeviceToHost, t->stream));
  CERT_CK(c, hipStreamSynchronize(t->stream));
  for (int k = 0; k < nbr; ++k) an[13] += hdeg[k];
  if (x.gather(an, x.hall)) return x.fail();
  const double *a0 = x.hall.data() + (size_t)14 * x.robot_holder[0];
  const std::vector<double> hT0(a0 + 1, a0 + 13);
  double nd = 0.0;
  for (int q = 0; q < x.world; ++q) nd += x.hall[(size_t)14 * q + 13];
  CERT_CK(c, hipMemcpyAsync(ws.T0, hT0.data(), sizeof(double) * 12, hipMemcpyHostToDevice, t->stream));
  if (!c.halted()) k_round_anchor<<<nbr, RD_WG, 0, t->stream>>>(ws.Tp, ws.T0, g0, N, ws.Ta);
  ws.rounded_cost();
  c.reduce({{c.slot(2), 9}});
  if (c.dead()) return x.fail();
  double f_rounded = 0.5 * (x.reduced()[0] + x.reduced()[4] + x.reduced()[8]);
  CERT_CK(c, hipGetLastError());
  CERT_CK(c, hipMemcpyAsync(T, ws.Ta, sizeof(double) * 3 * Ls, hipMemcpyDeviceToHost, t->stream));
  CERT_CK(c, hipStreamSynchronize(t->stream));
  out->f_relaxed = 0.5 * fx;
  out->f_rounded = f_rounded;
  out->r = r;
  out->reflected = hflag[0] < 0.0 ? 1 : 0;
  out->refined = 0;
  out->num_degenerate = (int)nd;
  if (!(flags & DPGO_ROUND_REFINE_TRANSLATIONS)) return x.finish() ? DPGO_ERR : DPGO_OK;

  // translations given the rounded rotations: every participant allgathers the measurements it owns with their current
  // weights (private ones; a shared edge from the copy of its lower robot) and the rounded rotations, and solves the same
  // problem in the global numbering (robots by id, then poses); each keeps its own poses' translations
  std::vector<double> recs;
  for (int k = 0; k < na && !x.bad; ++k) {
    const int id = t->ag[k]->id;
    const int cntm = dpgo_agent_get_measurements(t, id, nullptr);
    std::vector<dpgo_measurement_t> ma(std::max(cntm, 0));
    if (cntm < 0 || (cntm > 0 && dpgo_agent_get_measurements(t, id, ma.data()) != cntm)) { x.fail_local(g_err); break; }
    for (const auto &m : ma) {
      if (m.r1 != m.r2 && std::min(m.r1, m.r2) != id) continue;
      if (m.r1 < 0 || m.r1 >= x.num_robots || m.r2 < 0 || m.r2 >= x.num_robots) {
        x.fail_local("a measurement names a robot outside [0, num_robots)");
        break;
      }
      dpgo_measurement_t q = m;
      q.r1 = q.r2 = 0;
      q.p1 = (int)(x.robot_goff[m.r1] + m.p1);
      q.p2 = (int)(x.robot_goff[m.r2] + m.p2);
      recs.resize(recs.size() + RD_REC);
      pack_measurement(q, recs.data() + recs.size() - RD_REC);
    }
  }
  std::vector<double> cntv{0.0, (double)(recs.size() / RD_REC)};
  if (x.gather(cntv, x.hall)) return x.fail();
  std::vector<long long> nrec(x.world), nposes(x.world, 0);
  long long max_rec = 0, max_poses = 0;
  for (int q = 0; q < x.world; ++q) {
    nrec[q] = (long long)x.hall[2 * q + 1];
    max_rec = std::max(max_rec, nrec[q]);
  }
  for (int i = 0; i < x.num_robots; ++i) nposes[x.robot_holder[i]] += x.robot_n[i];
  for (int q = 0; q < x.world; ++q) max_poses = std::max(max_poses, nposes[q]);
  const size_t rl = 1 + (size_t)max_rec * RD_REC + (size_t)max_poses * 9;
  std::vector<double> rec(rl, 0.0);
  std::copy(recs.begin(), recs.end(), rec.begin() + 1);
  for (int g = 0; g < N; ++g)
    for (int e = 0; e < 9; ++e) rec[1 + (size_t)max_rec * RD_REC + (size_t)9 * g + e] = T[(size_t)12 * g + e];
  if (x.gather(rec, x.hall)) return x.fail();
  std::vector<dpgo_measurement_t> mm;
  std::vector<double> Tg((size_t)12 * x.nglob, 0.0);
  for (int q = 0; q < x.world; ++q) {
    const double *hq = x.hall.data() + (size_t)q * rl;
    for (long long e = 0; e < nrec[q]; ++e) mm.push_back(unpack_measurement(hq + 1 + (size_t)e * RD_REC));
    // participant q's poses in its team order
    std::vector<std::pair<int, int>> mine;
    for (int i = 0; i < x.num_robots; ++i)
      if (x.robot_holder[i] == q) mine.emplace_back(x.robot_lidx[i], i);
    std::sort(mine.begin(), mine.end());
    size_t g = 0;
    for (const auto &li : mine)
      for (int j = 0; j < x.robot_n[li.second]; ++j, ++g)
        for (int e = 0; e < 9; ++e)
          Tg[(size_t)12 * (x.robot_goff[li.second] + j) + e] = hq[1 + (size_t)max_rec * RD_REC + 9 * g + e];
  }
  if (!x.bad) {
    if (dpgo_translations_given_rotations(t->device, mm.data(), (int)mm.size(), (int)x.nglob, Tg.data()))
      x.fail_local(std::string("round: ") + dpgo_last_error());
    x.note(hipSetDevice(t->device), __LINE__);
  }
  if (!x.bad)
    for (int k = 0; k < na; ++k) {
      const long long go = x.robot_goff[t->ag[k]->id];
      for (int j = 0; j < t->ag[k]->n; ++j)
        for (int e = 9; e < 12; ++e) T[(size_t)12 * (offs[k] + j) + e] = Tg[(size_t)12 * (go + j) + e];
    }
  CERT_CK(c, hipMemcpyAsync(ws.Ta, T, sizeof(double) * 3 * Ls, hipMemcpyHostToDevice, t->stream));
  ws.rounded_cost();
  c.reduce({{c.slot(2), 9}});
  if (c.dead()) return x.fail();
  out->f_rounded = 0.5 * (x.reduced()[0] + x.reduced()[4] + x.reduced()[8]);
  out->refined = 1;
  return x.finish() ? DPGO_ERR : DPGO_OK;
}

}  // extern "C"

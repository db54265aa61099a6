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

__device__ __forceinline__ double rd_det3(const double A[3][4]) {
  return A[0][0] * (A[1][1] * A[2][2] - A[2][1] * A[1][2]) - A[0][1] * (A[1][0] * A[2][2] - A[2][0] * A[1][2]) +
         A[0][2] * (A[1][0] * A[2][1] - A[2][0] * A[1][1]);
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

// (v, p, q) a right-handed orthonormal frame for the unit vector v: p from the axis least aligned with v, q = v x p
__device__ __forceinline__ void rd_complement(const double v[3], double p[3], double q[3]) {
  int e = 0;
  if (fabs(v[1]) < fabs(v[e])) e = 1;
  if (fabs(v[2]) < fabs(v[e])) e = 2;
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = ((k == e) ? 1.0 : 0.0) - v[e] * v[k];
  const double n = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] /= n;
  q[0] = v[1] * p[2] - v[2] * p[1];
  q[1] = v[2] * p[0] - v[0] * p[2];
  q[2] = v[0] * p[1] - v[1] * p[0];
}

// nearest rotation to the 3 x 3 block A (A[k][c], c < 3), degenerate blocks included.  With A^T A = V diag(w) V^T (w
// descending: v1, v2, v3), w1 = A v1 / |A v1| and w2 = A v2 orthogonalised against w1 and normalised, the nearest rotation
// is w1 v1^T + w2 v2^T + det(V) (w1 x w2) v3^T -- for det A > 0 and det A < 0 alike -- and needs no division by the smallest
// singular value.  Returns true when that value is below 1e-12 of the largest (then the third direction is the cross
// product, and w2 an arbitrary unit vector orthogonal to w1 when the second is as small too; a zero block gives I).
__device__ __forceinline__ bool rd_nearest_rotation(const double A[3][4], double Rm[3][3]) {
  double S[9], w[3], V[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) S[3 * c + d] = A[0][c] * A[0][d] + A[1][c] * A[1][d] + A[2][c] * A[2][d];
  sym3_eig(S, w, V);
  int i1 = 0, i3 = 0;
  if (w[1] > w[i1]) i1 = 1;
  if (w[2] > w[i1]) i1 = 2;
  if (w[1] < w[i3]) i3 = 1;
  if (w[2] < w[i3]) i3 = 2;
  if (i3 == i1) i3 = (i1 + 1) % 3;  // (all three equal)
  const int i2 = 3 - i1 - i3;
  double v1[3], v2[3], v3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v1[c] = V[3 * c + i1];
    v2[c] = V[3 * c + i2];
    v3[c] = V[3 * c + i3];
  }
  double u1[3], u2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u1[k] = A[k][0] * v1[0] + A[k][1] * v1[1] + A[k][2] * v1[2];
    u2[k] = A[k][0] * v2[0] + A[k][1] * v2[1] + A[k][2] * v2[2];
  }
  const double s1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  if (!(s1 > 0.0)) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) Rm[k][c] = (k == c) ? 1.0 : 0.0;
    return true;
  }
  double w1[3] = {u1[0] / s1, u1[1] / s1, u1[2] / s1};
  if (w[i2] < 1e-4 * w[i1]) {
    // s2 < 1e-2 s1: v2 and v3, eigenvectors of A^T A, are resolved only to eps s1^2 / (s2^2 - s3^2) (1e-4 at singular
    // values 1, 1e-6, 1e-7), and the rotation built on them inherits that.  Resolve the complement of v1 as its own 2-D
    // problem instead: right-handed frames (v1, p, q) and (w1, s, t), C = [s t]^T A [p q], and the 2-D rotation nearest
    // to C maps (p, q) to (s, t); the answer is then determined to eps s1 / (s2 + s3), the problem's own conditioning.
    double p[3], q[3], s[3], t[3];
    rd_complement(v1, p, q);
    rd_complement(w1, s, t);
    double ap[3], aq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ap[k] = A[k][0] * p[0] + A[k][1] * p[1] + A[k][2] * p[2];
      aq[k] = A[k][0] * q[0] + A[k][1] * q[1] + A[k][2] * q[2];
    }
    const double c11 = s[0] * ap[0] + s[1] * ap[1] + s[2] * ap[2], c12 = s[0] * aq[0] + s[1] * aq[1] + s[2] * aq[2];
    const double c21 = t[0] * ap[0] + t[1] * ap[1] + t[2] * ap[2], c22 = t[0] * aq[0] + t[1] * aq[1] + t[2] * aq[2];
    // tr(R2^T C) = cos (c11 + c22) + sin (c21 - c12) is largest at the angle of (c11 + c22, c21 - c12)
    const double a = c11 + c22, b = c21 - c12;
    const double h = sqrt(a * a + b * b), h2 = sqrt((c11 - c22) * (c11 - c22) + (c21 + c12) * (c21 + c12));
    const double cs = h > 0.0 ? a / h : 1.0, sn = h > 0.0 ? b / h : 0.0;
    const double sg2 = 0.5 * (h + h2);  // the larger singular value of C: s2
    const bool degenerate = !(sg2 > 1e-12 * s1) || fabs(rd_det3(A)) < 1e-12 * s1 * s1 * sg2;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        Rm[k][c] = w1[k] * v1[c] + (cs * s[k] + sn * t[k]) * p[c] + (cs * t[k] - sn * s[k]) * q[c];
    return degenerate;
  }
  const double d12 = w1[0] * u2[0] + w1[1] * u2[1] + w1[2] * u2[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) u2[k] -= d12 * w1[k];
  double s2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  bool degenerate = false;
  if (!(s2 > 1e-12 * s1)) {
    // rank one: w2 from the axis least aligned with w1
    degenerate = true;
    int e = 0;
    if (fabs(w1[1]) < fabs(w1[e])) e = 1;
    if (fabs(w1[2]) < fabs(w1[e])) e = 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) u2[k] = ((k == e) ? 1.0 : 0.0) - w1[e] * w1[k];
    s2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  } else {
    // smallest singular value from |det A| = s1 s2 s3 (the eigenvalue of A^T A cannot resolve it below 1e-8 s1)
    if (fabs(rd_det3(A)) < 1e-12 * s1 * s1 * s2) degenerate = true;
  }
  const double w2[3] = {u2[0] / s2, u2[1] / s2, u2[2] / s2};
  const double detV = v1[0] * (v2[1] * v3[2] - v2[2] * v3[1]) - v1[1] * (v2[0] * v3[2] - v2[2] * v3[0]) +
                      v1[2] * (v2[0] * v3[1] - v2[1] * v3[0]);
  const double sg = detV < 0.0 ? -1.0 : 1.0;
  const double w3[3] = {sg * (w1[1] * w2[2] - w1[2] * w2[1]), sg * (w1[2] * w2[0] - w1[0] * w2[2]),
                        sg * (w1[0] * w2[1] - w1[1] * w2[0])};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) Rm[k][c] = w1[k] * v1[c] + w2[k] * v2[c] + w3[k] * v3[c];
  return degenerate;
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

// covariance_apply.hip -- X = Sigma V on the factors of a covariance path: the kernels behind the launch
// helpers of covariance_apply.h, and the public entry dpgo_team_covariance_apply.
//
// The path (covariance_nested.hip, covariance.hip) is handed a CovApply (certify_internal.h): it allocates V and X, has the
// hook write V once T is on the device, queues the products below between its own launches, and sets X before its epilogue
// runs.  Here the hook copies the caller's V to the device and the epilogue copies X back.
// Across teams (dpgo_team_covariance_apply_across; DESIGN.md 5m, "across teams") the path is covariance_schur_across with an
// ApplyStep, the path's AcrossStep with columns, that writes V the same way: its robots' steps queue u_a, W_a^T v_a and r_a, the r_a of every robot travel in its allgather C, and every
// participant forms x_S = Sigma_SS r_S itself.
// No floating-point atomics; every element's sum runs over k in index order: two calls give the same bytes.
#include <chrono>

#include "closure_frame.h"
#include "covariance_apply.h"

namespace dpgo {

// apply_tile for many products at once: the item rides on blockIdx.z, the grid covers the largest item and a tile outside
// its own item leaves at once
template <bool TA>
__global__ __launch_bounds__(256) void k_apply_gemm(const ApplyItem *__restrict__ items, int sub) {
  const ApplyItem g = items[blockIdx.z];
  const int i0 = 64 * blockIdx.x, j0 = 64 * blockIdx.y;
  if (i0 >= g.m || j0 >= g.n || g.k <= 0) return;
  apply_tile<TA>(g.A, g.lda, g.B, g.ldb, g.bmap, g.C, g.ldc, g.cmap, g.m, g.n, g.k, sub, i0, j0);
}

// R[r, c] = V[6 pose[r / 6] + r mod 6, c], one thread per element, r the faster index
__global__ __launch_bounds__(256) void k_apply_gather(const double *__restrict__ V, size_t ldv, const int *__restrict__ pose, int rows,
                                                      int cols, double *__restrict__ R) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)rows * cols) return;
  const int r = (int)(e % rows);
  const size_t c = e / rows;
  gp(R)[e] = gp(V)[c * ldv + apply_row(pose, r)];
}

// R[6 nb[i / 6] + i mod 6, c] -= P[i, c]: every element has one thread, the launches of two blocks are ordered on the stream
__global__ __launch_bounds__(256) void k_apply_scatter_sub(double *__restrict__ R, size_t ldr, const double *__restrict__ P, int K, int cols,
                                                           const int *__restrict__ nb) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * cols) return;
  const int i = (int)(e % K);
  const size_t c = e / K;
  double *r = R + c * ldr + apply_row(nb, i);
  gp(r)[0] = gp(r)[0] - gp(P)[e];
}

// D[drow(i), c] = S[srow(i), c] - P[i, c] (P null: nothing is subtracted), one thread per element, i the faster index; the rows
// of S and D through pose lists or the identity (apply_row)
__global__ __launch_bounds__(256) void k_apply_rows_sub(const double *__restrict__ S, size_t lds, const int *__restrict__ smap,
                                                        const double *__restrict__ P, double *__restrict__ D, size_t ldd,
                                                        const int *__restrict__ dmap, int K, int cols) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * cols) return;
  const int i = (int)(e % K);
  const size_t c = e / K;
  double v = gp(S)[c * lds + apply_row(smap, i)];
  if (P) v = v - gp(P)[e];
  gp(D)[c * ldd + apply_row(dmap, i)] = v;
}

}  // namespace dpgo

namespace dpgo_cert {

void launch_apply_gemm(hipStream_t s, bool ta, const ApplyItem *items_d, const ApplyItem *items_h, int count, bool sub) {
  int mm = 0, mn = 0, mk = 0;
  for (int q = 0; q < count; ++q) { mm = std::max(mm, items_h[q].m); mn = std::max(mn, items_h[q].n); mk = std::max(mk, items_h[q].k); }
  if (count <= 0 || mm <= 0 || mn <= 0 || mk <= 0) return;
  const dim3 grid((mm + 63) / 64, (mn + 63) / 64, count);
  if (ta) hipLaunchKernelGGL(k_apply_gemm<true>, grid, dim3(256), 0, s, items_d, sub ? 1 : 0);
  else hipLaunchKernelGGL(k_apply_gemm<false>, grid, dim3(256), 0, s, items_d, sub ? 1 : 0);
}

void launch_apply_gather(hipStream_t s, const double *V, size_t ldv, const int *pose, int count, int cols, double *R) {
  const size_t total = (size_t)6 * count * cols;
  if (total > 0) k_apply_gather<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(V, ldv, pose, 6 * count, cols, R);
}

void launch_apply_scatter_sub(hipStream_t s, double *R, size_t ldr, const double *P, int K, int cols, const int *nb) {
  const size_t total = (size_t)K * cols;
  if (total > 0) k_apply_scatter_sub<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(R, ldr, P, K, cols, nb);
}

void launch_apply_rows_sub(hipStream_t s, const double *S, size_t lds, const int *smap, const double *P, double *D, size_t ldd,
                           const int *dmap, int K, int cols) {
  const size_t total = (size_t)K * cols;
  if (total > 0) k_apply_rows_sub<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(S, lds, smap, P, D, ldd, dmap, K, cols);
}

double apply_flops(const ApplyItem *it, int count) {
  double f = 0.0;
  for (int q = 0; q < count; ++q) f += 2.0 * it[q].m * (double)it[q].n * it[q].k;
  return f;
}

namespace {

const ClosureCall APPLY = {"covariance_apply", "column"};

// the hook of the public call: V is the caller's
struct ApplyHost : CovApply {
  const double *V_host = nullptr;
  int rhs(const double *, int N, double *V, hipStream_t stream) override {
    HIPC(hipMemcpyAsync(V, V_host, sizeof(double) * 6 * (size_t)N * num_cols, hipMemcpyHostToDevice, stream));
    return DPGO_OK;
  }
};

// the step behind the path: X back to the caller
struct ApplyOut : ClosureEpilogue {
  ApplyHost *app = nullptr;
  double *X_host = nullptr;
  ApplyOut() : ClosureEpilogue(0) {}
  int run(const CovStage &st) override {
    if (!app->X) { set_err("covariance_apply: the covariance path formed no X"); return DPGO_ERR; }
    HIPC(hipMemcpyAsync(X_host, app->X, sizeof(double) * 6 * (size_t)st.N * app->num_cols, hipMemcpyDeviceToHost, st.stream));
    ran = true;
    return DPGO_OK;
  }
};

const ClosureCall APPLY_ACROSS = {"covariance_apply_across", "column"};

// the hook across teams: V is the caller's, X comes back into a host image that reaches the caller only when every
// participant has closed the call
struct ApplyAcross : ApplyStep {
  const double *V_host = nullptr;
  std::vector<double> X_image;
  bool ran = false;
  explicit ApplyAcross(int num_cols_) : ApplyStep(num_cols_) {}
  int rhs(const double *, int N, double *V, hipStream_t stream) override {
    HIPC(hipMemcpyAsync(V, V_host, sizeof(double) * 6 * (size_t)N * cols, hipMemcpyHostToDevice, stream));
    return DPGO_OK;
  }
  int taken(int N, hipStream_t stream) override {
    X_image.resize((size_t)6 * N * cols);
    HIPC(hipMemcpyAsync(X_image.data(), X, sizeof(double) * X_image.size(), hipMemcpyDeviceToHost, stream));
    ran = true;
    return DPGO_OK;
  }
};

// the first entry of V (ld rows, num_cols columns) outside rows [6 zero, 6 zero + 6) that is not finite: true and where
bool first_not_finite(const double *V, size_t ld, int num_cols, long long zero, size_t *row, int *column) {
  const size_t z0 = zero < 0 ? ld : (size_t)6 * zero;
  for (int c = 0; c < num_cols; ++c) {
    // (a column at a time by the exponent bits, which the compiler vectorises; the search for the entry only when there is one)
    const double *col = V + (size_t)c * ld;
    unsigned long long any = 0;
    for (size_t r = 0; r < ld; ++r) {
      unsigned long long b;
      std::memcpy(&b, col + r, sizeof b);
      any |= (unsigned long long)((b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull);
    }
    if (!any) continue;
    for (size_t r = 0; r < ld; ++r)
      if (!std::isfinite(col[r]) && (r < z0 || r >= z0 + 6)) { *row = r; *column = c; return true; }
  }
  return false;
}

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_covariance_apply_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot,
                                                 const double *T, int num_cols, const double *V, double *X, dpgo_covariance_t *res) {
  const ClosureCall &A = APPLY_ACROSS;
  const auto t_begin = std::chrono::steady_clock::now();
  if (res) std::memset(res, 0, sizeof *res);
  if (!t || !tr) return A.refuse("null argument");  // (nobody to tell)
  ApplyAcross app(num_cols);
  app.V_host = V;
  int N = 0;
  long long zero = -1;  // the team pose of the problem's pose 0, robot 0's first, when robot 0 lives here
  for (auto &a : t->ag) {
    if (a->id == 0) zero = N;
    N += a->n;
  }
  const size_t ld = (size_t)6 * N;
  // ---- the refusals of the call itself: decided here before any device work, told to everyone by the agreement record (a
  // participant that returned now would leave the others waiting)
  auto refusal = [&]() -> int {
    if (!owner_rank_of_robot || !T || !V || !X || !res) return A.refuse("null argument");
    if (num_cols <= 0) return A.refuse("num_cols must be positive, not " + std::to_string(num_cols));
    // V and X alone (the path accounts for the rest, and names it): decided before V is read
    const double vx = 2.0 * 8.0 * (double)ld * (double)num_cols;
    double avail = 0.0;
    if (hipSetDevice(t->device) != hipSuccess || A.device_avail(t, &avail)) return A.refuse("hipMemGetInfo failed");
    if (vx > avail) {
      char buf[300];
      std::snprintf(buf, sizeof buf, "V and X of %zu x %d need %.0f bytes on the device (2 x 8 x 6 N x num_cols), %.0f are available", ld,
                    num_cols, vx, avail);
      app.memerr = buf;
      return DPGO_OK;
    }
    size_t row = 0;
    int column = 0;
    if (first_not_finite(V, ld, num_cols, zero, &row, &column))
      return A.refuse("V is not finite at row " + std::to_string(row) + " (team pose " + std::to_string(row / 6) + ") of column " +
                      std::to_string(column));
    return DPGO_OK;
  };
  if (refusal()) app.argerr = A.refused();
  SchurAcrossArgs a(t, tr, owner_rank_of_robot, T);
  a.res = res;
  a.step = &app;
  if (const int rc = covariance_schur_across(a)) return rc;  // (res is then all zero)
  // (a problem of the anchor alone: nothing is free, the path staged nothing)
  if (app.ran) std::memcpy(X, app.X_image.data(), sizeof(double) * app.X_image.size());
  else std::memset(X, 0, sizeof(double) * ld * (size_t)num_cols);
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr,
                 "covariance_apply_across: rank %d of %d, %d columns on %d poses here, the apply's products %.3f ms (%.2f TFLOP/s), the whole "
                 "call %.3f ms\n",
                 tr->rank, tr->world, num_cols, N, app.ms_products, app.flops / (1e9 * std::max(app.ms_products, 1e-9)),
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  return DPGO_OK;
}

extern "C" int dpgo_team_covariance_apply(dpgo_team_t *t, const double *T, int method, int max_block, int num_cols, const double *V,
                                          double *X, dpgo_covariance_t *res) {
  const auto t_begin = std::chrono::steady_clock::now();
  if (res) std::memset(res, 0, sizeof *res);
  // ---- the refusals of the call itself: on the host, before any device work, X untouched
  if (!t || !T || !V || !X || !res) return APPLY.refuse("null argument");
  if (num_cols <= 0) return APPLY.refuse("num_cols must be positive, not " + std::to_string(num_cols));
  if (APPLY.check_method(method)) return DPGO_ERR;
  if (method == DPGO_GATE_SCHUR)
    return APPLY.refuse("there is no apply on the robot-wise Schur path: DPGO_GATE_NESTED (method=\"nested\") with no robot split has the "
                        "Schur path's sets");
  if (check_team_local(t, APPLY.name)) return DPGO_ERR;
  const int N = pose_offsets(t).back();
  const size_t ld = (size_t)6 * N;
  HIPC(hipSetDevice(t->device));
  {
    // V and X alone (the path accounts for the rest, and names it): decided before V is read
    const double vx = 2.0 * 8.0 * (double)ld * (double)num_cols;
    double avail = 0.0;
    if (APPLY.device_avail(t, &avail)) return DPGO_ERR;
    if (vx > avail) {
      char buf[300];
      std::snprintf(buf, sizeof buf, "V and X of %zu x %d need %.0f bytes on the device (2 x 8 x 6 N x num_cols), %.0f are available", ld,
                    num_cols, vx, avail);
      return APPLY.refuse(buf);
    }
  }
  size_t row = 0;
  int column = 0;
  if (first_not_finite(V, ld, num_cols, 0, &row, &column))
    return APPLY.refuse("V is not finite at row " + std::to_string(row) + " (pose " + std::to_string(row / 6) + ") of column " + std::to_string(column));
  ApplyHost app;
  app.num_cols = num_cols;
  app.V_host = V;
  ApplyOut out;
  out.app = &app;
  out.X_host = X;
  const int rc = method == DPGO_GATE_NESTED ? marginal_covariances_nested_call(t, T, max_block, 0, nullptr, nullptr, nullptr, res, &out, &app)
                                            : marginal_covariances_call(t, T, 0, 0, nullptr, nullptr, nullptr, res, &out, &app);
  if (rc != DPGO_OK) return rc;
  // (a team of the anchor alone: nothing is free, the path staged nothing)
  if (!out.ran) std::memset(X, 0, sizeof(double) * ld * (size_t)num_cols);
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing)
    std::fprintf(stderr, "covariance_apply: %d columns on %d poses, the apply's products %.3f ms (%.2f TFLOP/s), the whole call %.3f ms\n",
                 num_cols, N, app.ms_products, app.flops / (1e9 * std::max(app.ms_products, 1e-9)),
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  return DPGO_OK;
}

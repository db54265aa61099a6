// certify_internal.h -- the certificate's device workspace and host helpers (certify.hip), shared with the rounding of a
// certified point (round.hip).  The kernels stay in certify.hip; Cert's launching methods are defined there.
#pragma once
#include <initializer_list>
#include <string>
#include <vector>

#include "kernel_common.h"
#include "team_internal.h"

namespace dpgo {

constexpr int CG_CH = 128;   // columns per workgroup of a Gram launch
constexpr int CG_MAXK = 24;  // most rows of either operand (the 3K-row basis at K = 8)

// OUT = beta OUT + sum_t s_t A_t C_t, one thread per element (column, q).  C_t row-major k_t x ko on the device (null:
// the identity, k_t = ko).  No A_t may alias OUT.
struct CertTerm {
  const double *A;
  const double *C;
  int lda, ka;
  double s;
};
struct CertTerms {
  CertTerm t[3];
  int n;
};

}  // namespace dpgo

namespace dpgo_cert {
using namespace dpgo;
using namespace dpgo_host;

// cyclic Jacobi eigendecomposition of a symmetric n x n matrix (row-major): ascending eigenvalues w, eigenvectors as the
// columns of V (row-major, V[i * n + k] = component i of vector k)
void jacobi_eig(int n, std::vector<double> A, std::vector<double> &w, std::vector<double> &V);

// the certificate's device state for one call
struct Cert {
  dpgo_team_t *t = nullptr;
  int r = 0, K = 0, na = 0, N = 0, L = 0, max_n = 0, nz = 0;  // nz: rows of the orthonormal deflation basis Zo
  bool deflate = true, precond = true;
  double *Xt = nullptr, *E = nullptr, *lam = nullptr, *Zr = nullptr, *Zo = nullptr;
  double *U[2] = {nullptr, nullptr}, *AU[2] = {nullptr, nullptr}, *T = nullptr, *T2 = nullptr;
  double *part = nullptr, *G = nullptr, *gmax = nullptr;
  int *off = nullptr;
  int gstride = 0, nblk = 0;
  static constexpr int SLOT = CG_MAXK * CG_MAXK;
  // Gram slots: 0 basis x operator, 1 basis x basis, 2 residual x residual, 3 Cholesky failure word (read back together),
  // 4 X^T S X, 5 deflation products, 6 Cholesky coefficients, 7 coefficients from the host
  double *slot(int k) const { return G + (size_t)k * SLOT; }

  int setup(int K_);
  void apply(int k, const double *V, int ldv, double *out, int ldo, bool with_lam);
  void gram(const double *A, int lda, int ka, const double *B, int ldb, int kb, double *out);
  // out[o] = sum over the nblk partials part[k * m + o], in k order (one workgroup)
  void sum_partials(const double *p, int nblk_, int m, double *out);
  void update(double *out, int ldo, int ko, double beta, std::initializer_list<CertTerm> terms);
  // V <- V - Zo^T (Zo V^T): onto the complement of the deflation basis
  void project(double *V, int ld, int k);
  // rows of V orthonormal: V <- L^-1 V (CholQR) through scratch S (k rows, ld k)
  void cholqr(double *V, int ld, int k, double *S);
  void precondition(const double *V, int ldv, double *out, int ldo);
};

// every robot local and INITIALIZED, every neighbour inside the team; descriptors synchronised.  `what` prefixes the message.
int check_team(dpgo_team_t *t, const char *what);

}  // namespace dpgo_cert

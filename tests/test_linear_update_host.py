"""CPU check of csrc/linear_update_block.h, the block arithmetic of k_upd_b, k_upd_m and k_upd_finish, compiled
for the host: a stand-alone program forms B, M and xi from blocks of the numpy inverse with the functions the kernels call,
inverts M by a plain Cholesky of its own, and reduces, closes and retracts every pose and requested pair; the result stays
within the bounds of tests/updateref.py against the longdouble reference.  The largest error / bound ratios are printed
(DESIGN.md 5j records them)."""
import os
import shutil
import subprocess

import numpy as np

from tests import covnested_ref as NR
from tests import covref
from tests import jointref as J
from tests import updateref as R
from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "linear_update_block.h"
using namespace dpgo;
// in: K, m, N, P as doubles; T (12 N); diag (36 N); the N m rectangular blocks; the P pair blocks; the P pairs (2 doubles each);
// K records of 16 doubles (the first two hold the four ints i, j, rank of i, rank of j).
// out: B (36 N K, column-major, ld 6 N), M (36 K^2), xi (6 K), dx (6 N), T' (12 N), Sigma' diagonal (36 N), Sigma' pairs (36 P),
// xi_post (6 K), d2_joint, logdet_M, logdet_R
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const int K = (int)in[0], m = (int)in[1], N = (int)in[2], P = (int)in[3];
  const double *T = in.data() + 4, *diag = T + 12 * N, *rect = diag + 36 * N, *pblk = rect + 36 * (size_t)N * m, *pidx = pblk + 36 * P,
               *recs = pidx + 2 * P;
  if (in.size() != 4 + 48 * (size_t)N + 36 * (size_t)N * m + 38 * (size_t)P + 16 * (size_t)K) return 4;
  const size_t ld = 6 * (size_t)N, n = 6 * (size_t)K;
  std::vector<double> B(ld * n), M(n * n), xi(n), Rij(9 * K), tij(3 * K);
  std::vector<JointEnds> ends(K);
  for (int k = 0; k < K; ++k) {
    int ids[4];
    std::memcpy(ids, recs + 16 * k, sizeof ids);
    JointEnds &e = ends[k];
    e.i = ids[0]; e.j = ids[1]; e.ri = ids[2]; e.rj = ids[3];
    double Ri[3][3], Rj[3][3], ti[3], tj[3];
    gate_load_pose(T, e.i, Ri, ti);
    gate_load_pose(T, e.j, Rj, tj);
    gate_jacobians(Ri, ti, Rj, tj, *(double(*)[3][3])&Rij[9 * k], &tij[3 * k], e.Ji, e.Jj);
    for (int p = 0; p < N; ++p) {
      double Si[6][6], Sj[6][6], Bk[6][6];
      gate_load36(rect + 36 * upd_block_index(N, e.ri, p), Si);
      gate_load36(rect + 36 * upd_block_index(N, e.rj, p), Sj);
      upd_b_block(Si, Sj, e.Ji, e.Jj, Bk);
      for (int c = 0; c < 6; ++c)
        for (int a = 0; a < 6; ++a) B[(6 * (size_t)k + c) * ld + 6 * p + a] = Bk[a][c];
    }
  }
  for (int k = 0; k < K; ++k)
    for (int l = k; l < K; ++l) {
      double Gb[6][6];
      const int way = joint_orientation(ends[k].i, ends[k].j, ends[l].i, ends[l].j);
      const int kk = way < 0 ? l : k, ll = way < 0 ? k : l;
      upd_m_block(B.data(), ld, ends[kk], ll, Gb);
      if (k != l) {
        if (way == 0) joint_symmetrise(Gb);
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) M[(6 * kk + a) * n + 6 * ll + b] = M[(6 * ll + b) * n + 6 * kk + a] = Gb[a][b];
        continue;
      }
      const double *v = recs + 16 * k + 2;
      double S[6][6], x[6];
      joint_diagonal(Gb, v[12], v[13], S);
      gate_innovation(*(double(*)[3][3])&Rij[9 * k], &tij[3 * k], v, x);
      for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) M[(6 * k + a) * n + 6 * k + b] = S[a][b];
        xi[6 * k + a] = x[a];
      }
    }
  // G = M^-1 by a plain Cholesky (the device has dense_spd_inverse for this), log det M beside it
  std::vector<double> L(n * n, 0.0), Li(n * n, 0.0), G(n * n, 0.0);
  double logdet_M = 0.0;
  for (size_t c = 0; c < n; ++c) {
    double p = M[c * n + c];
    for (size_t q = 0; q < c; ++q) p -= L[c * n + q] * L[c * n + q];
    if (!(p > 0.0)) return 6;
    L[c * n + c] = std::sqrt(p);
    logdet_M += 2.0 * std::log(L[c * n + c]);
    for (size_t r = c + 1; r < n; ++r) {
      double v = M[r * n + c];
      for (size_t q = 0; q < c; ++q) v -= L[r * n + q] * L[c * n + q];
      L[r * n + c] = v / L[c * n + c];
    }
  }
  for (size_t c = 0; c < n; ++c)
    for (size_t r = c; r < n; ++r) {
      double v = r == c ? 1.0 : 0.0;
      for (size_t q = c; q < r; ++q) v -= L[r * n + q] * Li[q * n + c];
      Li[r * n + c] = v / L[r * n + r];
    }
  for (size_t r = 0; r < n; ++r)
    for (size_t c = 0; c < n; ++c) {
      double v = 0.0;
      for (size_t q = (r > c ? r : c); q < n; ++q) v += Li[q * n + r] * Li[q * n + c];
      G[r * n + c] = v;
    }
  std::vector<double> z(n), U(ld * n), post(n);
  double d2 = 0.0, logdet_R = 0.0;
  for (size_t r = 0; r < n; ++r) {
    double s = 0.0;
    for (size_t c = 0; c < n; ++c) s = __builtin_fma(G[c * n + r], xi[c], s);
    z[r] = s;
    const double *v = recs + 16 * (r / 6) + 2;
    post[r] = s * (r % 6 < 3 ? 1.0 / (2.0 * v[12]) : 1.0 / v[13]);
  }
  for (size_t c = 0; c < n; ++c) d2 = __builtin_fma(xi[c], z[c], d2);
  for (int k = 0; k < K; ++k) logdet_R += upd_logdet_meas(recs[16 * k + 14], recs[16 * k + 15]);
  for (size_t c = 0; c < n; ++c)
    for (size_t r = 0; r < ld; ++r) {
      double s = 0.0;
      for (size_t q = 0; q < n; ++q) s = __builtin_fma(B[q * ld + r], G[c * n + q], s);
      U[c * ld + r] = s;
    }
  std::vector<double> dx(6 * N), Tn(12 * N), Sd(36 * N), Sp(36 * (size_t)P);
  for (int p = 0; p < N; ++p) {
    double acc[UPD_SUMS] = {0.0};
    for (size_t c = 0; c < n; ++c) upd_accumulate(&U[c * ld + 6 * p], &B[c * ld + 6 * p], z[c], acc);
    double Sn[6][6], d[6], Rp[3][3], tp[3], Rn[3][3], tn[3];
    lin_close_pose<false>(diag + 36 * p, acc, Sn, d);
    gate_load_pose(T, p, Rp, tp);
    upd_retract(Rp, tp, d, Rn, tn);
    upd_store_pose(Rn, tn, &Tn[12 * p]);
    std::memcpy(&Sd[36 * p], Sn, sizeof Sn);
    std::memcpy(&dx[6 * p], d, sizeof d);
  }
  for (int e = 0; e < P; ++e) {
    const int p = (int)pidx[2 * e], q = (int)pidx[2 * e + 1];
    double acc[36] = {0.0};
    for (size_t c = 0; c < n; ++c) upd_accumulate_pair(&U[c * ld + 6 * p], &B[c * ld + 6 * q], acc);
    for (int x = 0; x < 36; ++x) Sp[36 * e + x] = pblk[36 * e + x] - acc[x];
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  std::vector<double> sc = {d2, logdet_M, logdet_R};
  for (const std::vector<double> *v : {&B, &M, &xi, &dx, &Tn, &Sd, &Sp, &post, &sc})
    if (std::fwrite(v->data(), sizeof(double), v->size(), f) != v->size()) return 5;
  std::fclose(f);
  return 0;
}
"""


def test_host_build_of_the_block_stays_within_the_bounds(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "update_host.cpp", tmp_path / "update_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    n, K = 12, 12
    m, T = NR.banded_chain(n, 2, window=8)
    Sigma = covref.dense_reference(covref.q_full(m, n), T, n)[1]
    Sigma = 0.5 * (Sigma + Sigma.T)
    # pose 0 at either end, a pair and its reverse, two exact duplicates
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, K, 5, outliers=0.0, fixed=((0, 5), (5, 0), (3, 9), (9, 3)))
    dup = np.r_[np.arange(K - 2), 4, 7]
    ends, Rm, tm, kap, ta = ends[dup], Rm[dup], tm[dup], kap[dup], ta[dup]
    poses = sorted(set(ends.reshape(-1).tolist()))
    pairs = np.array([(0, 4), (7, 7), (3, 9), (9, 3), (11, 1), (2, 0)])
    blk = J.blocks_from_sigma(Sigma)
    diag = np.array([blk(a, a) for a in range(n)])
    cross = np.array([blk(a, b) for a, b in np.r_[R.rect_pairs(poses, n), pairs]])
    rec = np.zeros((K, 16))
    rec[:, :2] = np.array([[i, j, poses.index(i), poses.index(j)] for i, j in ends], dtype=np.int32).view(F)
    rec[:, 2:11], rec[:, 11:14], rec[:, 14], rec[:, 15] = Rm.reshape(K, 9), tm, kap, ta
    np.concatenate([[K, len(poses), n, len(pairs)], T, diag.reshape(-1), cross.reshape(-1), pairs.reshape(-1).astype(F),
                    rec.reshape(-1)]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin")
    sizes = [36 * n * K, 36 * K * K, 6 * K, 6 * n, 12 * n, 36 * n, 36 * len(pairs), 6 * K, 3]
    assert out.size == sum(sizes)
    B, M, xi, dx, Tn, Sd, Sp, post, sc = np.split(out, np.cumsum(sizes)[:-1])
    got = dict(B=B.reshape(6 * K, 6 * n).T, M=M.reshape(6 * K, 6 * K), xi=xi.reshape(K, 6), delta=dx.reshape(n, 6), T=Tn,
               cov_diag=Sd.reshape(n, 6, 6), cov_pairs=Sp.reshape(-1, 6, 6), xi_post=post.reshape(K, 6), d2_joint=sc[0], logdet_M=sc[1],
               logdet_R=sc[2])
    ref = R.update(T, ends, Rm, tm, kap, ta, R.blocks_from_rect(poses, n, diag, cross), n, pairs=pairs)
    b = R.bounds(ref, T, ends, tm, n, pairs)
    assert (got["M"] == got["M"].T).all(), "M is not bitwise symmetric"
    assert (got["cov_diag"] == got["cov_diag"].transpose(0, 2, 1)).all(), "a diagonal block of Sigma' is not bitwise symmetric"
    assert (got["delta"][0] == 0).all() and (got["T"][:12] == T[:12]).all() and (got["B"][:6] == 0).all()
    worst = {}
    for key in ("B", "M", "xi", "delta", "T", "cov_diag", "cov_pairs", "xi_post", "d2_joint", "logdet_M", "logdet_R"):
        worst[key] = R.ratio(np.asarray(got[key] - np.asarray(ref[key], dtype=F)), b[key])
    print("host build of linear_update_block.h, %d closures on %d of %d poses, cond_2(M) = %.3g: largest error / bound: "
          % (K, len(poses), n, b["cond_M"]) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # duplicated records: identical rows of M against every third closure, identical innovations
    for a, c in ((4, K - 2), (7, K - 1)):
        assert got["xi"][a].tobytes() == got["xi"][c].tobytes()
        assert (got["M"][6 * a:6 * a + 6] == got["M"][6 * c:6 * c + 6])[:, np.repeat(~np.isin(np.arange(K), (a, c)), 6)].all()

"""CPU check of csrc/linear_removal_block.h, the block arithmetic of k_rem_b, k_rem_n, k_rem_z and k_rem_finish,
compiled for the host: a stand-alone program forms B~, N~, xi and every record's pivot_min from blocks of the numpy inverse with
the functions the kernels call, inverts N~ by a plain Cholesky of its own, and reduces, closes and retracts every pose and
requested pair; the result stays within the bounds of tests/removalref.py against the longdouble reference.  cond_2(N~) and
the largest error / bound ratios are printed (DESIGN.md 5l records them)."""
import os
import shutil
import subprocess

import numpy as np

from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import removalref as V
from tests import updateref as R
from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "linear_removal_block.h"
using namespace dpgo;
// in: K, m, N, P as doubles; T (12 N); diag (36 N); the N m rectangular blocks; the P pair blocks; the P pairs (2 doubles each);
// K records of 16 doubles (the first two hold the four ints i, j, rank of i, rank of j) and K RemRec.
// out: B~ (36 N K, column-major, ld 6 N), N~ (36 K^2), xi (6 K), dx (6 N), T' (12 N), Sigma' diagonal (36 N), Sigma' pairs (36 P),
// xi_loo (6 K), pivot_min (K), d2_joint, logdet_N, logdet_R, pivot_min_joint
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
  if (in.size() != 4 + 48 * (size_t)N + 36 * (size_t)N * m + 38 * (size_t)P + (16 + REM_REC) * (size_t)K) return 4;
  const RemRec *rem = (const RemRec *)(recs + 16 * (size_t)K);
  const size_t ld = 6 * (size_t)N, n = 6 * (size_t)K;
  std::vector<double> B(ld * n), M(n * n), xi(n), xit(n), pmin(K), Rij(9 * K), tij(3 * K);
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
      rem_scale_columns(Bk, rem[k].s_rot, rem[k].s_trn);
      for (int c = 0; c < 6; ++c)
        for (int a = 0; a < 6; ++a) B[(6 * (size_t)k + c) * ld + 6 * p + a] = Bk[a][c];
    }
  }
  for (int k = 0; k < K; ++k)
    for (int l = k; l < K; ++l) {
      double Gb[6][6];
      const int way = joint_orientation(ends[k].i, ends[k].j, ends[l].i, ends[l].j);
      const int kk = way < 0 ? l : k, ll = way < 0 ? k : l;
      const RemRec &r = rem[kk];
      rem_n_block(B.data(), ld, ends[kk], ll, r.s_rot, r.s_trn, Gb);
      if (k != l) {
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) M[(6 * kk + a) * n + 6 * ll + b] = M[(6 * ll + b) * n + 6 * kk + a] = Gb[a][b];
        continue;
      }
      const double *v = recs + 16 * k + 2;
      double S[6][6], x[6], xt[6];
      rem_diagonal(Gb, S);
      gate_innovation(*(double(*)[3][3])&Rij[9 * k], &tij[3 * k], v, x);
      rem_whiten(x, r.s_rot, r.s_trn, xt);
      pmin[k] = rem_pivot_min(S);
      for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) M[(6 * k + a) * n + 6 * k + b] = S[a][b];
        xi[6 * k + a] = x[a];
        xit[6 * k + a] = xt[a];
      }
    }
  // G~ = N~^-1 by a plain Cholesky (the device has dense_spd_inverse for this), log det N~ and the smallest pivot beside it
  std::vector<double> L(n * n, 0.0), Li(n * n, 0.0), Gm(n * n, 0.0);
  double logdet = 0.0, pj = INFINITY;
  for (size_t c = 0; c < n; ++c) {
    double p = M[c * n + c];
    for (size_t q = 0; q < c; ++q) p -= L[c * n + q] * L[c * n + q];
    if (!(p > 0.0)) return 6;
    pj = p < pj ? p : pj;
    L[c * n + c] = std::sqrt(p);
    logdet += 2.0 * std::log(L[c * n + c]);
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
      Gm[r * n + c] = v;
    }
  std::vector<double> z(n), U(ld * n), loo(n);
  double d2 = 0.0, logdet_R = 0.0;
  for (size_t r = 0; r < n; ++r) {
    double s = 0.0;
    for (size_t c = 0; c < n; ++c) s = __builtin_fma(Gm[c * n + r], xit[c], s);
    z[r] = s;
    loo[r] = s / rem_s((int)(r % 6), rem[r / 6].s_rot, rem[r / 6].s_trn);
  }
  for (size_t c = 0; c < n; ++c) d2 = __builtin_fma(xit[c], z[c], d2);
  for (int k = 0; k < K; ++k) logdet_R += rem_logdet_r(rem[k].kappa, rem[k].tau, rem[k].dw);
  for (size_t c = 0; c < n; ++c)
    for (size_t r = 0; r < ld; ++r) {
      double s = 0.0;
      for (size_t q = 0; q < n; ++q) s = __builtin_fma(B[q * ld + r], Gm[c * n + q], s);
      U[c * ld + r] = s;
    }
  std::vector<double> dx(6 * N), Tn(12 * N), Sd(36 * N), Sp(36 * (size_t)P);
  for (int p = 0; p < N; ++p) {
    double acc[UPD_SUMS] = {0.0};
    for (size_t c = 0; c < n; ++c) upd_accumulate(&U[c * ld + 6 * p], &B[c * ld + 6 * p], z[c], acc);
    double Sn[6][6], d[6], Rp[3][3], tp[3], Rn[3][3], tn[3];
    lin_close_pose<true>(diag + 36 * p, acc, Sn, d);
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
    for (int x = 0; x < 36; ++x) Sp[36 * e + x] = pblk[36 * e + x] + acc[x];
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  std::vector<double> sc = {d2, logdet + logdet_R, logdet_R, pj};
  for (const std::vector<double> *v : {&B, &M, &xi, &dx, &Tn, &Sd, &Sp, &loo, &pmin, &sc})
    if (std::fwrite(v->data(), sizeof(double), v->size(), f) != v->size()) return 5;
  std::fclose(f);
  return 0;
}
"""


def test_host_build_of_the_block_stays_within_the_bounds(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "removal_host.cpp", tmp_path / "removal_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    n = 12
    m, T = NR.banded_chain(n, 2, window=8)
    # the closure (0, 6) is in the graph a second time, stated as 6 -> 0: a reversed statement has its lever arm at the other
    # pose and is other information, so a record and its reverse are both in the graph only when the graph holds both
    e06 = [e for e in range(len(m)) if (int(m["p1"][e]), int(m["p2"][e])) == (0, 6)][0]
    back = m[e06:e06 + 1].copy()
    back["p1"], back["p2"] = 6, 0
    R60, t60 = G.relative_pose(T, 6, 0, F)
    back["R"], back["t"] = np.asarray(R60).reshape(1, 9), np.asarray(t60).reshape(1, 3)
    m = np.concatenate([m, back])
    Sigma = covref.dense_reference(covref.q_full(m, n), T, n)[1]
    Sigma = 0.5 * (Sigma + Sigma.T)
    e911, e911b = [e for e in range(len(m)) if (int(m["p1"][e]), int(m["p2"][e])) == (9, 11)]
    # (edge, w, w', kappa and tau as multiples of the edge's): pose 0 at either end -- a closure removed fully and its reverse
    # halved --, a closure and two odometry edges at partial weights 0.5 and 0.37 taken out, one of them in the graph at 0.8 by
    # the record's own word; and two parallel records on the ordered pair (9, 11) whose noise is not proportional (the graph
    # holds the edge twice; the second record claims a quarter of its edge's kappa): their block of N~ is not symmetric
    plan = [(e06, 1.0, 0.0, 1.0, 1.0), (len(m) - 1, 1.0, 0.5, 1.0, 1.0), (e911, 1.0, 0.63, 1.0, 1.0), (2, 1.0, 0.5, 1.0, 1.0),
            (9, 0.8, 0.3, 1.0, 1.0), (e911b, 1.0, 0.0, 0.25, 1.0)]
    K = len(plan)
    rng = np.random.default_rng(3)
    ends, Rm, tm = np.zeros((K, 2), dtype=np.int64), np.zeros((K, 3, 3)), np.zeros((K, 3))
    for k, e in enumerate(p[0] for p in plan):
        i, j = int(m["p1"][e]), int(m["p2"][e])
        Rij, tij = G.relative_pose(T, i, j, F)
        x = rng.standard_normal(6)
        x = 0.05 * x / np.linalg.norm(x)
        ends[k], Rm[k], tm[k] = (i, j), Rij @ covref.exp_so3(-x[:3]), tij - x[3:]
    kap = np.array(m["kappa"][[p[0] for p in plan]], dtype=F) * np.array([p[3] for p in plan])
    ta = np.array(m["tau"][[p[0] for p in plan]], dtype=F) * np.array([p[4] for p in plan])
    w, w_new = np.array([p[1] for p in plan]), np.array([p[2] for p in plan])
    dw = w - w_new
    poses = sorted(set(ends.reshape(-1).tolist()))
    pairs = np.array([(0, 4), (7, 7), (3, 9), (9, 3), (11, 1), (2, 0)])
    blk = J.blocks_from_sigma(Sigma)
    diag = np.array([blk(a, a) for a in range(n)])
    cross = np.array([blk(a, b) for a, b in np.r_[R.rect_pairs(poses, n), pairs]])
    rec = np.zeros((K, 16))
    rec[:, :2] = np.array([[i, j, poses.index(i), poses.index(j)] for i, j in ends], dtype=np.int32).view(F)
    rec[:, 2:11], rec[:, 11:14], rec[:, 14], rec[:, 15] = Rm.reshape(K, 9), tm, kap, ta
    rem = np.zeros((K, 8))
    rem[:, 0], rem[:, 1], rem[:, 2], rem[:, 3] = kap, ta, w, dw
    rem[:, 4], rem[:, 5] = np.sqrt(2.0 * kap * dw), np.sqrt(ta * dw)
    np.concatenate([[K, len(poses), n, len(pairs)], T, diag.reshape(-1), cross.reshape(-1), pairs.reshape(-1).astype(F),
                    rec.reshape(-1), rem.reshape(-1)]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin")
    sizes = [36 * n * K, 36 * K * K, 6 * K, 6 * n, 12 * n, 36 * n, 36 * len(pairs), 6 * K, K, 4]
    assert out.size == sum(sizes)
    B, M, xi, dx, Tn, Sd, Sp, loo, pm, sc = np.split(out, np.cumsum(sizes)[:-1])
    got = dict(Bt=B.reshape(6 * K, 6 * n).T, Nt=M.reshape(6 * K, 6 * K), xi=xi.reshape(K, 6), delta=dx.reshape(n, 6), T=Tn,
               cov_diag=Sd.reshape(n, 6, 6), cov_pairs=Sp.reshape(-1, 6, 6), xi_loo=loo.reshape(K, 6), pivot_min=pm, d2_joint=sc[0],
               logdet_N=sc[1], logdet_R=sc[2], pivot_min_joint=sc[3])
    ref = V.removal(T, ends, Rm, tm, kap, ta, w, w_new, R.blocks_from_rect(poses, n, diag, cross), n, pairs=pairs)
    assert ref["testable"] and float(ref["pivot_min_joint"]) >= 1e-3
    b = V.bounds(ref, T, ends, tm, n, pairs)
    assert (got["Nt"] == got["Nt"].T).all(), "N~ is not bitwise symmetric"
    par = np.asarray(ref["Nt"], dtype=F)[12:18, 30:36]
    assert np.abs(par - par.T).max() > 1e6 * b["Nt"][12:18, 30:36].max(), "the parallel records' block is meant to be unsymmetric"
    assert (got["cov_diag"] == got["cov_diag"].transpose(0, 2, 1)).all(), "a diagonal block of Sigma' is not bitwise symmetric"
    assert (got["delta"][0] == 0).all() and (got["T"][:12] == T[:12]).all() and (got["Bt"][:6] == 0).all()
    assert (got["cov_diag"][0] == 0).all() and (got["cov_pairs"][0] == 0).all() and (got["cov_pairs"][5] == 0).all()
    worst = {}
    for key in ("Bt", "Nt", "xi", "delta", "T", "cov_diag", "cov_pairs", "xi_loo", "pivot_min", "d2_joint", "logdet_N", "logdet_R", "pivot_min_joint"):
        worst[key] = V.ratio(np.asarray(got[key] - np.asarray(ref[key], dtype=F)), b[key])
    print("host build of linear_removal_block.h, %d records on %d of %d poses, cond_2(N~) = %.3g, smallest pivot %.3g: largest error / bound: "
          % (K, len(poses), n, b["cond_N"], got["pivot_min_joint"]) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # the removal gives uncertainty back: every diagonal block grows
    assert (np.einsum("gaa->g", got["cov_diag"]) >= np.einsum("gaa->g", diag) * (1 - 1e-12)).all()

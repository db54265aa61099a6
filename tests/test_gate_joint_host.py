"""CPU check of csrc/gate_joint_block.h, the block arithmetic of k_joint_blocks and k_joint_step, compiled for
the host: a stand-alone program forms M, xi and the marginal d2 from blocks of the numpy inverse and runs one greedy
elimination with the functions the kernels call, and the result stays within the bounds of tests/jointref.py against the
longdouble reference.  The largest error / bound ratios are printed (DESIGN.md 5i records them)."""
import os
import shutil
import subprocess

import numpy as np

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gate_joint_block.h"
using namespace dpgo;
// in: K, m, N, thr2 as doubles; T (12 N); diag (36 N); the m (m - 1) / 2 pair blocks; K records of 16 doubles (the first two
// hold the four ints i, j, rank of i, rank of j).  out: M (36 K^2), xi (6 K), d2 (K), xi_cond (6 K), d2_cond (K), rank (K)
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const int K = (int)in[0], m = (int)in[1], N = (int)in[2];
  const double thr2 = in[3];
  const double *T = in.data() + 4, *diag = T + 12 * N, *pairs = diag + 36 * N, *recs = pairs + 36 * (size_t)(m * (m - 1) / 2);
  if (in.size() != 4 + 48 * (size_t)N + 36 * (size_t)(m * (m - 1) / 2) + 16 * (size_t)K) return 4;
  const size_t ld = 6 * (size_t)K;
  std::vector<double> M(ld * ld), xi(6 * K), d2(K), xc(6 * K), d2c(K), D(36 * K), W(36 * (size_t)K * K);
  std::vector<int> state(K, 0), rank(K, -1);
  std::vector<JointEnds> ends(K);
  std::vector<double> Rij(9 * K), tij(3 * K);
  for (int k = 0; k < K; ++k) {
    int ids[4];
    std::memcpy(ids, recs + 16 * k, sizeof ids);
    JointEnds &e = ends[k];
    e.i = ids[0]; e.j = ids[1]; e.ri = ids[2]; e.rj = ids[3];
    double Ri[3][3], Rj[3][3], ti[3], tj[3];
    gate_load_pose(T, e.i, Ri, ti);
    gate_load_pose(T, e.j, Rj, tj);
    gate_jacobians(Ri, ti, Rj, tj, *(double(*)[3][3])&Rij[9 * k], &tij[3 * k], e.Ji, e.Jj);
  }
  for (int k = 0; k < K; ++k)
    for (int l = k; l < K; ++l) {
      double Gb[6][6];
      const int way = joint_orientation(ends[k].i, ends[k].j, ends[l].i, ends[l].j);
      const int kk = way < 0 ? l : k, ll = way < 0 ? k : l;
      joint_block(diag, pairs, m, ends[kk], ends[ll], Gb);
      if (k != l) {
        if (way == 0) joint_symmetrise(Gb);
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) M[(6 * kk + a) * ld + 6 * ll + b] = M[(6 * ll + b) * ld + 6 * kk + a] = Gb[a][b];
        continue;
      }
      const double *v = recs + 16 * k + 2;
      double S[6][6], x[6];
      joint_diagonal(Gb, v[12], v[13], S);
      gate_innovation(*(double(*)[3][3])&Rij[9 * k], &tij[3 * k], v, x);
      for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) M[(6 * k + a) * ld + 6 * k + b] = D[36 * k + 6 * a + b] = S[a][b];
        xi[6 * k + a] = xc[6 * k + a] = x[a];
      }
      d2[k] = d2c[k] = gate_distance(S, x);
    }
  for (int s = 0; s < K; ++s) {  // greedy
    double dp = INFINITY;
    int p = -1;
    for (int k = 0; k < K; ++k)
      if (state[k] == 0) joint_better(d2c[k], k, dp, p);
    if (!(p >= 0 && dp <= thr2)) break;
    double L[6][6], y[6];
    bool ok;
    std::memcpy(L, &D[36 * p], sizeof L);
    gate_cholesky(L, ok);
    (void)gate_forward(L, &xc[6 * p], y);
    state[p] = 1;
    rank[p] = s;
    for (int r = 0; r < K; ++r) {
      if (state[r] != 0) continue;
      double Gb[6][6], Dr[6][6], xr[6];
      for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) Gb[a][b] = M[(6 * r + a) * ld + 6 * p + b];
        xr[a] = xc[6 * r + a];
      }
      std::memcpy(Dr, &D[36 * r], sizeof Dr);
      for (int q = 0; q < s; ++q) joint_subtract_product(&W[36 * ((size_t)q * K + r)], &W[36 * ((size_t)q * K + p)], Gb);
      d2c[r] = joint_row_update(Gb, L, y, Dr, xr);
      std::memcpy(&W[36 * ((size_t)s * K + r)], Gb, sizeof Gb);
      std::memcpy(&D[36 * r], Dr, sizeof Dr);
      std::memcpy(&xc[6 * r], xr, sizeof xr);
    }
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  std::vector<double> rk(rank.begin(), rank.end());
  for (const std::vector<double> *v : {&M, &xi, &d2, &xc, &d2c, &rk})
    if (std::fwrite(v->data(), sizeof(double), v->size(), f) != v->size()) return 5;
  std::fclose(f);
  return 0;
}
"""


def test_host_build_of_the_block_stays_within_the_bounds(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "joint_host.cpp", tmp_path / "joint_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    n, K = 12, 40
    thr2 = capi.error_threshold_at_quantile(0.99, 6) ** 2
    m, T = NR.banded_chain(n, 2, window=8)
    Sigma = covref.dense_reference(covref.q_full(m, n), T, n)[1]
    Sigma = 0.5 * (Sigma + Sigma.T)
    # pose 0 both ways round, a pair and its reverse, a shared pose, exact duplicates
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, 5, fixed=((0, 5), (5, 0), (3, 9), (9, 3), (3, 7), (2, 3)))
    dup = np.r_[np.arange(K - 2), 4, 7]
    ends, Rm, tm, kap, ta = ends[dup], Rm[dup], tm[dup], kap[dup], ta[dup]
    poses = sorted(set(ends.reshape(-1).tolist()))
    blk = J.blocks_from_sigma(Sigma)
    diag = np.array([blk(a, a) for a in range(n)])
    cross = np.array([blk(a, b) for a, b in J.all_pairs(poses)])
    rec = np.zeros((K, 16))
    rec[:, :2] = np.array([[i, j, poses.index(i), poses.index(j)] for i, j in ends], dtype=np.int32).view(F)
    rec[:, 2:11], rec[:, 11:14], rec[:, 14], rec[:, 15] = Rm.reshape(K, 9), tm, kap, ta
    np.concatenate([[K, len(poses), n, thr2], T, diag.reshape(-1), cross.reshape(-1), rec.reshape(-1)]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin")
    assert out.size == 36 * K * K + 15 * K
    M, rest = out[:36 * K * K].reshape(6 * K, 6 * K), out[36 * K * K:]
    xi, d2, xc, d2c, rank = rest[:6 * K].reshape(K, 6), rest[6 * K:7 * K], rest[7 * K:13 * K].reshape(K, 6), rest[13 * K:14 * K], rest[14 * K:].astype(int)
    worst = dict(M=0.0, xi=0.0, d2=0.0, xi_cond=0.0, d2_cond=0.0)
    # M, xi and the marginal d2 against the reference on the same blocks
    assert (M == M.T).all(), "M is not bitwise symmetric"
    Mref = J.joint_M(T, ends, kap, ta, J.blocks_from_pairs(poses, diag, cross))
    xref = J.innovations(T, ends, Rm, tm)
    for k, (ik, jk) in enumerate(ends):
        for l, (il, jl) in enumerate(ends):
            b = J.m_block_bound(T, ik, jk, il, jl, blk)
            e = np.abs(M[6 * k:6 * k + 6, 6 * l:6 * l + 6] - np.asarray(Mref[6 * k:6 * k + 6, 6 * l:6 * l + 6], dtype=F))
            assert (e <= b).all(), (k, l)
            worst["M"] = max(worst["M"], (e[b > 0] / b[b > 0]).max(initial=0.0))
        b_x = G.xi_bound(T, ik, jk, tm[k])
        b_s = J.m_block_bound(T, ik, jk, ik, jk, blk)
        gx, gd, _, S = G.gate(T, ik, jk, Rm[k], tm[k], kap[k], ta[k], diag[ik], diag[jk], blk(ik, jk))
        b_d = G.d2_bound(gx, S, gd, b_x, b_s)
        worst["xi"] = max(worst["xi"], (np.abs(xi[k] - np.asarray(xref[k], dtype=F)) / b_x).max())
        worst["d2"] = max(worst["d2"], abs(d2[k] - float(gd)) / b_d)
        assert (np.abs(xi[k] - np.asarray(xref[k], dtype=F)) <= b_x).all() and abs(d2[k] - float(gd)) <= b_d
    # duplicated records: identical marginal bits, the lower index first
    for a, b in ((4, K - 2), (7, K - 1)):
        assert xi[a].tobytes() == xi[b].tobytes() and d2[a] == d2[b]
        assert not (rank[b] >= 0 and (rank[a] < 0 or rank[a] > rank[b])), "the lower index of a duplicated record goes first"
        assert (M[6 * a:6 * a + 6] == M[6 * b:6 * b + 6])[:, np.repeat(~np.isin(np.arange(K), (a, b)), 6)].all()
    # the elimination: the program's own order replayed in the reference on the program's own M and xi
    acc = np.argsort(np.where(rank >= 0, rank, K), kind="stable")[:(rank >= 0).sum()]
    assert 4 <= len(acc) < K
    ref = J.run(M, xi, thr2, "greedy", pivots=acc)
    conds = J.prefix_conditions(M, acc)
    assert (ref["rank"] == rank).all()
    for s in ref["steps"]:
        k, cA = s["k"], conds[s["n_acc"]]
        b_x, b_d = J.conditional_bounds(s, cA)
        accepted_here = s["n_acc"] < len(acc) and acc[s["n_acc"]] == k
        assert (s["d2"][k] <= thr2) == accepted_here
        assert s["d2"][k] <= s["d2"][s["choice"]] + J.conditional_bounds(s, cA, s["choice"])[1] + b_d
        for r in (sorted(s["rows"]) if s["stop"] else [k]):  # (the stop: every candidate left has its final values)
            b_x, b_d = J.conditional_bounds(s, cA, r)
            ex, ed = np.abs(xc[r] - np.asarray(ref["xi_cond"][r], dtype=F)), abs(d2c[r] - float(ref["d2_cond"][r]))
            worst["xi_cond"] = max(worst["xi_cond"], (ex / b_x).max())
            worst["d2_cond"] = max(worst["d2_cond"], ed / b_d)
            assert (ex <= b_x).all() and ed <= b_d, (r, s["n_acc"], ex / b_x, ed / b_d)
    print("host build of gate_joint_block.h, %d candidates on %d poses, %d accepted, cond_2(M_AA) = %.3g: largest error / bound: "
          % (K, len(poses), len(acc), conds[-1]) + ", ".join("%s %.3g" % kv for kv in worst.items()))

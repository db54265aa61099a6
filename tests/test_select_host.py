"""CPU check of csrc/select_block.h, the block arithmetic of k_select_open and k_select_step, compiled for the
host: a stand-alone program forms the diagonal blocks and the marginal gains from blocks of the numpy inverse and runs one
greedy selection and one in the given order with the functions the kernels call, the pivot's block column of M formed on the
fly, and the result stays within the bounds of tests/selectref.py against the longdouble reference.  The largest error / bound
ratios are printed (DESIGN.md 5k records them)."""
import os
import shutil
import subprocess

import numpy as np

from tests import covnested_ref as NR
from tests import covref
from tests import jointref as J
from tests import selectref as S
from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "select_block.h"
using namespace dpgo;
// in: P, m, N, budget, order (0 greedy, 1 given) as doubles; T (12 N); diag (36 N); the m (m - 1) / 2 pair blocks; P records of
// 16 doubles (the first two hold the four ints i, j, rank of i, rank of j; kappa and tau are doubles 14 and 15).
// out: D as opened (36 P), gain (P), gain_cond (P), rank (P), gain_total, logdet_joint
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const int P = (int)in[0], m = (int)in[1], N = (int)in[2], budget = (int)in[3], given = (int)in[4];
  const double *T = in.data() + 5, *diag = T + 12 * N, *pairs = diag + 36 * N, *recs = pairs + 36 * (size_t)(m * (m - 1) / 2);
  if (in.size() != 5 + 48 * (size_t)N + 36 * (size_t)(m * (m - 1) / 2) + 16 * (size_t)P) return 4;
  std::vector<double> D0(36 * P), D(36 * P), lm(P), gain(P), gc(P), W(36 * (size_t)budget * P), at, ld;
  std::vector<int> state(P, 0), rank(P, -1);
  std::vector<JointEnds> ends(P);
  for (int k = 0; k < P; ++k) {  // k_select_open
    int ids[4];
    std::memcpy(ids, recs + 16 * k, sizeof ids);
    JointEnds &e = ends[k];
    e.i = ids[0]; e.j = ids[1]; e.ri = ids[2]; e.rj = ids[3];
    double Ri[3][3], Rj[3][3], ti[3], tj[3], Rij[3][3], tij[3], G[6][6], Sd[6][6];
    gate_load_pose(T, e.i, Ri, ti);
    gate_load_pose(T, e.j, Rj, tj);
    gate_jacobians(Ri, ti, Rj, tj, Rij, tij, e.Ji, e.Jj);
    joint_block(diag, pairs, m, e, e, G);
    const double kappa = recs[16 * k + 14], tau = recs[16 * k + 15];
    joint_diagonal(G, kappa, tau, Sd);
    lm[k] = select_logdet_meas(kappa, tau);
    gain[k] = gc[k] = select_gain(Sd, lm[k]);
    std::memcpy(&D0[36 * k], Sd, sizeof Sd);
    std::memcpy(&D[36 * k], Sd, sizeof Sd);
  }
  for (int s = 0; s < budget; ++s) {  // k_select_step
    double gp = -INFINITY;
    int p = -1;
    if (given) { p = s; gp = gc[s]; }
    else
      for (int k = 0; k < P; ++k)
        if (state[k] == 0) select_better(gc[k], k, gp, p);
    if (!(p >= 0 && gp > -INFINITY)) break;
    double L[6][6];
    bool ok;
    std::memcpy(L, &D[36 * p], sizeof L);
    gate_cholesky(L, ok);
    state[p] = 1;
    rank[p] = s;
    at.push_back(gp);
    ld.push_back(joint_logdet(L));
    for (int r = 0; r < P; ++r) {
      if (state[r] != 0) continue;
      int ka, kb;
      bool sym;
      const bool tr = select_cross_order(r, ends[r].i, ends[r].j, p, ends[p].i, ends[p].j, ka, kb, sym);
      double Gb[6][6], Dr[6][6];
      select_cross(diag, pairs, m, ends[ka], ends[kb], tr, sym, Gb);
      std::memcpy(Dr, &D[36 * r], sizeof Dr);
      for (int q = 0; q < s; ++q) joint_subtract_product(&W[36 * ((size_t)q * P + r)], &W[36 * ((size_t)q * P + p)], Gb);
      gc[r] = select_row_update(Gb, L, Dr, lm[r]);
      std::memcpy(&W[36 * ((size_t)s * P + r)], Gb, sizeof Gb);
      std::memcpy(&D[36 * r], Dr, sizeof Dr);
    }
  }
  double gt = 0.0, lj = 0.0;  // k_select_finish
  for (size_t q = 0; q < at.size(); ++q) { gt += at[q]; lj += ld[q]; }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  std::vector<double> rk(rank.begin(), rank.end()), sc = {gt, lj};
  for (const std::vector<double> *v : {&D0, &gain, &gc, &rk, &sc})
    if (std::fwrite(v->data(), sizeof(double), v->size(), f) != v->size()) return 5;
  std::fclose(f);
  return 0;
}
"""


def test_host_build_of_the_block_stays_within_the_bounds(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "select_host.cpp", tmp_path / "select_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    n, P, budget = 12, 40, 12
    m, T = NR.banded_chain(n, 2, window=8)
    Sigma = covref.dense_reference(covref.q_full(m, n), T, n)[1]
    Sigma = 0.5 * (Sigma + Sigma.T)
    # pose 0 both ways round, a pair and its reverse, a shared pose, and two exact duplicates at the end
    ends, kap, ta = S.seeded_pool(T, n, P, 5, fixed=((0, 5), (5, 0), (3, 9), (9, 3), (3, 7), (2, 3)), duplicates=((4, P - 2), (7, P - 1)))
    poses = sorted(set(ends.reshape(-1).tolist()))
    blk = J.blocks_from_sigma(Sigma)
    diag = np.array([blk(a, a) for a in range(n)])
    cross = np.array([blk(a, b) for a, b in J.all_pairs(poses)])
    rec = np.zeros((P, 16))
    rec[:, :2] = np.array([[i, j, poses.index(i), poses.index(j)] for i, j in ends], dtype=np.int32).view(F)
    rec[:, 2:11], rec[:, 14], rec[:, 15] = np.eye(3).reshape(-1), kap, ta
    Mref = J.joint_M(T, ends, kap, ta, J.blocks_from_pairs(poses, diag, cross))
    ldR = S.logdet_meas(kap, ta)
    bD = [S.d_bound(T, int(i), int(j), blk) for i, j in ends]
    worst = {}
    for order in ("greedy", "given"):
        np.concatenate([[P, len(poses), n, budget, order == "given"], T, diag.reshape(-1), cross.reshape(-1), rec.reshape(-1)]).tofile(tmp_path / "in.bin")
        subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        raw = np.fromfile(tmp_path / "out.bin")
        assert raw.size == 39 * P + 2
        D0, rest = raw[:36 * P].reshape(P, 6, 6), raw[36 * P:]
        rank = rest[2 * P:3 * P].astype(int)
        out = dict(gain=rest[:P], gain_cond=rest[P:2 * P], rank=rank, num_selected=int((rank >= 0).sum()), gain_total=rest[3 * P],
                   logdet_joint=rest[3 * P + 1])
        out["selected"] = np.argsort(np.where(rank >= 0, rank, P), kind="stable")[:out["num_selected"]]
        assert out["num_selected"] == budget
        # D_k within the block bound, bitwise symmetric; the marginal gains; duplicated records: identical bits
        assert D0.tobytes() == np.ascontiguousarray(D0.transpose(0, 2, 1)).tobytes()
        for k in range(P):
            e = np.abs(D0[k] - np.asarray(Mref[6 * k:6 * k + 6, 6 * k:6 * k + 6], dtype=F))
            worst["D"] = max(worst.get("D", 0.0), (e / bD[k]).max())
            assert (e <= bD[k]).all(), k
        S.check_marginal(out, Mref, ldR, bD, worst)
        for a, b in ((4, P - 2), (7, P - 1)):
            assert out["gain"][a] == out["gain"][b] and D0[a].tobytes() == D0[b].tobytes()
            if order == "greedy":  # the duplicate of lower index goes first; its copy is then worth less
                assert not (rank[b] >= 0 and (rank[a] < 0 or rank[a] > rank[b])), "the lower index of a duplicated record goes first"
                if rank[a] >= 0:
                    assert out["gain_cond"][b] < out["gain_cond"][a]
        # the selection: the program's own order replayed in the reference
        S.check_replay(out, Mref, ldR, bD, order, budget, worst)
        if order == "greedy":
            assert list(out["selected"]) != list(range(budget))
            greedy = out
        else:
            assert list(out["selected"]) == list(range(budget)) and out["gain_total"] <= greedy["gain_total"]
    conds = J.prefix_conditions(Mref, greedy["selected"])
    print("host build of select_block.h, %d candidates on %d poses, budget %d, cond_2(M_AA) = %.3g: largest error / bound: "
          % (P, len(poses), budget, conds[-1]) + ", ".join("%s %.3g" % kv for kv in worst.items()))

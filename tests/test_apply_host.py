"""CPU check of csrc/apply_block.h, the block arithmetic of k_apply_rhs_closures, compiled for the host: a
stand-alone program writes V = A^T for 12 closures with the functions the kernel calls -- the Jacobians of k_upd_b, then
apply_rhs_closure -- and every entry stays within 4 u |J| of the longdouble A of tests/updateref.py; pose 0's rows are zero."""
import os
import shutil
import subprocess

import numpy as np

from tests import covnested_ref as NR
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
#include "apply_block.h"
using namespace dpgo;
// in: K, N as doubles; T (12 N); K pairs of endpoints (2 doubles each).  out: V (6 N x 6 K, column-major, ld 6 N)
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const int K = (int)in[0], N = (int)in[1];
  if (in.size() != 2 + 12 * (size_t)N + 2 * (size_t)K) return 4;
  const double *T = in.data() + 2, *ends = T + 12 * N;
  const size_t ld = 6 * (size_t)N;
  std::vector<double> V(ld * 6 * K, 0.0);
  for (int k = 0; k < K; ++k) {
    const int i = (int)ends[2 * k], j = (int)ends[2 * k + 1];
    double Ri[3][3], Rj[3][3], ti[3], tj[3], Rij[3][3], tij[3], Ji[6][6], Jj[6][6];
    gate_load_pose(T, i, Ri, ti);
    gate_load_pose(T, j, Rj, tj);
    gate_jacobians(Ri, ti, Rj, tj, Rij, tij, Ji, Jj);
    apply_rhs_closure(Ji, Jj, i, j, k, ld, V.data());
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(V.data(), sizeof(double), V.size(), f) != V.size()) return 5;
  std::fclose(f);
  return 0;
}
"""


def test_host_build_of_the_block_writes_the_transposed_A(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "apply_host.cpp", tmp_path / "apply_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    n, K = 12, 12
    m, T = NR.banded_chain(n, 2, window=8)
    # pose 0 at either end, a pair and its reverse, two exact duplicates
    ends = J.seeded_batch(T, n, K, 5, outliers=0.0, fixed=((0, 5), (5, 0), (3, 9), (9, 3)))[0]
    ends = ends[np.r_[np.arange(K - 2), 4, 7]]
    np.concatenate([[K, n], T, ends.reshape(-1).astype(F)]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    V = np.fromfile(tmp_path / "out.bin").reshape(6 * K, 6 * n).T
    A = R.a_full(T, ends, n)
    ref = np.array(A.T)
    ref[:6] = 0  # (a_full keeps J at pose 0's columns: what multiplies them is zero; V leaves the rows zero)
    assert (V[:6] == 0).all(), "pose 0's rows are written"
    worst = R.ratio(V - ref, 4 * R.U * np.abs(np.asarray(ref, dtype=F)))
    print("host build of apply_block.h, %d closures on %d poses: largest error / (4 u |J|) %.3g" % (K, n, worst))
    assert worst <= 1.0
    # duplicated closures write equal column blocks; nothing lies outside the rows of the two endpoints
    for a, c in ((4, K - 2), (7, K - 1)):
        assert (V[:, 6 * a:6 * a + 6] == V[:, 6 * c:6 * c + 6]).all()
    for k, (i, j) in enumerate(ends):
        other = np.ones(6 * n, dtype=bool)
        other[6 * i:6 * i + 6] = other[6 * j:6 * j + 6] = False
        assert (V[other, 6 * k:6 * k + 6] == 0).all()

"""CPU check of the fixed-pose argument of csrc/refine_block.h (DESIGN.md 5n "Across teams"), compiled for the host: a participant
of a split team fixes the team pose that is the problem's pose 0, or none (-1) when it does not hold robot 0.
  fixed = 0    the gradient rows and the trial poses are bitwise those of the four-argument forms the single team calls
  fixed = -1   local pose 0 gets the ordinary rows and the ordinary trial pose: those of a copy of the trajectory in which the
               same pose sits at index 1
  fixed = 5    pose 5's rows are zero and its trial pose is copied; every other pose, pose 0 included, is ordinary"""
import os
import shutil
import subprocess

import numpy as np

from tests import covref
from tests import refineref as RR
from tests.util import ROOT

F = np.float64
LD = np.longdouble

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "refine_block.h"
using namespace dpgo;
// in: N, alpha as doubles; T (12 N); E (12 N); X (6 N)
// out: for fixed = -2 (the four-argument forms), 0, -1, 5: g (6 N) and the trial trajectory (12 N)
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const int N = (int)in[0];
  const double alpha = in[1];
  if (in.size() != 2 + 30 * (size_t)N) return 4;
  const double *T = in.data() + 2, *E = T + 12 * N, *X = E + 12 * N;
  const int fixed[4] = {-2, 0, -1, 5};
  std::vector<double> out(4 * 18 * (size_t)N);
  for (int v = 0; v < 4; ++v)
    for (int p = 0; p < N; ++p) {
      double R[3][3], t[3], Ep[12], x[6];
      gate_load_pose(T, p, R, t);
      gate_load_pairs<6>(E + 12 * p, Ep);
      gate_load_pairs<3>(X + 6 * p, x);
      double *g = out.data() + (size_t)v * 18 * N + 6 * p, *P = out.data() + (size_t)v * 18 * N + 6 * N + 12 * p;
      if (fixed[v] == -2) {
        refine_grad_rows(p, R, Ep, g);
        refine_trial_pose(p, R, t, x, alpha, P);
      } else {
        refine_grad_rows(p, fixed[v], R, Ep, g);
        refine_trial_pose(p, fixed[v], R, t, x, alpha, P);
      }
    }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 5;
  std::fclose(f);
  return 0;
}
"""


def run(exe, tmp_path, n, alpha, T, E, X):
    np.concatenate([[n, alpha], T, E, X]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin").reshape(4, 18 * n)
    return [(o[:6 * n].reshape(n, 6), o[6 * n:].reshape(n, 12)) for o in out]


def test_the_fixed_pose_is_an_argument(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "refine_fixed.cpp", tmp_path / "refine_fixed"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    c = RR.case("chain12")
    n, Q = c["n"], c["Q"]
    T = RR.start(c["Tstar"], n, 1e-2, 11)
    # (a pose 0 that is not the identity, as a participant without robot 0 has it)
    T = np.r_[T[12 * 3:12 * 4], T[12:]]
    E = np.asarray((covref.as_matrix(T, 3, n).astype(LD) @ np.asarray(Q.toarray(), dtype=LD)).T.reshape(-1), dtype=F)
    alpha = 0.5
    X = np.random.default_rng(3).standard_normal(6 * n)
    (g_old, P_old), (g0, P0), (gn, Pn), (g5, P5) = run(exe, tmp_path, n, alpha, T, E, X)
    # fixed = 0: the present bytes
    assert g0.tobytes() == g_old.tobytes() and P0.tobytes() == P_old.tobytes()
    assert (g0[0] == 0).all() and P0[0].tobytes() == T[:12].tobytes()
    # fixed = -1: pose 0 is ordinary -- what the same pose, E and x give at index 1 of a swapped copy
    sw = lambda a, w: np.r_[a[w:2 * w], a[:w], a[2 * w:]]
    (gs, Ps) = run(exe, tmp_path, n, alpha, sw(T, 12), sw(E, 12), sw(X, 6))[0]
    assert gn[0].tobytes() == gs[1].tobytes() and Pn[0].tobytes() == Ps[1].tobytes()
    assert np.abs(gn[0]).min() > 0 and Pn[0].tobytes() != T[:12].tobytes(), "pose 0 did not move"
    assert gn[1:].tobytes() == g0[1:].tobytes() and Pn[1:].tobytes() == P0[1:].tobytes()
    ref = covref.perturb(T, -alpha * X, n).reshape(n, 12)
    assert np.abs(Pn - ref).max() <= 64 * RR.U * np.abs(T).max()
    # fixed = 5
    assert (g5[5] == 0).all() and P5[5].tobytes() == T[60:72].tobytes()
    keep = [p for p in range(n) if p != 5]
    assert g5[keep].tobytes() == gn[keep].tobytes() and P5[keep].tobytes() == Pn[keep].tobytes()
    print("host build of refine_block.h: fixed = 0 bitwise the four-argument forms, fixed = -1 and 5 as stated on %d poses" % n)

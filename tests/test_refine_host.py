"""CPU check of csrc/refine_block.h, the per-pose and per-edge arithmetic of the Newton refinement, compiled for
the host: a stand-alone program runs the functions the kernels call on the 12-pose case of tests/refineref.py.
  gradient   refine_grad_rows against J^T vec(E) in longdouble for the same float64 E, every entry within 6 u sum |terms| (a
             chain of six fused multiply-adds; the translation rows are copies); pose 0's rows are zero
  trial      refine_trial_pose against the longdouble T [+] (-alpha x): rotation entries within 16 u, translations within
             4 u (|t| + |alpha x|); rotation steps of angle 0, 1e-9, 1e-4 (1 -+ 1e-3) -- either side of upd_exp_so3's series
             threshold th^2 = 1e-8 --, 0.3 and 2.5; pose 0 is copied bit for bit whatever its rows of x hold
  edge       refine_edge_cost against the longdouble terms within refineref.edge_bounds"""
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
// in: N, M, alpha as doubles; T (12 N); E (12 N); X (6 N); M edges of 16 doubles (i, j, R~ row-major, t~, w kappa, w tau)
// out: g (6 N), the trial trajectory (12 N), the M terms
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const int N = (int)in[0], M = (int)in[1];
  const double alpha = in[2];
  if (in.size() != 3 + 30 * (size_t)N + 16 * (size_t)M) return 4;
  const double *T = in.data() + 3, *E = T + 12 * N, *X = E + 12 * N, *ed = X + 6 * N;
  std::vector<double> out(18 * (size_t)N + M);
  for (int p = 0; p < N; ++p) {
    double R[3][3], t[3], Ep[12];
    gate_load_pose(T, p, R, t);
    gate_load_pairs<6>(E + 12 * p, Ep);
    refine_grad_rows(p, R, Ep, out.data() + 6 * p);
    double x[6];
    gate_load_pairs<3>(X + 6 * p, x);
    refine_trial_pose(p, R, t, x, alpha, out.data() + 6 * N + 12 * p);
  }
  for (int k = 0; k < M; ++k) {
    const double *e = ed + 16 * k;
    double Ri[3][3], ti[3], Rj[3][3], tj[3];
    gate_load_pose(T, (int)e[0], Ri, ti);
    gate_load_pose(T, (int)e[1], Rj, tj);
    out[18 * (size_t)N + k] = refine_edge_cost(Ri, ti, Rj, tj, e + 2);
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 5;
  std::fclose(f);
  return 0;
}
"""

ANGLES = (0.0, 1e-9, 1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), 0.3, 2.5)


def test_host_build_of_the_block_against_the_longdouble_reference(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "refine_host.cpp", tmp_path / "refine_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    c = RR.case("chain12")
    n, m, Q = c["n"], c["m"], c["Q"]
    T = RR.start(c["Tstar"], n, 1e-2, 11)
    E = np.asarray((covref.as_matrix(T, 3, n).astype(LD) @ np.asarray(Q.toarray(), dtype=LD)).T.reshape(-1), dtype=F)
    alpha = 0.25
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, 6))
    for p in range(n):  # alpha |x_rot| = the listed angles, twice over
        X[p, :3] *= ANGLES[p % len(ANGLES)] / (alpha * np.linalg.norm(X[p, :3]))
    X[0] = 1.0  # (pose 0's rows are not applied)
    X = X.reshape(-1)
    edges = np.zeros((len(m), 16))
    edges[:, 0], edges[:, 1] = m["p1"], m["p2"]
    edges[:, 2:11], edges[:, 11:14] = m["R"], m["t"]
    edges[:, 14], edges[:, 15] = m["kappa"] * m["weight"], m["tau"] * m["weight"]
    np.concatenate([[n, len(m), alpha], T, E, X, edges.reshape(-1)]).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin")
    g, Tl, terms = out[:6 * n], out[6 * n:18 * n], out[18 * n:]

    gref, mag = RR.gradient_from_E(T, E, n)
    assert (g[:6] == 0).all(), "pose 0's rows are not zero"
    err = np.abs(np.asarray(g - gref, dtype=F))[6:]
    ratio = float((err / (6 * RR.U * mag[6:])).max())
    print("host build of refine_block.h, gradient rows of %d poses: largest error / (6 u sum |terms|) %.3g" % (n, ratio))
    assert ratio <= 1.0
    assert (g.reshape(n, 6)[1:, 3:] == E.reshape(n, 12)[1:, 9:]).all()
    # against the gradient of the reference itself, within its bound for the device
    assert (np.abs(np.asarray(g - RR.gradient(Q, T, n), dtype=F)) <= RR.gradient_bound(Q, T, n)).all()

    ref = RR.trial_ld(T, X, alpha, n)
    assert Tl[:12].tobytes() == T[:12].tobytes(), "pose 0 is not copied"
    d = np.abs(np.asarray(Tl - ref, dtype=F)).reshape(n, 12)
    tb = 4 * RR.U * (np.abs(T.reshape(n, 12)[:, 9:]) + alpha * np.abs(X.reshape(n, 6)[:, 3:]))
    rr, tr = float(d[:, :9].max() / (16 * RR.U)), float((d[1:, 9:] / tb[1:]).max())
    print("trial poses at angles %s: rotation entries %.3g of 16 u, translations %.3g of 4 u (|t| + |alpha x|)" % (ANGLES, rr, tr))
    assert rr <= 1.0 and tr <= 1.0
    assert np.abs(Tl - covref.perturb(T, -alpha * np.r_[np.zeros(6), X[6:]], n)).max() <= 64 * RR.U * np.abs(T).max()

    tref = RR.edge_terms(m, T, n, LD)
    er = float((np.abs(np.asarray(terms - tref, dtype=F)) / RR.edge_bounds(m, T, n)).max())
    print("edge terms of %d measurements: largest error / bound %.3g" % (len(m), er))
    assert er <= 1.0 and (terms >= 0).all()

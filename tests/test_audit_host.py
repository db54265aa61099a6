"""CPU check of csrc/audit_block.h, the per-record arithmetic of k_audit, compiled for the host: a stand-alone
program runs it on records made from blocks of the numpy inverse, and the result stays within the bounds of tests/auditref.py
against the longdouble reference.  The largest error / bound ratios are printed (DESIGN.md 5h records them)."""
import os
import shutil
import subprocess

import numpy as np

from tests import auditref as A
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "audit_block.h"
// in: per record 64 doubles -- R_ij row-major (9), t_ij (3), Sigma_rel (36), the measurement part of the record (16)
// out: per record 52 doubles -- xi (6), xi_loo (6), d2, rho, pmin, testable, Sigma_loo (36)
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const double min_redundancy = std::atof(argv[3]);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[64];
  while (std::fread(buf, sizeof(double), 64, f) == 64) in.insert(in.end(), buf, buf + 64);
  std::fclose(f);
  const size_t n = in.size() / 64;
  std::vector<double> out(52 * n);
  for (size_t k = 0; k < n; ++k) {
    const double *r = in.data() + 64 * k;
    double M[3][3], S[6][6], SL[6][6];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) M[a][b] = r[3 * a + b];
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) S[a][b] = r[12 + 6 * a + b];
    dpgo::AuditOut o;
    dpgo::audit_record<true>(M, r + 9, S, r + 48, min_redundancy, o, SL);
    double *q = &out[52 * k];
    for (int a = 0; a < 6; ++a) { q[a] = o.xi[a]; q[6 + a] = o.xi_loo[a]; }
    q[12] = o.d2; q[13] = o.rho; q[14] = o.pmin; q[15] = o.testable ? 1.0 : 0.0;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) q[16 + 6 * a + b] = SL[a][b];
    // without Sigma_loo the other outputs are the same bits
    dpgo::AuditOut o2;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) S[a][b] = r[12 + 6 * a + b];
    dpgo::audit_record<false>(M, r + 9, S, r + 48, min_redundancy, o2, SL);
    if (!(o2.d2 == o.d2) || o2.rho != o.rho || !(o2.pmin == o.pmin) || o2.testable != o.testable) return 5;
    for (int a = 0; a < 6; ++a)
      if (o2.xi[a] != o.xi[a] || o2.xi_loo[a] != o.xi_loo[a]) return 5;
  }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
  std::fclose(f);
  return 0;
}
"""

WEIGHTS = (1.0, 0.37, 0.0, 1e-3, 1.0)
ANGLES = (0.0, 1e-9, 0.3, 3.0)


def test_host_build_of_the_block_stays_within_the_bounds(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "audit_host.cpp", tmp_path / "audit_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    n = 12
    m, T = NR.banded_chain(n, 2, window=8)
    Sigma = covref.dense_reference(covref.q_full(m, n), T, n)[1]
    rng = np.random.default_rng(3)
    recs, rows = [], []
    for k in range(15 * len(m)):  # every edge under every pair of a weight and a scale; the angles go round at their own pace
        e = m[k % len(m)]
        i, j = int(e["p1"]), int(e["p2"])
        w, th = WEIGHTS[(k // len(m) + k % len(m)) % 5], ANGLES[k % 4]
        a = rng.standard_normal(3)
        Rm = np.asarray(e["R"]).reshape(3, 3) @ covref.exp_so3(th * a / np.linalg.norm(a)).T if th else np.asarray(e["R"]).reshape(3, 3)
        tm = e["t"] + (0.05 * rng.standard_normal(3) if th else 0.0)
        scale = (1.0, 0.5, 0.25)[k // len(m) % 3]  # (at most 1: a record that claims more information than the graph holds has no PSD A)
        kappa, tau = e["kappa"] * scale, e["tau"] * scale
        recs.append((i, j, Rm, tm, kappa, tau, w))
        Rij, tij = G.relative_pose(T, i, j, F)
        Sr = G.sigma_rel(T, i, j, *G.blocks_of(Sigma, i, j), F)
        rows.append(np.r_[Rij.reshape(-1), tij, Sr.reshape(-1), Rm.reshape(-1), tm, kappa, tau, w, 0.0])
    np.array(rows).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "1e-6"])
    out = np.fromfile(tmp_path / "out.bin").reshape(len(recs), 52)
    worst = dict(xi=0.0, xi_loo=0.0, d2=0.0, rho=0.0, pmin=0.0, sigma_loo=0.0)
    held = bridges = 0
    for (i, j, Rm, tm, kappa, tau, w), o in zip(recs, out):
        blocks = G.blocks_of(Sigma, i, j)
        r = A.audit(T, i, j, Rm, tm, kappa, tau, w, *blocks)
        gx, gl, gd, grho, gp, gt, gs = o[:6], o[6:12], o[12], o[13], o[14], o[15] != 0.0, o[16:].reshape(6, 6)
        assert (gs == gs.T).all(), "Sigma_loo is not bitwise symmetric"
        b_x = G.xi_bound(T, i, j, tm)
        worst["xi"] = max(worst["xi"], (np.abs(gx - np.asarray(r["xi"], dtype=F)) / b_x).max())
        assert (np.abs(gx - np.asarray(r["xi"], dtype=F)) <= b_x).all()
        if w == 0.0:
            assert grho == 1.0 and gp == 1.0 and gt
        if float(r["pmin"]) < 1e-3:  # a bridge at full weight: the graph knows this relative pose through the edge alone
            assert float(r["pmin"]) < 1e-6 and not gt and gd == np.inf and not gl.any() and not gs.any()
            assert abs(grho - float(r["rho"])) <= A.rho_bound(r, G.sigma_rel_bound(T, i, j, *blocks)) and abs(float(r["rho"])) <= 1e-9
            bridges += 1
            continue
        held += 1
        b = A.record_bounds(T, i, j, tm, *blocks, r)
        assert gt and r["testable"]
        for key, got in (("xi_loo", gl), ("d2", gd), ("rho", grho), ("pmin", gp), ("sigma_loo", gs)):
            ratio = np.max(np.abs(got - np.asarray(r[key], dtype=F)) / b[key])
            worst[key] = max(worst[key], ratio)
            assert ratio <= 1.0, (key, i, j, w, ratio)
    assert held >= 50 and bridges >= 1
    print("host build of audit_block.h, %d records (%d on bridges): largest error / bound: " % (len(recs), bridges)
          + ", ".join("%s %.3g" % kv for kv in worst.items()))

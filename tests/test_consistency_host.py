"""CPU check of csrc/consistency_block.h, the per-pair arithmetic of k_consistency, compiled for the host: a
stand-alone program runs it on records made from blocks of the numpy inverse, and the result stays within the bounds of
tests/pcmref.py against the longdouble reference.  The largest error / bound ratios are printed (DESIGN.md 5g records them)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import covref
from tests import gateref as G
from tests import pcmref as P
from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "consistency_block.h"
// in: per pair 130 doubles -- the records of candidates p and q (16 each), of A_pq and B_pq (48 each), has_a, has_b
// out: per pair 43 doubles -- xi (6), S (36), d2
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[130];
  while (std::fread(buf, sizeof(double), 130, f) == 130) in.insert(in.end(), buf, buf + 130);
  std::fclose(f);
  const size_t n = in.size() / 130;
  std::vector<double> out(43 * n);
  for (size_t k = 0; k < n; ++k) {
    const double *r = in.data() + 130 * k;
    out[43 * k + 42] = dpgo::pcm_pair(r, r + 16, r + 32, r[128] != 0.0, r + 80, r[129] != 0.0, &out[43 * k], &out[43 * k + 6]);
  }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
  std::fclose(f);
  return 0;
}
"""


def cand_record(c):
    r = np.zeros(16)
    r[:9], r[9:12], r[12], r[13] = c["R"], c["t"], c["kappa"], c["tau"]
    return r


def seg_record(T, a, b, sig):
    """(record, present): what k_segments leaves for the segment (T_a)^-1 T_b, formed in float64"""
    if a == b:
        return np.full(48, np.nan), 0.0  # never used: the arithmetic must not let it through
    R, t = G.relative_pose(T, a, b, F)
    return np.r_[R.reshape(-1), t, np.asarray(sig(a, b), dtype=F).reshape(-1)], 1.0


def test_host_build_of_the_block_stays_within_the_bounds(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "pcm_host.cpp", tmp_path / "pcm_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    ma, Ta, mb, Tb, cand, is_true = P.planted_case()
    n = P.PLANTED["n"]
    # the mix of the edge tests in front (coinciding segments, pose 0, exact candidates, residual angles up to 3.0 rad), the
    # planted candidates behind them: the loops between the two kinds are outliers
    cand = np.concatenate([P.mixed_candidates(Ta, Tb, 12, seed=2), cand])
    Sa = covref.dense_reference(covref.q_full(ma, n), Ta, n)[1]
    Sb = covref.dense_reference(covref.q_full(mb, n), Tb, n)[1]
    sig_a = lambda a, b: G.sigma_rel(Ta, a, b, *G.blocks_of(Sa, a, b), F)
    sig_b = lambda a, b: G.sigma_rel(Tb, a, b, *G.blocks_of(Sb, a, b), F)
    i, j = P.endpoints(cand, {0: 0}, {0: 0})
    pairs = list(itertools.combinations(range(12), 2)) + [(3, 20), (4, 23), (15, 22), (12, 13), (14, 30), (20, 35)]
    rows = []
    for k, l in pairs:
        ra, ha = seg_record(Ta, int(i[l]), int(i[k]), sig_a)
        rb, hb = seg_record(Tb, int(j[k]), int(j[l]), sig_b)
        rows.append(np.r_[cand_record(cand[k]), cand_record(cand[l]), ra, rb, ha, hb])
    assert any(r[128] == 0.0 for r in rows) and any(r[129] == 0.0 for r in rows) and any(r[128] == 0.0 and r[129] == 0.0 for r in rows)
    np.array(rows).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin").reshape(len(pairs), 43)
    worst, checked = dict(S=0.0, xi_R=0.0, xi_t=0.0, d2=0.0), 0
    for (k, l), o in zip(pairs, out):
        args = P.pair_inputs(cand, Ta, Tb, i, j, k, l, sig_a, sig_b)
        xi, d2, S = P.pair(*args)
        b_s, b_x, b_d = P.bounds(cand, Ta, Tb, i, j, k, l, args, xi, S, d2)
        gx, gS, gd = o[:6], o[6:42].reshape(6, 6), o[42]
        assert (gS == gS.T).all(), "S is not bitwise symmetric"
        es, ex, ed = np.abs(gS - np.asarray(S, dtype=F)), np.abs(gx - np.asarray(xi, dtype=F)), abs(gd - float(d2))
        worst["S"] = max(worst["S"], (es / b_s).max())
        worst["xi_t"] = max(worst["xi_t"], (ex[3:] / b_x[3:]).max())
        assert (es <= b_s).all() and (ex[3:] <= b_x[3:]).all(), (k, l, (es / b_s).max(), (ex / b_x).max())
        if np.linalg.norm(np.asarray(xi[:3], dtype=F)) > 3.0 + 1e-9:  # beyond the angles the bound of xi_R is stated for
            assert np.isfinite(gx).all() and np.isfinite(gd)
            continue
        checked += 1
        worst["xi_R"], worst["d2"] = max(worst["xi_R"], (ex[:3] / b_x[:3]).max()), max(worst["d2"], ed / b_d)
        assert (ex[:3] <= b_x[:3]).all() and ed <= b_d, (k, l, (ex / b_x).max(), ed / b_d)
    assert checked >= 50
    print("host build of consistency_block.h, %d pairs: largest error / bound: S %.3g, xi_R %.3g, xi_t %.3g, d2 %.3g"
          % (len(pairs), worst["S"], worst["xi_R"], worst["xi_t"], worst["d2"]))

"""measurements of profiles/r14_consistency.md: K candidates between the two halves of sphere2500 taken as two single-robot
teams, method="nested".  usage: python profiles/experiments/consistency_time.py K [K ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ["DPGO_TIMING"] = "1"

import numpy as np

from dpgo_ros_amd import capi
from tests import pcmref as P
from tests.test_gpu_certificate import RTR_NESTEROV
from tests.util import DATA


def half(m, lo, hi):
    keep = (m["p1"] >= lo) & (m["p1"] < hi) & (m["p2"] >= lo) & (m["p2"] < hi)
    h = m[keep].copy()
    h["p1"] -= lo
    h["p2"] -= lo
    h["r1"] = h["r2"] = 0
    return h, hi - lo


def solved(m, n):
    t = capi.Team.from_measurements(m, capi.default_params(r=5, num_robots=1, **RTR_NESTEROV))
    t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(5))
    t0 = time.time()
    t.run(200)
    T = t.round()[1]
    print("half of %d poses, %d edges: cost %.9g after 200 iterations (%.1f s)" % (n, len(m), t.cost(), time.time() - t0), flush=True)
    return t, T


def candidates(Ta, Tb, K, seed):
    rng = np.random.default_rng(seed)
    na, nb = len(Ta) // 12, len(Tb) // 12
    f = np.float64
    c = np.zeros(K, dtype=capi.MEAS_DTYPE)
    true = rng.random(K) < 0.5
    for k in range(K):
        i, j = int(rng.integers(0, na)), int(rng.integers(0, nb))
        c[k]["p1"], c[k]["p2"], c[k]["kappa"], c[k]["tau"] = i, j, 10000.0, 100.0
        if true[k]:
            Z = P.mul(P.inv(P.pose_of(Ta, i, f)), P.pose_of(Tb, j, f))
            Z = P.perturb(Z, np.r_[rng.standard_normal(3) / np.sqrt(2e4), rng.standard_normal(3) / 10.0], f)
        else:
            Z = P.random_pose(rng, 30.0)
        c[k]["R"], c[k]["t"] = np.asarray(Z[0]).reshape(-1), Z[1]
    return c, true


def main():
    m, n = capi.read_g2o(os.path.join(DATA, "sphere2500.g2o"))
    (ma, na), (mb, nb) = half(m, 0, n // 2), half(m, n // 2, n)
    ta, Ta = solved(ma, na)
    tb, Tb = solved(mb, nb)
    for K in [int(x) for x in sys.argv[1:]]:
        cand, true = candidates(Ta, Tb, K, seed=K)
        for rep in range(2):  # the second call has the pooled buffers and the plans
            t0 = time.time()
            out = capi.pairwise_consistency(ta, tb, cand, Ta, Tb, method="nested", max_nodes=5_000_000)
            wall = time.time() - t0
        hit = np.isin(np.flatnonzero(true), out["inliers"]).sum()
        print("K = %d: wall %.3f s, %d inliers (%d of the %d true ones), proven %s, res_a %r" % (K, wall, len(out["inliers"]), hit, true.sum(), out["proven"], out["res_a"]), flush=True)
        # the float64 form of the reference on a sample of pairs, one core, scaled to K (K - 1) / 2 pairs
        rng = np.random.default_rng(1)
        i, j = P.endpoints(cand, {0: 0}, {0: 0})
        sample = []
        while len(sample) < 200:
            k, l = sorted(int(x) for x in rng.integers(0, K, 2))
            if k != l and i[k] != i[l] and j[k] != j[l]:
                sample.append((k, l))
        ra = ta.relative_covariances([(int(i[l]), int(i[k])) for k, l in sample], Ta, method="nested")
        rb = tb.relative_covariances([(int(j[k]), int(j[l])) for k, l in sample], Tb, method="nested")
        t0 = time.time()
        worst = 0.0
        for q, (k, l) in enumerate(sample):
            args = P.pair_inputs(cand, Ta, Tb, i, j, k, l, lambda a, b: ra[q], lambda a, b: rb[q], np.float64)
            d = P.pair(*args, dtype=np.float64)[1]
            worst = max(worst, abs(d - out["d2"][k, l]) / max(1.0, abs(d)))
        per = (time.time() - t0) / len(sample)
        print("K = %d: pcmref in float64 %.3f ms per pair on one core -> %.1f s for the %d pairs; largest relative difference to the GPU on the sample %.3g"
              % (K, per * 1e3, per * K * (K - 1) / 2, K * (K - 1) // 2, worst), flush=True)


main()

"""The joint gate (Team.gate_jointly, csrc/gate_joint.hip) at the rounded optimum of sphere2500 held by ONE robot,
method="nested", on K = 64 / 256 / 1024 seeded candidates (tests/jointref.seeded_batch: 70 % from their own noise model, 30 % off
by 0.3 rad and 0.3 m).  Per K one warm-up call, then the median wall time of three whole Python calls (each ends in the call's
own stream synchronisation), the same with M brought to the host, a call whose threshold accepts nothing (every launch of the
elimination but the first returns at once: the cost of a launch), and tests/jointref.py in float64 on one core for the same M
and the same order.  With DPGO_TIMING=1 the library prints the covariance path's phases, k_joint_blocks and the elimination
(device time between events) on stderr.
python profiles/experiments/gate_joint_time.py [K ...] -> one JSON line per K"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests import jointref as J
from tests.test_gpu_certificate import OPTIMA, converge, team_at

ds, N, at_opt, kw = OPTIMA[0]
Ks = [int(a) for a in sys.argv[1:]] or [64, 256, 1024]
t5, m, n = team_at(ds, N, **kw)
assert converge(t5, at_opt) > 0
_, T = t5.round()
t5.close()
t, _, _ = team_at(ds, 1, T=T, **kw)
kappa, tau = float(np.median(m["kappa"])), float(np.median(m["tau"]))
thr2 = capi.error_threshold_at_quantile(0.99, 6) ** 2


def median_of(call, reps=3):
    wall = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
    return float(np.median(wall[1:])), out


for K in Ks:
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, seed=K, kappa=kappa, tau=tau)
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    cand["p1"], cand["p2"], cand["R"], cand["t"], cand["kappa"], cand["tau"] = ends[:, 0], ends[:, 1], Rm.reshape(K, 9), tm, kap, ta
    sys.stderr.write("---- K = %d, %d distinct endpoint poses\n" % (K, len(set(ends.reshape(-1).tolist()))))
    call_s, out = median_of(lambda: t.gate_jointly(cand, T, method="nested"))
    with_M_s, full = median_of(lambda: t.gate_jointly(cand, T, method="nested", innovation_covariance=True), reps=1)
    none_s, none = median_of(lambda: t.gate_jointly(cand, T, method="nested", quantile=1e-12))
    assert none["num_accepted"] == 0 and full["rank"].tobytes() == out["rank"].tobytes()
    gate = t.gate(cand, T, method="nested")
    t0 = time.perf_counter()
    ref = J.run(full["M"], full["xi"], thr2, "greedy", pivots=out["accepted"], dtype=np.float64)
    ref_s = time.perf_counter() - t0
    agree = bool((ref["rank"] == out["rank"]).all())
    w = np.linalg.eigvalsh(full["M"]) if K <= 256 else None
    print(json.dumps(dict(K=K, poses=len(set(ends.reshape(-1).tolist())), true_inliers=int(inl.sum()),
                          gate_accepts=int(gate[3].sum()), gate_outliers=int((gate[3] & ~inl).sum()),
                          joint_accepts=int(out["num_accepted"]), joint_outliers=int((out["accept"] & ~inl).sum()),
                          joint_accept=out["joint_accept"], cond_M=None if w is None else float(w[-1] / w[0]),
                          call_ms=1e3 * call_s, call_with_M_ms=1e3 * with_M_s, call_accepting_nothing_ms=1e3 * none_s,
                          jointref_float64_ms=1e3 * ref_s, jointref_agrees=agree,
                          largest_d2_cond_difference=float(np.abs(np.asarray(ref["d2_cond"], dtype=np.float64) - out["d2_cond"]).max()))),
          flush=True)
t.close()

"""The leave-one-out audit (Team.audit, csrc/audit.hip) at the rounded optimum of sphere2500 / 5 under each covariance method, on
the team's own measurements with their current weights (Team.measurements_once: every edge of the graph once).  Medians of 5
calls after one warm-up, with the spread (max - min) beside them; wall time around the whole Python call (it ends in the call's
own stream synchronisation).  With DPGO_TIMING=1 the library prints the audit kernel's device time on stderr.
python profiles/experiments/audit_time.py -> one JSON line per method"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests.test_gpu_certificate import OPTIMA, converge, team_at

ds, N, at_opt, kw = OPTIMA[0]
t, m, n = team_at(ds, N, **kw)
assert converge(t, at_opt) > 0
_, T = t.round()
meas = t.measurements_once()
sys.stderr.write("%s / %d: %d poses, %d measurements\n" % (ds, N, n, len(meas)))


def median_of(call):
    wall = []
    for k in range(6):
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
    return float(np.median(wall[1:])), float(max(wall[1:]) - min(wall[1:])), out


for method, mb in (("dense", None), ("schur", None), ("nested", 128)):
    sys.stderr.write("== %s\n" % method); sys.stderr.flush()
    audit_s, spread_s, out = median_of(lambda: t.audit(meas, T, method=method, max_block=mb))
    loo_s, loo_spread_s, _ = median_of(lambda: t.audit(meas, T, method=method, max_block=mb, sigma_loo=True))
    res = out["covariance"]
    print(json.dumps(dict(method=method, max_block=mb, records=len(meas), audit_wall_s=audit_s, audit_wall_spread_s=spread_s,
                          audit_with_sigma_loo_wall_s=loo_s, audit_with_sigma_loo_wall_spread_s=loo_spread_s,
                          testable=int(out["testable"].sum()), accepted=int(out["accept"].sum()),
                          device_assemble_s=res.seconds_assemble, device_invert_s=res.seconds_invert)))
    sys.stdout.flush()
t.close()

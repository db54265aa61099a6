"""Team.refine (csrc/refine.hip) at the rounded point of sphere2500 after a 5-robot run to the pinned optimum's 1e-6 relative
gap, the trajectory held by ONE robot, method="nested" at the default max_block: one warm-up call, then five whole Python calls
(each ends in the call's own stream synchronisation): iterations, the median wall time, |g|_inf before and after.  With
DPGO_TIMING=1 the library prints on stderr the call's split into gradient and cost, covariance paths, k_refine_trials and
k_refine_cost with its sums.
Then the other route to the same |g|_inf: the 5-robot team goes on with its RBCD iterations from the same point, 100 at a time (the
wall time of Team.run and its synchronisation alone is counted; the robots' own gradient tolerance is set to 1e-13 so that
they keep working), and after every 100 the rounding's |g|_inf is read with Team.refine(max_iters=0), which runs no covariance
path -- until it is below what the refinement reached, or LIMIT iterations.
python profiles/experiments/refine_time.py [LIMIT] -> one JSON line per route"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests.test_gpu_certificate import OPTIMA, converge, team_at

ds, N, at_opt, kw = OPTIMA[0]
LIMIT = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
# (the tests' configuration stops a robot's solve at a gradient norm of 1e-2: the iterations past the pinned cost would be idle)
t5, m, n = team_at(ds, N, **dict(kw, gradnorm_tol=1e-13))
its = converge(t5, at_opt)
assert its > 0
_, T = t5.round()
t, _, _ = team_at(ds, 1, T=T, **kw)
sys.stderr.write("---- %s: %d poses, %d measurements, %d iterations to the pinned cost; plan %r\n" % (ds, n, len(m), its, t.covariance_plan()[1]))

wall, out = [], None
for rep in range(6):  # (the first call is the warm-up)
    if rep == 1:
        sys.stderr.write("---- timed calls\n")
    t0 = time.perf_counter()
    out = t.refine(T, method="nested")
    if rep > 0:
        wall.append(time.perf_counter() - t0)
h = out["history"]
print(json.dumps(dict(route="refine", status=out["status"], iterations=out["iterations"], ms=1e3 * float(np.median(wall)),
                      all_ms=[round(1e3 * x, 2) for x in wall], ms_per_iteration=1e3 * float(np.median(wall)) / max(out["iterations"], 1),
                      grad_inf=[float(v) for v in h["grad_inf"]], f=[float(v) for v in h["f"]], alpha=[float(v) for v in h["alpha"]],
                      decrement=[float(v) for v in h["decrement"]], pivot_min=[float(v) for v in h["pivot_min"]])))
sys.stdout.flush()

target, spent, k, g = out["grad_inf"], 0.0, 0, out["grad_inf0"]
trace = []
while k < LIMIT and g > target:
    t0 = time.perf_counter()
    t5.run(100)
    t5.synchronize()
    spent += time.perf_counter() - t0
    k += 100
    g = t.refine(t5.round()[1], max_iters=0)["grad_inf0"]
    trace.append(float(g))
print(json.dumps(dict(route="rbcd", iterations=k, ms=1e3 * spent, reached=bool(g <= target), target=float(target), grad_inf_every_100=trace,
                      cost=t5.cost())))
t.close()
t5.close()

"""Rounding cost at the converged sphere2500 / 5-agent point (RTR + Nesterov from chordal, to the 1e-6 gap): wall time of
dpgo_team_round with and without the translation refinement (median of warm calls), and numpy's rounding of the same X
on one CPU core (the CPU baseline; with the scipy refinement as well).  Prints one JSON line; with an argument, also writes
it to that file.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python profiles/experiments/round_time.py`."""
import os
import sys

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = "1"  # numpy baseline on one core
import json
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dpgo_ros_amd import capi  # noqa: E402
from tests.test_rounding import refine_translations, round_numpy  # noqa: E402

FSTAR = 843.5029071410438
REPS = 20
m, n = capi.read_g2o(os.path.join(ROOT, "data", "sphere2500.g2o"))
mp = capi.partition(m, n, 5)
kw = dict(method=capi.METHOD_RTR, acceleration=1, rtr_iterations=3, rtr_tcg_iterations=50, gradnorm_tol=1e-2,
          restart_interval=50)
t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=5, **kw))
t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(5))
k = 0
while (t.cost() - FSTAR) / FSTAR > 1e-6 and k < 5000:
    t.run(10)
    k += 10
gap = (t.cost() - FSTAR) / FSTAR
res = dict(dataset="sphere2500", agents=5, solve_iterations=k, gap=gap)
for name, refine in (("unrefined", False), ("refined", True)):
    rd, T = t.round(refine_translations=refine)  # warm-up (workspace allocation)
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        rd, T = t.round(refine_translations=refine)
        times.append(1e3 * (time.perf_counter() - t0))
    res[name] = dict(ms=float(np.median(times)), ms_min=float(np.min(times)), ms_all=times, f_relaxed=rd.f_relaxed,
                     f_rounded=rd.f_rounded, gap_rel=(rd.f_rounded - rd.f_relaxed) / rd.f_relaxed,
                     sigma=list(rd.sigma[:5]), reflected=rd.reflected, num_degenerate=rd.num_degenerate)
X = t.global_X()
t0 = time.perf_counter()
Tn, _, _ = round_numpy(X, 5, n)
t1 = time.perf_counter()
refine_translations(m, n, Tn)
t2 = time.perf_counter()
res["numpy_round_1core"] = dict(ms=1e3 * (t1 - t0), refine_ms=1e3 * (t2 - t1))
t.close()
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")

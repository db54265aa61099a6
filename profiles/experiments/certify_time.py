"""Certificate cost at the converged sphere2500 / 5-agent point (RTR + Nesterov from chordal, to the 1e-6 gap):
wall time of dpgo_team_certify (median of warm calls), LOBPCG iterations, lambda_min, and scipy eigsh on one CPU core
for the same S (the CPU baseline).  Prints one JSON line; with an argument, also writes it to that file.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python profiles/experiments/certify_time.py`."""
import os
import sys

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = "1"  # scipy baseline on one core
import json
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dpgo_ros_amd import capi  # noqa: E402
from tests.test_certificate import certificate_matrix, deflation_basis, q_full  # noqa: E402,F401

FSTAR = 843.5029071410438
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
for name, kwc in (("deflated_precond", {}), ("deflated_noprecond", dict(precondition=False)),
                  ("undeflated_precond", dict(deflate=False))):
    c, v = t.certify(eta=1e-6, **kwc)  # warm-up (workspace allocation)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        c, v = t.certify(eta=1e-6, **kwc)
        times.append(1e3 * (time.perf_counter() - t0))
    res[name] = dict(ms=float(np.median(times)), ms_all=times, iterations=c.iterations, lambda_min=c.lambda_min,
                     residual=c.residual, norm_bound=c.norm_bound, certified=c.certified)
X = t.global_X()
S = certificate_matrix(q_full(m, n), X, 5, n)
t0 = time.perf_counter()
lam = spla.eigsh(S, k=1, which="SA", tol=1e-8)[0][0]
res["scipy_eigsh_SA_1core"] = dict(ms=1e3 * (time.perf_counter() - t0), lambda_min=float(lam))
t.close()
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")

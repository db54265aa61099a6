"""Sigma applied to vectors (Team.covariance_apply, csrc/covariance_apply.hip) and the first-order update on that solve
(Team.linear_update(columns="solve")) against the update on extracted blocks (columns="blocks"), at the rounded optimum of
sphere2500 held by ONE robot, method="nested" at the default max_block, on the sets Team.gate_jointly accepts out of
K = 64 / 256 / 1024 seeded candidates (the batches of linear_update_time.py).  Per K one warm-up call of either route, then
five whole Python calls of each, alternating (each ends in the call's own stream synchronisation): the median wall time of
either and the largest difference between their outputs.  Then covariance_apply alone on seeded normal columns at
m = 64 / 1024 / 6144, median of five.  With DPGO_TIMING=1 the library prints the covariance path's phases and the apply's own
products (time and achieved TFLOP/s) on stderr.
python profiles/experiments/covariance_apply_time.py [K ...] -> one JSON line per K and per m"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests import jointref as J
from tests.test_gpu_certificate import OPTIMA, R as RANK, converge, team_at

ds, N, at_opt, kw = OPTIMA[0]
Ks = [int(a) for a in sys.argv[1:]] or [64, 256, 1024]
t5, m, n = team_at(ds, N, **kw)
assert converge(t5, at_opt) > 0
_, T = t5.round()
t5.close()
t, _, _ = team_at(ds, 1, T=T, **kw)
kappa, tau = float(np.median(m["kappa"])), float(np.median(m["tau"]))
plan = t.covariance_plan()[1]
sys.stderr.write("---- plan: %r\n" % (plan,))


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


for K in Ks:
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, seed=K, kappa=kappa, tau=tau)
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    cand["p1"], cand["p2"], cand["R"], cand["t"], cand["kappa"], cand["tau"] = ends[:, 0], ends[:, 1], Rm.reshape(K, 9), tm, kap, ta
    acc = np.sort(t.gate_jointly(cand, T, method="nested")["accepted"])
    c = cand[acc]
    poses = sorted(set(ends[acc].reshape(-1).tolist()))
    sys.stderr.write("---- K = %d: %d accepted closures on %d distinct endpoint poses, %d pair blocks under \"blocks\", %d columns under "
                     "\"solve\"\n" % (K, len(c), len(poses), n * len(poses), 6 * len(c)))
    routes = {"blocks": lambda: t.linear_update(c, T, method="nested"), "solve": lambda: t.linear_update(c, T, method="nested", columns="solve")}
    wall, out = {"blocks": [], "solve": []}, {}
    for rep in range(6):  # (the first round is the warm-up)
        for name in ("blocks", "solve"):
            if rep == 1:
                sys.stderr.write("---- K = %d, columns=\"%s\"\n" % (K, name))
            s, out[name] = timed(routes[name])
            if rep > 0:
                wall[name].append(s)
    a, b = out["blocks"], out["solve"]
    scale = np.abs(a["cov_diag"]).max()
    print(json.dumps(dict(K=K, accepted=len(c), poses=len(poses), pair_blocks=n * len(poses), columns=6 * len(c),
                          blocks_ms=1e3 * float(np.median(wall["blocks"])), solve_ms=1e3 * float(np.median(wall["solve"])),
                          blocks_all_ms=[round(1e3 * x, 2) for x in wall["blocks"]], solve_all_ms=[round(1e3 * x, 2) for x in wall["solve"]],
                          delta_difference=float(np.abs(a["delta"] - b["delta"]).max()), largest_delta=float(np.abs(a["delta"]).max()),
                          cov_diag_difference=float(np.abs(a["cov_diag"] - b["cov_diag"]).max() / scale),
                          d2_joint=[a["d2_joint"], b["d2_joint"]], logdet_M=[a["logdet_M"], b["logdet_M"]])), flush=True)

rng = np.random.default_rng(5)
for cols in (64, 1024, 6144):
    V = np.asfortranarray(rng.standard_normal((6 * n, cols)))
    wall = []
    for rep in range(6):
        if rep == 1:
            sys.stderr.write("---- covariance_apply alone, m = %d\n" % cols)
        s, (res, X) = timed(lambda: t.covariance_apply(V, T, method="nested"))
        if rep > 0:
            wall.append(s)
    # the residual of the solve through the blocks the path returns is out of reach at this size; the symmetry of Sigma is not:
    # w^T (Sigma v) = v^T (Sigma w) for the first two columns
    sym = None
    if cols >= 2:
        sym = float(abs(V[:, 1] @ X[:, 0] - V[:, 0] @ X[:, 1]) / (np.linalg.norm(X[:, 0]) * np.linalg.norm(V[:, 1])))
    print(json.dumps(dict(m=cols, rows=6 * n, apply_ms=1e3 * float(np.median(wall)), apply_all_ms=[round(1e3 * x, 2) for x in wall],
                          symmetry_defect=sym)), flush=True)
t.close()

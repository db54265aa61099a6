"""The first-order removal (Team.linear_removal, csrc/linear_removal.hip) at the rounded optimum of sphere2500 held by ONE robot,
method="nested": r17's accepted closures (the sets Team.gate_jointly accepts out of K = 64 / 256 / 1024 seeded candidates, the
batches of linear_update_time.py) are IN the graph -- a team on the extended list, their measurements set to T's own relative
poses so that T is a minimum of it -- and are removed again.  Per K one warm-up call, then the median wall time of three whole
Python calls (each ends in the call's own stream synchronisation); beside it the only other route to the same Sigma' and T' -- a
team without the closures (their weights at zero), solved again from T, rounded, and covariances(method="nested") there --, and
the float64 numpy statement of the removal on one core from the blocks a covariance call returns for the rectangular set (the
time of that call is given apart).  With DPGO_TIMING=1 the library prints the covariance path's phases (the extraction of the
N m pair blocks among them) and the device time of each new kernel on stderr.
python profiles/experiments/linear_removal_time.py [K ...] -> one JSON line per K"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ["OPENBLAS_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests import gateref as G
from tests import jointref as J
from tests import updateref as R
from tests.test_gpu_certificate import OPTIMA, R as RANK, converge, team_at

ds, N, at_opt, kw = OPTIMA[0]
Ks = [int(a) for a in sys.argv[1:]] or [64, 256, 1024]
t5, m, n = team_at(ds, N, **kw)
assert converge(t5, at_opt) > 0
_, T = t5.round()
t5.close()
t, _, _ = team_at(ds, 1, T=T, **kw)
kappa, tau = float(np.median(m["kappa"])), float(np.median(m["tau"]))
base_diag = t.covariances(T, method="nested")[1]


def median_of(call, reps=3):
    wall = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
    return float(np.median(wall[1:])), out


def numpy_removal(T, ends, Rm, tm, kap, ta, poses, diag, cross):
    """the removal at full weight in float64 with BLAS, the blocks as one 6 n x 6 m matrix: (dx, the diagonal blocks of Sigma',
    d2_joint)"""
    K, mm = len(ends), len(poses)
    rank = {e: a for a, e in enumerate(poses)}
    S = cross[:mm * n].reshape(mm, n, 6, 6).transpose(1, 2, 0, 3).reshape(6 * n, 6 * mm)
    A = np.zeros((6 * K, 6 * mm))
    for k, (i, j) in enumerate(ends):
        Ji, Jj = G.jacobians(T, int(i), int(j), np.float64)
        A[6 * k:6 * k + 6, 6 * rank[int(i)]:6 * rank[int(i)] + 6], A[6 * k:6 * k + 6, 6 * rank[int(j)]:6 * rank[int(j)] + 6] = Ji, Jj
    s = 1.0 / np.sqrt(np.asarray(R.r_diagonal(kap, ta, np.float64)))
    Bt = (S @ A.T) * s[None, :]
    rows = np.concatenate([np.arange(6 * e, 6 * e + 6) for e in poses])
    Nt = np.eye(6 * K) - (s[:, None] * A) @ Bt[rows]
    xit = s * np.asarray(J.innovations(T, ends, Rm, tm, np.float64)).reshape(-1)
    Gm = np.linalg.inv(0.5 * (Nt + Nt.T))
    z = Gm @ xit
    Um = Bt @ Gm
    corr = np.einsum("pac,pbc->pab", Um.reshape(n, 6, 6 * K), Bt.reshape(n, 6, 6 * K))
    return (Bt @ z).reshape(n, 6), diag + corr, float(xit @ z)


for K in Ks:
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, seed=K, kappa=kappa, tau=tau)
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    cand["p1"], cand["p2"], cand["R"], cand["t"], cand["kappa"], cand["tau"] = ends[:, 0], ends[:, 1], Rm.reshape(K, 9), tm, kap, ta
    acc = np.sort(t.gate_jointly(cand, T, method="nested")["accepted"])
    c = cand[acc]
    ends, kap, ta = ends[acc], kap[acc], ta[acc]
    rel = [G.relative_pose(T, int(i), int(j), np.float64) for i, j in ends]
    Rm, tm = np.array([r[0] for r in rel]), np.array([r[1] for r in rel])
    c["R"], c["t"], c["weight"] = Rm.reshape(-1, 9), tm, 1.0
    poses = sorted(set(ends.reshape(-1).tolist()))
    sys.stderr.write("---- K = %d: %d closures in the graph on %d distinct endpoint poses, %d pair blocks\n" % (K, len(c), len(poses), n * len(poses)))
    tx = capi.Team.from_measurements(np.concatenate([m, c]), capi.default_params(r=RANK, num_robots=1, **kw))
    tx.set_initial(T, capi.fixed_stiefel(RANK))
    call_s, out = median_of(lambda: tx.linear_removal(c, T=T, method="nested"))

    # the other route: the graph without the closures, solved again from T (one chunk of 50 iterations: T is its optimum
    # already, which is the least such a solve can cost), rounded, and its covariances
    def resolve():
        ty = capi.Team.from_measurements(m, capi.default_params(r=RANK, num_robots=1, **kw))
        ty.set_initial(T, capi.fixed_stiefel(RANK))
        t0 = time.perf_counter()
        ty.run(50)
        _, Ty = ty.round()
        solve_s = time.perf_counter() - t0
        try:
            return solve_s, ty.covariances(Ty, method="nested")[1]
        finally:
            ty.close()

    route_s, (solve_s, diag_y) = median_of(resolve, reps=1)
    t0 = time.perf_counter()
    _, diag, cross = tx.covariances(T, R.rect_pairs(poses, n), method="nested")
    blocks_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    dx, Sd, d2 = numpy_removal(T, ends, Rm, tm, kap, ta, poses, diag, cross)
    numpy_s = time.perf_counter() - t0
    tx.close()
    scale = np.abs(base_diag).max()
    print(json.dumps(dict(K=K, records=len(c), poses=len(poses), pair_blocks=n * len(poses), call_ms=1e3 * call_s,
                          new_team_solve_round_covariances_ms=1e3 * route_s, of_which_solve_and_round_ms=1e3 * solve_s,
                          covariances_of_the_rectangular_set_to_the_host_ms=1e3 * blocks_s, numpy_float64_one_core_ms=1e3 * numpy_s,
                          d2_joint=out["d2_joint"], information_loss=out["information_loss"], pivot_min_joint=out["pivot_min_joint"],
                          smallest_pivot_min=float(out["pivot_min"].min()), largest_dx=float(np.abs(out["delta"]).max()),
                          dx_against_numpy=float(np.abs(out["delta"] - dx).max()),
                          cov_diag_against_numpy=float(np.abs(out["cov_diag"] - Sd).max() / scale),
                          cov_diag_against_the_graph_without_them=float(np.abs(out["cov_diag"] - base_diag).max() / scale),
                          cov_diag_against_the_re_solved_graph=float(np.abs(out["cov_diag"] - diag_y).max() / scale),
                          trace_ratio=float(np.einsum("gaa->", out["cov_diag"]) / np.einsum("gaa->", diag)))), flush=True)
t.close()

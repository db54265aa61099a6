"""The first-order update (Team.linear_update, csrc/linear_update.hip) at the rounded optimum of sphere2500 held by ONE robot,
method="nested", on the sets Team.gate_jointly accepts out of K = 64 / 256 / 1024 seeded candidates (the batches of
gate_joint_time.py).  Per K one warm-up call, then the median wall time of three whole Python calls (each ends in the call's
own stream synchronisation); beside it the only route to the same blocks without the call -- a new Team.from_measurements on
the extended list, initialised at the same T, and covariances(method="nested") there --, and the float64 numpy statement of the
update on one core from the blocks a covariance call returns for the rectangular set (the time of that call is given apart).
With DPGO_TIMING=1 the library prints the covariance path's phases (the extraction of the N m pair blocks among them) and the
device time of each new kernel on stderr.
python profiles/experiments/linear_update_time.py [K ...] -> one JSON line per K"""
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


def median_of(call, reps=3):
    wall = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
    return float(np.median(wall[1:])), out


def numpy_update(T, ends, Rm, tm, kap, ta, poses, diag, cross):
    """the update in float64 with BLAS, the blocks as one 6 n x 6 m matrix: (dx, the diagonal blocks of Sigma', d2_joint)"""
    K, mm = len(ends), len(poses)
    rank = {e: a for a, e in enumerate(poses)}
    S = cross[:mm * n].reshape(mm, n, 6, 6).transpose(1, 2, 0, 3).reshape(6 * n, 6 * mm)
    A = np.zeros((6 * K, 6 * mm))
    for k, (i, j) in enumerate(ends):
        Ji, Jj = G.jacobians(T, int(i), int(j), np.float64)
        A[6 * k:6 * k + 6, 6 * rank[int(i)]:6 * rank[int(i)] + 6], A[6 * k:6 * k + 6, 6 * rank[int(j)]:6 * rank[int(j)] + 6] = Ji, Jj
    B = S @ A.T
    rows = np.concatenate([np.arange(6 * e, 6 * e + 6) for e in poses])
    M = A @ B[rows] + np.diag(np.asarray(R.r_diagonal(kap, ta, np.float64)))
    xi = np.asarray(J.innovations(T, ends, Rm, tm, np.float64)).reshape(-1)
    Gm = np.linalg.inv(0.5 * (M + M.T))
    z = Gm @ xi
    Um = B @ Gm
    corr = np.einsum("pac,pbc->pab", Um.reshape(n, 6, 6 * K), B.reshape(n, 6, 6 * K))
    return -(B @ z).reshape(n, 6), diag - corr, float(xi @ z)


for K in Ks:
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, seed=K, kappa=kappa, tau=tau)
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    cand["p1"], cand["p2"], cand["R"], cand["t"], cand["kappa"], cand["tau"] = ends[:, 0], ends[:, 1], Rm.reshape(K, 9), tm, kap, ta
    gate = t.gate_jointly(cand, T, method="nested")
    acc = np.sort(gate["accepted"])
    c = cand[acc]
    ends, Rm, tm, kap, ta = ends[acc], Rm[acc], tm[acc], kap[acc], ta[acc]
    poses = sorted(set(ends.reshape(-1).tolist()))
    sys.stderr.write("---- K = %d: %d accepted closures on %d distinct endpoint poses, %d pair blocks\n" % (K, len(c), len(poses), n * len(poses)))
    call_s, out = median_of(lambda: t.linear_update(c, T, method="nested"))
    # the only route to the same blocks without the call: a new team on the extended list, covariances at the same T.  With the
    # closures as measured T is no minimum of the extended graph and the path may refuse it (reported with the time it took);
    # with their measurements replaced by T's own relative poses T is a minimum, the sparsity and the work are the same, and
    # the covariance there is Sigma', which does not depend on the innovations
    def rebuild(records):
        tx = capi.Team.from_measurements(np.concatenate([m, records]), capi.default_params(r=RANK, num_robots=1, **kw))
        tx.set_initial(T, capi.fixed_stiefel(RANK))
        try:
            return tx.covariances(T, method="nested")[1]
        except capi.DpgoError as e:
            return str(e)
        finally:
            tx.close()

    ext = c.copy()
    ext["weight"] = 1.0
    as_measured_s, as_measured = median_of(lambda: rebuild(ext), reps=1)
    rel = [G.relative_pose(T, int(i), int(j), np.float64) for i, j in ends]
    ext["R"], ext["t"] = np.array([r[0].reshape(-1) for r in rel]), np.array([r[1] for r in rel])
    rebuild_s, diag_x = median_of(lambda: rebuild(ext), reps=1)
    # the numpy statement on one core, from the blocks of a covariance call for the rectangular set
    t0 = time.perf_counter()
    _, diag, cross = t.covariances(T, R.rect_pairs(poses, n), method="nested")
    blocks_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    dx, Sd, d2 = numpy_update(T, ends, Rm, tm, kap, ta, poses, diag, cross)
    numpy_s = time.perf_counter() - t0
    scale = np.abs(diag).max()
    print(json.dumps(dict(K=K, accepted=len(c), poses=len(poses), pair_blocks=n * len(poses), call_ms=1e3 * call_s,
                          new_team_and_covariances_ms=1e3 * rebuild_s, new_team_as_measured_ms=1e3 * as_measured_s,
                          new_team_as_measured=as_measured if isinstance(as_measured, str) else "ok", covariances_of_the_rectangular_set_to_the_host_ms=1e3 * blocks_s,
                          numpy_float64_one_core_ms=1e3 * numpy_s, d2_joint=out["d2_joint"], gate_jointly_d2_joint=gate["d2_joint"],
                          information_gain=out["information_gain"], largest_dx=float(np.abs(out["delta"]).max()),
                          dx_against_numpy=float(np.abs(out["delta"] - dx).max()),
                          cov_diag_against_numpy=float(np.abs(out["cov_diag"] - Sd).max() / scale),
                          cov_diag_against_the_rebuilt_graph=float(np.abs(out["cov_diag"] - diag_x).max() / scale),
                          trace_ratio=float(np.einsum("gaa->", out["cov_diag"]) / np.einsum("gaa->", diag)))), flush=True)
t.close()

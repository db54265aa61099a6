"""The Mahalanobis gate (Team.gate, csrc/gate.hip) at the rounded optimum of sphere2500 / 5 under each covariance method, against
the route without it: Team.covariances(pairs=...) plus the numpy post-processing of tests/gateref.py in float64.  Candidates:
the graph's own loop-closure edges (as measured) plus 100 000 seeded random pairs whose measurement is the estimate's relative
pose with a seeded residual.  Medians of 5 calls after one warm-up; wall time around the whole Python call (it ends in the
call's own stream synchronisation).  With DPGO_TIMING=1 the library prints the gate kernel's device time on stderr.
python profiles/experiments/gate_time.py [random pairs] -> one JSON line per method"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests import covref, gateref as G
from tests.test_gpu_certificate import OPTIMA, converge, team_at

ds, N, at_opt, kw = OPTIMA[0]
extra = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
t, m, n = team_at(ds, N, **kw)
assert converge(t, at_opt) > 0
_, T = t.round()
offs = np.cumsum([0] + [t.agents[i].n for i in t.ids])
zero = {i: o for i, o in zip(t.ids, offs)}
mm, _ = covref.team_measurements_global(t)
lc = mm[mm["p2"] != mm["p1"] + 1]
rng = np.random.default_rng(0)
pr = rng.integers(0, n, (extra, 2))
pr = pr[pr[:, 0] != pr[:, 1]]
P = np.asarray(T).reshape(n, 4, 3)
R, tr = P[:, :3, :].transpose(0, 2, 1), P[:, 3, :]
Rij = np.einsum("eji,ejk->eik", R[pr[:, 0]], R[pr[:, 1]])
tij = np.einsum("eji,ej->ei", R[pr[:, 0]], tr[pr[:, 1]] - tr[pr[:, 0]])
w = 0.05 * rng.standard_normal((len(pr), 3))
cand = np.zeros(len(lc) + len(pr), dtype=capi.MEAS_DTYPE)
cand[:len(lc)] = lc
cand["R"][len(lc):] = np.einsum("eij,ekj->eik", Rij, np.array([covref.exp_so3(x) for x in w])).reshape(-1, 9)
cand["t"][len(lc):] = tij + 0.05 * rng.standard_normal((len(pr), 3))
cand["kappa"][len(lc):], cand["tau"][len(lc):] = np.median(mm["kappa"]), np.median(mm["tau"])
cand["p1"][len(lc):], cand["p2"][len(lc):] = pr[:, 0], pr[:, 1]
# team-order pose -> (robot, pose)
for a, b in (("r1", "p1"), ("r2", "p2")):
    k = np.searchsorted(offs, cand[b], side="right") - 1
    cand[a], cand[b] = np.asarray(t.ids)[k], cand[b] - offs[k]
pairs = np.c_[[zero[r] for r in cand["r1"]] + cand["p1"], [zero[r] for r in cand["r2"]] + cand["p2"]].astype(np.int32)
sys.stderr.write("%s / %d: %d poses, %d loop closures + %d random pairs\n" % (ds, N, n, len(lc), len(pr)))


def numpy_gate(diag, cross):
    """tests/gateref.py in float64, vectorised over the candidates"""
    i, j = pairs[:, 0], pairs[:, 1]
    K = len(pairs)
    Ri = R[i]
    Rr = np.einsum("eji,ejk->eik", Ri, R[j])
    tt = np.einsum("eji,ej->ei", Ri, tr[j] - tr[i])
    Ji, Jj = np.zeros((K, 6, 6)), np.zeros((K, 6, 6))
    Ji[:, :3, :3] = -Rr.transpose(0, 2, 1)
    Ji[:, 3, 1], Ji[:, 3, 2], Ji[:, 4, 0], Ji[:, 4, 2], Ji[:, 5, 0], Ji[:, 5, 1] = -tt[:, 2], tt[:, 1], tt[:, 2], -tt[:, 0], -tt[:, 1], tt[:, 0]
    Ji[:, 3:, 3:] = -Ri.transpose(0, 2, 1)
    Jj[:, :3, :3] = np.eye(3)
    Jj[:, 3:, 3:] = Ri.transpose(0, 2, 1)
    C = Ji @ cross @ Jj.transpose(0, 2, 1)
    A = Ji @ diag[i] @ Ji.transpose(0, 2, 1) + Jj @ diag[j] @ Jj.transpose(0, 2, 1) + C + C.transpose(0, 2, 1)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    E = np.einsum("eji,ejk->eik", cand["R"].reshape(K, 3, 3), Rr)
    a = 0.5 * np.c_[E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]]
    s = np.linalg.norm(a, axis=1)
    th = np.arctan2(s, 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0))
    xi = np.c_[a * (th / np.maximum(s, 1e-300))[:, None], tt - cand["t"]]  # (no residual near pi among these candidates)
    S = A.copy()
    for q in range(3):
        S[:, q, q] += 0.5 / cand["kappa"]
        S[:, 3 + q, 3 + q] += 1.0 / cand["tau"]
    d2 = np.einsum("ei,ei->e", xi, np.linalg.solve(S, xi[:, :, None])[:, :, 0])
    return xi, d2, A


def median_of(call):
    wall = []
    for k in range(6):
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
    return float(np.median(wall[1:])), out


for method, mb in (("dense", None), ("schur", None), ("nested", 128)):
    sys.stderr.write("== %s\n" % method); sys.stderr.flush()
    gate_s, (res, xi, d2, accept) = median_of(lambda: t.gate(cand, T, method=method, max_block=mb))
    rel_s, _ = median_of(lambda: t.relative_covariances(pairs, T, method=method, max_block=mb))
    cov = (lambda: t.covariances_nested(T, pairs, max_block=mb)) if method == "nested" else (lambda: t.covariances(T, pairs, method=method))
    cov_s, (_, diag, cross) = median_of(cov)
    np_s, (xi_n, d2_n, _) = median_of(lambda: numpy_gate(diag, cross))
    path_s, _ = median_of((lambda: t.covariances_nested(T, max_block=mb)) if method == "nested" else (lambda: t.covariances(T, method=method)))
    print(json.dumps(dict(method=method, max_block=mb, candidates=len(cand), gate_wall_s=gate_s, relative_covariances_wall_s=rel_s,
                          covariances_with_pairs_wall_s=cov_s, numpy_postprocessing_s=np_s, covariances_without_pairs_wall_s=path_s,
                          accepted=int(accept.sum()), accepted_loop_closures=int(accept[:len(lc)].sum()), loop_closures=len(lc),
                          d2_rel_diff_numpy=float(np.abs(d2 - d2_n).max() / np.abs(d2_n).max()), device_assemble_s=res.seconds_assemble,
                          device_invert_s=res.seconds_invert)))
    sys.stdout.flush()
t.close()

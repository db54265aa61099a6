"""Schur path against the dense path of Team.covariances on the same rounded T: medians of 5 calls after one warm-up (wall, device
assembly, device inversion + products).  With DPGO_TIMING=1 the library prints the phases and every product's shape and TFLOP/s
on stderr.  python profiles/experiments/covariance_schur_time.py [--pairs K] [--methods schur,dense] [dataset ...] -> one JSON
line per case.  --pairs K: every call also asks for the K pairs of tests/test_gpu_covariance_schur.py::pair_cases (seed 7)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests.test_gpu_certificate import OPTIMA, RTR_NESTEROV, converge, team_at
from tests.test_gpu_covariance_schur import pair_cases

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--methods", default="schur,dense")
ap.add_argument("datasets", nargs="*")
args = ap.parse_args()

cases = [(o[0], o[1], o[2], o[3]) for o in OPTIMA] + [("parking-garage", 2, None, RTR_NESTEROV)]
only = args.datasets
out = {}
for ds, N, at_opt, kw in cases:
    if only and ds not in only:
        continue
    t, m, n = team_at(ds, N, **kw)
    if at_opt is None:
        t.run(500)
    else:
        assert converge(t, at_opt) > 0
    _, T = t.round()
    pairs = pair_cases(m, n, N, args.pairs, seed=7) if args.pairs else None
    row = {}
    for method in args.methods.split(","):
        sys.stderr.write("== %s / %d %s\n" % (ds, N, method)); sys.stderr.flush()
        wall, asm, inv = [], [], []
        for k in range(6):
            t0 = time.perf_counter()
            res, diag, _ = t.covariances(T, pairs, method=method)
            wall.append(time.perf_counter() - t0); asm.append(res.seconds_assemble); inv.append(res.seconds_invert)
        row[method] = dict(wall_s=float(np.median(wall[1:])), assemble_s=float(np.median(asm[1:])), invert_s=float(np.median(inv[1:])),
                           wall_all_s=wall[1:], logdet=res.logdet, min_pivot=res.min_pivot)
        row[method + "_diag"] = diag
    if "schur_diag" in row and "dense_diag" in row:
        row["diag_rel_diff"] = float(np.linalg.norm(row["schur_diag"] - row["dense_diag"]) / np.linalg.norm(row["dense_diag"]))
    row = {k: v for k, v in row.items() if not k.endswith("_diag")}
    row["n"] = 6 * (n - 1)
    out[ds + " / %d" % N] = row
    print(json.dumps({ds + " / %d" % N: row})); sys.stdout.flush()
    t.close()

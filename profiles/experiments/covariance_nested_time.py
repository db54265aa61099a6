"""Nested path of the marginal covariances against the dense and the Schur path on the same rounded T, in one process:
medians of 5 calls after one warm-up (wall, device assembly, device factorisations + products).  Per dataset of
tests/test_gpu_certificate.OPTIMA: the N-robot team is brought to the pinned optimum and rounded; nested at max_block in
{64, 128, 256, 512} against method="schur" on that team, then against method="dense" on a ONE-robot team on the unpartitioned
measurements, initialised at the same T.  With DPGO_TIMING=1 the library prints the five phases, the bytes and the TFLOP/s of the
batched factorisations and products on stderr.
python profiles/experiments/covariance_nested_time.py [--pairs K] [--blocks 64,128,..] [--team-only] [dataset ...] -> one JSON
line per team.  --pairs K: every call on the N-robot team also asks for the K pairs of
tests/test_gpu_covariance_schur.py::pair_cases (seed 7); --team-only: without the one-robot team"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests.test_gpu_certificate import OPTIMA, RTR_NESTEROV, converge, team_at
from tests.test_gpu_covariance_schur import pair_cases

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--blocks", default="64,128,256,512")
ap.add_argument("--team-only", action="store_true")
ap.add_argument("datasets", nargs="*")
args = ap.parse_args()
BLOCKS = tuple(int(b) for b in args.blocks.split(","))


def timed(call):
    wall, asm, inv = [], [], []
    for k in range(6):
        t0 = time.perf_counter()
        res, diag, _ = call()
        wall.append(time.perf_counter() - t0); asm.append(res.seconds_assemble); inv.append(res.seconds_invert)
    return dict(wall_s=float(np.median(wall[1:])), assemble_s=float(np.median(asm[1:])), invert_s=float(np.median(inv[1:])),
                wall_all_s=wall[1:], logdet=res.logdet, min_pivot=res.min_pivot), diag


def sweep(tag, t, T, other, pairs=None):
    sys.stderr.write("== %s %s\n" % (tag, other)); sys.stderr.flush()
    row = {}
    row[other], ref = timed(lambda: t.covariances(T, pairs, method=other))
    for mb in BLOCKS:
        sys.stderr.write("== %s nested %d\n" % (tag, mb)); sys.stderr.flush()
        r, diag = timed(lambda: t.covariances_nested(T, pairs, max_block=mb))
        r["plan"] = t.covariance_plan(mb)[1]
        r["diag_rel_diff"] = float(np.linalg.norm(diag - ref) / np.linalg.norm(ref))
        row["nested_%d" % mb] = r
    print(json.dumps({tag: row})); sys.stdout.flush()


only = args.datasets
for ds, N, at_opt, kw in OPTIMA:
    if only and ds not in only:
        continue
    t, m, n = team_at(ds, N, **kw)
    assert converge(t, at_opt) > 0
    _, T = t.round()
    sweep("%s / %d" % (ds, N), t, T, "schur", pair_cases(m, n, N, args.pairs, seed=7) if args.pairs else None)
    t.close()
    if args.team_only:
        continue
    one = capi.Team.from_measurements(m, capi.default_params(r=5, num_robots=1, **RTR_NESTEROV))
    one.set_initial(T, capi.fixed_stiefel(5))
    sweep("%s / 1" % ds, one, T, "dense")
    one.close()

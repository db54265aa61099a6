"""Marginal covariances at the converged, rounded point (RTR + Nesterov from chordal, to the pinned SE-Sync optimum):
device seconds of the assembly and of the inverse (dpgo_covariance_t, events on the team's stream), of the extraction
(the library's DPGO_TIMING line), wall time of the call, the inverse's share of the fp64 matrix peak, and -- with
--numpy-inv, sphere2500 only -- numpy.linalg.inv of the same H_red on one CPU core.
    python profiles/experiments/covariance_time.py [--numpy-inv] [--out FILE] [dataset:robots ...]
Prints one JSON line per dataset.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python ...`."""
import os
import sys

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = "1"  # the numpy baseline on one core
os.environ["DPGO_TIMING"] = "1"
import json
import re
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dpgo_ros_amd import capi  # noqa: E402
from tests import covref  # noqa: E402
from tests.test_gpu_certificate import OPTIMA, converge, team_at  # noqa: E402

PEAK_FP64_MATRIX = 78.6e12  # AMD's published fp64 matrix rate of the MI355X, FLOP/s


def stderr_of(fn):
    """fn() with the process's stderr captured (the library writes its DPGO_TIMING lines there)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def main():
    args = sys.argv[1:]
    numpy_inv = "--numpy-inv" in args
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    cases = [a for a in args if ":" in a] or ["sphere2500:5", "torus3D:8", "cubicle:4"]
    lines = []
    for case in cases:
        ds, N = case.split(":")
        N = int(N)
        _, _, at_optimum, kw = [o for o in OPTIMA if o[0] == ds][0]
        t, m, n = team_at(ds, N, **kw)
        k = converge(t, at_optimum)
        rd, T = t.round()
        pairs = np.stack([np.arange(n), np.full(n, n - 1)], axis=1)
        t.covariances(T, pairs)  # warm-up: first launches, allocations
        reps, rec = 3, []
        for _ in range(reps):
            t0 = time.perf_counter()
            (res, diag, cross), err = stderr_of(lambda: t.covariances(T, pairs))
            wall = time.perf_counter() - t0
            mx = re.search(r"marginal_covariances: n (\d+), (\d+) blocks, assemble ([\d.]+) ms, invert ([\d.]+) ms, extract ([\d.]+) ms", err)
            rec.append(dict(wall_s=wall, assemble_s=res.seconds_assemble, invert_s=res.seconds_invert,
                            extract_s=1e-3 * float(mx.group(5)), blocks=int(mx.group(2))))
        nn = res.n
        inv = float(np.median([r["invert_s"] for r in rec]))
        flops = float(nn) ** 3  # n^3 / 3 each: Cholesky, triangular inverse, W^T W
        line = dict(dataset=ds, robots=N, poses=n, n=nn, solve_iterations=k, f_rounded=rd.f_rounded, blocks=rec[0]["blocks"],
                    bytes_three_matrices=3 * 8 * nn * nn, logdet=res.logdet, min_pivot=res.min_pivot, max_pivot=res.max_pivot,
                    assemble_s=float(np.median([r["assemble_s"] for r in rec])), invert_s=inv,
                    extract_s=float(np.median([r["extract_s"] for r in rec])), wall_s=float(np.median([r["wall_s"] for r in rec])),
                    all=rec, invert_flops=flops, invert_tflops=1e-12 * flops / inv, invert_share_of_fp64_matrix_peak=flops / inv / PEAK_FP64_MATRIX)
        Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
        Cp = cross[1:].reshape(nn, 6)
        E = np.zeros_like(Cp)
        E[-6:] = np.eye(6)
        line["residual_last_pose"] = float(np.linalg.norm(Hr @ Cp - E))
        if numpy_inv and ds == "sphere2500":
            Hd = Hr.toarray()
            t0 = time.perf_counter()
            Sd = np.linalg.inv(Hd)
            line["numpy_inv_1core_s"] = time.perf_counter() - t0
            line["numpy_vs_gpu_last_column_rel"] = float(np.linalg.norm(Sd[:, -6:] - Cp) / np.linalg.norm(Sd[:, -6:]))
        t.close()
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

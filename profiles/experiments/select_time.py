"""The selection under a budget (Team.select_closures, csrc/select.hip) at the rounded optimum of sphere2500 held by ONE robot,
method="nested", on pools of P = 1024 / 4096 seeded pose pairs (the pairs, kappa and tau of tests/jointref.seeded_batch at the
graph's median kappa and tau) with budgets 16 / 64 / 256.  Per (P, budget) one warm-up call, then the median wall time of three
whole Python calls (each ends in the call's own stream synchronisation).  With DPGO_TIMING=1 the library prints the covariance
path's phases, k_select_open and the elimination (device time between events) on stderr.  Two references, both measured:
  the only route without this call: gate_jointly(..., innovation_covariance=True) forms all of M and brings it to the host
    (one call, timed), and the greedy runs there;
  the greedy on the host: tests/selectref.run in float64 on one core on that M, whose blocks are bit for bit the ones
    k_select_step forms on the fly.
python profiles/experiments/select_time.py [--select-only] [P ...] -> one JSON line per (P, budget)"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests import jointref as J
from tests import selectref as S
from tests.test_gpu_certificate import OPTIMA, converge, team_at

args = sys.argv[1:]
select_only = "--select-only" in args
Ps = [int(a) for a in args if not a.startswith("--")] or [1024, 4096]
BUDGETS = (16, 64, 256)
ds, N, at_opt, kw = OPTIMA[0]
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


for P in Ps:
    ends, _, _, kap, ta, _ = J.seeded_batch(T, n, P, seed=P, outliers=0.0, kappa=kappa, tau=tau)
    pool = t.candidates_from_pairs(ends, kap, ta)
    poses = len(set(ends.reshape(-1).tolist()))
    outs = {}
    for b in BUDGETS:
        sys.stderr.write("---- P = %d, budget %d, %d distinct endpoint poses\n" % (P, b, poses))
        try:
            call_s, out = median_of(lambda: t.select_closures(pool, b, T, method="nested"))
        except capi.DpgoError as e:
            print(json.dumps(dict(P=P, budget=b, poses=poses, refused=str(e))), flush=True)
            continue
        outs[b] = (call_s, out)
        if select_only:
            print(json.dumps(dict(P=P, budget=b, poses=poses, call_ms=1e3 * call_s, gain_total=out["gain_total"])), flush=True)
    if select_only or not outs:
        continue
    sys.stderr.write("---- P = %d, all of M by gate_jointly\n" % P)
    t0 = time.perf_counter()
    try:
        full = t.gate_jointly(pool, T, method="nested", innovation_covariance=True)
        joint_s = time.perf_counter() - t0
    except capi.DpgoError as e:
        full, joint_s = None, None
        sys.stderr.write("gate_jointly refused: %s\n" % e)
    ldR = np.asarray(S.logdet_meas(kap, ta), dtype=np.float64)
    for b, (call_s, out) in outs.items():
        rec = dict(P=P, budget=b, poses=poses, call_ms=1e3 * call_s, selected=int(out["num_selected"]), gain_total=out["gain_total"],
                   largest_marginal_gains=float(np.sort(out["gain"])[-b:].sum()))
        if full is not None:
            t0 = time.perf_counter()
            ref = S.run(full["M"], ldR, b, dtype=np.float64)
            ref_s = time.perf_counter() - t0
            rec.update(gate_jointly_with_M_ms=1e3 * joint_s, selectref_float64_ms=1e3 * ref_s,
                       selectref_agrees=bool(list(ref["selected"]) == list(out["selected"])),
                       largest_gain_cond_difference=float(np.abs(np.asarray(ref["gain_cond"], dtype=np.float64) - out["gain_cond"]).max()))
        print(json.dumps(rec), flush=True)
t.close()

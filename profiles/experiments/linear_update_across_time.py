"""The first-order update over a split team (Team.linear_update with transport=, dpgo_team_linear_update_across) at the rounded
optimum of sphere2500 as 5 robots, on the sets Team.gate_jointly accepts out of K = 64 / 256 / 1024 seeded candidates (the 51 /
218 / 834 closures of linear_update_time.py, renumbered to the five robots): one participant that holds every robot, the split
[[0, 2, 4], [1, 3]] and five participants of one robot, as LocalGroup THREADS ON ONE DEVICE -- all that exists where this was
measured: the participants share the device's queues and the host's interpreter lock between their library calls, so a figure
here is an upper bound on what one process per GPU would take, not a measurement of it.
Baseline: the joined team's linear_update(columns="solve", method="nested") at the default max_block on the same T and closures.
Per configuration and K one warm-up call, then five whole calls (each ends when every participant has returned): the median
wall time, beside it the median of covariances(transport=) with no pairs in the same configuration -- the path the call rides
on --, the bytes every allgather moved (8 x the record x the participants, summed over the call's allgathers) and, with
DPGO_TIMING=1, the library's own lines on stderr: the path's phases and the new kernels' times per rank.
python profiles/experiments/linear_update_across_time.py [K ...] -> one JSON line per configuration and K"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests import jointref as J
from tests.test_gpu_certificate import OPTIMA, converge, team_at
from tests.test_gpu_certify_across import Split

ds, N, at_opt, kw = OPTIMA[0]
Ks = [int(a) for a in sys.argv[1:]] or [64, 256, 1024]
t5, m, n = team_at(ds, N, **kw)
assert converge(t5, at_opt) > 0
_, T = t5.round()
X0 = t5.global_X()
mp = capi.partition(m, n, N)
t1, _, _ = team_at(ds, 1, T=T, **kw)
kappa, tau = float(np.median(m["kappa"])), float(np.median(m["tau"]))
CONFIGS = [("one participant", [[0, 1, 2, 3, 4]]), ("[[0, 2, 4], [1, 3]]", [[0, 2, 4], [1, 3]]), ("five participants", [[i] for i in range(N)])]
KEYS = ("T", "delta", "cov_diag")


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def counting(group, tally):
    """the group's transports with their allgathers' bytes added to tally[0]"""
    for tr in group:
        inner = tr.allgather

        def counted(x, inner=inner, tr=tr):
            if tr.rank == 0:
                tally[0] += 8 * len(x) * tr.world
            return inner(x)
        tr.allgather = counted
    return group


for K in Ks:
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, seed=K, kappa=kappa, tau=tau)
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    cand["p1"], cand["p2"], cand["R"], cand["t"], cand["kappa"], cand["tau"] = ends[:, 0], ends[:, 1], Rm.reshape(K, 9), tm, kap, ta
    acc = np.sort(t1.gate_jointly(cand, T, method="nested")["accepted"])
    c = cand[acc]
    sp0 = Split(mp, N, CONFIGS[0][1], X0)
    goff = np.asarray(sp0.goff)
    sp0.close()
    for a, b in (("r1", "p1"), ("r2", "p2")):  # (the contiguous partition: global pose = the single robot's pose)
        g = c[b].copy()
        c[a] = np.searchsorted(goff, g, side="right") - 1
        c[b] = g - goff[c[a]]
    poses = len(set(ends[acc].reshape(-1).tolist()))
    wall = []
    for rep in range(6):  # (the first call is the warm-up)
        if rep == 1:
            sys.stderr.write("---- the joined team, columns=\"solve\", method=\"nested\", K = %d accepted of %d\n" % (len(c), K))
        s, joined = timed(lambda: t5.linear_update(c, T, method="nested", columns="solve"))
        if rep > 0:
            wall.append(s)
    print(json.dumps(dict(config="joined team, solve on nested", K=K, accepted=len(c), poses=poses, call_ms=1e3 * float(np.median(wall)),
                          all_ms=[round(1e3 * x, 2) for x in wall])), flush=True)
    first = None
    for name, parts in CONFIGS:
        sp = Split(mp, N, parts, X0)
        wall, path, tally, calls = [], [], [0], None
        Tq = [np.ascontiguousarray(T[sp.cols(q, 12)]) for q in range(len(parts))]
        for rep in range(6):
            s, _ = timed(lambda: sp.run(lambda tm_, tr: tm_.covariances(Tq[tr.rank], transport=tr, owner_of_robot=sp.owner)))
            if rep > 0:
                path.append(s)
        for rep in range(6):
            if rep == 1:
                sys.stderr.write("---- %s, K = %d accepted of %d\n" % (name, len(c), K))
            tally[0] = 0
            g = counting(capi.LocalGroup(len(parts)), tally)
            s, outs = timed(lambda: sp.run(lambda tm_, tr: tm_.linear_update(c, Tq[tr.rank], transport=tr, owner_of_robot=sp.owner), g))
            calls = dict(g[0].calls)
            if rep > 0:
                wall.append(s)
        whole = dict(T=np.zeros(12 * n), delta=np.zeros((n, 6)), cov_diag=np.zeros((n, 6, 6)))
        for q, o in enumerate(outs):
            whole["T"][sp.cols(q, 12)], whole["delta"][sp.cols(q, 1)], whole["cov_diag"][sp.cols(q, 1)] = o["T"], o["delta"], o["cov_diag"]
        blob = b"".join(whole[k].tobytes() for k in KEYS) + outs[0]["xi"].tobytes() + outs[0]["xi_post"].tobytes()
        if first is None:
            first = blob
        scale = np.abs(joined["cov_diag"]).max()
        print(json.dumps(dict(config=name, K=K, accepted=len(c), poses=poses, call_ms=1e3 * float(np.median(wall)),
                              all_ms=[round(1e3 * x, 2) for x in wall], path_ms=1e3 * float(np.median(path)), allgathers=calls["allgather"],
                              exchanges=calls["exchange"], gathered_bytes=tally[0], same_bits_as_one_participant=bool(blob == first),
                              delta_against_joined=float(np.abs(whole["delta"] - joined["delta"]).max()),
                              cov_diag_against_joined=float(np.abs(whole["cov_diag"] - joined["cov_diag"]).max() / scale),
                              d2_joint=outs[0]["d2_joint"], joined_d2_joint=joined["d2_joint"],
                              information_gain=outs[0]["information_gain"])), flush=True)
        sp.close()
t1.close()
t5.close()

"""Sigma applied to vectors over a split team (Team.covariance_apply with transport=, dpgo_team_covariance_apply_across) at
the rounded optimum of sphere2500 as 5 robots, on seeded normal columns at m = 64 and 1024: one participant that holds every
robot, the split [[0, 2, 4], [1, 3]] and five participants of one robot, as LocalGroup THREADS ON ONE DEVICE -- all that
exists where this was measured: the participants share the device's queues and the host's interpreter lock between their
library calls, so a figure here is an upper bound on what one process per GPU would take, not a measurement of it.
Baseline: the single team's covariance_apply(method="nested") at the default max_block on the same T and V.
Per configuration and m one warm-up call, then five whole calls (each ends when every participant has returned; every
participant's rows of V and poses of T are cut out beforehand): the median wall time, beside it the median of
covariances(transport=) with no pairs in the same configuration -- the path the call rides on --, the bytes every allgather moved (8 x the record x the participants, summed over the call's allgathers) and, with
DPGO_TIMING=1, the library's own lines on stderr: the path's phases and the apply's products with their TFLOP/s per rank.
python profiles/experiments/covariance_apply_across_time.py [m ...] -> one JSON line per configuration and m"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests.test_gpu_certificate import OPTIMA, converge, team_at
from tests.test_gpu_certify_across import Split

ds, N, at_opt, kw = OPTIMA[0]
cols_list = [int(a) for a in sys.argv[1:]] or [64, 1024]
t5, m, n = team_at(ds, N, **kw)
assert converge(t5, at_opt) > 0
_, T = t5.round()
X0 = t5.global_X()
mp = capi.partition(m, n, N)
CONFIGS = [("one participant", [[0, 1, 2, 3, 4]]), ("[[0, 2, 4], [1, 3]]", [[0, 2, 4], [1, 3]]), ("five participants", [[i] for i in range(N)])]


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


rng = np.random.default_rng(5)
for cols in cols_list:
    V = np.asfortranarray(rng.standard_normal((6 * n, cols)))
    wall = []
    for rep in range(6):  # (the first call is the warm-up)
        if rep == 1:
            sys.stderr.write("---- the single team, method=\"nested\", m = %d\n" % cols)
        s, (res0, Xn) = timed(lambda: t5.covariance_apply(V, T, method="nested"))
        if rep > 0:
            wall.append(s)
    print(json.dumps(dict(config="single team, nested", m=cols, rows=6 * n, call_ms=1e3 * float(np.median(wall)),
                          all_ms=[round(1e3 * x, 2) for x in wall])), flush=True)
    first = None
    for name, parts in CONFIGS:
        sp = Split(mp, N, parts, X0)
        wall, path, tally, calls = [], [], [0], None
        Vq = [np.asfortranarray(V[sp.cols(q, 6)]) for q in range(len(parts))]
        Tq = [np.ascontiguousarray(T[sp.cols(q, 12)]) for q in range(len(parts))]
        for rep in range(6):
            s, _ = timed(lambda: sp.run(lambda tm, tr: tm.covariances(Tq[tr.rank], transport=tr, owner_of_robot=sp.owner)))
            if rep > 0:
                path.append(s)
        for rep in range(6):
            if rep == 1:
                sys.stderr.write("---- %s, m = %d\n" % (name, cols))
            tally[0] = 0
            g = counting(capi.LocalGroup(len(parts)), tally)
            s, outs = timed(lambda: sp.run(lambda tm, tr: tm.covariance_apply(Vq[tr.rank], Tq[tr.rank], transport=tr, owner_of_robot=sp.owner), g))
            calls = dict(g[0].calls)
            if rep > 0:
                wall.append(s)
        X = np.zeros((6 * n, cols))
        for q, (_, Xq) in enumerate(outs):
            X[sp.cols(q, 6)] = Xq
        if first is None:
            first = X
        print(json.dumps(dict(config=name, m=cols, rows=6 * n, call_ms=1e3 * float(np.median(wall)), all_ms=[round(1e3 * x, 2) for x in wall],
                              path_ms=1e3 * float(np.median(path)), allgathers=calls["allgather"], exchanges=calls["exchange"], gathered_bytes=tally[0],
                              same_bits_as_one_participant=bool(X.tobytes() == first.tobytes()),
                              against_nested=float(np.abs(X - Xn).max() / np.abs(Xn).max()), logdet=outs[0][0].logdet)), flush=True)
        sp.close()
t5.close()

"""Team.refine over a split team (transport=, dpgo_team_refine_across; csrc/refine.hip) at the rounded point of sphere2500 after
a 5-robot run to the pinned optimum's 1e-6 relative gap -- the point of profiles/experiments/refine_time.py: one participant
that holds every robot, the split [[0, 2, 4], [1, 3]] and five participants of one robot, as LocalGroup THREADS ON ONE DEVICE
-- all that exists where this was measured: the participants share the device's queues and the host's interpreter lock between
their library calls, so a figure here is an upper bound on what one process per GPU would take, not a measurement of it.
Baselines: the single team's refine(method="nested") at the default max_block on the joined team (r23), and as many
covariance_apply(transport=) calls at m = 1 as the refinement took steps -- the path the call rides on (r24).
Per configuration one warm-up call, then five whole calls (each ends when every participant has returned; every participant's
poses of T are cut out beforehand): iterations, |g|_inf per iterate, the median wall time, the bytes of every allgather of the
call (8 x the record x the participants) and, with DPGO_TIMING=1, the library's own lines on stderr: the call's split into
gradient and cost, the paths, the trial kernels and the robots' cost kernels, per rank.
python profiles/experiments/refine_across_time.py -> one JSON line per configuration"""
import json, os, sys, time
os.environ.setdefault("OMP_NUM_THREADS", "1")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from dpgo_ros_amd import capi
from tests.test_gpu_certificate import OPTIMA, converge, team_at
from tests.test_gpu_certify_across import Split

ds, N, at_opt, kw = OPTIMA[0]
t5, m, n = team_at(ds, N, **kw)
its = converge(t5, at_opt)
assert its > 0
_, T = t5.round()
X0 = t5.global_X()
mp = capi.partition(m, n, N)
CONFIGS = [("one participant", [[0, 1, 2, 3, 4]]), ("[[0, 2, 4], [1, 3]]", [[0, 2, 4], [1, 3]]), ("five participants", [[i] for i in range(N)])]
sys.stderr.write("---- %s: %d poses, %d measurements, %d iterations to the pinned cost\n" % (ds, n, len(m), its))


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def counting(group, tally):
    """the group's transports with the bytes of rank 0's allgathers listed in tally"""
    for tr in group:
        inner = tr.allgather

        def counted(x, inner=inner, tr=tr):
            if tr.rank == 0:
                tally.append(8 * len(x) * tr.world)
            return inner(x)
        tr.allgather = counted
    return group


wall, single = [], None
for rep in range(6):  # (the first call is the warm-up)
    if rep == 1:
        sys.stderr.write("---- the joined team, method=\"nested\"\n")
    s, single = timed(lambda: t5.refine(T, method="nested"))
    if rep > 0:
        wall.append(s)
print(json.dumps(dict(config="joined team, nested", status=single["status"], iterations=single["iterations"],
                      call_ms=1e3 * float(np.median(wall)), all_ms=[round(1e3 * x, 2) for x in wall],
                      grad_inf=[float(v) for v in single["history"]["grad_inf"]], f=[float(v) for v in single["history"]["f"]])), flush=True)
first = None
for name, parts in CONFIGS:
    sp = Split(mp, N, parts, X0)
    Tq = [np.ascontiguousarray(T[sp.cols(q, 12)]) for q in range(len(parts))]
    Vq = [np.ones(6 * (len(Tq[q]) // 12)) for q in range(len(parts))]
    wall, tally, calls, outs = [], [], None, None
    for rep in range(6):
        if rep == 1:
            sys.stderr.write("---- %s\n" % name)
        del tally[:]
        g = counting(capi.LocalGroup(len(parts)), tally)
        s, outs = timed(lambda: sp.run(lambda tm, tr: tm.refine(Tq[tr.rank], transport=tr, owner_of_robot=sp.owner), g))
        calls = dict(g[0].calls)
        if rep > 0:
            wall.append(s)
    steps = outs[0]["iterations"]
    rides = []
    for rep in range(6):  # the path the call rides on: as many applies of one column as the refinement took steps
        s, _ = timed(lambda: [sp.run(lambda tm, tr: tm.covariance_apply(Vq[tr.rank], Tq[tr.rank], transport=tr, owner_of_robot=sp.owner))
                              for _ in range(steps)])
        if rep > 0:
            rides.append(s)
    Tg = np.zeros(12 * n)
    for q, o in enumerate(outs):
        Tg[sp.cols(q, 12)] = o["T"]
    if first is None:
        first = Tg
    h = outs[0]["history"]
    print(json.dumps(dict(config=name, status=outs[0]["status"], iterations=steps, call_ms=1e3 * float(np.median(wall)),
                          all_ms=[round(1e3 * x, 2) for x in wall], applies_ms=1e3 * float(np.median(rides)),
                          grad_inf=[float(v) for v in h["grad_inf"]], f=[float(v) for v in h["f"]], alpha=[float(v) for v in h["alpha"]],
                          allgathers=calls["allgather"], exchanges=calls["exchange"], allgather_bytes=list(tally),
                          same_bits_as_one_participant=bool(Tg.tobytes() == first.tobytes()),
                          against_joined_team=float(np.abs(Tg - single["T"]).max()))), flush=True)
    sp.close()
t5.close()

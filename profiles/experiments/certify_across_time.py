"""Certificate and rounding across teams at the converged sphere2500 / 5-agent point (RTR + Nesterov from chordal, to the
1e-6 gap; the point of r07_certify.md and r08_round.md): wall time of certify (eta 1e-6, tol 1e-8) and of round (with and
without the translation refinement) for the single team, a one-participant transport, 2 and 5 teams driven from threads
of one process on one GPU, and 2 processes on one GPU over gloo.  Median of warm calls; LOBPCG iterations and transport
calls per call.  Prints one JSON line; with an argument, also writes it to that file."""
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dpgo_ros_amd import capi  # noqa: E402

FSTAR = 843.5029071410438
REPS = 5
CERT = dict(eta=1e-6, tol=1e-8, max_iters=1000)


def load():
    m, n = capi.read_g2o(os.path.join(ROOT, "data", "sphere2500.g2o"))
    return m, capi.partition(m, n, 5), n


def split_teams(mp, parts, X):
    sizes = [capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=5), local_ids=[i]).agents[i].n
             for i in range(5)]
    goff = np.concatenate([[0], np.cumsum(sizes)])
    owner = np.zeros(5, dtype=np.int32)
    teams = []
    for q, ids in enumerate(parts):
        owner[ids] = q
        t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=5), local_ids=ids)
        for i in ids:
            t.agents[i].set_X(X[goff[i] * 20:goff[i + 1] * 20])
        teams.append(t)
    return teams, owner


def timed(fn):
    fn()  # warm-up (workspace allocation)
    ts, out = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), out


def measure(calls, counters):
    """calls: {name: fn() -> result}; counters() -> transport calls so far (None for the single team)"""
    res = {}
    for name, fn in calls.items():
        c0 = counters()
        ms, out = timed(fn)
        c1 = counters()
        res[name] = dict(ms=ms)
        if c0 is not None:
            res[name]["transport_calls_per_call"] = {k: (c1[k] - c0[k]) / (REPS + 1) for k in c0}
        if name == "certify":
            res[name]["iterations"] = out.iterations
            res[name]["certified"] = out.certified
    return res


def threads(mp, parts, X):
    teams, owner = split_teams(mp, parts, X)
    g = capi.LocalGroup(len(teams))

    def run(call):
        r = g.run([lambda q=q: call(teams[q], g[q]) for q in range(len(teams))])
        for _, e in r:
            if e is not None:
                raise e
        return r[0][0]

    calls = {"certify": lambda: run(lambda t, tr: t.certify(transport=tr, owner_of_robot=owner, **CERT)[0]),
             "round": lambda: run(lambda t, tr: t.round(False, transport=tr, owner_of_robot=owner)),
             "round_refined": lambda: run(lambda t, tr: t.round(True, transport=tr, owner_of_robot=owner))}
    res = measure(calls, lambda: dict(g[0].calls))
    for t in teams:
        t.close()
    return res


def _gloo_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from dpgo_ros_amd.distributed import TorchTransport
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, mp, _ = load()
    X = np.load(os.path.join(outdir, "X.npy"))
    teams, owner = split_teams(mp, [[[0, 2, 4], [1, 3]][rank]], X)
    owner = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    t, tr = teams[0], TorchTransport(dist)

    def sync(fn):
        def f():
            dist.barrier()
            return fn()
        return f

    calls = {"certify": sync(lambda: t.certify(transport=tr, owner_of_robot=owner, **CERT)[0]),
             "round": sync(lambda: t.round(False, transport=tr, owner_of_robot=owner)),
             "round_refined": sync(lambda: t.round(True, transport=tr, owner_of_robot=owner))}
    res = measure(calls, lambda: dict(tr.calls))
    with open(os.path.join(outdir, "r%d.json" % rank), "w") as f:
        json.dump(res, f)
    t.close()
    dist.destroy_process_group()


def main():
    m, mp, n = load()
    kw = dict(method=capi.METHOD_RTR, acceleration=1, rtr_iterations=3, rtr_tcg_iterations=50, gradnorm_tol=1e-2,
              restart_interval=50)
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=5, **kw))
    t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(5))
    k = 0
    while (t.cost() - FSTAR) / FSTAR > 1e-6 and k < 5000:
        t.run(10)
        k += 10
    out = dict(dataset="sphere2500", agents=5, solve_iterations=k, gap=(t.cost() - FSTAR) / FSTAR, reps=REPS)
    X = t.global_X()
    out["single_team"] = measure({"certify": lambda: t.certify(**CERT)[0], "round": lambda: t.round(False),
                                  "round_refined": lambda: t.round(True)}, lambda: None)
    g1 = capi.LocalGroup(1)
    own = np.zeros(5, dtype=np.int32)
    out["one_participant"] = measure(
        {"certify": lambda: t.certify(transport=g1[0], owner_of_robot=own, **CERT)[0],
         "round": lambda: t.round(False, transport=g1[0], owner_of_robot=own),
         "round_refined": lambda: t.round(True, transport=g1[0], owner_of_robot=own)}, lambda: dict(g1[0].calls))
    t.close()
    out["two_teams_threads"] = threads(mp, [[0, 2, 4], [1, 3]], X)
    out["five_teams_threads"] = threads(mp, [[0], [1], [2], [3], [4]], X)
    import torch.multiprocessing as mp_
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "X.npy"), X)
        mp_.spawn(_gloo_worker, args=(2, port, d), nprocs=2, join=True)
        out["two_processes_gloo"] = [json.load(open(os.path.join(d, "r%d.json" % q))) for q in range(2)]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

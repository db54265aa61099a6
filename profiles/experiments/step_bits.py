"""the bit comparison of profiles/r19_nesterov_step.md: the iterates of the accelerated-RGD iteration in its three device
forms -- default (the deep-carried form where the team allows it), DPGO_FE_DEEP=0 (k_step_fe), DPGO_FUSED_EVAL=0 (k_precond +
k_eval_stats) -- under the cases of tests/test_gpu_fused_step.py: sphere2500 over (robots, r) = (5, 5), (8, 5), (5, 3), (6, 4),
and its first 2494 poses over 5 robots with a restart every 7 iterations; DPGO_FE_MIN_N=32 throughout.  After runs of 23, 300,
64, 7 and 129 iterations every case leaves a SHA-256 of X, Y and V of every agent, of the status of the last agent and of the
team's cost.  One process per library (DPGO_HIP_LIB names the other one); two dumps are compared array by array.
usage: python profiles/experiments/step_bits.py OUT.json            run the cases, write the dump
       python profiles/experiments/step_bits.py A.json B.json       -> arrays, arrays that differ"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RUNS = (23, 300, 64, 7, 129)
FORMS = (("default", {}), ("DPGO_FE_DEEP=0", {"DPGO_FE_DEEP": "0"}), ("DPGO_FUSED_EVAL=0", {"DPGO_FUSED_EVAL": "0"}))
# (robots, r, poses kept or None for all, restart interval)
CASES = ((5, 5, None, 20), (8, 5, None, 20), (5, 3, None, 20), (6, 4, None, 20), (5, 5, 2494, 7))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    if sorted(A) != sorted(B):
        print("the dumps hold different arrays")
        return 1
    differ = [k for k in sorted(A) if A[k] != B[k]]
    for k in differ:
        print("%s differs" % k)
    print(json.dumps(dict(arrays=len(A), arrays_differing=len(differ))))
    return 1 if differ else 0


if len(sys.argv) == 3:
    sys.exit(compare(sys.argv[1], sys.argv[2]))

import numpy as np

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests.util import load

RGD = dict(method=1, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def team(robots, r, keep, restart, env):
    m, _, n = load("sphere2500", 1)
    if keep:
        n = keep
        m = m[(m["p1"] < n) & (m["p2"] < n)].copy()
    mp = O.partition(m, n, robots)
    names = ("DPGO_FUSED_EVAL", "DPGO_FE_DEEP", "DPGO_FE_MIN_N")
    old = {k: os.environ.get(k) for k in names}
    try:  # (the three are read when a team is created)
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(env, DPGO_FE_MIN_N="32")
        t = capi.Team.from_measurements(mp.view(capi.MEAS_DTYPE), capi.default_params(r=r, num_robots=robots, restart_interval=restart, **RGD))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    t.set_initial(O.odometry_init(m, n), O.fixed_stiefel(r))
    return t


out = {}
for robots, r, keep, restart in CASES:
    for form, env in FORMS:
        t = team(robots, r, keep, restart, env)
        done = 0
        for iters in RUNS:
            t.run(iters)
            t.synchronize()
            done += iters
            key = "robots %d r %d poses %s restart %d | %s | after %d" % (robots, r, keep or "all", restart, form, done)
            for k in t.ids:
                a = t.agents[k]
                for name, v in (("X", a.get_X()), ("Y", a.get_Y()), ("V", a.get_V())):
                    out["%s | agent %d %s" % (key, k, name)] = sha(np.ascontiguousarray(v).tobytes())
            s = t.agents[t.ids[-1]].status()
            out[key + " | status of the last agent"] = sha(repr([(f[0], getattr(s, f[0])) for f in s._fields_]).encode())
            out[key + " | cost"] = sha(np.array([t.cost()]).tobytes())
        c = t.counters()
        sys.stderr.write("robots %d r %d poses %s | %s: one-launch iterations %d, carried %d, deep-carried %d\n"
                         % (robots, r, keep or "all", form, c[7], c[8], c[9]))
        t.close()
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
json.dump(out, open(sys.argv[1], "w"), indent=0)
sys.stderr.write("%d arrays, library %s\n" % (len(out), capi.LIB_PATH))

"""The deep-carried one-launch iteration (csrc/step_deep.hip, k_step_fd) forms its first requests from a packed head of
thirteen leading arguments (csrc/step_head.h) and derives every work vector of the agent from its first one and n.  Bit
for bit the two-launch sequence (DPGO_FUSED_EVAL=0) at the shapes where a packed field or a derived address can go wrong:

  * an agent of exactly 512 poses -- the upper limit of the n field and of the 2048-row pass;
  * agents with an odd pose count (499): their last workgroup steps ONE pose;
  * agents of different sizes in one team (512 / 499 / 498 / 499 / 486): workgroups beyond an agent's columns;
  * r = 3, 4, 5;
  * runs of 4, 5, 7 and 23 iterations: both parities, the first deep launches directly behind the producers, the closing
    launches that leave the statistics;
  * restart_interval = 3: a restart falls inside every window.

The team is sphere2500 cut to its first 2494 poses, partitioned by hand (the library's rule gives every robot but the last
the same size); every agent keeps >= 24 private chunks, so the team runs deep-carried (counters()[9])."""
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests.util import load

pytestmark = pytest.mark.gpu

SIZES = (512, 499, 498, 499, 486)
RUNS = (4, 5, 7, 23)


def _partition(m, sizes):
    lo = np.concatenate([[0], np.cumsum(sizes)])
    mp = m.copy()
    for p, r in (("p1", "r1"), ("p2", "r2")):
        owner = np.searchsorted(lo, m[p], side="right") - 1
        mp[r] = owner
        mp[p] = m[p] - lo[owner]
    return mp


@pytest.fixture(scope="module")
def graph():
    m, _, _ = load("sphere2500", 1)
    n = sum(SIZES)
    m = m[(m["p1"] < n) & (m["p2"] < n)].copy()
    return m, _partition(m, SIZES), n, O.odometry_init(m, n)


def _teams(graph, r):
    m, mp, n, T = graph
    kw = dict(method=1, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=3)
    Y = O.fixed_stiefel(r)
    teams = []
    old = {k: os.environ.get(k) for k in ("DPGO_FUSED_EVAL", "DPGO_FE_MIN_N", "DPGO_FE_DEEP")}
    try:
        os.environ["DPGO_FE_MIN_N"] = "32"
        os.environ["DPGO_FE_DEEP"] = "1"
        for fe in ("0", "1"):
            os.environ["DPGO_FUSED_EVAL"] = fe
            t = capi.Team.from_measurements(mp.view(capi.MEAS_DTYPE), capi.default_params(r=r, num_robots=len(SIZES), **kw))
            t.set_initial(T, Y)
            teams.append(t)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return teams


@pytest.mark.parametrize("r", [3, 4, 5])
def test_head_formed_launches_are_bitwise_the_two_launch_sequence(graph, r):
    two, deep = _teams(graph, r)
    assert tuple(deep.agents[k].n for k in deep.ids) == SIZES
    for iters in RUNS:
        for t in (two, deep):
            t.run(iters)
            t.synchronize()
        for k in two.ids:
            a, b = two.agents[k], deep.agents[k]
            assert np.array_equal(a.get_X(), b.get_X()), (r, iters, k, "X")
            assert np.array_equal(a.get_Y(), b.get_Y()), (r, iters, k, "Y")
            assert np.array_equal(a.get_V(), b.get_V()), (r, iters, k, "V")
        sa, sb = two.agents[two.ids[-1]].status(), deep.agents[deep.ids[-1]].status()
        assert sa.iteration_number == sb.iteration_number and sa.relative_change == sb.relative_change
    c = deep.counters()
    print("r = %d: one-launch %d, carried %d, deep-carried %d" % (r, c[7], c[8], c[9]))
    assert two.counters()[7] == 0
    # (runs of 7 and 23 iterations: 6 + 22 deep-carried launches; runs of 4 and 5 are too short for the form)
    assert c[9] > 0, "the deep-carried form did not run"
    for t in (two, deep):
        t.close()

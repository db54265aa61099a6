"""The deep-carried one-launch iteration (csrc/step_deep.hip, k_step_fd) counts its waves 4-7 in at FD_SY_RQ behind their
last request, not behind its data (tests/test_step_count_in_build.py holds that on the assembly).  What moved for it: the
Nesterov state is requested in front of the count-in and brought to scalar registers behind it (the chain waves and wave 7),
wave 7 chooses its lane's agent among values held in scalar registers, the chain waves request 12 bytes of their front-table
record and only the rotation block of their point.  No expression changed, so the iterates must stay bitwise those of the
same run with DPGO_FE_DEEP=0 (k_step_fe, the carried one-launch form of round 5):

  * the team of tests/test_gpu_step_front.py: sphere2500 cut to 2494 poses, agents of 512 / 499 / 498 / 499 / 486 poses -- the
    smallest agents of this graph that keep 24 private chunks (its rings of 50 poses make the first and the last 50 poses of
    a middle agent public: chunks 0-3 and 28-31 of 498 poses; with agents of 400 the team does not take the deep-carried form
    at all, and the test asserts that it is taken);
  * r = 3, 4, 5 -- every instance of the kernel;
  * restart intervals 3 and 7: restart_now, restart_next, restart_next2 and restart_next3 of the Nesterov state each fall
    inside deep launches (with 3 every launch has one of them set, with 7 launches with none lie between);
  * runs of 6 (the shortest deep-carried window), 23 and 64 iterations, one behind the other on the same teams: both parities,
    the opening and the closing launches, the status the last iterations leave;
  * X, Y, V of every agent, every agent's status, the team's cost: np.array_equal / ==.

Wave 7's look-ahead addresses come from scalar registers and not from a per-agent record in the front table, so there is no
record to keep current: the teams of unequal agents and of 8 agents that the table route would have needed are not here."""
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests.util import load

pytestmark = pytest.mark.gpu

SIZES = (512, 499, 498, 499, 486)
RUNS = (6, 23, 64)


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
    return _partition(m, SIZES), O.odometry_init(m, n)


def _pair(mp, T, r, restart_interval):
    """the same team twice: DPGO_FE_DEEP=0 (k_step_fe serves every run) and the deep-carried form"""
    kw = dict(method=1, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=restart_interval)
    Y = O.fixed_stiefel(r)
    teams = []
    old = {k: os.environ.get(k) for k in ("DPGO_FUSED_EVAL", "DPGO_FE_MIN_N", "DPGO_FE_DEEP")}
    try:
        os.environ["DPGO_FE_MIN_N"] = "32"
        os.environ["DPGO_FUSED_EVAL"] = "1"
        for deep in ("0", "1"):
            os.environ["DPGO_FE_DEEP"] = deep
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


def _status(t):
    out = []
    for k in t.ids:
        s = t.agents[k].status()
        out.append((s.agent_id, s.state, s.instance_number, s.iteration_number, s.ready_to_terminate, s.relative_change))
    return out


@pytest.mark.parametrize("restart_interval", [3, 7])
@pytest.mark.parametrize("r", [3, 4, 5])
def test_deep_carried_runs_are_bitwise_the_carried_one_launch_form(graph, r, restart_interval):
    mp, T = graph
    flat, deep = _pair(mp, T, r, restart_interval)
    assert tuple(deep.agents[k].n for k in deep.ids) == SIZES
    before = deep.counters()[9]
    for iters in RUNS:
        for t in (flat, deep):
            t.run(iters)
            t.synchronize()
        tag = (r, restart_interval, iters)
        for k in flat.ids:
            a, b = flat.agents[k], deep.agents[k]
            assert np.array_equal(a.get_X(), b.get_X()), (tag, k, "X")
            assert np.array_equal(a.get_Y(), b.get_Y()), (tag, k, "Y")
            assert np.array_equal(a.get_V(), b.get_V()), (tag, k, "V")
        sa, sb = _status(flat), _status(deep)
        assert sa == sb, (tag, sa, sb)
        ca, cb = flat.cost(), deep.cost()
        assert ca == cb, (tag, ca, cb)
        now = deep.counters()[9]
        print("r = %d, restart %d, run of %d: deep-carried launches %d -> %d, cost %.15g" % (r, restart_interval, iters, before, now, cb))
        assert now > before, (tag, "the deep-carried form did not run")
        before = now
    assert flat.counters()[9] == 0 and flat.counters()[7] > 0
    for t in (flat, deep):
        t.close()

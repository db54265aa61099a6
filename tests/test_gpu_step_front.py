"""The deep-carried one-launch iteration (csrc/step_deep.hip, k_step_fd) resolves its shared edges' neighbour poses and its
public poses from a static per-agent table behind the packed coefficients (csrc/step_front.h), built where the descriptor is
built (csrc/assembly.hip).  Bit for bit the two-launch sequence (DPGO_FUSED_EVAL=0), as tests/test_gpu_step_head.py
compares, at the shapes where a slot of the table can go wrong:

  * the base team of that file: sphere2500 cut to 2494 poses, agents of 512 / 499 / 498 / 499 / 486 poses with 51 / 102 / 102 /
    102 / 51 shared edges on 50 / 100 / 100 / 100 / 50 public poses, every agent with >= 24 private chunks;
  * synthetic closures between poses that are ALREADY public (the private chunks and npub stay; the relative pose is the
    initial guess's, so the problem stays well-posed) move the edge counts to the edges of wave 6's three trips of 64:
        team A  65 / 129 / 128 / 160 /  96   (+14, 13, 13, 45 closures between agents 0-1, 1-2, 2-3, 3-4)
        team B  64 / 128 / 129 / 129 /  64   (+13, 13, 14, 13)
        team C  team A with 3 closures between the non-adjacent agents 0 and 3: agents 0 and 3 read neighbours in three
                agents.  Agent 3 stands at the limit of 160 in team A, so three of its closures with agent 4 make room:
                68 / 129 / 128 / 160 / 93 -- the team must still run deep-carried, and agent 3 still fills every slot
        team D  team A with one more closure between agents 3 and 4: 161 edges, beyond the table -- the team falls back
                (counters()[9] == 0) and stays bitwise;
  * runs of 4, 5, 7 and 23 iterations at restart_interval = 3, r = 3 and 5: both parities, the closing launches;
  * the table's lifetime (team A, r = 5, GNC weights): a weight update re-sends the image behind the coefficients, a second
    set_initial goes through the descriptors again -- both still bitwise, both still deep-carried."""
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests.util import load

pytestmark = pytest.mark.gpu

SIZES = (512, 499, 498, 499, 486)
RUNS = (4, 5, 7, 23)
BASE_SHARED = (51, 102, 102, 102, 51)
BASE_PUB = (50, 100, 100, 100, 50)
TEAMS = {
    "A": ({(0, 1): 14, (1, 2): 13, (2, 3): 13, (3, 4): 45}, (65, 129, 128, 160, 96)),
    "B": ({(0, 1): 13, (1, 2): 13, (2, 3): 14, (3, 4): 13}, (64, 128, 129, 129, 64)),
    "C": ({(0, 1): 14, (1, 2): 13, (2, 3): 13, (3, 4): 42, (0, 3): 3}, (68, 129, 128, 160, 93)),
    "D": ({(0, 1): 14, (1, 2): 13, (2, 3): 13, (3, 4): 46}, (65, 129, 128, 161, 97)),
}


def _partition(m, sizes):
    lo = np.concatenate([[0], np.cumsum(sizes)])
    mp = m.copy()
    for p, r in (("p1", "r1"), ("p2", "r2")):
        owner = np.searchsorted(lo, m[p], side="right") - 1
        mp[r] = owner
        mp[p] = m[p] - lo[owner]
    return mp


def _owner(p):
    return np.searchsorted(np.concatenate([[0], np.cumsum(SIZES)]), p, side="right") - 1


def _shared_counts(m):
    o1, o2 = _owner(m["p1"]), _owner(m["p2"])
    x = o1 != o2
    shared = tuple(int(np.sum(x & ((o1 == a) | (o2 == a)))) for a in range(len(SIZES)))
    pub = tuple(len(set(m["p1"][x & (o1 == a)]) | set(m["p2"][x & (o2 == a)])) for a in range(len(SIZES)))
    return shared, pub


def _closures(m, T, add):
    """`add[(a, b)]` closures between global poses of agents a < b that already carry a shared edge, none a repeat of an
    existing pair; the relative pose is the one of the initial guess T (12 doubles per pose: R column-major, t)"""
    o1, o2 = _owner(m["p1"]), _owner(m["p2"])
    x = o1 != o2
    have = set(zip(m["p1"][x].tolist(), m["p2"][x].tolist()))
    pubs = [sorted(set(m["p1"][x & (o1 == a)].tolist()) | set(m["p2"][x & (o2 == a)].tolist())) for a in range(len(SIZES))]
    out = []
    for (a, b), count in sorted(add.items()):
        # (the poses of a that face a higher agent, the poses of b that face a lower one: the ends of the two trajectories)
        pa = [p for p in pubs[a] if p >= np.cumsum(SIZES)[a] - 60] or pubs[a]
        pb = [p for p in pubs[b] if p < np.cumsum(SIZES)[b - 1] + 60] or pubs[b]
        k = made = 0
        while made < count:
            i, j = pa[(5 * k + a) % len(pa)], pb[(7 * k + 3) % len(pb)]
            k += 1
            assert k < 10000
            if (i, j) in have:
                continue
            have.add((i, j))
            e = m[0:1].copy()
            Ri, Rj = T[12 * i:12 * i + 9].reshape(3, 3).T, T[12 * j:12 * j + 9].reshape(3, 3).T
            e["p1"], e["p2"] = i, j
            e["R"] = (Ri.T @ Rj).reshape(9)
            e["t"] = Ri.T @ (T[12 * j + 9:12 * j + 12] - T[12 * i + 9:12 * i + 12])
            out.append(e)
            made += 1
    return np.concatenate(out)


@pytest.fixture(scope="module")
def graph():
    m, _, _ = load("sphere2500", 1)
    n = sum(SIZES)
    m = m[(m["p1"] < n) & (m["p2"] < n)].copy()
    assert _shared_counts(m) == (BASE_SHARED, BASE_PUB)
    return m, n, O.odometry_init(m, n)


def _team_graph(graph, name):
    m, n, T = graph
    add, want = TEAMS[name]
    mm = np.concatenate([m, _closures(m, T, add)])
    shared, pub = _shared_counts(mm)
    assert shared == want and pub == BASE_PUB, (name, shared, pub)
    return _partition(mm, SIZES)


def _pair(mp, T, r, **extra):
    kw = dict(method=1, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=3)
    kw.update(extra)
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


def _run_and_compare(two, deep, iters, tag):
    for t in (two, deep):
        t.run(iters)
        t.synchronize()
    for k in two.ids:
        a, b = two.agents[k], deep.agents[k]
        assert np.array_equal(a.get_X(), b.get_X()), (tag, iters, k, "X")
        assert np.array_equal(a.get_Y(), b.get_Y()), (tag, iters, k, "Y")
        assert np.array_equal(a.get_V(), b.get_V()), (tag, iters, k, "V")
    sa, sb = two.agents[two.ids[-1]].status(), deep.agents[deep.ids[-1]].status()
    assert sa.iteration_number == sb.iteration_number and sa.relative_change == sb.relative_change, (tag, iters)


@pytest.mark.parametrize("r", [3, 5])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_table_resolved_launches_are_bitwise_the_two_launch_sequence(graph, name, r):
    two, deep = _pair(_team_graph(graph, name), graph[2], r)
    assert tuple(deep.agents[k].n for k in deep.ids) == SIZES
    for iters in RUNS:
        _run_and_compare(two, deep, iters, (name, r))
    c = deep.counters()
    print("team %s, r = %d: one-launch %d, carried %d, deep-carried %d" % (name, r, c[7], c[8], c[9]))
    assert two.counters()[7] == 0
    if name == "D":
        assert c[9] == 0, "an agent of 161 shared edges must not run deep-carried"
    else:
        assert c[9] > 0, "the deep-carried form did not run"
    for t in (two, deep):
        t.close()


def test_table_follows_a_weight_update_and_a_second_set_initial(graph):
    r = 5
    two, deep = _pair(_team_graph(graph, "A"), graph[2], r, robust_cost_type=5, gnc_barc=5.0)
    _run_and_compare(two, deep, 7, "first")
    c0 = deep.counters()[9]
    assert c0 > 0, "the deep-carried form did not run"
    assert two.update_weights() == deep.update_weights()
    _run_and_compare(two, deep, 7, "behind the weight update")
    c1 = deep.counters()[9]
    assert c1 > c0, "the deep-carried form did not run behind the weight update"
    Y = O.fixed_stiefel(r)
    for t in (two, deep):
        t.set_initial(graph[2], Y)
    _run_and_compare(two, deep, 7, "behind the second set_initial")
    assert deep.counters()[9] > c1, "the deep-carried form did not run behind the second set_initial"
    assert two.counters()[7] == 0
    for t in (two, deep):
        t.close()

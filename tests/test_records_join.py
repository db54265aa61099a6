"""capi.join_records_by_robot, the pure function behind Team.audit(measurements=None, transport=...) and
Team.zero_weight_measurements(transport=...): per-rank record lists joined into the single team's measurements_once().  Hand-made
lists, no device."""
import numpy as np

from dpgo_ros_amd import capi

HOLDS = [[2], [0, 3], [1]]  # rank -> robots
OWNER = np.array([1, 2, 0, 1], dtype=np.int32)  # robot -> rank


def rec(r1, p1, r2, p2, w, tag):
    e = np.zeros(1, dtype=capi.MEAS_DTYPE)[0]
    e["r1"], e["p1"], e["r2"], e["p2"] = r1, p1, r2, p2
    e["R"], e["t"] = np.eye(3).reshape(-1), (tag, 0.0, 0.0)
    e["kappa"], e["tau"], e["weight"] = 10.0 + tag, 20.0 + tag, w
    return e


def robot_lists():
    """per robot, its own measurements in its own order: odometry, and a shared edge with every other robot (in both directions
    of storage: the edge a -> b is listed by a and by b); the weight is the OWNER's (the lower robot's) -- the higher robot's
    copy carries a stale one"""
    shared = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    tag = [0]
    lists = {i: [] for i in range(4)}
    for i in range(4):
        for p in range(2):
            tag[0] += 1
            lists[i].append(rec(i, p, i, p + 1, 1.0, tag[0]))
    for k, (a, b) in enumerate(shared):
        tag[0] += 1
        # alternate the direction the edge was measured in: (r1, r2) = (a, b) or (b, a); the owner is min(a, b) either way
        r1, r2 = (a, b) if k % 2 == 0 else (b, a)
        w = 0.25 * (k % 5)
        lists[a].append(rec(r1, k, r2, k + 1, w, tag[0]))
        lists[b].insert(1, rec(r1, k, r2, k + 1, 0.875, tag[0]))  # the stale copy, in the middle of b's odometry
    return lists


def owner_of(e):
    return int(e["r1"]) if e["r1"] == e["r2"] else min(int(e["r1"]), int(e["r2"]))


def as_array(recs):
    return np.array(recs, dtype=capi.MEAS_DTYPE) if recs else np.zeros(0, dtype=capi.MEAS_DTYPE)


def check(lists_per_rank, lists):
    out = capi.join_records_by_robot(lists_per_rank, OWNER)
    # the single team's measurements_once(): robot after robot, each robot's own records it owns, in its order
    want = as_array([e for i in range(4) for e in lists[i] if owner_of(e) == i])
    assert out.dtype == capi.MEAS_DTYPE and out.tobytes() == want.tobytes()
    # the order of ONE list sorted by owner robot, ties in input order
    keys = [owner_of(e) for e in out]
    assert keys == sorted(keys)
    # each shared edge exactly once, with the owner's weight
    edges = [(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"])) for e in out if e["r1"] != e["r2"]]
    assert len(edges) == 6 and len(set(edges)) == 6
    assert all(e["weight"] != 0.875 for e in out)
    assert sorted(float(e["weight"]) for e in out if e["r1"] != e["r2"]) == sorted(0.25 * (k % 5) for k in range(6))
    return out


def test_lists_with_the_lower_robots_copy_alone():
    lists = robot_lists()
    # what Team.measurements_once() of each participant gives: its robots in id order, the copies it owns
    per_rank = [as_array([e for i in sorted(ids) for e in lists[i] if owner_of(e) == i]) for ids in HOLDS]
    check(per_rank, lists)


def test_lists_with_both_copies_present():
    lists = robot_lists()
    # everything a participant's robots store, robots in id order: the higher robot's stale copies among them, and the edge
    # 0 - 3 twice on rank 1, which holds both of its robots
    per_rank = [as_array([e for i in sorted(ids) for e in lists[i]]) for ids in HOLDS]
    assert sum(1 for e in per_rank[1] if {int(e["r1"]), int(e["r2"])} == {0, 3}) == 2
    check(per_rank, lists)


def test_an_empty_rank_and_an_empty_problem():
    lists = robot_lists()
    per_rank = [as_array([e for i in sorted(ids) for e in lists[i] if owner_of(e) == i]) for ids in HOLDS]
    per_rank[0] = as_array([])  # robot 2's rank lists nothing: its records are missing, the others are in place
    out = capi.join_records_by_robot(per_rank, OWNER)
    assert [owner_of(e) for e in out] == sorted(owner_of(e) for e in out) and all(owner_of(e) != 2 for e in out)
    assert len(capi.join_records_by_robot([as_array([])] * 3, OWNER)) == 0


def test_records_survive_the_trip_as_doubles():
    lists = robot_lists()
    recs = as_array([e for i in range(4) for e in lists[i]])
    recs["fixed_weight"][::2], recs["is_known_inlier"][1::3] = 1, 1
    x = capi.records_to_doubles(recs)
    assert x.shape == (len(recs), 21)
    assert capi.records_from_doubles(x.reshape(-1)).tobytes() == recs.tobytes()

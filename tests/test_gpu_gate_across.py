"""GPU checks of the Mahalanobis gate over a split team (dpgo_team_gate_candidates_across, csrc/gate.hip behind
csrc/covariance_schur.hip; Team.gate / Team.relative_covariances with transport=, DESIGN.md 5f "across teams"): LocalGroup
threads on one device.  The contract is bitwise, so there is no tolerance: whatever the split, every xi, d2 and sigma_rel
equals the single team's method="schur" call on the same T and candidates, and is identical on every participant.  The
single-team call is held to gateref and the numpy inverse by tests/test_gpu_gate.py; that accuracy carries over."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import covschur_ref
from tests import gateref as G
from tests.test_gpu_certify_across import JOIN, Split, _expect_refusal, bits, problem, robot_sizes, single_team
from tests.test_gpu_covariance_across import point, scalars
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_covariance_schur import pair_cases

pytestmark = pytest.mark.gpu

SPLITS = [("smallGrid3D", 3, [[0, 1], [2]]), ("smallGrid3D", 3, [[0], [1], [2]]), ("sphere2500", 5, [[0, 2, 4], [1, 3]])]


def make_candidates(T, goff, pairs, seed):
    """one candidate per pair of global poses (i, j), i != j: the relative pose at T composed with a seeded perturbation --
    a rotation by up to 0.3 rad about a random axis, a translation of length up to 0.5 -- and kappa, tau log-uniform in
    [1, 1e3]"""
    rng = np.random.default_rng(seed)
    goff = np.asarray(goff)
    c = np.zeros(len(pairs), dtype=capi.MEAS_DTYPE)
    for k, (i, j) in enumerate(pairs):
        Rij, tij = G.relative_pose(T, int(i), int(j), np.float64)
        a = rng.standard_normal(3)
        a *= rng.uniform(0.0, 0.3) / np.linalg.norm(a)
        d = rng.standard_normal(3)
        d *= rng.uniform(0.0, 0.5) / np.linalg.norm(d)
        ri, rj = int(np.searchsorted(goff, i, side="right")) - 1, int(np.searchsorted(goff, j, side="right")) - 1
        c[k]["r1"], c[k]["p1"], c[k]["r2"], c[k]["p2"] = ri, i - goff[ri], rj, j - goff[rj]
        c[k]["R"], c[k]["t"] = (Rij @ covref.exp_so3(a)).reshape(-1), tij + d
        c[k]["kappa"], c[k]["tau"] = 10.0 ** rng.uniform(0.0, 3.0, 2)
        c[k]["weight"] = 1.0
    return c


def global_poses(cand, goff):
    goff = np.asarray(goff)
    return np.stack([goff[cand["r1"]] + cand["p1"], goff[cand["r2"]] + cand["p2"]], axis=1)


def case_candidates(m, mp, n, N, T):
    """the candidates of the split tests, from the pairs of pair_cases(m, n, N, 120, seed=11): one per pair that joins two
    different poses (a candidate that joins a pose to itself is refused), four more on the two pairs that name pose 0 (both
    ways round), and six exact copies of earlier candidates"""
    goff = np.concatenate([[0], np.cumsum(robot_sizes(mp, N))])
    pairs = pair_cases(m, n, N, 120, seed=11)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    zero = pairs[(pairs == 0).any(axis=1)]
    assert len(zero) == 2
    cand = np.concatenate([make_candidates(T, goff, pairs, 21), make_candidates(T, goff, zero[:, ::-1], 22),
                           make_candidates(T, goff, zero, 23)])
    return np.concatenate([cand, cand[[5, 17, 29, 41, 53, 65]]]), goff


def kinds(cand, goff, mp, n, N, parts):
    """how many candidates of each kind the list holds"""
    robot_of, public = covschur_ref.partition(mp, n, N)
    holder = {i: q for q, ids in enumerate(parts) for i in ids}
    g = global_poses(cand, goff)
    cnt = dict(far=0, interior_public=0, public_public=0, pose0=0, duplicate=0)
    seen = set()
    for k, (a, b) in enumerate(g):
        key = cand[k].tobytes()
        cnt["duplicate"] += key in seen
        seen.add(key)
        if a == 0 or b == 0:
            cnt["pose0"] += 1
        elif public[a] and public[b]:
            cnt["public_public"] += 1
        elif public[a] != public[b]:
            cnt["interior_public"] += 1
        elif holder[robot_of[a]] != holder[robot_of[b]]:
            cnt["far"] += 1
    return cnt


_REF = {}


def reference(ds, N):
    """(m, mp, n, X, T, cand, goff, the single team's gate(..., method="schur", sigma_rel=True)), computed once per dataset"""
    if (ds, N) not in _REF:
        m, mp, n = problem(ds, N)
        X, T = point(ds, N, n)
        cand, goff = case_candidates(m, mp, n, N, T)
        t = single_team(mp, N, X)
        ref = t.gate(cand, T, method="schur", sigma_rel=True)
        t.close()
        _REF[(ds, N)] = (m, mp, n, X, T, cand, goff, ref)
    return _REF[(ds, N)]


def same_gate(out, ref):
    (r, xi, d2, acc, sg), (r0, xi0, d20, acc0, sg0) = out, ref
    return scalars(r) == scalars(r0) and bits(xi) == bits(xi0) and bits(d2) == bits(d20) and bits(acc) == bits(acc0) and \
        bits(sg) == bits(sg0)


def test_one_participant_equals_the_single_team_bitwise():
    ds, N = "smallGrid3D", 3
    m, mp, n, X, T, cand, goff, ref = reference(ds, N)
    t = single_team(mp, N, X)
    g = capi.LocalGroup(1)
    own = np.zeros(N, dtype=np.int32)
    assert same_gate(t.gate(cand, T, sigma_rel=True, transport=g[0], owner_of_robot=own), ref)
    assert same_gate(t.gate(cand, T, method="schur", sigma_rel=True, transport=g[0], owner_of_robot=own), ref)
    # without sigma_rel: the same xi, d2, accept
    r, xi, d2, acc = t.gate(cand, T, transport=g[0], owner_of_robot=own)
    assert scalars(r) == scalars(ref[0]) and bits(xi) == bits(ref[1]) and bits(d2) == bits(ref[2]) and bits(acc) == bits(ref[3])
    # the relative covariances alone: global pose ids are team-order ids when one participant holds every robot
    pr = global_poses(cand, goff)
    s0 = t.relative_covariances(pr, T, method="schur")
    s1 = t.relative_covariances(pr, T, transport=g[0], owner_of_robot=own)
    assert bits(s0) == bits(ref[4]) and bits(s1) == bits(s0)
    # T = None rounds across first: the single team's own rounding
    assert same_gate(t.gate(cand, sigma_rel=True, transport=g[0], owner_of_robot=own), t.gate(cand, method="schur", sigma_rel=True))
    t.close()


@pytest.mark.parametrize("ds,N,parts", SPLITS)
def test_split_equals_the_single_team_bitwise(ds, N, parts):
    m, mp, n, X, T, cand, goff, ref = reference(ds, N)
    cnt = kinds(cand, goff, mp, n, N, parts)
    print("%s %s: %d candidates, %s" % (ds, parts, len(cand), cnt))
    assert min(cnt.values()) >= 5, cnt  # (before anything is called)
    sp = Split(mp, N, parts, X)
    g = capi.LocalGroup(len(parts))
    out = sp.run(lambda tm, tr: tm.gate(cand, T[sp.cols(tr.rank, 12)], sigma_rel=True, transport=tr, owner_of_robot=sp.owner), g)
    for q, o in enumerate(out):
        assert same_gate(o, ref), q
    # exactly one allgather more than the covariances across with the same pairs, and as many exchanges
    calls = [dict(tr.calls) for tr in g]
    pr = []
    for p in map(tuple, global_poses(cand, goff)):
        if p not in pr:
            pr.append(p)
    g2 = capi.LocalGroup(len(parts))
    sp.run(lambda tm, tr: tm.covariances(T[sp.cols(tr.rank, 12)], np.array(pr), transport=tr, owner_of_robot=sp.owner), g2)
    for q in range(len(parts)):
        assert calls[q]["allgather"] == g2[q].calls["allgather"] + 1 and calls[q]["exchange"] == g2[q].calls["exchange"], (q, calls[q], g2[q].calls)
    # the relative covariances alone, by global pose ids
    sg = sp.run(lambda tm, tr: tm.relative_covariances(global_poses(cand, goff), T[sp.cols(tr.rank, 12)], transport=tr,
                                                       owner_of_robot=sp.owner))
    for q, s in enumerate(sg):
        assert bits(s) == bits(ref[4]), q
    sp.close()


def test_the_smallest_shapes():
    """a banded chain of 40 poses as 3 robots, one participant per robot: one interior-interior candidate across participants
    (K = 1), K = 257 (one lane into a second workgroup), and one candidate between the first poses of two robots"""
    n, N, parts = 40, 3, [[0], [1], [2]]
    m, T = NR.banded_chain(n, 5, window=8)
    mp = capi.partition(m, n, N)
    t = team_of(m, n, N, T)
    X = t.global_X()
    goff = np.concatenate([[0], np.cumsum([t.agents[i].n for i in range(N)])])
    robot_of, public = covschur_ref.partition(mp, n, N)
    interior = [[g for g in range(1, n) if robot_of[g] == a and not public[g]] for a in range(N)]
    assert len(interior[0]) >= 2 and len(interior[2]) >= 1
    rng = np.random.default_rng(8)
    one = [(interior[0][1], interior[2][0])]
    many = []  # poses of two different robots, whatever their kind
    for k in range(257):
        a, b = [(0, 1), (0, 2), (1, 2), (2, 0)][k % 4]
        many.append((int(rng.integers(goff[a], goff[a + 1])), int(rng.integers(goff[b], goff[b + 1]))))
    first = [(int(goff[1]), int(goff[2])), (int(goff[2]), int(goff[0]))]  # (the second names pose 0)
    sp = Split(mp, N, parts, X)
    for tag, pairs in (("K = 1", one), ("K = 257", many), ("first poses", first[:1]), ("first poses and pose 0", first)):
        cand = make_candidates(T, goff, pairs, 31)
        ref = t.gate(cand, T, method="schur", sigma_rel=True)
        assert np.isfinite(ref[2]).all()
        out = sp.run(lambda tm, tr: tm.gate(cand, T[sp.cols(tr.rank, 12)], sigma_rel=True, transport=tr, owner_of_robot=sp.owner))
        for q, o in enumerate(out):
            assert same_gate(o, ref), (tag, q)
    sp.close()
    t.close()


def raw_gate_across(tm, tr, own, T, cand, outs, res, num=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dpgo_team_gate_candidates_across(tm.h, C.byref(tr.struct), p(own), p(T), len(cand) if num is None else num, p(cand),
                                                     *[p(a) for a in outs], C.byref(res))
    return rc, capi.lib().dpgo_last_error().decode()


def refused_everywhere(sp, own, args, match, raw, nouts):
    """raw(tm, tr, own, T, records, outs, res) on every participant with args(q) = (T, records): DPGO_ERR and `match` in the
    message everywhere, every output untouched, *res all zero; the messages in rank order"""
    g = capi.LocalGroup(len(sp.teams), timeout=60.0)

    def call(q):
        Tq, rec = args(q)
        K = len(rec)
        outs = [np.full(s, 7.25) for s in nouts(K)]
        res = capi.Covariance()
        rc, msg = raw(sp.teams[q], g[q], own, np.ascontiguousarray(Tq), np.ascontiguousarray(rec), outs, res)
        return rc, msg, all((o == 7.25).all() for o in outs), bytes(res) == bytes(capi.Covariance())

    msgs = []
    for q, (r, e) in enumerate(g.run([lambda q=q: call(q) for q in range(len(sp.teams))], timeout=JOIN)):
        assert e is None, (q, e)
        rc, msg, untouched, zero = r
        assert rc == capi.ERR and match in msg, (q, rc, msg)
        assert untouched and zero, (q, msg)
        msgs.append(msg)
    return msgs


def gate_outs(K):
    return [(K, 6), (K,), (K, 6, 6)]


def test_refusals_reach_every_participant():
    ds, N, parts = "smallGrid3D", 3, [[0, 1], [2]]
    m, mp, n, X, T, cand, goff, ref = reference(ds, N)
    sp = Split(mp, N, parts, X)
    own = capi._owner_array(sp.owner)
    Tq = [T[sp.cols(q, 12)] for q in range(2)]
    sizes = np.diff(goff)

    def good():  # the transport is not left half-way: a good call goes through and gives the single team's bits
        out = sp.run(lambda tm, tr: tm.gate(cand, Tq[tr.rank], sigma_rel=True, transport=tr, owner_of_robot=sp.owner))
        assert all(same_gate(o, ref) for o in out)

    def refused(args, match):
        msgs = refused_everywhere(sp, own, args, match, raw_gate_across, gate_outs)
        good()
        return msgs

    # a list shorter by one on rank 1; one record's tau changed on rank 1
    refused(lambda q: (Tq[q], cand[:len(cand) - q]), "the number of records")
    other = cand.copy()
    other[7]["tau"] *= 1.0 + 2.0 ** -40
    refused(lambda q: (Tq[q], other if q else cand), "the record list")
    # an endpoint (robot, pose) outside the problem: behind the agreement, the same words everywhere
    for field, value, words in (("p2", int(sizes[2]), "names pose %d of robot 2, outside [0, %d)" % (sizes[2], sizes[2])),
                                ("r1", N, "names robot %d, outside" % N), ("p1", -1, "names pose -1")):
        out_ = cand.copy()
        out_[3]["r2"] = 2
        out_[3][field] = value
        msgs = refused(lambda q: (Tq[q], out_), words)
        assert msgs[0] == msgs[1] and "candidate 3" in msgs[0]
    # i = j, and kappa = 0, on all ranks: the single team's words
    same = cand.copy()
    same[4]["r2"], same[4]["p2"] = same[4]["r1"], same[4]["p1"]
    refused(lambda q: (Tq[q], same), "candidate 4 joins a pose to itself")
    zero = cand.copy()
    zero[9]["kappa"] = 0.0
    refused(lambda q: (Tq[q], zero), "candidate 9 has kappa = 0")
    # kappa = 0 on rank 1 only: rank 1 says why, rank 0 learns that rank 1's arguments are invalid
    msgs = refused(lambda q: (Tq[q], zero if q else cand), "")
    assert "rank 1: invalid arguments" in msgs[0] and "candidate 9 has kappa = 0" in msgs[1], msgs
    # a T off SE(3) on rank 1 only
    Tb = Tq[1].copy()
    Tb[12 * 4] *= 1.001
    msgs = refused(lambda q: (Tb if q else Tq[0], cand), "rank 1")
    assert "SE(3)" in msgs[1], msgs
    # through the Python interface: the refusal is a DpgoError on every participant
    _expect_refusal(sp, lambda q, tm, tr: tm.gate(cand[:len(cand) - q], Tq[q], transport=tr, owner_of_robot=sp.owner), "the number of records")
    good()
    # method="nested" (or "dense", or a max_block) with a transport: a ValueError before any transport call
    g = capi.LocalGroup(2)
    for kw in (dict(method="nested"), dict(method="dense"), dict(max_block=16)):
        with pytest.raises(ValueError, match="transport"):
            sp.teams[0].gate(cand, Tq[0], transport=g[0], owner_of_robot=sp.owner, **kw)
        with pytest.raises(ValueError, match="transport"):
            sp.teams[0].relative_covariances(global_poses(cand, goff), Tq[0], transport=g[0], owner_of_robot=sp.owner, **kw)
    assert g[0].calls == dict(allgather=0, exchange=0)
    sp.close()

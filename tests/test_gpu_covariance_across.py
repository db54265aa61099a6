"""GPU checks of the marginal covariances over a split team (dpgo_team_marginal_covariances_across, csrc/covariance_schur.hip,
DESIGN.md 5e): LocalGroup threads on one device, and one two-process gloo case.  The contract is bitwise: whatever the split,
every diagonal block, pair block, log det and pivot equals the single team's Schur call, and the scalars are identical on
every participant."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covschur_ref
from tests.test_certificate import random_manifold_point
from tests.test_gpu_certificate import RTR_NESTEROV
from tests.test_gpu_certify_across import JOIN, R, Split, _expect_refusal, bits, optimum, problem, single_team
from tests.test_gpu_covariance_schur import pair_cases
from tests.util import ROOT

pytestmark = pytest.mark.gpu


def scalars(res):
    return (res.n, res.logdet, res.min_pivot, res.max_pivot)


def point(ds, N, n):
    """(X, T): the iterate the teams are set to and the trajectory the covariances are taken at.  sphere2500: the solver's
    optimum and its rounding; smallGrid3D: 300 iterations from the chordal point"""
    m, mp, _ = problem(ds, N)
    if ds == "sphere2500":
        X = optimum(ds, N)
    else:
        t = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=N, **RTR_NESTEROV))
        t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(R))
        t.run(300)
        X = t.global_X()
        t.close()
    t = single_team(mp, N, X)
    _, T = t.round()
    t.close()
    return X, T


def all_cases(m, n, N, ds):
    return pair_cases(m, n, N, 200 if ds == "sphere2500" else 120, seed=11)


@pytest.mark.parametrize("ds,N", [("smallGrid3D", 3), ("sphere2500", 5)])
def test_one_participant_equals_the_single_team_bitwise(ds, N):
    m, mp, n = problem(ds, N)
    X, T = point(ds, N, n)
    pairs = all_cases(m, n, N, ds)
    t = single_team(mp, N, X)
    g = capi.LocalGroup(1)
    own = np.zeros(N, dtype=np.int32)
    r0, d0, c0 = t.covariances(T, pairs, method="schur")
    r1, d1, c1 = t.covariances(T, pairs, transport=g[0], owner_of_robot=own)
    assert scalars(r0) == scalars(r1), (r0, r1)
    assert bits(d0) == bits(d1) and bits(c0) == bits(c1)
    # T = None rounds across first
    r2, d2, _ = t.covariances(transport=g[0], owner_of_robot=own)
    assert bits(d2) == bits(d0) and scalars(r2) == scalars(r0)
    t.close()


SPLITS = [("smallGrid3D", 3, [[0, 1], [2]]), ("smallGrid3D", 3, [[0], [1], [2]]), ("sphere2500", 5, [[0, 2, 4], [1, 3]]),
          ("sphere2500", 5, [[0], [1], [2], [3], [4]])]


@pytest.mark.parametrize("ds,N,parts", SPLITS)
def test_split_equals_the_single_team_bitwise(ds, N, parts):
    """every block, every pair of every case (interior poses on different participants among them), log det and pivots"""
    m, mp, n = problem(ds, N)
    X, T = point(ds, N, n)
    pairs = all_cases(m, n, N, ds)
    robot_of, public = covschur_ref.partition(mp, n, N)
    holder = {i: q for q, ids in enumerate(parts) for i in ids}
    far = [k for k, (a, b) in enumerate(pairs) if a and b and not public[a] and not public[b]
           and holder[robot_of[a]] != holder[robot_of[b]]]
    assert len(far) >= 5  # pairs of interior poses held by different participants
    t = single_team(mp, N, X)
    r0, d0, c0 = t.covariances(T, pairs, method="schur")
    t.close()
    sp = Split(mp, N, parts, X)
    out = sp.run(lambda tm, tr: tm.covariances(T[sp.cols(sp.teams.index(tm), 12)], pairs, transport=tr, owner_of_robot=sp.owner))
    for q, (r, d, c) in enumerate(out):
        assert scalars(r) == scalars(r0), (q, r, r0)
        assert bits(c) == bits(c0), q
        assert bits(d) == bits(d0.reshape(-1)[sp.cols(q, 36)]), q
    sp.close()


def test_refusals_reach_every_participant():
    ds, N = "smallGrid3D", 3
    m, mp, n = problem(ds, N)
    X, T = point(ds, N, n)
    pairs = all_cases(m, n, N, ds)
    sp = Split(mp, N, [[0, 1], [2]], X)  # (robot 1 has no interior pose: the second participant holds robot 2)
    own = sp.owner
    Tq = [T[sp.cols(q, 12)] for q in range(2)]
    # a pair list that differs on one participant, in length and in content
    _expect_refusal(sp, lambda q, tm, tr: tm.covariances(Tq[q], pairs[:len(pairs) - q], transport=tr, owner_of_robot=own), "num_pairs")
    other = pairs.copy()
    other[5] = other[5][::-1] + 1
    _expect_refusal(sp, lambda q, tm, tr: tm.covariances(Tq[q], other if q else pairs, transport=tr, owner_of_robot=own), "the pair list")
    # a trajectory off SE(3) on one participant only
    Tb = Tq[1].copy()
    Tb[12 * 4] *= 1.001
    _expect_refusal(sp, lambda q, tm, tr: tm.covariances(Tb if q else Tq[0], pairs, transport=tr, owner_of_robot=own), "rank 1")
    # a pair out of range: the same refusal everywhere
    _expect_refusal(sp, lambda q, tm, tr: tm.covariances(Tq[q], np.array([[1, n]]), transport=tr, owner_of_robot=own), "outside")
    # not a minimum on one participant only: the other's poses stay at T, participant 1's interiors are taken from a random
    # trajectory -- a non-positive pivot there, told by both with robot and pose
    Tr = random_manifold_point(np.random.default_rng(100), 3, n)
    P = Tr.reshape(n, 4, 3).copy()
    Rm = P[:, :3, :].transpose(0, 2, 1)
    P[np.linalg.det(Rm) < 0, 2, :] *= -1.0
    Tbad = P.reshape(-1)[sp.cols(1, 12)]
    g = capi.LocalGroup(2, timeout=60.0)
    res = g.run([lambda q=q: sp.teams[q].covariances(Tbad if q else Tq[0], pairs, transport=g[q], owner_of_robot=own) for q in range(2)],
                timeout=JOIN)
    msgs = [str(e) for _, e in res]
    assert all(isinstance(e, capi.DpgoError) for _, e in res), msgs
    assert msgs[0] == msgs[1] and "not a minimum" in msgs[0] and "pivot" in msgs[0], msgs
    assert "rank 1" in msgs[0] and "robot 2" in msgs[0] and "pose" in msgs[0], msgs
    # an uninitialised robot on one participant
    sp.teams[1].close()
    sp.teams[1] = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=N), local_ids=[2])
    _expect_refusal(sp, lambda q, tm, tr: tm.covariances(Tq[q], pairs, transport=tr, owner_of_robot=own), "not initialized")
    sp.close()


def test_refused_calls_leave_the_outputs_untouched():
    import ctypes as C
    ds, N = "smallGrid3D", 3
    m, mp, n = problem(ds, N)
    X, T = point(ds, N, n)
    sp = Split(mp, N, [[0, 2], [1]], X)
    own = capi._owner_array(sp.owner)
    g = capi.LocalGroup(2, timeout=60.0)

    def call(q):
        tm = sp.teams[q]
        Tl = np.ascontiguousarray(T[sp.cols(q, 12)])
        if q == 1:
            Tl[12 * 2] *= 1.001
        nl = len(Tl) // 12
        pr = np.array([[1, 2], [5, 100]], dtype=np.int32)
        diag, cross, res = np.full((nl, 6, 6), 7.25), np.full((2, 6, 6), 7.25), capi.Covariance()
        rc = capi.lib().dpgo_team_marginal_covariances_across(tm.h, C.byref(g[q].struct), capi._d(own), capi._d(Tl), capi.COV_SCHUR, 2,
                                                              capi._d(pr), capi._d(diag), capi._d(cross), C.byref(res))
        return rc, (diag == 7.25).all() and (cross == 7.25).all(), bytes(res) == bytes(capi.Covariance())

    for (rc, untouched, zero), e in g.run([lambda q=q: call(q) for q in range(2)], timeout=JOIN):
        assert e is None and rc == capi.ERR and untouched and zero
    sp.close()


def test_the_call_has_no_side_effects_on_the_solver():
    ds, N = "smallGrid3D", 3
    m, mp, n = problem(ds, N)
    X, T = point(ds, N, n)
    pairs = all_cases(m, n, N, ds)
    outs = []
    for with_call in (False, True):
        t = single_team(mp, N, X, **RTR_NESTEROV)
        t.run(20)
        if with_call:
            g = capi.LocalGroup(1)
            t.covariances(T, pairs, transport=g[0], owner_of_robot=np.zeros(N, dtype=np.int32))
        t.run(40)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert bits(a) == bits(b)


def _gloo_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd.distributed import TorchTransport, certify_and_round
    dist.init_process_group("gloo", rank=rank, world_size=world)
    X, T, pairs = (np.load(os.path.join(outdir, f + ".npy")) for f in ("X", "T", "pairs"))
    m, mp, n = problem("smallGrid3D", 4)
    sp = Split(mp, 4, [[0, 2], [1, 3]], X)
    tm = sp.teams[rank]
    res, diag, cross = tm.covariances(T[sp.cols(rank, 12)], pairs, transport=TorchTransport(dist), owner_of_robot=sp.owner)
    np.save(os.path.join(outdir, "out%d.npy" % rank), np.concatenate([[res.n, res.logdet, res.min_pivot, res.max_pivot],
                                                                      diag.ravel(), cross.ravel()]))
    out = certify_and_round(tm, dist, sp.owner, covariances=True, pairs=pairs)
    cres, dg, cr = out["covariances"]
    np.save(os.path.join(outdir, "helper%d.npy" % rank), np.concatenate([[cres.logdet], out["T"], dg.ravel(), cr.ravel()]))
    sp.close()
    dist.destroy_process_group()


def test_two_processes_over_gloo_equal_two_threads_and_the_helper_returns_the_global_diagonal():
    import torch.multiprocessing as mp_
    ds, N = "smallGrid3D", 4
    m, mp, n = problem(ds, N)
    X, T = point(ds, N, n)
    pairs = pair_cases(m, n, N, 60, seed=2)
    parts = [[0, 2], [1, 3]]
    sp = Split(mp, N, parts, X)
    res = sp.run(lambda tm, tr: tm.covariances(T[sp.cols(sp.teams.index(tm), 12)], pairs, transport=tr, owner_of_robot=sp.owner))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        for f, v in (("X", X), ("T", T), ("pairs", pairs)):
            np.save(os.path.join(d, f + ".npy"), v)
        mp_.spawn(_gloo_worker, args=(2, port, d), nprocs=2, join=True)
        for q in range(2):
            r, dg, cr = res[q]
            want = np.concatenate([[r.n, r.logdet, r.min_pivot, r.max_pivot], dg.ravel(), cr.ravel()])
            assert bits(np.load(os.path.join(d, "out%d.npy" % q))) == bits(want), q
        # the helper: certify, round, then the covariances at ITS rounded T -- the single team's at the same T, in global order
        h = [np.load(os.path.join(d, "helper%d.npy" % q)) for q in range(2)]
        assert bits(h[0]) == bits(h[1])
        Tg = h[0][1:1 + 12 * n]
        t = single_team(mp, N, X)
        r0, d0, c0 = t.covariances(Tg, pairs, method="schur")
        t.close()
        assert h[0][0] == r0.logdet
        assert bits(h[0][1 + 12 * n:1 + 12 * n + 36 * n]) == bits(d0) and bits(h[0][1 + 48 * n:]) == bits(c0)
    sp.close()

"""GPU checks of the certificate and the rounding across teams (csrc/certify_across.hip): one participant reproduces the
single-team calls bit for bit; a split operator equals the single team's on the same columns bit for bit; split
certificates and roundings agree with the single team's; determinism across runs, participants and a two-process gloo
run; no side effects; refusals that reach every participant without a hang."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests.test_certificate import as_matrix, certificate_matrix, q_full, random_manifold_point
from tests.test_gpu_certificate import ETA, RTR_NESTEROV, converge
from tests.util import DATA, ROOT

pytestmark = pytest.mark.gpu

R = 5
JOIN = 600.0  # seconds a participant may take before the test fails (a protocol hang must not stall the run)


def problem(ds, N):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    return m, (capi.partition(m, n, N) if N > 1 else m), n


def single_team(mp, N, X, r=R, **kw):
    t = capi.Team.from_measurements(mp, capi.default_params(r=r, num_robots=N, **kw))
    set_X(t, X, r)
    return t


def robot_sizes(mp, N):
    t = capi.Team.from_measurements(mp, capi.default_params(r=3, num_robots=N))
    sizes = [t.agents[i].n for i in range(N)]
    t.close()
    return sizes


def set_X(t, X, r, goff=None):
    ofs = 0
    for i in t.ids:
        n = t.agents[i].n
        o = ofs if goff is None else goff[i]
        t.agents[i].set_X(X[o * 4 * r:(o + n) * 4 * r])
        ofs += n


class Split:
    """the teams of a partition of the robots (parts: lists of robot ids, one per participant) at the global point X"""

    def __init__(self, mp, N, parts, X, r=R, **kw):
        self.N, self.parts, self.r = N, parts, r
        sizes = robot_sizes(mp, N)
        self.goff = np.concatenate([[0], np.cumsum(sizes)])
        self.owner = np.zeros(N, dtype=np.int32)
        for q, ids in enumerate(parts):
            self.owner[ids] = q
        self.teams = []
        for ids in parts:
            t = capi.Team.from_measurements(mp, capi.default_params(r=r, num_robots=N, **kw), local_ids=sorted(ids))
            set_X(t, X, r, self.goff)
            self.teams.append(t)

    def cols(self, q, per_pose):
        """indices of team q's poses' entries in a global array of `per_pose` doubles per pose"""
        idx = [np.arange(self.goff[i] * per_pose, self.goff[i + 1] * per_pose) for i in self.teams[q].ids]
        return np.concatenate(idx)

    def run(self, call, group=None):
        """call(team, transport) on every participant, one thread each: the results in rank order (raises the first error)"""
        g = group or capi.LocalGroup(len(self.teams))
        res = g.run([lambda q=q: call(self.teams[q], g[q]) for q in range(len(self.teams))], timeout=JOIN)
        for _, e in res:
            if e is not None:
                raise e
        return [x for x, _ in res]

    def close(self):
        for t in self.teams:
            t.close()


_OPT = {}


def optimum(ds, N):
    """the team solver's optimum of ds at rank R (cached per dataset)"""
    if ds not in _OPT:
        at = {"sphere2500": lambda f: abs(f - 843.5029071410438) <= 1e-6 * 843.5029071410438,
              "torus3D": lambda f: abs(2 * f - 2.4227e4) < 0.5}[ds]
        m, mp, n = problem(ds, N)
        t = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=N, **RTR_NESTEROV))
        t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(R))
        assert converge(t, at) > 0
        _OPT[ds] = t.global_X()
        t.close()
    return _OPT[ds]


def bits(x):
    return np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize("ds,N", [("smallGrid3D", 2), ("sphere2500", 5)])
def test_one_participant_equals_the_single_team_bitwise(ds, N):
    m, mp, n = problem(ds, N)
    X = optimum(ds, N) if ds == "sphere2500" else random_manifold_point(np.random.default_rng(3), R, n)
    t = single_team(mp, N, X)
    g = capi.LocalGroup(1)
    own = np.zeros(N, dtype=np.int32)
    V = np.random.default_rng(4).standard_normal(6 * 4 * n)
    assert bits(t.certificate_apply(V, transport=g[0], owner_of_robot=own)) == bits(t.certificate_apply(V))
    c0, v0 = t.certify(eta=ETA, tol=1e-6, max_iters=500)
    c1, v1 = t.certify(eta=ETA, tol=1e-6, max_iters=500, transport=g[0], owner_of_robot=own)
    assert bytes(c0) == bytes(c1) and bits(v0) == bits(v1), (c0, c1)
    for refine in (False, True):
        r0, T0 = t.round(refine_translations=refine)
        r1, T1 = t.round(refine_translations=refine, transport=g[0], owner_of_robot=own)
        assert bytes(r0) == bytes(r1) and bits(T0) == bits(T1), (r0, r1)
    t.close()


SPLITS = [("smallGrid3D", 2, [[0], [1]]), ("sphere2500", 5, [[0, 2, 4], [1, 3]]), ("sphere2500", 5, [[0], [1], [2], [3], [4]]),
          ("torus3D", 8, [[0, 1, 2, 3], [4, 5, 6, 7]]), ("torus3D", 8, [[0, 4], [1, 5], [2, 6], [3, 7]])]


@pytest.mark.parametrize("ds,N,parts", SPLITS)
def test_split_operator_is_bitwise_the_single_teams(ds, N, parts):
    m, mp, n = problem(ds, N)
    rng = np.random.default_rng(7)
    X = random_manifold_point(rng, R, n)
    t = single_team(mp, N, X)
    sp = Split(mp, N, parts, X)
    S = certificate_matrix(q_full(m, n), X, R, n) if ds == "smallGrid3D" else None
    for K in range(3, 9):
        V = rng.standard_normal(K * 4 * n)
        ref = t.certificate_apply(V)
        def rows(q):  # team q's entries of a K-row block in the iterate layout
            return np.concatenate([np.arange(c * K, (c + 1) * K) for c in sp.cols(q, 4)])
        outs = sp.run(lambda tm, tr: tm.certificate_apply(V[rows(tr.rank)], transport=tr, owner_of_robot=sp.owner))
        for q, o in enumerate(outs):
            assert bits(o) == bits(ref[rows(q)]), (K, q)
        if S is not None:
            want = as_matrix(V, K, n) @ S  # (S symmetric)
            assert np.abs(as_matrix(ref, K, n) - want).max() <= 1e-12 * np.abs(want).max()
    sp.close()
    t.close()


def assemble(sp, parts_out, per_pose):
    total = sp.goff[-1] * per_pose
    out = np.zeros(total)
    for q, x in enumerate(parts_out):
        out[sp.cols(q, per_pose)] = x
    return out


@pytest.mark.parametrize("ds,N,parts", [s for s in SPLITS if s[0] != "smallGrid3D"])
def test_split_certificate_and_rounding_agree_with_the_single_team(ds, N, parts):
    m, mp, n = problem(ds, N)
    X = optimum(ds, N)
    t = single_team(mp, N, X)
    sp = Split(mp, N, parts, X)
    kw = dict(eta=ETA, tol=1e-5, max_iters=3000)
    c0, _ = t.certify(**kw)
    res = sp.run(lambda tm, tr: tm.certify(transport=tr, owner_of_robot=sp.owner, **kw))
    cs = [c for c, _ in res]
    assert all(bytes(c) == bytes(cs[0]) for c in cs)
    c1 = cs[0]
    print("%s %s: single %r, split %r" % (ds, parts, c0, c1))
    assert c0.certified == 1 and c1.certified == 1
    assert c1.norm_bound == c0.norm_bound
    assert abs(c1.lambda_min - c0.lambda_min) <= 10 * kw["tol"] * c0.norm_bound
    for refine in (False, True):
        r0, T0 = t.round(refine_translations=refine)
        res = sp.run(lambda tm, tr: tm.round(refine_translations=refine, transport=tr, owner_of_robot=sp.owner))
        rs = [r for r, _ in res]
        assert all(bytes(r) == bytes(rs[0]) for r in rs)
        r1 = rs[0]
        T1 = assemble(sp, [T for _, T in res], 12)
        assert np.abs(T1 - T0).max() <= 1e-9 * max(1.0, np.abs(T0).max()), refine
        assert abs(r1.f_relaxed - r0.f_relaxed) <= 1e-12 * r0.f_relaxed
        assert abs(r1.f_rounded - r0.f_rounded) <= 1e-12 * r0.f_rounded
        assert (r1.reflected, r1.refined, r1.num_degenerate) == (r0.reflected, r0.refined, r0.num_degenerate)
    # determinism: a second split run gives the same bits
    res2 = sp.run(lambda tm, tr: tm.certify(transport=tr, owner_of_robot=sp.owner, **kw))
    assert all(bytes(a) == bytes(b) and bits(va) == bits(vb) for (a, va), (b, vb) in zip(
        sp.run(lambda tm, tr: tm.certify(transport=tr, owner_of_robot=sp.owner, **kw)), res2))
    sp.close()
    t.close()


def test_split_certificate_finds_negative_curvature():
    ds, N, r = "smallGrid3D", 2, 3
    m, mp, n = problem(ds, N)
    X = random_manifold_point(np.random.default_rng(1), r, n)
    t = single_team(mp, N, X, r=r)
    sp = Split(mp, N, [[0], [1]], X, r=r)
    c0, v0 = t.certify(eta=ETA)
    res = sp.run(lambda tm, tr: tm.certify(eta=ETA, transport=tr, owner_of_robot=sp.owner))
    c1 = res[0][0]
    assert bytes(res[1][0]) == bytes(c1)
    assert c0.certified == 0 and c1.certified == 0, (c0, c1)
    s = c0.norm_bound
    assert abs(c1.lambda_min - c0.lambda_min) <= 1e-8 * s
    v1 = assemble(sp, [v for _, v in res], 4)
    sgn = np.sign(v1 @ v0)
    assert np.abs(sgn * v1 / np.linalg.norm(v1) - v0 / np.linalg.norm(v0)).max() <= 1e-6
    V = np.zeros((3, 4 * n))
    V[0] = v1
    SV = as_matrix(t.certificate_apply(np.ascontiguousarray(V.T).reshape(-1)), 3, n)
    assert SV[0] @ v1 / (v1 @ v1) < -ETA * s
    sp.close()
    t.close()


def test_split_calls_have_no_side_effects():
    """a 200-iteration run of the bench configuration with a split certify and round in the middle leaves X, Y and V
    bitwise those of a run without them"""
    kw = dict(method=capi.METHOD_RGD, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=20)
    m, mp, n = problem("sphere2500", 5)
    outs = []
    for with_calls in (False, True):
        t = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=5, **kw))
        t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(R))
        t.run(100)
        if with_calls:
            sp = Split(mp, 5, [[0, 2, 4], [1, 3]], t.global_X())
            sp.run(lambda tm, tr: tm.certify(eta=ETA, transport=tr, owner_of_robot=sp.owner))
            sp.run(lambda tm, tr: tm.round(transport=tr, owner_of_robot=sp.owner))
            sp.close()
            g = capi.LocalGroup(1)
            own = np.zeros(5, dtype=np.int32)
            t.certify(eta=ETA, transport=g[0], owner_of_robot=own)
            t.round(transport=g[0], owner_of_robot=own)
        t.run(100)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert bits(a) == bits(b)


def _expect_refusal(sp, call, match):
    g = capi.LocalGroup(len(sp.teams), timeout=60.0)
    res = g.run([lambda q=q: call(q, sp.teams[q], g[q]) for q in range(len(sp.teams))], timeout=JOIN)
    for q, (_, e) in enumerate(res):
        assert isinstance(e, capi.DpgoError), (q, e)
        assert match in str(e), (q, str(e))


def test_refusals_reach_every_participant():
    ds, N = "sphere2500", 5
    m, mp, n = problem(ds, N)
    X = random_manifold_point(np.random.default_rng(2), R, n)
    sp = Split(mp, N, [[0, 2, 4], [1, 3]], X)
    own = sp.owner
    # a mismatched eta, a mismatched block
    _expect_refusal(sp, lambda q, tm, tr: tm.certify(eta=ETA * (1 + q), transport=tr, owner_of_robot=own), "disagree on eta")
    _expect_refusal(sp, lambda q, tm, tr: tm.certify(block=5 + q, transport=tr, owner_of_robot=own), "block size")
    # a robot on two participants / on none
    two = own.copy()
    two[1] = 0
    _expect_refusal(sp, lambda q, tm, tr: tm.round(transport=tr, owner_of_robot=two), "rank")
    # an uninitialised robot on one participant
    sp2 = Split(mp, N, [[0, 2, 4], [1, 3]], X)
    sp2.teams[1].close()
    sp2.teams[1] = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=N), local_ids=[1, 3])
    _expect_refusal(sp2, lambda q, tm, tr: tm.certificate_apply(np.zeros(3 * 4 * sum(tm.agents[i].n for i in tm.ids)),
                                                                transport=tr, owner_of_robot=own), "not initialized")
    sp2.close()
    sp.close()


def _gloo_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd.distributed import TorchTransport, certify_and_round
    dist.init_process_group("gloo", rank=rank, world_size=world)
    X = np.load(os.path.join(outdir, "X.npy"))
    m, mp, n = problem("smallGrid3D", 4)
    sp = Split(mp, 4, [[0, 2], [1, 3]], X)
    tm = sp.teams[rank]
    tr = TorchTransport(dist)
    c, v = tm.certify(eta=ETA, transport=tr, owner_of_robot=sp.owner)
    rd, T = tm.round(transport=tr, owner_of_robot=sp.owner)
    np.save(os.path.join(outdir, "out%d.npy" % rank),
            np.concatenate([np.frombuffer(bytes(c), np.uint8).astype(float), v, np.frombuffer(bytes(rd), np.uint8).astype(float), T]))
    # the helper: the global trajectory (robots by id) on every rank
    out = certify_and_round(tm, dist, sp.owner, eta=ETA)
    assert bytes(out["certificate"]) == bytes(c) and bytes(out["rounding"]) == bytes(rd)
    np.save(os.path.join(outdir, "T%d.npy" % rank), out["T"])
    sp.close()
    dist.destroy_process_group()


def test_two_processes_over_gloo_equal_two_threads():
    import torch.multiprocessing as mp_
    m, mp, n = problem("smallGrid3D", 4)
    X = random_manifold_point(np.random.default_rng(9), R, n)
    sp = Split(mp, 4, [[0, 2], [1, 3]], X)
    res = sp.run(lambda tm, tr: (tm.certify(eta=ETA, transport=tr, owner_of_robot=sp.owner),
                                 tm.round(transport=tr, owner_of_robot=sp.owner)))
    sp.close()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "X.npy"), X)
        mp_.spawn(_gloo_worker, args=(2, port, d), nprocs=2, join=True)
        for q in range(2):
            (c, v), (rd, T) = res[q]
            want = np.concatenate([np.frombuffer(bytes(c), np.uint8).astype(float), v,
                                   np.frombuffer(bytes(rd), np.uint8).astype(float), T])
            assert bits(np.load(os.path.join(d, "out%d.npy" % q))) == bits(want), q
        Tg = assemble(Split(mp, 4, [[0, 2], [1, 3]], X), [res[q][1][1] for q in range(2)], 12)
        for q in range(2):
            assert bits(np.load(os.path.join(d, "T%d.npy" % q))) == bits(Tg), q

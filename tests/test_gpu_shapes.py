"""Every rank r = 3..8 and the lane-tile edges of the kernels, against the extended-precision reference tests/xref.py under
componentwise bounds.  One team per rank holds agents of exactly 1, 2, PPB - 1, PPB, PPB + 1, 64, 65 and 257 poses (PPB =
64 / r poses per wave of the sparse kernels; 64 / 256 the tiles of the per-pose kernels), a pose whose row of Q has exactly
8 blocks (the full ELL part) and one with 9 (the CSR tail), an agent with no shared edge and one whose every pose has
shared edges.  Checked through the C-ABI: eval, hessvec, precondition (dense, two-level and block-Jacobi), get_G, the
public poses, the preconditioner residual, the manifold maps on both QF branches, and S(X) V for K = 3..8."""
import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import np_crosscheck as NP
from tests import xref
from tests.test_xref import C_PROD, ratio
from tests.util import synthetic_chain

pytestmark = pytest.mark.gpu

RANKS = [3, 4, 5, 6, 7, 8]
U = xref.U64


def sizes_of(r):
    ppb = 64 // r
    # the last agent is the one without shared edges
    return [1, 2, ppb - 1, ppb, ppb + 1, 64, 65, 257, ppb + 1]


def rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q * np.sign(np.linalg.det(Q))


_GRAPHS = {}


def graph(r):
    """(measurements in robot numbering, sizes, hub poses (agent, pose, blocks in its row))"""
    if r in _GRAPHS:
        return _GRAPHS[r]
    rng = np.random.default_rng(100 + r)
    sizes = sizes_of(r)
    off = np.r_[0, np.cumsum(sizes)]
    total = int(off[-1])
    m, _ = synthetic_chain(total, seed=r, lc_every=total + 1)
    robot = np.searchsorted(off, np.arange(total), side="right") - 1
    last = len(sizes) - 1
    # cut the chain in front of the isolated agent
    m = m[~((robot[m["p1"]] != last) & (robot[m["p2"]] == last))]
    extra = []
    # agent 7 (257 poses): pose 0 with 8 neighbours (9 blocks), pose 20 with 7 (8 blocks); loop closures every 40 poses
    g7 = int(off[7])
    extra += [(g7, g7 + k) for k in range(2, 9)]
    extra += [(g7 + 20, g7 + k) for k in range(22, 27)]
    extra += [(g7 + k, g7 + k + 20) for k in range(40, 230, 40)]
    # agent 4 (PPB + 1): every pose has a shared edge (to agent 5's poses)
    extra += [(int(off[4]) + k, int(off[5]) + 3 + k) for k in range(sizes[4])]
    # agent 5 (64): shared edges to agent 7 and a loop closure inside
    extra += [(int(off[5]) + 10, g7 + 100), (int(off[5]) + 5, int(off[5]) + 40)]
    e = np.zeros(len(extra), dtype=m.dtype)
    for k, (i, j) in enumerate(extra):
        e[k]["p1"], e[k]["p2"] = i, j
        e[k]["R"], e[k]["t"] = rotation(rng).reshape(-1), rng.standard_normal(3)
        e[k]["kappa"], e[k]["tau"], e[k]["weight"] = 20.0 + k % 7, 3.0 + k % 5, 1.0
    m = np.concatenate([m, e])
    mp = m.copy()
    mp["r1"], mp["p1"] = robot[m["p1"]], m["p1"] - off[robot[m["p1"]]]
    mp["r2"], mp["p2"] = robot[m["p2"]], m["p2"] - off[robot[m["p2"]]]
    hubs = [(7, 0, 9), (7, 20, 8)]
    _GRAPHS[r] = (mp, sizes, hubs)
    return _GRAPHS[r]


def make_team(r, mode):
    mp, sizes, hubs = graph(r)
    prm = capi.default_params(r=r, num_robots=len(sizes), precond_mode=mode)
    t = capi.Team.from_measurements(mp.view(capi.MEAS_DTYPE), prm)
    m_glob = mp.copy()
    off = np.r_[0, np.cumsum(sizes)]
    m_glob["p1"] = mp["p1"] + off[mp["r1"]]
    m_glob["p2"] = mp["p2"] + off[mp["r2"]]
    t.set_initial(capi.odometry_init(m_glob.view(capi.MEAS_DTYPE), int(off[-1])), capi.fixed_stiefel(r))
    return t, mp, sizes, hubs


def stiefel_blocks(rng, r, n):
    return NP.flat(NP.project_manifold(rng.standard_normal((r, 4 * n)), n))


MODES = [capi.PRECOND_DENSE, capi.PRECOND_TWO_LEVEL, capi.PRECOND_BLOCK_JACOBI]


@pytest.mark.parametrize("mode", MODES, ids=["dense", "two_level", "block_jacobi"])
@pytest.mark.parametrize("r", RANKS)
def test_agent_products_at_every_size(r, mode):
    t, mp, sizes, hubs = make_team(r, mode)
    rng = np.random.default_rng(r * 10 + mode)
    shared_any = []
    for a, n in enumerate(sizes):
        ag = t.agents[a]
        assert ag.n == n
        # neighbour poses of our own choosing: G is a function of them alone
        nbr_poses = {}
        for b in ag.neighbors():
            ids = ag.neighbor_pose_ids(b)
            P = stiefel_blocks(rng, r, len(ids))
            ag.update_neighbor_poses(b, ids, P, False)
            for k, p in enumerate(ids):
                nbr_poses[(b, int(p))] = P[k * 4 * r:(k + 1) * 4 * r]
        ag.build_problem(False)
        ref = xref.Agent(mp, a, n, r, nbr_poses)
        shared_any.append(len(ag.neighbors()) > 0)
        rp, _, _ = ag.get_Q()
        for (ha, hp, nb) in hubs:
            if ha == a:
                assert rp[hp + 1] - rp[hp] == nb
        # G: neighbour poses times the shared edges' coefficients
        G, Gm = ref.G()
        assert ratio(ag.get_G(), xref.flat(G), xref.flat(Gm), C_PROD) <= 1, (r, a)
        # public poses: a gather of the agent's own iterate, bit for bit
        X0 = xref.blocks(ag.get_X(), r, n)
        for b in ag.neighbors():
            ids, P = ag.get_public_poses(b)
            assert np.array_equal(ids, ref.public_pose_ids(b))
            assert np.array_equal(P, xref.flat(X0[ids]))
        X = stiefel_blocks(rng, r, n)
        Xb = xref.blocks(X, r, n)
        f, eg, rg = ag.eval(X)
        fr, fm = ref.f(Xb)
        assert ratio(f, fr, fm, 4 * r * n) <= 1, (r, a)  # f sums 4 r n products
        E, Em = ref.egrad(Xb)
        assert ratio(eg, xref.flat(E), xref.flat(Em), C_PROD) <= 1, (r, a)
        g, gm = ref.rgrad(Xb)
        assert ratio(rg, xref.flat(g), xref.flat(gm), C_PROD) <= 1, (r, a)
        eb, _ = xref.tangent_project(Xb, xref.blocks(rng.standard_normal(X.size), r, n))
        eta = xref.flat(eb)
        h, hm = ref.hessvec(Xb, xref.blocks(eta, r, n))
        assert ratio(ag.hessvec(X, eta), xref.flat(h), xref.flat(hm), C_PROD) <= 1, (r, a)
        # preconditioner: |z - z_ref|_2 <= 4n u kappa_2(P) |P^-1|_2 |v|_2 (an inverse formed by elimination over 4n
        # unknowns) plus the tangent projection's own c u mag
        V = rng.standard_normal(X.size)
        z, Z, kappa, pinv = ref.precondition(Xb, xref.blocks(V, r, n), block_jacobi=(mode == capi.PRECOND_BLOCK_JACOBI))
        assert ag.preconditioner() == mode
        _, zm = xref.tangent_project(Xb, Z)
        err = np.linalg.norm(ag.precondition(X, V) - xref.flat(z))
        bound = 4 * n * U * kappa * pinv * np.linalg.norm(V) + C_PROD * U * np.linalg.norm(xref.flat(zm))
        assert err <= bound, (r, a, err, bound)
        # the residual |z (Q + shift I) - v| / |v| of the exact forms: <= 4n u kappa_2(P).  Block-Jacobi is an approximation
        # of Q + shift I, and its residual measures that, not round-off
        res = ag.preconditioner_residual()
        if mode == capi.PRECOND_BLOCK_JACOBI:
            assert np.isfinite(res) and res > 0, (r, a, res)
        else:
            assert res <= 4 * n * U * kappa, (r, a, res)
    assert not shared_any[-1] and all(shared_any[:-1])
    t.close()


@pytest.mark.parametrize("r", RANKS)
def test_manifold_maps_at_every_size(r):
    t = capi.Team(capi.default_params(r=r, num_robots=1), [0])
    rng = np.random.default_rng(r)
    L = capi.lib()
    branches = [0, 0]
    for n in sorted(set(sizes_of(r) + [256])):
        X = stiefel_blocks(rng, r, n)
        Xb = xref.blocks(X, r, n)
        V = rng.standard_normal(X.size)
        tp = np.zeros_like(X)
        capi._chk(L.dpgo_tangent_project(t.h, capi._d(X), capi._d(V), n, capi._d(tp)), "tangent")
        want, mag = xref.tangent_project(Xb, xref.blocks(V, r, n))
        assert ratio(tp, xref.flat(want), xref.flat(mag), C_PROD) <= 1
        tang = xref.flat(want)
        for scale in (0.02, 0.5):
            eta = scale * tang
            rt = np.zeros_like(X)
            capi._chk(L.dpgo_retract(t.h, capi._d(X), capi._d(eta), n, capi._d(rt)), "retract")
            ref, cond, dev = xref.retract_qf(Xb, xref.blocks(eta, r, n))
            branches[0] += int((dev < 0.05).sum())
            branches[1] += int((dev >= 0.05).sum())
            # per pose: Gram-Schmidt errs by c u cond(A), the Cholesky branch (dev < 0.05: cond < 1.3) by c u cond(A)^2;
            # c = 64 for the 3 r-term products of each column
            d = np.abs(xref.blocks(rt, r, n) - ref).max(axis=(1, 2))
            assert (d <= C_PROD * U * cond ** 2).all(), (r, n, scale, d.max())
        Y = X + 0.2 * rng.standard_normal(X.size)
        pm = np.zeros_like(X)
        capi._chk(L.dpgo_project_manifold(t.h, capi._d(Y), n, capi._d(pm)), "project")
        ref, cond = xref.polar(xref.blocks(Y, r, n))
        # the polar factor through the eigen-decomposition of A^T A: c u cond(A)^2 per pose, c = 256 for the 3 x 3
        # eigensolver's sweeps and the recomposition A V diag(w^-1/2) V^T
        d = np.abs(xref.blocks(pm, r, n) - ref).max(axis=(1, 2))
        assert (d <= 256 * U * cond ** 2).all(), (r, n, d.max())
    assert branches[0] > 0 and branches[1] > 0, branches
    t.close()


@pytest.mark.parametrize("r", RANKS)
def test_certificate_operator_every_block_size(r):
    t, mp, sizes, _ = make_team(r, capi.PRECOND_DENSE)
    rng = np.random.default_rng(50 + r)
    N = int(sum(sizes))
    Xs = []
    for a, n in enumerate(sizes):
        X = stiefel_blocks(rng, r, n)
        t.agents[a].set_X(X)
        Xs.append(xref.blocks(X, r, n))
    t.exchange_all()
    Xg = np.concatenate(Xs)
    team = xref.Team(mp, sizes)
    for K in range(3, 9):
        V = rng.standard_normal(K * 4 * N)
        out = t.certificate_apply(V)
        want, mag = team.certificate_apply(Xg, xref.blocks(V, K, N))
        assert ratio(out, xref.flat(want), xref.flat(mag), C_PROD) <= 1, (r, K)
    t.close()

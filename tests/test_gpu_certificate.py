"""GPU checks of the certificate (csrc/certify.hip): the operator S(X) V against the numpy statement of
tests/test_certificate.py, its smallest eigenvalue against scipy / dense eigh, certificates at the SE-Sync optima of the
bundled datasets, the Riemannian staircase, determinism, no side effects, and the refusals."""
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests.test_certificate import (as_flat, as_matrix, certificate_matrix, deflation_basis, q_full,
                                    random_manifold_point)
from tests.util import DATA

pytestmark = pytest.mark.gpu

R = 5
ETA = 1e-6  # relative to the Gershgorin bound s on |S| (certificate)


def team_at(ds, N, X=None, T=None, r=R, **kw):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N) if N > 1 else m
    t = capi.Team.from_measurements(mp, capi.default_params(r=r, num_robots=N, **kw))
    if X is not None:
        ofs = 0
        for i in t.ids:
            na = t.agents[i].n
            t.agents[i].set_X(X[ofs:ofs + r * 4 * na])
            ofs += r * 4 * na
        t.exchange_all()
    else:
        t.set_initial(T if T is not None else capi.chordal_init(m, n), capi.fixed_stiefel(r))
    return t, m, n


@pytest.mark.parametrize("ds,N", [("tinyGrid3D", 1), ("smallGrid3D", 2), ("sphere2500", 5), ("torus3D", 8)])
def test_operator_matches_numpy(ds, N):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    rng = np.random.default_rng(11)
    X = random_manifold_point(rng, R, n)
    t, _, _ = team_at(ds, N, X=X)
    S = certificate_matrix(q_full(m, n), X, R, n)
    for K in range(3, 9):
        V = rng.standard_normal(K * 4 * n)
        got = as_matrix(t.certificate_apply(V), K, n)
        ref = (S @ as_matrix(V, K, n).T).T
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), K
    # S X^T = the Riemannian gradients dpgo_agent_eval returns, stacked
    XS = t.certificate_apply(X)
    ofs = 0
    for i in t.ids:
        a = t.agents[i]
        a.build_problem()
        Xa = X[ofs:ofs + R * 4 * a.n]
        _, _, rg = a.eval(Xa)
        got = XS[ofs:ofs + R * 4 * a.n]
        assert np.abs(got - rg).max() <= 1e-12 * max(1.0, np.abs(rg).max())
        ofs += R * 4 * a.n
    t.close()


def _vSv(t, v, n):
    V = np.zeros((3, 4 * n))
    V[0] = v
    V[1:] = np.random.default_rng(0).standard_normal((2, 4 * n))
    SV = as_matrix(t.certificate_apply(as_flat(V)), 3, n)
    return float(SV[0] @ v) / float(v @ v)


@pytest.mark.parametrize("ds,N", [("smallGrid3D", 2), ("sphere2500", 5)])
def test_smallest_eigenvalue_at_a_random_point(ds, N):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    X = random_manifold_point(np.random.default_rng(5), R, n)
    t, _, _ = team_at(ds, N, X=X)
    S = certificate_matrix(q_full(m, n), X, R, n)
    # undeflated: plain lambda_min(S) (eta out of reach: the solver runs to convergence)
    c, v = t.certify(eta=1e300, eta_relative=False, tol=1e-10, max_iters=5000, deflate=False)
    s = c.norm_bound
    assert c.certified == 1 and c.deflated == 0 and c.block == R
    if 4 * n < 2000:
        lam = np.linalg.eigvalsh(S.toarray())[0]
    else:
        lam = spla.eigsh(S, k=1, which="SA", tol=1e-14)[0][0]
    assert lam < -1e-3 * s  # indefinite at a random point
    assert abs(c.lambda_min - lam) <= 1e-8 * s, (c, lam)
    assert abs(_vSv(t, v, n) - c.lambda_min) <= 1e-8 * s
    assert c.residual <= 1e-10 * s
    if 4 * n < 2000:
        # deflated: lambda_min of P S P on Z-perp
        c2, v2 = t.certify(eta=1e300, eta_relative=False, tol=1e-10, max_iters=5000)
        B = deflation_basis(X, R, n)
        lam2 = np.linalg.eigvalsh(B.T @ (S @ B))[0]
        assert c2.deflated == 1 and abs(c2.lambda_min - min(0.0, lam2)) <= 1e-8 * s, (c2, lam2)
        Z = np.vstack([as_matrix(X, R, n), np.tile([0.0, 0.0, 0.0, 1.0], n)])
        assert (np.abs(Z @ v2) <= 1e-10 * np.linalg.norm(Z, axis=1) * np.linalg.norm(v2)).all()
        # a negative Ritz value stops the solver early, with a direction of negative curvature
        c3, v3 = t.certify(eta=ETA)
        assert c3.certified == 0 and c3.lambda_min < -ETA * c3.norm_bound and _vSv(t, v3, n) < -ETA * c3.norm_bound
    t.close()


RTR_NESTEROV = dict(method=capi.METHOD_RTR, acceleration=1, rtr_iterations=3, rtr_tcg_iterations=50, gradnorm_tol=1e-2,
                    restart_interval=50)
# (parking-garage is left out: the team solver does not reach its pinned optimum in a test's time)
OPTIMA = [  # dataset, agents, how the pinned cost is checked (tests/test_oracle_kats.py), solver
    ("sphere2500", 5, lambda f: abs(f - 843.5029071410438) <= 1e-6 * 843.5029071410438, RTR_NESTEROV),
    ("torus3D", 8, lambda f: abs(2 * f - 2.4227e4) < 0.5, RTR_NESTEROV),
    ("cubicle", 4, lambda f: abs(2 * f - 7.1713e2) < 0.005, RTR_NESTEROV),
]


def converge(t, at_optimum, chunk=50, limit=6000):
    k = 0
    while k < limit:
        t.run(chunk)
        k += chunk
        if at_optimum(t.cost()):
            return k
    return -k


@pytest.mark.parametrize("ds,N,at_optimum,kw", OPTIMA, ids=[o[0] for o in OPTIMA])
def test_certified_at_the_sesync_optima(ds, N, at_optimum, kw):
    t, m, n = team_at(ds, N, **kw)
    k = converge(t, at_optimum)
    assert k > 0, "the pinned optimum was not reached in %d iterations (cost %.12g)" % (-k, t.cost())
    c, v = t.certify(eta=ETA, tol=1e-5, max_iters=3000)  # (cubicle: 3.7e-6 s of residual after 1000 iterations)
    print("%s / %d: %d iterations, %r" % (ds, N, k, c))
    assert c.certified == 1, c
    t.close()


def test_staircase_escapes_a_saddle_and_ends_certified():
    """No pinned stall: the staircase starts from a seeded random point at r = 3 (first_iters = 0), which the certificate
    rejects, and must escape with a cost decrease at every escape, end certified and at the r = 5 chordal-start cost"""
    ds = "smallGrid3D"
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    prm = capi.default_params(r=3, num_robots=1, method=capi.METHOD_RTR, rtr_iterations=10, rtr_tcg_iterations=100,
                              gradnorm_tol=1e-9)
    X0 = random_manifold_point(np.random.default_rng(1), 3, n)
    out = capi.riemannian_staircase(m, prm, r0=3, r_max=8, eta=ETA, X0=X0, iters=40, first_iters=0)
    assert len(out["ranks"]) >= 2 and out["ranks"][0] == 3
    assert all(after < before for before, after in out["escape_costs"])
    assert out["certificate"].certified == 1, out["certificate"]
    ref, _, _ = team_at(ds, 1, method=capi.METHOD_RTR, rtr_iterations=10, rtr_tcg_iterations=100, gradnorm_tol=1e-9)
    ref.run(40)
    f5 = ref.cost()
    ref.close()
    assert abs(out["costs"][-1] - f5) <= 1e-6 * f5, (out["costs"], f5)


def test_certify_is_deterministic_and_has_no_side_effects():
    """two calls give the same bits; a 200-iteration run of the bench configuration with a certify in the middle leaves
    X, Y and V bitwise those of a run without it"""
    kw = dict(method=capi.METHOD_RGD, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=20)
    outs = []
    for with_cert in (False, True):
        t, m, n = team_at("sphere2500", 5, **kw)
        t.run(100)
        if with_cert:
            c1, v1 = t.certify(eta=ETA)
            c2, v2 = t.certify(eta=ETA)
            assert bytes(c1) == bytes(c2) and v1.tobytes() == v2.tobytes()
        t.run(100)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_refusals():
    m, n = capi.read_g2o(os.path.join(DATA, "smallGrid3D.g2o"))
    mp = capi.partition(m, n, 2)
    part = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=2), local_ids=[0])
    part.agents[0].set_X(random_manifold_point(np.random.default_rng(2), R, part.agents[0].n))
    with pytest.raises(capi.DpgoError, match="every robot"):
        part.certify()
    part.close()
    t = capi.Team.from_measurements(mp, capi.default_params(r=R, num_robots=2))
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.certify()
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.certificate_apply(np.zeros(3 * 4 * n))
    t.close()

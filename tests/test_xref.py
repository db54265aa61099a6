"""CPU checks of the extended-precision reference tests/xref.py: it agrees with the independent fp64 statement of
oracle/np_crosscheck.py under its own componentwise bounds, with closed forms (an exact trajectory has zero gradient, an
improper lift rounds to F R_0^T R_i F), and every bound rejects a reference with one edge dropped, one pose block zeroed or
the reflection rule inverted."""
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import np_crosscheck as NP
from tests import xref
from tests.test_certificate import as_matrix, certificate_matrix, q_full
from tests.util import DATA, synthetic_chain

LD = xref.LD
# c of the componentwise bounds |x - ref| <= c 2^-53 sum |a||b|.  Products: a row of Q has at most 1 + deg blocks of 4
# columns (36 terms at the 9-block rows of the tests), each entry of Q itself a sum over the deg <= 8 edges at the pose of
# 4-term products (32 more); the tangent projection adds 2 x 3 terms.  128 is twice that sum; the cost f sums 4 r n such
# terms, so its c is 4 r n.
C_PROD = 128


def ratio(x, ref, mag, c):
    """max |x - ref| / (c u mag); entries with mag = 0 must be exact"""
    d = np.abs(np.asarray(x, dtype=LD) - np.asarray(ref, dtype=LD))
    mag = np.asarray(mag, dtype=LD)
    if np.any(d[mag == 0] != 0):
        return np.inf
    return float((d[mag > 0] / (c * xref.U64 * mag[mag > 0])).max(initial=0.0))


def to_meas(edges):
    m = np.zeros(len(edges), dtype=capi.MEAS_DTYPE)
    for k, e in enumerate(edges):
        m[k]["r1"], m[k]["p1"], m[k]["r2"], m[k]["p2"] = e["r1"], e["p1"], e["r2"], e["p2"]
        m[k]["R"], m[k]["t"] = np.asarray(e["R"]).reshape(-1), e["t"]
        m[k]["kappa"], m[k]["tau"], m[k]["weight"] = e["kappa"], e["tau"], e["w"]
    return m


def np_case(ds, N, r, aid, seed=3):
    edges, n = NP.read_g2o(os.path.join(DATA, ds + ".g2o"))
    pe = NP.partition(edges, n, N)
    rng = np.random.default_rng(seed)
    nbr = {}
    for e in pe:
        for a, p in ((e["r1"], e["p1"]), (e["r2"], e["p2"])):
            if a != aid and (a, p) not in nbr:
                nbr[(a, p)] = NP.project_manifold(rng.standard_normal((r, 4)), 1)
    prob = NP.Problem(pe, aid, r, nbr)
    ref = xref.Agent(to_meas(pe), aid, prob.n, r, {k: NP.flat(v) for k, v in nbr.items()})
    X = NP.project_manifold(rng.standard_normal((r, 4 * prob.n)), prob.n)
    eta = NP.tangent_project(X, rng.standard_normal(X.shape), prob.n)
    V = rng.standard_normal(X.shape)
    return prob, ref, X, eta, V


def B(Xm, r, n):
    return xref.blocks(NP.flat(Xm), r, n)


@pytest.mark.parametrize("ds,N,r,aid", [("tinyGrid3D", 2, 5, 0), ("smallGrid3D", 2, 3, 1), ("smallGrid3D", 3, 7, 1)])
def test_agrees_with_the_numpy_statement(ds, N, r, aid):
    prob, ref, X, eta, V = np_case(ds, N, r, aid)
    n = prob.n
    Xb, eb, Vb = B(X, r, n), B(eta, r, n), B(V, r, n)
    G, Gm = ref.G()
    assert ratio(NP.flat(prob.G), xref.flat(G), xref.flat(Gm), C_PROD) <= 1
    f, fm = ref.f(Xb)
    assert ratio(prob.f(X), f, fm, 4 * r * n) <= 1
    E, Em = ref.egrad(Xb)
    assert ratio(NP.flat(prob.egrad(X)), xref.flat(E), xref.flat(Em), C_PROD) <= 1
    g, gm = ref.rgrad(Xb)
    assert ratio(NP.flat(prob.rgrad(X)), xref.flat(g), xref.flat(gm), C_PROD) <= 1
    h, hm = ref.hessvec(Xb, eb)
    assert ratio(NP.flat(prob.hess(X, eta)), xref.flat(h), xref.flat(hm), C_PROD) <= 1
    tp, tpm = xref.tangent_project(Xb, Vb)
    assert ratio(NP.flat(NP.tangent_project(X, V, n)), xref.flat(tp), xref.flat(tpm), C_PROD) <= 1
    # the preconditioner: |z - z_ref|_2 <= c u kappa_2(P) |P^-1|_2 |v|_2, c = 4n (an elimination over the 4n unknowns)
    z, _, kappa, pinv = ref.precondition(Xb, Vb)
    err = np.linalg.norm(NP.flat(prob.precond(X, V)) - xref.flat(z))
    assert err <= 4 * n * xref.U64 * kappa * pinv * np.linalg.norm(V)
    assert np.abs(ref.q_dense() - prob.Q).max() <= C_PROD * xref.U64 * np.abs(prob.Q).max()
    # QF retraction and polar factor: normwise per pose, c u cond(A) (Gram-Schmidt) and c u cond(A)^2 (polar by the
    # Gram matrix), c = 64
    rt, cond, _ = xref.retract_qf(Xb, 0.3 * eb)
    d = np.abs(B(NP.retract(X, 0.3 * eta, n), r, n) - rt).max(axis=(1, 2))
    assert (d <= C_PROD * xref.U64 * cond).all()
    pp, cond = xref.polar(Xb + 0.2 * Vb)
    d = np.abs(B(NP.project_manifold(X + 0.2 * V, n), r, n) - pp).max(axis=(1, 2))
    assert (d <= C_PROD * xref.U64 * cond ** 2).all()


def test_certificate_operator_agrees_with_the_sparse_statement():
    ms, n = synthetic_chain(150, seed=4)
    r, K = 5, 4
    rng = np.random.default_rng(1)
    X = NP.flat(NP.project_manifold(rng.standard_normal((r, 4 * n)), n))
    V = rng.standard_normal(K * 4 * n)
    S = certificate_matrix(q_full(ms, n), X, r, n)
    want = (S @ as_matrix(V, K, n).T).T
    team = xref.Team(ms, [n])
    out, mag = team.certificate_apply(xref.blocks(X, r, n), xref.blocks(V, K, n))
    got = as_matrix(xref.flat(out), K, n)
    assert ratio(want, got, as_matrix(xref.flat(mag), K, n), C_PROD) <= 1


def exact_chain(n, seed=0):
    """a synthetic chain without noise, ground truth recovered by composing the odometry in long double"""
    m, n = synthetic_chain(n, seed=seed, noise=0.0)
    T = NP.odometry([dict(i=int(e["p1"]), j=int(e["p2"]), R=np.asarray(e["R"]).reshape(3, 3), t=e["t"]) for e in m], n)
    return m, n, T


def test_exact_trajectory_has_zero_gradient():
    m, n, T = exact_chain(120)
    r = 6
    Y = np.zeros((r, 3))
    Y[:3] = np.eye(3)
    X = xref.blocks(NP.flat(Y @ T), r, n)
    ref = xref.Agent(m, 0, n, r)
    g, gm = ref.rgrad(X)
    # the ground truth composed in fp64 over up to n odometry steps and the measurements rounded to fp64: each residual
    # is a few ulps per step of the chain, c = 4096 > 8 (terms) x 120 (steps) x 4; a zeroed pose block leaves O(mag).
    # (A dropped edge changes nothing here: every residual is zero -- test_bounds_bite drops edges at random points.)
    assert ratio(0.0, xref.flat(g), xref.flat(gm), 4096) <= 1
    X0 = X.copy()
    X0[7] = 0
    g3, _ = ref.rgrad(X0)
    assert ratio(0.0, xref.flat(g3), xref.flat(gm), 4096) > 1


def test_improper_lift_rounds_to_the_reflected_trajectory():
    m, n, T = exact_chain(40, seed=2)
    r = 5
    Fm = np.diag([1.0, 1.0, -1.0])
    Rs = T[:, :].reshape(3, n, 4)[:, :, :3].transpose(1, 0, 2)
    Y = np.linalg.qr(np.random.default_rng(0).standard_normal((r, 3)))[0]
    Xb = np.zeros((n, r, 4))
    for i in range(n):
        Xb[i, :, :3] = Y @ Rs[i] @ Fm
        Xb[i, :, 3] = Y @ T[:, 4 * i + 3]
    Tr, reflected, sv, _ = xref.round_team(Xb.astype(LD))
    want = np.array([Fm @ Rs[0].T @ Rs[i] @ Fm for i in range(n)])
    got = Tr.reshape(n, 12)[:, :9].reshape(n, 3, 3).transpose(0, 2, 1)
    # R_i composed from 40 fp64 odometry steps is orthogonal to ~1e-14, and its nearest rotation moves it that much
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(sv - 1).max() <= 1e-12
    # the bound the GPU tests use (1e-12 on a proper rotation) rejects the inverted reflection rule
    Tb, _, _, _ = xref.round_team(Xb.astype(LD), reflect=1 - reflected)
    gotb = Tb.reshape(n, 12)[:, :9].reshape(n, 3, 3).transpose(0, 2, 1)
    assert np.abs(gotb - want).max() > 1e-3


@pytest.mark.parametrize("ds,N,r,aid", [("smallGrid3D", 2, 5, 0)])
def test_bounds_bite(ds, N, r, aid):
    """every product bound rejects the reference of a problem with one edge dropped, or of an input with one pose block
    zeroed"""
    prob, ref, X, eta, V = np_case(ds, N, r, aid)
    n = prob.n
    Xb, eb, Vb = B(X, r, n), B(eta, r, n), B(V, r, n)
    dropped = xref.Agent.__new__(xref.Agent)
    dropped.__dict__.update(ref.__dict__)
    i, j, T, om = ref.priv
    dropped.priv = (i[1:], j[1:], T[1:], om[1:])
    Xz = Xb.copy()
    Xz[n // 2] = 0
    for fn in (lambda a, x: a.egrad(x), lambda a, x: a.rgrad(x), lambda a, x: a.hessvec(x, eb), lambda a, x: a.f(x)):
        want, mag = fn(ref, Xb)
        c = 4 * r * n if np.ndim(want) == 0 else C_PROD
        assert ratio(fn(dropped, Xb)[0], want, mag, c) > 1
        assert ratio(fn(ref, Xz)[0], want, mag, c) > 1
    # G: drop a shared edge
    G, Gm = ref.G()
    d2 = xref.Agent.__new__(xref.Agent)
    d2.__dict__.update(ref.__dict__)
    i, T, om, Z = ref.sh1 if len(ref.sh1[0]) else ref.sh2
    part = (i[1:], T[1:], om[1:], Z[1:])
    if len(ref.sh1[0]):
        d2.sh1 = part
    else:
        d2.sh2 = part
    assert ratio(d2.G()[0], G, Gm, C_PROD) > 1
    # the preconditioner's normwise bound
    z, _, kappa, pinv = ref.precondition(Xb, Vb)
    zb = z.copy()
    zb[n // 2] = 0
    assert np.linalg.norm(xref.flat(zb) - xref.flat(z)) > 4 * n * xref.U64 * kappa * pinv * np.linalg.norm(V)
    # certificate operator: one edge fewer
    team = xref.Team(ref.m[(ref.m["r1"] == aid) & (ref.m["r2"] == aid)], [n])
    Kb = Vb[:, :4, :]
    out, mag = team.certificate_apply(Xb, Kb)
    t2 = xref.Team(ref.m[(ref.m["r1"] == aid) & (ref.m["r2"] == aid)][1:], [n])
    assert ratio(t2.certificate_apply(Xb, Kb)[0], out, mag, C_PROD) > 1

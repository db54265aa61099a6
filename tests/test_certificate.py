"""No-GPU checks of the certificate: an independent numpy/scipy statement of S(X) = Q - Lambda(X) (checked against the
stacked Riemannian gradients of oracle/np_crosscheck.Problem) and the host-side staircase step dpgo_escape_point."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from dpgo_ros_amd import capi
from oracle import np_crosscheck as NP
from tests.util import DATA


def q_full(m, n):
    """the data matrix of the whole problem, sparse 4n x 4n, straight from the edge cost
    w/2 |(X_j - X_i T) Omega^(1/2)|^2, T = [[R, t], [0, 1]], Omega = diag(kappa, kappa, kappa, tau)"""
    rows, cols, vals = [], [], []

    def put(i, j, B):
        ii, jj = np.meshgrid(np.arange(4 * i, 4 * i + 4), np.arange(4 * j, 4 * j + 4), indexing="ij")
        rows.append(ii.ravel()); cols.append(jj.ravel()); vals.append(B.ravel())

    for e in m:
        i, j = int(e["p1"]), int(e["p2"])
        T = np.eye(4)
        T[:3, :3] = np.asarray(e["R"]).reshape(3, 3)
        T[:3, 3] = e["t"]
        Om = np.diag([e["kappa"]] * 3 + [e["tau"]]) * e["weight"]
        put(i, i, T @ Om @ T.T)
        put(j, j, Om)
        put(i, j, -T @ Om)
        put(j, i, -Om @ T.T)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(4 * n, 4 * n))


def global_pose_index(mp):
    """(robot, local pose) -> index of the pose in team order (robots by id, the partition keeps poses contiguous)"""
    n_of = {}
    for e in mp:
        n_of[int(e["r1"])] = max(n_of.get(int(e["r1"]), 0), int(e["p1"]) + 1)
        n_of[int(e["r2"])] = max(n_of.get(int(e["r2"]), 0), int(e["p2"]) + 1)
    off = np.concatenate([[0], np.cumsum([n_of[k] for k in sorted(n_of)])])
    return off


def as_matrix(x, rows, n):
    """iterate layout (rows x 4n column-major, [(4 g + c) rows + a]) -> rows x 4n matrix"""
    return np.asarray(x).reshape(4 * n, rows).T


def as_flat(Xm):
    return np.ascontiguousarray(Xm.T).reshape(-1)


def certificate_matrix(Q, X, r, n):
    """S(X) = Q - blockdiag_i [[Sym(Y_i^T (X Q)_i,rot), 0], [0, 0]] for X in the iterate layout"""
    Xm = as_matrix(X, r, n)
    E = np.asarray((Q.T @ Xm.T).T)  # X Q
    Y = Xm.reshape(r, n, 4)[:, :, :3]
    Er = E.reshape(r, n, 4)[:, :, :3]
    Lam = np.einsum("anp,anq->npq", Y, Er)
    Lam = 0.5 * (Lam + Lam.transpose(0, 2, 1))
    blocks = np.zeros((n, 4, 4))
    blocks[:, :3, :3] = Lam
    return (Q - sp.block_diag(list(blocks), format="csr")).tocsr()


def deflation_basis(X, r, n):
    """orthonormal basis (columns) of Z-perp, Z = [rows of X; e_t]"""
    Z = np.vstack([as_matrix(X, r, n), np.tile([0.0, 0.0, 0.0, 1.0], n)])
    U, s, Vt = np.linalg.svd(Z.T, full_matrices=True)
    return U[:, Z.shape[0]:]


def random_manifold_point(rng, r, n):
    Xm = rng.standard_normal((r, 4 * n))
    return as_flat(NP.project_manifold(Xm, n))


@pytest.mark.parametrize("ds,N", [("tinyGrid3D", 1), ("smallGrid3D", 2), ("smallGrid3D", 3)])
def test_reference_S_times_X_is_the_stacked_riemannian_gradient(ds, N):
    """S(X) X^T = the Riemannian gradients of the agents' problems (np_crosscheck.Problem, neighbour poses from X), stacked"""
    r = 5
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    Q = q_full(m, n)
    X = random_manifold_point(np.random.default_rng(7), r, n)
    S = certificate_matrix(Q, X, r, n)
    XS = (S @ as_matrix(X, r, n).T).T  # X S (S symmetric)
    edges, n2 = NP.read_g2o(os.path.join(DATA, ds + ".g2o"))
    assert n2 == n
    parts = NP.partition(edges, n, N)
    mp = capi.partition(m, n, N)
    off = global_pose_index(mp)
    Xm = as_matrix(X, r, n)
    nbr = {(k, p): Xm[:, 4 * (off[k] + p):4 * (off[k] + p) + 4] for k in range(N) for p in range(off[k + 1] - off[k])}
    for k in range(N):
        prob = NP.Problem(parts, k, r, nbr)
        Xa = Xm[:, 4 * off[k]:4 * off[k + 1]]
        ref = prob.rgrad(Xa)
        got = XS[:, 4 * off[k]:4 * off[k + 1]]
        assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())
    assert abs((S - S.T)).max() <= 1e-9 * abs(S).max()


def test_escape_point_at_zero_step_is_the_lifted_point_bitwise():
    rng = np.random.default_rng(3)
    r, n = 4, 37
    X = random_manifold_point(rng, r, n)
    v = rng.standard_normal(4 * n)
    out = capi.escape_point(X, r, n, v, 0.0)
    lifted = np.vstack([as_matrix(X, r, n), np.zeros((1, 4 * n))])
    assert out.tobytes() == as_flat(lifted).tobytes()


@pytest.mark.parametrize("r", [3, 5, 7])
def test_escape_point_matches_numpy_and_stays_on_the_manifold(r):
    rng = np.random.default_rng(r)
    n = 29
    X = random_manifold_point(rng, r, n)
    v = rng.standard_normal(4 * n)
    alpha = 0.37
    out = as_matrix(capi.escape_point(X, r, n, v, alpha), r + 1, n)
    A = np.vstack([as_matrix(X, r, n), alpha * v[None, :]])
    ref = NP.project_manifold(A, n)
    assert np.abs(out - ref).max() < 1e-13
    for i in range(n):
        Yi = out[:, 4 * i:4 * i + 3]
        assert np.abs(Yi.T @ Yi - np.eye(3)).max() < 1e-14
        assert np.array_equal(out[:, 4 * i + 3], A[:, 4 * i + 3])  # translations: [p; alpha v_t]


def test_escape_point_rejects_rank_8():
    n = 3
    X = np.zeros(8 * 4 * n)
    with pytest.raises(capi.DpgoError, match="3..7"):
        capi.escape_point(X, 8, n, np.zeros(4 * n), 0.1)

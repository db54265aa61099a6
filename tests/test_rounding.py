"""No-GPU checks of the SE-Sync rounding (csrc/round.hip): an independent numpy statement of it -- top-3 left singular
vectors of the rotation block, the determinant majority, the nearest rotation per pose, the gauge of the first pose --
and of the translation refinement (a scipy sparse solve), next to the helpers of tests/test_certificate.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from dpgo_ros_amd import capi
from tests.test_certificate import as_flat, as_matrix, q_full, random_manifold_point
from tests.util import DATA


def nearest_rotations(B):
    """nearest rotation to every 3 x 3 block of B (n x 3 x 3), through the SVD"""
    W, _, Vt = np.linalg.svd(B)
    d = np.ones((len(B), 3))
    d[:, 2] = np.sign(np.linalg.det(W @ Vt))
    return W @ (d[:, :, None] * Vt)


def to_T(R, t):
    """rotations n x 3 x 3 and translations 3 x n -> 12 doubles per pose (R column-major, then t)"""
    n = len(R)
    T = np.zeros((n, 12))
    T[:, :9] = R.transpose(0, 2, 1).reshape(n, 9)
    T[:, 9:] = t.T
    return T.reshape(-1)


def from_T(T):
    T = np.asarray(T).reshape(-1, 12)
    return T[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1), T[:, 9:].T.copy()


def anchored(T):
    """every pose relative to the first: T_i <- T_0^-1 T_i"""
    R, t = from_T(T)
    R0, t0 = R[0], t[:, 0]
    return to_T(np.einsum("mk,nmc->nkc", R0, R), R0.T @ (t - t0[:, None]))


def round_numpy(X, r, n):
    """SE-Sync rounding of X (iterate layout, r x 4n) -> (T anchored at pose 0, reflected, singular values descending)"""
    P = as_matrix(X, r, n).reshape(r, n, 4)
    Y, p = P[:, :, :3], P[:, :, 3]
    Yf = Y.reshape(r, 3 * n)
    w, V = np.linalg.eigh(Yf @ Yf.T)
    U = V[:, ::-1][:, :3]
    sigma = np.sqrt(np.maximum(w[::-1], 0.0))
    B = np.einsum("ak,anc->nkc", U, Y)
    t = U.T @ p
    d = np.linalg.det(B)
    reflected = bool((d < 0).sum() > (d > 0).sum())
    if reflected:
        B[:, 2, :] *= -1.0
        t[2] *= -1.0
    return anchored(to_T(nearest_rotations(B), t)), reflected, sigma


def cost_numpy(m, n, T):
    """1/2 <T, T Q> of a trajectory (3 x 4n in the iterate layout) with the weights of m"""
    Tm = as_matrix(T, 3, n)
    return 0.5 * float(np.sum(Tm * (q_full(m, n) @ Tm.T).T))


def refine_translations(m, n, T):
    """the translations minimising sum_e w tau |t_j - t_i - R_i t~|^2 with t_0 = 0 for the rotations of T (scipy sparse)"""
    R, t = from_T(T)
    keep = m["p1"] != m["p2"]
    i, j = m["p1"][keep].astype(int), m["p2"][keep].astype(int)
    wt = (m["weight"] * m["tau"])[keep]
    v = np.einsum("ekc,ec->ek", R[i], m["t"][keep])
    L = sp.csr_matrix((np.concatenate([wt, wt, -wt, -wt]), (np.concatenate([i, j, i, j]), np.concatenate([i, j, j, i]))),
                      shape=(n, n))
    b = np.zeros((n, 3))
    np.add.at(b, i, -wt[:, None] * v)
    np.add.at(b, j, wt[:, None] * v)
    x = spla.spsolve(L[1:, 1:].tocsc(), b[1:])
    t = np.zeros((3, n))
    t[:, 1:] = np.asarray(x).reshape(n - 1, 3).T
    return to_T(R, t)


def random_trajectory(rng, n):
    R = nearest_rotations(rng.standard_normal((n, 3, 3)))
    return to_T(R, 10.0 * rng.standard_normal((3, n)))


def lifted(T, n, Ylift, r):
    """X = Ylift [R_i | t_i] in the iterate layout (the numpy statement of dpgo_lift)"""
    R, t = from_T(T)
    Xm = np.zeros((r, 4 * n))
    Yl = np.asarray(Ylift).reshape(3, r).T  # r x 3, column-major
    for k in range(n):
        Xm[:, 4 * k:4 * k + 3] = Yl @ R[k]
        Xm[:, 4 * k + 3] = Yl @ t[:, k]
    return as_flat(Xm)


@pytest.mark.parametrize("r", [3, 4, 5, 6, 7, 8])
def test_rounding_a_lifted_trajectory_returns_it_anchored(r):
    rng = np.random.default_rng(r)
    n = 41
    T = random_trajectory(rng, n)
    X = capi.lift(T, n, capi.fixed_stiefel(r), r)
    assert np.abs(X - lifted(T, n, capi.fixed_stiefel(r), r)).max() < 1e-12
    got, _, sigma = round_numpy(X, r, n)
    ref = anchored(T)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (sigma[3:] <= 1e-12 * sigma[0]).all()


@pytest.mark.parametrize("r", [4, 5, 8])
def test_rounding_is_invariant_under_orthogonal_transforms(r):
    rng = np.random.default_rng(10 + r)
    n = 57
    X = random_manifold_point(rng, r, n)
    O, _ = np.linalg.qr(rng.standard_normal((r, r)))
    if np.linalg.det(O) > 0:
        O[:, 0] *= -1.0  # (a reflection as well)
    T1, _, s1 = round_numpy(X, r, n)
    T2, _, s2 = round_numpy(as_flat(O @ as_matrix(X, r, n)), r, n)
    assert np.abs(T1 - T2).max() <= 1e-10 * np.abs(T1).max()
    assert np.abs(s1 - s2).max() <= 1e-12 * s1[0]


def _mixed_point(rng, n, flipped, r=5):
    """[Z; 0] with Z_i = S_i [R_i | t_i], S_i = diag(1, 1, -1) for the poses in `flipped`, I for the others"""
    T = random_trajectory(rng, n)
    R, t = from_T(T)
    Xm = np.zeros((r, 4 * n))
    for k in range(n):
        S = np.diag([1.0, 1.0, -1.0]) if k in flipped else np.eye(3)
        Xm[:3, 4 * k:4 * k + 3] = S @ R[k]
        Xm[:3, 4 * k + 3] = S @ t[:, k]
    return as_flat(Xm), T


def test_reflection_rule_follows_the_determinant_majority():
    rng = np.random.default_rng(4)
    n = 30
    # 18 of 30 blocks reflected, pose 0 among them: the rule turns the majority proper, and those poses come back exactly
    flipped = set(range(18))
    X, T = _mixed_point(rng, n, flipped)
    got, _, _ = round_numpy(X, 5, n)
    ref = anchored(T)
    g, rf = got.reshape(n, 12), ref.reshape(n, 12)
    assert np.abs(g[:18] - rf[:18]).max() <= 1e-12 * np.abs(ref).max()
    # and the rounded blocks of the majority are rotations (det +1) before the gauge
    P = as_matrix(X, 5, n).reshape(5, n, 4)
    Yf = P[:, :, :3].reshape(5, 3 * n)
    U = np.linalg.eigh(Yf @ Yf.T)[1][:, ::-1][:, :3]
    d = np.linalg.det(np.einsum("ak,anc->nkc", U, P[:, :, :3]))
    _, reflected, _ = round_numpy(X, 5, n)
    assert reflected == bool((d < 0).sum() > (d > 0).sum())
    assert ((d if not reflected else -d)[:18] > 0).all()
    # a tie keeps U
    X2, _ = _mixed_point(rng, n, set(range(15)))
    assert round_numpy(X2, 5, n)[1] is False


@pytest.mark.parametrize("ds", ["smallGrid3D", "sphere2500"])
def test_translation_refinement_never_raises_the_cost(ds):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    rng = np.random.default_rng(2)
    for r in (3, 5):
        X = random_manifold_point(rng, r, n)
        T0, _, _ = round_numpy(X, r, n)
        T1 = refine_translations(m, n, T0)
        f0, f1 = cost_numpy(m, n, T0), cost_numpy(m, n, T1)
        assert f1 <= f0 * (1 + 1e-12), (f0, f1)
        assert np.array_equal(from_T(T1)[0], from_T(T0)[0])
        # a critical point in the translations: the translation columns of T Q vanish away from the pinned pose
        G = (q_full(m, n) @ as_matrix(T1, 3, n).T).T.reshape(3, n, 4)[:, 1:, 3]
        assert np.abs(G).max() <= 1e-8 * np.abs(q_full(m, n)).max() * np.abs(T1).max()


def test_translations_given_rotations_refuses_a_disconnected_graph():
    """host-side check ahead of any device work: edges of zero weight that cut pose 1 off"""
    m, n = capi.read_g2o(os.path.join(DATA, "tinyGrid3D.g2o"))
    m = m.copy()
    touch = (m["p1"] == 1) | (m["p2"] == 1)
    m["weight"][touch] = 0.0
    with pytest.raises(capi.DpgoError, match="disconnected"):
        capi.translations_given_rotations(m, n, np.tile([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], n))

"""Edge cases of the SE-Sync rounding (csrc/round.hip) against the 40-digit reference of tests/xref.py: poses that stay
exactly on the Stiefel manifold while their projection onto the top-3 subspace has rank 2, 1 or 0 (r >= 6), full-rank blocks
with singular values (1, 1e-6, 1e-7), the determinant vote (a fully improper lift, an exact tie) and the same inputs split
across teams."""
import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import xref
from tests.test_gpu_certify_across import Split
from tests.util import synthetic_chain

pytestmark = pytest.mark.gpu

Fm = np.diag([1.0, 1.0, -1.0])


def rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def planted(rng, r, sv):
    """an r x 3 block with orthonormal columns whose top 3 x 3 part has singular values sv (0 <= s <= 1), the rest of every
    column in rows 3, 4, 5"""
    Ua, Va = rotation(rng), rotation(rng)
    Y = np.zeros((r, 3))
    Y[:3] = Ua @ np.diag(sv) @ Va.T
    row = 3
    for k, s in enumerate(sv):
        if s < 1:
            Y[row] = np.sqrt(1 - s * s) * Va[:, k]
            row += 1
    return Y


def rank_deficient(rng, r, rank):
    """top 3 x 3 part [u_0 .. u_(rank-1), 0 ..] (columns of a random rotation), the other columns coordinate vectors in
    rows 3, 4, 5: the top rows are exactly orthogonal to the others, so the Gram matrix has no top / bottom cross term and
    U lies exactly in rows 0..2"""
    Ua = rotation(rng)
    Y = np.zeros((r, 3))
    Y[:3, :rank] = Ua[:, :rank]
    for k in range(rank, 3):
        Y[3 + k - rank, k] = 1.0
    return Y


def team_with(Xb, r, N=2):
    """a chain over the poses of Xb ((n, r, 4)), split over N robots, set to that iterate"""
    n = Xb.shape[0]
    m, _ = synthetic_chain(n, seed=1)
    per = n // N
    mp = m.copy()
    mp["r1"], mp["r2"] = np.minimum(m["p1"] // per, N - 1), np.minimum(m["p2"] // per, N - 1)
    mp["p1"], mp["p2"] = m["p1"] - mp["r1"] * per, m["p2"] - mp["r2"] * per
    X = xref.flat(Xb)
    t = capi.Team.from_measurements(mp, capi.default_params(r=r, num_robots=N))
    ofs = 0
    for i in t.ids:
        k = t.agents[i].n
        t.agents[i].set_X(X[ofs * 4 * r:(ofs + k) * 4 * r])
        ofs += k
    t.exchange_all()
    return t, mp, X


def rotations_of(T):
    return T.reshape(-1, 12)[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)


def proper(T):
    R = rotations_of(T)
    return max(np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max(), np.abs(np.linalg.det(R) - 1).max())


def generic_point(rng, r, n):
    Xb = np.zeros((n, r, 4))
    for i in range(n):
        Xb[i, :3, :3] = rotation(rng)
        Xb[i, :, 3] = rng.standard_normal(r)
    return Xb


def check_against_reference(Xb, T, skip=()):
    Tref, _, sv, _ = xref.round_team(Xb.astype(xref.LD))
    R, Rr = rotations_of(T), rotations_of(Tref)
    for i in range(Xb.shape[0]):
        if i in skip:
            continue
        # the nearest rotation is determined to u s1 / (s2 + s3) (rank 2: s3 = 0); c = 1024 covers the Gram matrix, the
        # eigenvectors U on the host and the 3 x 3 products, each a few u
        tol = 1024 * xref.U64 * max(1.0, sv[i, 0] / (sv[i, 1] + sv[i, 2]))
        assert np.abs(R[i] - Rr[i]).max() <= tol, (i, sv[i], np.abs(R[i] - Rr[i]).max(), tol)


@pytest.mark.parametrize("r", [6, 8])
def test_rank_deficient_blocks(r):
    rng = np.random.default_rng(r)
    n = 150
    Xb = generic_point(rng, r, n)
    plant = {5: 2, 70: 2, 71: 1, 130: 0}
    for i, k in plant.items():
        Xb[i, :, :3] = rank_deficient(rng, r, k)
    t, _, _ = team_with(Xb, r)
    rd, T = t.round(refine_translations=False)
    assert rd.num_degenerate == len(plant), rd
    assert proper(T) <= 1e-12
    # rank 2 has a unique answer; rank 1 and 0 do not
    check_against_reference(Xb, T, skip=(71, 130))
    t.close()


@pytest.mark.parametrize("r", [5, 7])
def test_ill_conditioned_full_rank_blocks(r):
    """singular values (1, 1e-6, 1e-7): v2 and v3 of A^T A are resolved only to u / 1e-12, the rotation to u 1e6"""
    rng = np.random.default_rng(20 + r)
    n = 150
    Xb = generic_point(rng, r, n)
    plant = [9, 64, 90, 149]
    for i in plant:
        Xb[i, :, :3] = planted(rng, r, (1, 1e-6, 1e-7))
    Y = Xb[:, :, :3]
    assert np.abs(Y.transpose(0, 2, 1) @ Y - np.eye(3)).max() < 1e-15
    t, _, _ = team_with(Xb, r)
    rd, T = t.round(refine_translations=False)
    assert rd.num_degenerate == 0, rd  # |det| = 1e-13 >> 1e-12 s1^2 s2
    assert proper(T) <= 1e-12
    check_against_reference(Xb, T)
    t.close()


def exact_diagonal_point(rng, r, n_lift, improper):
    """lifted signed-permutation rotations (improper where `improper`) in rows 0..2, plus a rank-2 (columns e0, e1, e3), a
    rank-1 (e0, e3, e4) and a rank-0 (e3, e4, e5) pose: every Gram entry is an exact integer, the diagonal strictly
    decreasing over rows 0, 1, 2, so the host eigensolver returns U = [e0 e1 e2] exactly and the vote is determined"""
    perms = []
    for _ in range(n_lift):
        P = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)
        perms.append(P * np.linalg.det(P))
    Xb = np.zeros((n_lift + 3, r, 4))
    for i, P in enumerate(perms):
        Xb[i, :3, :3] = P @ Fm if improper[i] else P
        Xb[i, :3, 3] = rng.integers(-4, 5, 3)
    for k, cols in enumerate([(0, 1, 3), (0, 3, 4), (3, 4, 5)]):
        for c, a in enumerate(cols):
            Xb[n_lift + k, a, c] = 1.0
    return Xb, perms


def test_a_fully_improper_lift_is_reflected():
    r, n_lift = 6, 61
    rng = np.random.default_rng(5)
    Xb, P = exact_diagonal_point(rng, r, n_lift, [True] * n_lift)
    t, _, _ = team_with(Xb, r)
    rd, T = t.round(refine_translations=False)
    assert rd.reflected == 1 and rd.num_degenerate == 3, rd  # the rank-2, rank-1 and rank-0 poses
    R = rotations_of(T)
    for i in range(n_lift):
        assert np.abs(R[i] - Fm @ P[0].T @ P[i] @ Fm).max() <= 1e-14
    # the rank-2 pose: D U^T Y = diag(1, 1, 0), whose nearest rotation is I, anchored
    assert np.abs(R[n_lift] - Fm @ P[0].T @ Fm).max() <= 1e-14
    assert proper(T) <= 1e-12
    t.close()


def test_an_exact_tie_keeps_U():
    r, n_lift = 6, 60
    rng = np.random.default_rng(6)
    improper = [i % 2 == 1 for i in range(n_lift)]
    Xb, P = exact_diagonal_point(rng, r, n_lift, improper)
    t, _, _ = team_with(Xb, r)
    rd, T = t.round(refine_translations=False)
    assert rd.reflected == 0, rd
    R = rotations_of(T)
    for i in range(0, n_lift, 2):  # the proper poses are their own nearest rotations
        assert np.abs(R[i] - P[0].T @ P[i]).max() <= 1e-14
    assert proper(T) <= 1e-12
    t.close()
    # one improper pose more: reflected
    improper[0] = True
    Xb, P = exact_diagonal_point(np.random.default_rng(6), r, n_lift, improper)
    t, _, _ = team_with(Xb, r)
    rd, _ = t.round(refine_translations=False)
    assert rd.reflected == 1, rd
    t.close()


def test_split_across_teams():
    """one participant reproduces the single team bit for bit on these blocks; a split over two participants gives the
    same bits on both, the single team's flags, and rotations within the reference's bound (its partial sums are added in
    rank order, so its Gram matrix, and with it U, differs from the single team's in the last bits)"""
    r, N = 6, 3
    rng = np.random.default_rng(8)
    n = 150
    Xb = generic_point(rng, r, n)
    for i, k in {5: 2, 71: 1, 130: 0}.items():
        Xb[i, :, :3] = rank_deficient(rng, r, k)
    Xb[90, :, :3] = planted(rng, r, (1, 1e-6, 1e-7))
    t, mp, X = team_with(Xb, r, N)
    rd, T = t.round(refine_translations=False)
    g = capi.LocalGroup(1)
    r1, T1 = t.round(refine_translations=False, transport=g[0], owner_of_robot=np.zeros(N, dtype=np.int32))
    assert bytes(r1) == bytes(rd) and T1.tobytes() == T.tobytes()
    sp = Split(mp, N, [[0, 2], [1]], X, r=r)
    res = sp.run(lambda tm, tr: tm.round(refine_translations=False, transport=tr, owner_of_robot=sp.owner))
    assert all(bytes(rq) == bytes(res[0][0]) for rq, _ in res)
    rs = res[0][0]
    assert (rs.reflected, rs.num_degenerate) == (rd.reflected, rd.num_degenerate)
    Ts = np.zeros_like(T)
    for q, (_, Tq) in enumerate(res):
        Ts[sp.cols(q, 12)] = Tq
    assert proper(Ts) <= 1e-12
    check_against_reference(Xb, Ts, skip=(71, 130))
    sp.close()
    t.close()

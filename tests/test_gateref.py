"""CPU checks of tests/gateref.py, the reference of the Mahalanobis gate: the Jacobians against central
differences of the relative-pose map, the measurement noise against the Hessian of the cost itself, and that the tolerances
of tests/test_gpu_gate.py reject the mistakes the conventions invite."""
import numpy as np
import pytest

from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G


def log_f64(E):
    return G.log_so3(E, np.float64)


def random_T(n, seed):
    return NR.banded_chain(n, seed, window=8)[1]


def relative_coordinates(T0, T1, i, j):
    """the perturbation (phi_ij, delta_ij) that takes the relative pose at T0 to the one at T1"""
    R0, t0 = G.relative_pose(T0, i, j, np.float64)
    R1, t1 = G.relative_pose(T1, i, j, np.float64)
    return np.r_[log_f64(R0.T @ R1), t1 - t0]


@pytest.mark.parametrize("i,j", [(1, 4), (4, 1), (0, 3), (3, 0)])
def test_jacobians_match_central_differences(i, j):
    """step h = 1e-6: truncation ~ h^2 = 1e-12, round-off ~ u |t| / h ~ 2e-16 x 20 / 1e-6 = 4e-9: held to 1e-8"""
    n, h = 6, 1e-6
    T = random_T(n, 3)
    Ji, Jj = G.jacobians(T, i, j, np.float64)
    worst = 0.0
    for g, J in ((i, Ji), (j, Jj)):
        for c in range(6):
            xi = np.zeros((n, 6))
            xi[g, c] = h
            d = (relative_coordinates(T, covref.perturb(T, xi, n), i, j) - relative_coordinates(T, covref.perturb(T, -xi, n), i, j)) / (2 * h)
            worst = max(worst, np.abs(d - J[:, c]).max())
    print("J against central differences: %.3e" % worst)
    assert worst <= 1e-8


def one_edge(seed, kappa=100.0, tau=50.0):
    """two poses joined by one noise-free edge; pose 0 is NOT the identity"""
    m, T = NR.banded_chain(3, seed, window=2)
    T = T.reshape(3, 4, 3)[1:].reshape(-1).copy()
    (Rij, tij) = G.relative_pose(T, 0, 1, np.float64)
    e = m[:1].copy()
    e["p1"], e["p2"], e["R"], e["t"], e["kappa"], e["tau"] = 0, 1, Rij.reshape(-1), tij, kappa, tau
    return e, T


def test_sigma_meas_is_the_inverse_hessian_of_one_edge():
    """second central differences (h = 1e-4) of the project's own cost 1/2 <T, T Q> of a one-edge graph in the coordinates of
    pose 1: round-off ~ u f / h^2 with f ~ kappa |R|^2: 2e-16 x 300 / 1e-8 = 6e-6, truncation ~ h^2 x 2 kappa = 2e-6; held to
    1e-4 of the largest entry"""
    kappa, tau, h = 100.0, 50.0, 1e-4
    e, T = one_edge(5, kappa, tau)
    Q = covref.q_full(e, 2)

    def f(x):
        return covref.cost(Q, covref.perturb(T, np.r_[np.zeros(6), x], 2), 2)

    H = np.zeros((6, 6))
    for a in range(6):
        for b in range(6):
            ea, eb = np.eye(6)[a] * h, np.eye(6)[b] * h
            H[a, b] = (f(ea + eb) - f(ea - eb) - f(eb - ea) + f(-ea - eb)) / (4 * h * h)
    # the coordinates of pose 1 are those of the relative pose up to J_j = diag(I, R_0^T): an orthogonal change of delta
    want = np.diag([2 * kappa] * 3 + [tau] * 3)
    err = np.abs(H - want).max()
    print("edge Hessian by finite differences: %.3e of %.3g" % (err, 2 * kappa))
    assert err <= 1e-4 * 2 * kappa
    assert np.abs(np.linalg.inv(want) - G.sigma_meas(kappa, tau, np.float64)).max() <= 1e-18


def test_two_pose_graph_gives_the_measurement_noise():
    kappa, tau = 100.0, 50.0
    e, T = one_edge(7, kappa, tau)
    _, Sigma, _ = covref.dense_reference(covref.q_full(e, 2), T, 2)
    _, Jj = G.jacobians(T, 0, 1, np.float64)
    got = Jj @ Sigma @ Jj.T
    want = G.sigma_meas(kappa, tau, np.float64)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # and through the whole reference: pose 0's blocks are zero
    Sr = G.sigma_rel(T, 0, 1, *G.blocks_of(Sigma, 0, 1))
    assert np.abs(np.asarray(Sr, dtype=np.float64) - want).max() <= 1e-12 * np.abs(want).max()


def test_log_edge_cases():
    assert not G.log_so3(np.eye(3)).any()
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    w = G.log_so3(2.0 * np.outer(ax, ax) - np.eye(3))  # the rotation by pi
    assert np.isfinite(np.asarray(w, dtype=np.float64)).all() and abs(float(np.sqrt(w @ w)) - np.pi) <= 1e-12
    for th in (1e-9, 0.3, 3.0, np.pi - 1e-6):
        w = G.log_so3(covref.exp_so3(th * ax))
        assert np.abs(np.asarray(w, dtype=np.float64) - th * ax).max() <= 1e-9 * max(th, 1e-9) + 4e-16


def test_the_tolerances_reject_the_mistakes():
    """the bounds of tests/test_gpu_gate.py (gateref.sigma_rel_bound, xi_bound, d2_bound) against four wrong readings of the
    definitions, each computed in float64 from the same blocks: every one must leave its bound on the candidates below"""
    n = 12
    m, T = NR.banded_chain(n, 2, window=8)
    _, Sigma, _ = covref.dense_reference(covref.q_full(m, n), T, n)
    rng = np.random.default_rng(4)
    kappa, tau = 100.0, 50.0
    worst = dict(swapped=0.0, transposed=0.0, cross_sign=0.0, kappa=0.0, swapped_d2=0.0, transposed_d2=0.0, cross_sign_d2=0.0)
    for _ in range(20):
        i, j = rng.choice(np.arange(1, n), 2, replace=False)
        Rij, tij = G.relative_pose(T, i, j, np.float64)
        Rm = Rij @ covref.exp_so3(0.3 * rng.standard_normal(3) / np.sqrt(3))
        tm = tij + 0.1 * rng.standard_normal(3)
        Sii, Sjj, Sij = G.blocks_of(Sigma, i, j)
        xi, d2, Sr, S = G.gate(T, i, j, Rm, tm, kappa, tau, Sii, Sjj, Sij)
        b_s, b_x = G.sigma_rel_bound(T, i, j, Sii, Sjj, Sij), G.xi_bound(T, i, j, tm)
        b_d = G.d2_bound(xi, S, d2, b_x, b_s)
        f64 = np.float64

        def ratio_d2(Sr_wrong, xi_wrong=None, noise=None):
            Sw = np.asarray(Sr_wrong, dtype=f64) + (G.sigma_meas(kappa, tau, f64) if noise is None else noise)
            x = np.asarray(xi if xi_wrong is None else xi_wrong, dtype=f64)
            return abs(x @ np.linalg.solve(Sw, x) - float(d2)) / b_d

        # i and j swapped: the candidate read as j -> i
        Sw = G.sigma_rel(T, j, i, Sjj, Sii, np.asarray(Sij).T, f64)
        worst["swapped"] = max(worst["swapped"], (np.abs(Sw - np.asarray(Sr, dtype=f64)) / b_s).max())
        worst["swapped_d2"] = max(worst["swapped_d2"], ratio_d2(Sw, G.innovation(T, j, i, Rm, tm, f64)))
        # Sigma_ij transposed
        Sw = G.sigma_rel(T, i, j, Sii, Sjj, np.asarray(Sij).T, f64)
        worst["transposed"] = max(worst["transposed"], (np.abs(Sw - np.asarray(Sr, dtype=f64)) / b_s).max())
        worst["transposed_d2"] = max(worst["transposed_d2"], ratio_d2(Sw))
        # the sign of [t_ij]x flipped
        Ji, Jj = G.jacobians(T, i, j, f64)
        Ji[3:, :3] *= -1.0
        A = Ji @ Sii @ Ji.T + Ji @ Sij @ Jj.T + Jj @ Sij.T @ Ji.T + Jj @ Sjj @ Jj.T
        Sw = 0.5 * (A + A.T)
        worst["cross_sign"] = max(worst["cross_sign"], (np.abs(Sw - np.asarray(Sr, dtype=f64)) / b_s).max())
        worst["cross_sign_d2"] = max(worst["cross_sign_d2"], ratio_d2(Sw))
        # 1 / kappa in the place of 1 / (2 kappa)
        worst["kappa"] = max(worst["kappa"], ratio_d2(Sr, noise=np.diag([1 / kappa] * 3 + [1 / tau] * 3)))
    print("largest error / bound of each mistake:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v > 1e3, "the tolerance lets the mistake '%s' pass (error / bound %.3g)" % (k, v)

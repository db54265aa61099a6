"""CPU checks of the marginal-covariance feature: the numpy reference of tests/covref.py against central
second differences of the cost, the body-frame conversion against a direct statement, and the C entry's declaration."""
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests import covref
from tests.util import DATA, ROOT


@pytest.mark.parametrize("ds", ["tinyGrid3D", "smallGrid3D"])
def test_reference_hessian_matches_second_differences(ds):
    """u^T H v against (g(hu + hv) - g(hu - hv) - g(-hu + hv) + g(-hu - hv)) / 4 h^2 at the chordal initialisation (not a
    critical point), 20 random direction pairs, h = 1e-4: relative 1e-5 (measured 3e-7 / 2e-7); H symmetric"""
    m, n = O.read_g2o(os.path.join(DATA, ds + ".g2o"))
    T = O.chordal_init(m, n)
    Q = covref.q_full(m, n)
    S = covref.certificate_matrix(Q, T, 3, n)
    J = covref.jacobian(T, n)
    H = (J.T @ covref.sp.kron(S, covref.sp.identity(3), format="csr") @ J).toarray()
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    assert np.abs(covref.hessian(Q, T, n).toarray() - H).max() <= 1e-12 * np.abs(H).max()
    rng = np.random.default_rng(5)
    h = 1e-4
    g = lambda xi: covref.cost(Q, covref.perturb(T, xi, n), n)
    exact, fd = [], []
    for _ in range(20):
        u, v = rng.standard_normal(6 * n), rng.standard_normal(6 * n)  # (every component moves by about h)
        exact.append(u @ H @ v)
        fd.append((g(h * (u + v)) - g(h * (u - v)) - g(h * (v - u)) + g(-h * (u + v))) / (4 * h * h))
    exact, fd = np.array(exact), np.array(fd)
    rel = np.linalg.norm(fd - exact) / np.linalg.norm(exact)
    print("%s: second differences against H, relative %.3e" % (ds, rel))
    assert rel <= 1e-5
    # the reduced Hessian at this point is positive definite (cond_2 2.0e3 / 7.5e6)
    w = np.linalg.eigvalsh(covref.reduced(covref.hessian(Q, T, n)).toarray())
    print("%s: cond_2(H_red) = %.3e" % (ds, w[-1] / w[0]))
    assert w[0] > 0


def test_body_frame_conversion_matches_direct_statement():
    rng = np.random.default_rng(3)
    N = 7
    T = np.zeros((N, 4, 3))
    for g in range(N):
        Qm, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        T[g, :3, :] = (Qm * np.sign(np.linalg.det(Qm))).T  # R column-major
        T[g, 3, :] = rng.standard_normal(3)
    R = covref.rotations(T.reshape(-1), N)
    cov = rng.standard_normal((N, 6, 6))
    out = capi.covariance_to_body_frame(cov, T.reshape(-1))
    for g in range(N):
        A = np.eye(6)
        A[3:, 3:] = R[g].T
        assert np.abs(out[g] - A @ cov[g] @ A.T).max() <= 1e-14
    pairs = np.array([[1, 4], [6, 2], [3, 3]])
    cross = rng.standard_normal((len(pairs), 6, 6))
    Tm = T.reshape(N, 12)
    out = capi.covariance_to_body_frame(cross, (Tm[pairs[:, 0]], Tm[pairs[:, 1]]))
    for k, (a, b) in enumerate(pairs):
        Aa, Ab = np.eye(6), np.eye(6)
        Aa[3:, 3:], Ab[3:, 3:] = R[a].T, R[b].T
        assert np.abs(out[k] - Aa @ cross[k] @ Ab.T).max() <= 1e-14
    with pytest.raises(ValueError):
        capi.covariance_to_body_frame(cov[:3], T.reshape(-1))


def test_entry_is_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+dpgo_team_marginal_covariances\s*\(", txt)
    assert re.search(r"\}\s*dpgo_covariance_t\s*;", txt)
    assert "dpgo_team_marginal_covariances" in capi.EXPORTS
    assert hasattr(capi.lib(), "dpgo_team_marginal_covariances")
    assert [f[0] for f in capi.Covariance._fields_] == ["n", "logdet", "min_pivot", "max_pivot", "seconds_assemble",
                                                        "seconds_invert"]
    assert callable(capi.Team.covariances)

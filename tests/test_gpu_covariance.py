"""GPU checks of the marginal pose covariances (csrc/covariance.hip, Team.covariances) against the numpy /
scipy reference of tests/covref.py.

Bounds.  An inverse through Cholesky has the textbook forward error n eps cond_2(H_red) (n = 6 (N - 1), eps = 2.2e-16):
    |Sigma_gpu - Sigma_ref|_F <= n eps cond_2 |Sigma_ref|_F       (small graphs: dense reference, cond_2 from eigvalsh)
    |H_red C_p - E_p|_F <= n eps cond_est                          (large graphs: sparse reference, cond_est from eigsh)
Nothing in them is tuned; the measured ratios are in profiles/r10_covariance.md."""
import ctypes as C
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests import covref
from tests.test_certificate import random_manifold_point
from tests.test_gpu_certificate import OPTIMA, RTR_NESTEROV, converge, team_at
from tests.util import DATA, add_outliers

pytestmark = pytest.mark.gpu

EPS = covref.EPS
BENCH = dict(method=capi.METHOD_RGD, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=20)


def all_pairs(n):
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1)


def check_against_dense(tag, t, m, n, T):
    """items 4 and 5 at one point"""
    Q = covref.q_full(m, n)
    Hr, Sref, w = covref.dense_reference(Q, T, n)
    assert w[0] > 0, "%s: the reference H_red is not positive definite (%.3e)" % (tag, w[0])
    cond, nn = w[-1] / w[0], 6 * (n - 1)
    bound = nn * EPS * cond
    pairs = all_pairs(n)
    res, diag, cross = t.covariances(T, pairs)
    S = covref.full_sigma(diag, cross, pairs, n)
    err = np.linalg.norm(S - Sref) / np.linalg.norm(Sref)
    # the diagonal blocks as returned (symmetrised) and as cross blocks (a, a) (not symmetrised) agree to round-off
    for g in range(n):
        Bc = cross[g * n + g]
        assert np.abs(diag[g] - 0.5 * (Bc + Bc.T)).max() == 0.0
    sign, logdet = np.linalg.slogdet(Hr)
    lerr = abs(res.logdet - logdet) / abs(logdet)
    print("%s: n = %d, cond_2 = %.3e, |Sigma - ref|_F / |ref|_F = %.3e (bound %.3e, ratio %.3e), logdet %.12g (rel %.3e), %r"
          % (tag, nn, cond, err, bound, err / bound, res.logdet, lerr, res))
    assert res.n == nn
    assert err <= bound
    assert sign > 0 and lerr <= bound
    assert res.min_pivot > 0 and res.max_pivot >= res.min_pivot
    # pose 0: exactly zero, alone and in every pair
    assert not diag[0].any()
    zero = (pairs[:, 0] == 0) | (pairs[:, 1] == 0)
    assert not cross[zero].any() and cross[~zero].any()
    for g in range(1, n):
        assert diag[g].tobytes() == np.ascontiguousarray(diag[g].T).tobytes()
        assert np.linalg.eigvalsh(diag[g])[0] > 0
    return res


@pytest.mark.parametrize("ds,N", [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 2), ("smallGrid3D", 3)])
def test_blocks_match_dense_inverse(ds, N):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    Tc = capi.chordal_init(m, n)
    t, _, _ = team_at(ds, N, T=Tc, **RTR_NESTEROV)
    check_against_dense("%s / %d, chordal T" % (ds, N), t, m, n, Tc)
    t.run(300)
    rd, T = t.round()
    check_against_dense("%s / %d, rounded T (f %.9g)" % (ds, N, rd.f_rounded), t, m, n, T)
    # T = None rounds the current iterate first
    a, d0, _ = t.covariances()
    b, d1, _ = t.covariances(T)
    assert d0.tobytes() == d1.tobytes() and a.logdet == b.logdet
    t.close()


def column_block_residual(tag, t, Hr, n, T, p):
    """item 6: the pairs (i, p) for all i, stacked into C_p; |H_red C_p - E_p|_F"""
    pairs = np.stack([np.arange(n), np.full(n, p)], axis=1)
    res, diag, cross = t.covariances(T, pairs)
    Cp = cross[1:].reshape(6 * (n - 1), 6)
    E = np.zeros_like(Cp)
    E[6 * (p - 1):6 * p] = np.eye(6)
    rr = np.linalg.norm(Hr @ Cp - E)
    assert np.abs(0.5 * (cross[p] + cross[p].T) - diag[p]).max() == 0.0
    print("%s: p = %d, |H_red C_p - E_p|_F = %.3e, %r" % (tag, p, rr, res))
    return rr, res


def at_scale(ds, N, at_optimum, kw, ps):
    t, m, n = team_at(ds, N, **kw)
    k = converge(t, at_optimum)
    assert k > 0, "the pinned optimum was not reached in %d iterations (cost %.12g)" % (-k, t.cost())
    rd, T = t.round()
    Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
    lo, hi = covref.extreme_eigenvalues(Hr)
    nn = 6 * (n - 1)
    print("%s / %d: %d iterations, n = %d, eigenvalues %.3e .. %.3e, cond_est %.3e, bound %.3e" %
          (ds, N, k, nn, lo, hi, hi / lo, nn * EPS * hi / lo))
    assert lo > 0
    bound = nn * EPS * hi / lo
    for p in [q % n for q in ps]:
        rr, res = column_block_residual("%s / %d" % (ds, N), t, Hr, n, T, p)
        assert res.n == nn and rr <= bound, (rr, bound)
    t.close()


def test_sphere2500_column_blocks_at_the_optimum():
    ds, N, at_optimum, kw = OPTIMA[0]
    assert ds == "sphere2500"
    at_scale(ds, N, at_optimum, kw, [-1, 1250, 1])


def test_torus3D_column_block_at_the_optimum():
    ds, N, at_optimum, kw = OPTIMA[1]
    assert ds == "torus3D"
    at_scale(ds, N, at_optimum, kw, [-1])


def test_cubicle_column_block_at_the_optimum():
    """order 34 494: 3 x 9.5 GB, element indices beyond 2^30 -- the index arithmetic of the dense inverse at scale"""
    ds, N, at_optimum, kw = OPTIMA[2]
    assert ds == "cubicle"
    at_scale(ds, N, at_optimum, kw, [-1])


def test_parking_garage_column_block_where_the_solver_stops():
    """kappa from 2e-9 to 2: the Hessian sits at the edge of what fp64 Cholesky resolves.  The case found: the team solver
    does not reach the pinned optimum (2f = 1.2625) in a test's time -- RTR + Nesterov stops at its own gradient tolerance
    with 2f = 1.26967, and 4000 iterations at gradnorm_tol 1e-6 reach 1.26333 --, and at the rounded point where it stops the
    reference H_red IS positive definite on the CPU (shift-invert: 3.9e-9 .. 6.2e2, the next ones 7e-9, 5.5e-8; 4.06e-9 after
    4000 iterations), so the case enters: n eps cond_est = 0.35, measured residual 1.8e-8, pivots 2.8e-3 .. 6.1e2.  At the
    chordal T the reference has the eigenvalue -3.1e-8 and the call refuses (a non-positive pivot); that is recorded in
    profiles/r10_covariance.md and not asserted: -3e-8 is within the factorisation's own error."""
    ds, N = "parking-garage", 2
    t, m, n = team_at(ds, N, **RTR_NESTEROV)
    t.run(500)
    rd, T = t.round()
    Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
    lo, hi = covref.extreme_eigenvalues(Hr)
    nn = 6 * (n - 1)
    print("%s / %d: 2f = %.9g, n = %d, eigenvalues %.3e .. %.3e, bound %.3e" % (ds, N, 2 * t.cost(), nn, lo, hi, nn * EPS * hi / lo))
    assert lo > 0
    rr, res = column_block_residual("%s / %d" % (ds, N), t, Hr, n, T, n - 1)
    assert res.n == nn and res.min_pivot > 0 and rr <= nn * EPS * hi / lo
    t.close()


def gather(t):
    return covref.team_measurements_global(t)


def test_current_weights_are_honoured():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    t.run(300)
    _, T = t.round()
    _, d_before, _ = t.covariances(T)
    lc = [k for k in range(len(mp)) if not (mp["r1"][k] == mp["r2"][k] and mp["p1"][k] + 1 == mp["p2"][k])]
    e = mp[lc[len(lc) // 2]]
    for a in {int(e["r1"]), int(e["r2"])}:
        assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
        t.agents[a].clear_data_matrices()
    mw, nw = gather(t)
    assert nw == n and len(mw) == len(m) and (mw["weight"] == 0).sum() == 1
    check_against_dense("%s / %d, one loop closure at weight 0" % (ds, N), t, mw, n, T)
    _, d_after, _ = t.covariances(T)
    assert np.abs(d_after - d_before).max() > 1e-9 * np.abs(d_before).max()  # (the weight matters)
    t.close()


def test_weights_after_an_update_round_are_honoured():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mo = add_outliers(m.view(O.MEAS_DTYPE), n, frac=0.1, seed=0).view(capi.MEAS_DTYPE)
    mp = capi.partition(mo, n, N)
    kw = dict(RTR_NESTEROV, robust_cost_type=capi.COST_GNC_TLS, gnc_barc=3.0, gnc_mu_step=2.0, gnc_init_mu=1e-2)
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **kw))
    t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(5))
    t.run(100)
    t.update_weights()
    t.run(300)
    mw, nw = gather(t)
    w = mw["weight"]
    print("after one update round: %d of %d weights changed, range %.3g .. %.3g" % ((w != 1.0).sum(), len(w), w.min(), w.max()))
    assert nw == n and (w != 1.0).any()
    _, T = t.round()
    check_against_dense("%s / %d + 10 %% outliers, one update round" % (ds, N), t, mw, n, T)
    t.close()


def raw_call(t, T, pairs, diag, cross, res):
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return capi.lib().dpgo_team_marginal_covariances(t.h, capi._d(np.ascontiguousarray(T)), 0, len(pr), capi._d(pr) if len(pr) else None,
                                                     capi._d(diag), capi._d(cross) if len(pr) else None, C.byref(res))


def test_refusals_leave_the_outputs_untouched():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    Q = covref.q_full(m, n)
    # a random trajectory is not a minimum: the seed is picked on the CPU so that the reference H_red has an eigenvalue
    # below -1e-6 of the largest, far beyond the factorisation's own error
    for seed in range(20):
        T = random_manifold_point(np.random.default_rng(100 + seed), 3, n)
        R = covref.rotations(T, n)
        if (np.linalg.det(R) < 0).any():  # (the Stiefel projection gives O(3): flip the reflected ones)
            P = T.reshape(n, 4, 3).copy()
            P[np.linalg.det(R) < 0, 2, :] *= -1.0
            T = P.reshape(-1)
        w = np.linalg.eigvalsh(covref.reduced(covref.hessian(Q, T, n)).toarray())
        if w[0] < -1e-6 * w[-1]:
            break
    else:
        raise AssertionError("no seed gave an indefinite reference Hessian")
    print("random T (seed %d): eigenvalues %.3e .. %.3e" % (seed, w[0], w[-1]))
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    pairs = np.array([[1, 2], [5, 100]])
    diag, cross, res = np.full((n, 6, 6), 7.25), np.full((2, 6, 6), 7.25), capi.Covariance()
    assert raw_call(t, T, pairs, diag, cross, res) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    assert "not positive definite at this T: not a minimum" in msg and "pivot" in msg, msg
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.covariances(T)
    # a pair index N
    Tc = capi.chordal_init(m, n)
    assert raw_call(t, Tc, np.array([[1, n]]), diag, cross, res) == capi.ERR
    assert "outside" in capi.lib().dpgo_last_error().decode()
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    # T outside SE(3)
    Tb = Tc.copy()
    Tb[12 * 17] *= 1.001
    with pytest.raises(capi.DpgoError, match="pose 17 of T is not in SE"):
        t.covariances(Tb)
    # a graph cut in two by zero weights: every edge between the two robots
    for e in mp[mp["r1"] != mp["r2"]]:
        for a in (int(e["r1"]), int(e["r2"])):
            assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
    for a in t.ids:
        t.agents[a].clear_data_matrices()
    res.n = 5
    assert raw_call(t, Tc, pairs, diag, cross, res) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    assert "is not joined to pose 0 by edges of positive weight" in msg and msg.startswith("marginal_covariances"), msg
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    t.close()
    # the certificate's refusals
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N))
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.covariances(Tc)
    t.close()


def test_two_calls_give_the_same_bits_and_the_solver_is_untouched():
    """100 iterations of the bench configuration, two calls, 200 more iterations: X, Y and V bitwise those of the run
    without the calls"""
    outs = []
    for with_call in (False, True):
        t, m, n = team_at("sphere2500", 5, **BENCH)
        t.run(100)
        if with_call:
            pairs = np.array([[1, 2], [2499, 7], [0, 3]])
            T = capi.chordal_init(m, n)
            a1, d1, c1 = t.covariances(T, pairs)
            a2, d2, c2 = t.covariances(T, pairs)
            assert d1.tobytes() == d2.tobytes() and c1.tobytes() == c2.tobytes()
            assert (a1.logdet, a1.min_pivot, a1.max_pivot, a1.n) == (a2.logdet, a2.min_pivot, a2.max_pivot, a2.n)
            print("sphere2500 / 5 at the chordal T: %r" % a1)
        t.run(200)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_solve_certified_returns_the_covariances_on_request():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    prm = capi.default_params(r=5, num_robots=N, **RTR_NESTEROV)
    Tc = capi.chordal_init(m, n)
    plain = capi.solve_certified(mp, prm, r0=5, T=Tc, iters=300)
    assert sorted(plain) == sorted(["T", "r", "ranks", "certificate", "rounding", "f_relaxed", "f_rounded", "gap_rel",
                                    "escape_costs"])
    out = capi.solve_certified(mp, prm, r0=5, T=Tc, iters=300, covariances=True)
    assert sorted(out) == sorted(list(plain) + ["covariances"])
    assert out["T"].tobytes() == plain["T"].tobytes()
    res, diag = out["covariances"]
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    res2, diag2, _ = t.covariances(out["T"])
    t.close()
    assert diag.shape == (n, 6, 6) and diag.tobytes() == diag2.tobytes() and res.logdet == res2.logdet

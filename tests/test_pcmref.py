"""CPU checks of tests/pcmref.py, the reference of pairwise consistency maximisation: the Jacobians of all four
factors against central differences of the perturbed loop, that the bounds of the GPU and host tests reject the mistakes the
conventions invite, and the planted case that tests/test_gpu_consistency.py runs end to end."""
import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covref
from tests import gateref as G
from tests import pcmref as P

F = np.float64


@pytest.fixture(scope="module")
def planted():
    ma, Ta, mb, Tb, cand, is_true = P.planted_case()
    n = P.PLANTED["n"]
    Sa = covref.dense_reference(covref.q_full(ma, n), Ta, n)
    Sb = covref.dense_reference(covref.q_full(mb, n), Tb, n)
    assert Sa[2][0] > 0 and Sb[2][0] > 0
    i, j = P.endpoints(cand, {0: 0}, {0: 0})
    return dict(Ta=Ta, Tb=Tb, cand=cand, is_true=is_true, i=i, j=j, sig_a=P.sigma_from_dense(Ta, Sa[1]), sig_b=P.sigma_from_dense(Tb, Sb[1]))


def test_jacobians_match_central_differences(planted):
    """step h = 1e-6: truncation ~ h^2 |t| = 1e-11, round-off ~ u |t| / h ~ 2e-16 x 30 / 1e-6 = 6e-9: held to 5e-8"""
    c = planted
    h, worst = 1e-6, 0.0
    for k, l in ((0, 1), (2, 9), (5, 6)):
        Zk, Zl, A, B = P.pair_inputs(c["cand"], c["Ta"], c["Tb"], c["i"], c["j"], k, l, c["sig_a"], c["sig_b"], F)[:4]
        E0 = P.loop(Zk, Zl, A, B)
        Js = dict(zip("lAkB", P.jacobians(Zk, Zl, A, B, F)))

        def moved(which, x):
            X = dict(k=Zk, l=Zl, A=A, B=B)
            X[which] = P.perturb(X[which], x, F)
            E = P.loop(X["k"], X["l"], X["A"], X["B"])
            return np.r_[G.log_so3(E0[0].T @ E[0], F), E[1] - E0[1]]

        for which, J in Js.items():
            for q in range(6):
                x = np.zeros(6)
                x[q] = h
                d = (moved(which, x) - moved(which, -x)) / (2 * h)
                worst = max(worst, np.abs(d - J[:, q]).max())
    print("J against central differences: %.3e" % worst)
    assert worst <= 5e-8


def test_the_bounds_reject_the_mistakes(planted):
    """each wrong reading of the definitions, computed in float64 from the same inputs, must leave the bound on d2 (and, where
    it changes S, the elementwise bound on S) by more than 1000 x on every pair of true candidates tried"""
    c = planted
    cand, Ta, Tb, i, j = c["cand"], c["Ta"], c["Tb"], c["i"], c["j"]
    true = np.flatnonzero(c["is_true"])
    worst = {}

    def note(name, v):
        worst[name] = min(worst.get(name, np.inf), v)

    for k, l in [(int(true[a]), int(true[b])) for a, b in ((0, 1), (2, 5), (3, 11), (7, 15), (4, 9), (6, 12))]:
        if i[k] == i[l] or j[k] == j[l]:
            continue
        args = P.pair_inputs(cand, Ta, Tb, i, j, k, l, c["sig_a"], c["sig_b"])
        xi, d2, S = P.pair(*args)
        b_s, b_x, b_d = P.bounds(cand, Ta, Tb, i, j, k, l, args, xi, S, d2)
        a64 = P.pair_inputs(cand, Ta, Tb, i, j, k, l, c["sig_a"], c["sig_b"], F)
        Zk, Zl, A, B, SA, SB, Nk, Nl = a64
        # the float64 form itself stays inside
        x0, d0, S0 = P.pair(*a64, dtype=F)
        assert abs(d0 - float(d2)) <= b_d and (np.abs(S0 - np.asarray(S, dtype=F)) <= b_s).all()

        def off(xw, Sw):
            xw, Sw = np.asarray(xw, dtype=F), np.asarray(Sw, dtype=F)
            return abs(xw @ np.linalg.solve(Sw, xw) - float(d2)) / b_d, (np.abs(Sw - np.asarray(S, dtype=F)) / b_s).max()

        # k and l swapped in one factor: Z_k in the place of Z_l^-1's argument
        xw, _, Sw = P.pair(Zl, Zl, A, B, SA, SB, Nk, Nl, dtype=F)
        note("swapped_d2", off(xw, Sw)[0])
        # a segment taken in the reverse order
        Ar, SAr = P.segment(Ta, i[k], i[l], F), c["sig_a"](int(i[k]), int(i[l]))
        xw, _, Sw = P.pair(Zk, Zl, Ar, B, np.asarray(SAr, dtype=F), SB, Nk, Nl, dtype=F)
        r = off(xw, Sw)
        note("reversed_d2", r[0]); note("reversed_S", r[1])
        # Z_l not inverted
        E = P.mul(P.mul(P.mul(Zl, A), Zk), B)
        note("not_inverted_d2", off(P.coordinates(E, F), S)[0])
        # a flipped sign of a [.]x term
        Jl, JA, Jk, JB = P.jacobians(Zk, Zl, A, B, F)
        JA = JA.copy()
        JA[3:, :3] *= -1.0
        Sw = JA @ SA @ JA.T + JB @ SB @ JB.T + Jk @ Nk @ Jk.T + Jl @ Nl @ Jl.T
        r = off(xi, 0.5 * (Sw + Sw.T))
        note("cross_sign_d2", r[0]); note("cross_sign_S", r[1])
        # 1 / kappa in the place of 1 / (2 kappa)
        Nw = [np.diag(np.r_[np.full(3, 1 / float(cand[q]["kappa"])), np.full(3, 1 / float(cand[q]["tau"]))]) for q in (k, l)]
        _, _, Sw = P.pair(Zk, Zl, A, B, SA, SB, Nw[0], Nw[1], dtype=F)
        r = off(xi, Sw)
        note("kappa_d2", r[0]); note("kappa_S", r[1])
    print("smallest error / bound of each mistake:", {k: "%.3g" % v for k, v in worst.items()})
    assert len(worst) == 8
    for k, v in worst.items():
        assert v > 1e3, "the bound lets the mistake '%s' pass (error / bound %.3g)" % (k, v)


def test_planted_case_is_recovered_by_the_reference_alone(planted):
    c = planted
    D = np.asarray(P.d2_matrix(c["cand"], c["Ta"], c["Tb"], c["i"], c["j"], c["sig_a"], c["sig_b"], F))
    assert (D == D.T).all() and not D.diagonal().any()
    thr = capi.error_threshold_at_quantile(P.PLANTED["quantile"], 6)
    adj = D <= thr * thr
    np.fill_diagonal(adj, False)
    clique = P.max_clique_brute(adj)
    true = np.flatnonzero(c["is_true"])
    print("d2 among the true: max %.3g; true-outlier: min %.3g (threshold^2 %.3g)"
          % (D[np.ix_(true, true)].max(), D[np.ix_(true, ~c["is_true"])].min(), thr * thr))
    assert clique == true.tolist() and len(clique) == P.PLANTED["inliers"]
    for o in np.flatnonzero(~c["is_true"]):
        assert adj[o, true].sum() <= 1


def test_brute_force_clique():
    adj = np.zeros((6, 6), dtype=bool)
    for a, b in ((0, 1), (0, 2), (1, 2), (2, 3), (3, 4), (4, 5), (3, 5)):
        adj[a, b] = adj[b, a] = True
    assert P.max_clique_brute(adj) == [0, 1, 2]
    assert P.max_clique_brute(np.zeros((3, 3), dtype=bool)) == [0]

"""CPU checks of tests/auditref.py, the reference of the leave-one-out audit: the formula against an actual
leave-one-out solve of a linear Gaussian graph, Sigma_loo against the covariance of the SE(3) graph without the edge, the sum
identity of the redundancy numbers, that the bounds of tests/test_gpu_audit.py reject the wrong readings the definitions
invite, and the gap in p_min between bridges and the other edges that the GPU tests lean on."""
import numpy as np
import pytest

from tests import auditref as A
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G

F = np.float64
U = G.U
KAPPA, TAU = 100.0, 50.0


def linear_graph(seed):
    """8 nodes in R^6, node 0 fixed, 11 edges x_j - x_i = y_e + noise with W0_e = diag(s_e)^2: a ring and three chords, so no
    edge is a bridge.  Weights 1, fractions and, on a chord, 0."""
    rng = np.random.default_rng(seed)
    n = 8
    edges = [(k, (k + 1) % n) for k in range(n)] + [(0, 4), (2, 6), (1, 5)]
    x = rng.standard_normal((n, 6))
    x[0] = 0.0
    kap, tau = rng.uniform(50, 200, len(edges)), rng.uniform(20, 100, len(edges))
    w = np.array([1.0, 0.37, 1.0, 0.6, 1.0, 0.37, 1.0, 0.6, 0.0, 1.0, 1e-3])  # (an edge of weight 0 on the ring would make its neighbour a bridge)
    y = np.array([x[j] - x[i] for i, j in edges]) + 0.05 * rng.standard_normal((len(edges), 6))
    return n, edges, kap, tau, w, y


def linear_solve(n, edges, kap, tau, w, y):
    """(estimate [n, 6], Sigma of the nodes 1 .., cond_2 of the reduced Hessian)"""
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for (i, j), k, t, we, ye in zip(edges, kap, tau, w, y):
        W = we * np.asarray(A.scaling(k, t, F)) ** 2
        E = np.zeros((6, 6 * n))
        E[:, 6 * j:6 * j + 6], E[:, 6 * i:6 * i + 6] = np.eye(6), -np.eye(6)
        H += E.T @ (W[:, None] * E)
        b += E.T @ (W * ye)
    Hr = H[6:, 6:]
    S = np.linalg.inv(Hr)
    return np.r_[np.zeros(6), S @ b[6:]].reshape(n, 6), S, np.linalg.cond(Hr)


def linear_rel(S, i, j):
    blk = lambda a, b: np.zeros((6, 6)) if a == 0 or b == 0 else S[6 * (a - 1):6 * a, 6 * (b - 1):6 * b]
    return blk(i, i) + blk(j, j) - blk(i, j) - blk(j, i)


def test_linear_leave_one_out_identity():
    """For a linear graph the claim is exact: the audit's d2 of an edge is the gate's d2 of that edge against the solve without
    it.  Both sides come from float64 inverses of reduced Hessians H and H' (relative error of every block about u cond_2),
    and the audit divides by A, which multiplies a relative error by cond_2(A): the two sides agree within
    64 u (cond_2(H) + cond_2(H')) cond_2(A) d2.  The largest error / bound is printed; 1e-15 relative was seen."""
    n, edges, kap, tau, w, y = linear_graph(1)
    x, S, cH = linear_solve(n, edges, kap, tau, w, y)
    worst = worst_rel = 0.0
    for e, (i, j) in enumerate(edges):
        r = A.audit_from(linear_rel(S, i, j), x[j] - x[i] - y[e], kap[e], tau[e], w[e], dtype=F)
        assert r["testable"]
        keep = np.arange(len(edges)) != e
        x1, S1, cH1 = linear_solve(n, [edges[k] for k in np.flatnonzero(keep)], kap[keep], tau[keep], w[keep], y[keep])
        xi1 = x1[j] - x1[i] - y[e]
        want = xi1 @ np.linalg.solve(linear_rel(S1, i, j) + np.asarray(G.sigma_meas(kap[e], tau[e], F)), xi1)
        bound = 64 * U * (cH + cH1) * np.linalg.cond(np.asarray(r["A"], dtype=F)) * want
        worst, worst_rel = max(worst, abs(r["d2"] - want) / bound), max(worst_rel, abs(r["d2"] - want) / want)
        assert abs(r["d2"] - want) <= bound, (e, w[e], r["d2"], want)
        # the innovation and the covariance of the solve without the edge, too
        assert np.abs(r["xi_loo"] - xi1).max() <= bound / want * np.abs(xi1).max()
        assert np.abs(r["sigma_loo"] - linear_rel(S1, i, j)).max() <= bound / want * np.abs(r["sigma_loo"]).max()
        if w[e] == 0.0:
            assert r["rho"] == 1.0 and r["pmin"] == 1.0
    print("linear leave-one-out, %d edges: largest |d2 - gate of the re-solve| / bound %.3g, relative %.3g" % (len(edges), worst, worst_rel))


def chain_records(n, seed):
    """banded_chain(n, seed, window=8) with its dense reference: (m, T, Sigma, eigenvalues, references of every edge at its own
    weight with the exact measurement)"""
    m, T = NR.banded_chain(n, seed, window=8)
    _, Sigma, ev = covref.dense_reference(covref.q_full(m, n), T, n)
    refs = [A.audit(T, int(e["p1"]), int(e["p2"]), e["R"], e["t"], e["kappa"], e["tau"], e["weight"],
                    *G.blocks_of(Sigma, int(e["p1"]), int(e["p2"]))) for e in m]
    return m, T, Sigma, ev, refs


def loo_bound(T, n, i, j, ev, Sigma, ev1, Sigma1, r):
    """|Sigma_loo(formula on the full graph) - Sigma_rel(graph without the edge)|_F.  The covariance tests hold the blocks of a
    graph to B = 6 (n - 1) u cond_2(H_red) |Sigma|_F, so |d Sigma_rel|_F <= |[J_i J_j]|_2^2 B for either graph.  Through the
    formula: with D = diag(s), d(A^-1 C) = A^-1 dC A^-1 (because I + w A^-1 C = A^-1), so d Sigma_loo = G dSigma_rel G^T with
    G = D^-1 A^-1 D, whose norm grows like 1 / p_min: |G|_2^2 |J|_2^2 B(full), doubled for the terms beyond first order, plus
    |J|_2^2 B(reduced) of the other side"""
    Ji, Jj = G.jacobians(T, i, j, F)
    J2 = np.linalg.norm(np.c_[Ji, Jj], 2) ** 2
    B0 = 6 * (n - 1) * U * (ev[-1] / ev[0]) * np.linalg.norm(Sigma)
    B1 = 6 * (n - 1) * U * (ev1[-1] / ev1[0]) * np.linalg.norm(Sigma1)
    s = np.asarray(r["s"], dtype=F)
    Gm = np.linalg.inv(np.asarray(r["A"], dtype=F)) * np.outer(1 / s, s)
    return 2 * np.linalg.norm(Gm, 2) ** 2 * J2 * B0 + J2 * B1


@pytest.mark.parametrize("w", [1.0, 0.37])
def test_sigma_loo_is_the_relative_covariance_without_the_edge(w):
    """banded_chain(12, 2): for every edge that is not a bridge, at weight w in the graph, Sigma_loo from the blocks of the full
    graph against Sigma_rel from the dense inverse of the graph without the edge, within loo_bound"""
    n = 12
    m, T = NR.banded_chain(n, 2, window=8)
    worst, worst_rel, done = 0.0, 0.0, 0
    for e in range(len(m)):
        mw = m.copy()
        mw["weight"][e] = w
        _, Sigma, ev = covref.dense_reference(covref.q_full(mw, n), T, n)
        i, j = int(m["p1"][e]), int(m["p2"][e])
        r = A.audit(T, i, j, m["R"][e], m["t"][e], m["kappa"][e], m["tau"][e], w, *G.blocks_of(Sigma, i, j))
        if r["pmin"] < 1e-3:
            assert r["pmin"] < 1e-6  # a bridge
            continue
        _, Sigma1, ev1 = covref.dense_reference(covref.q_full(np.delete(m, e), n), T, n)
        assert ev1[0] > 0
        want = np.asarray(G.sigma_rel(T, i, j, *G.blocks_of(Sigma1, i, j)), dtype=F)
        err, bound = np.linalg.norm(np.asarray(r["sigma_loo"], dtype=F) - want), loo_bound(T, n, i, j, ev, Sigma, ev1, Sigma1, r)
        worst, worst_rel, done = max(worst, err / bound), max(worst_rel, err / np.linalg.norm(want)), done + 1
        assert err <= bound, (e, i, j, err, bound)
    assert done >= 8
    print("w = %g: Sigma_loo against the graph without the edge, %d edges: largest error / bound %.3g, relative %.3g" % (w, done, worst, worst_rel))


@pytest.mark.parametrize("n,seed", [(12, 2), (40, 3)])
def test_sum_identity_of_the_redundancy_numbers(n, seed):
    """sum_e w_e tr(C_e) = tr(H_red^-1 sum_e w_e J_e^T W0_e J_e) = tr(I) = 6 (n - 1), for weights that are those of the graph.
    Every tr(C_e) moves by at most 6 max(s^2) |J|_2^2 B with B the covariance tests' bound on the blocks"""
    m, T = NR.banded_chain(n, seed, window=8)
    rng = np.random.default_rng(seed)
    m["weight"] = rng.choice([1.0, 0.37, 1e-3, 1.0], len(m))
    m["weight"][:n - 1] = 1.0  # the odometry keeps the graph joined whatever the closures weigh
    _, Sigma, ev = covref.dense_reference(covref.q_full(m, n), T, n)
    B = 6 * (n - 1) * U * (ev[-1] / ev[0]) * np.linalg.norm(Sigma)
    total, bound = 0.0, 0.0
    for e in m:
        i, j = int(e["p1"]), int(e["p2"])
        r = A.audit(T, i, j, e["R"], e["t"], e["kappa"], e["tau"], e["weight"], *G.blocks_of(Sigma, i, j))
        total += float(e["weight"] * np.trace(r["C"]))
        assert abs(float(r["rho"]) - (1 - e["weight"] * float(np.trace(r["C"])) / 6)) <= 1e-15
        Ji, Jj = G.jacobians(T, i, j, F)
        bound += e["weight"] * 6 * max(2 * e["kappa"], e["tau"]) * np.linalg.norm(np.c_[Ji, Jj], 2) ** 2 * B
    print("n = %d: sum w tr(C) = %.15g, 6 (n - 1) = %d, difference / bound %.3g" % (n, total, 6 * (n - 1), abs(total - 6 * (n - 1)) / bound))
    assert abs(total - 6 * (n - 1)) <= bound


def wrong_d2(Sr, xi, kappa, tau, w, a_sign=-1.0, drop_b=False, half=2.0):
    """d2 and Sigma_loo in float64 with one reading changed: the sign in A, B^-1 left out, 1 / kappa for 1 / (2 kappa)"""
    s = np.r_[np.full(3, np.sqrt(half * kappa)), np.full(3, np.sqrt(tau))]
    z, Cm = s * np.asarray(xi, dtype=F), np.asarray(Sr, dtype=F) * np.outer(s, s)
    Am, Bm = np.eye(6) + a_sign * w * Cm, np.eye(6) + (1 - w) * Cm
    u = np.linalg.solve(Am, z)
    X = np.linalg.solve(Am, Cm)
    return u @ (u if drop_b else np.linalg.solve(Bm, z)), (X + X.T) / 2 / np.outer(s, s)


def test_the_bounds_reject_the_wrong_readings():
    """the bounds of tests/test_gpu_audit.py (auditref.record_bounds) against six wrong readings of the definitions, each in
    float64 from the same blocks, on testable records with w = 0.37 and a residual of 0.3 rad: every one must leave the bound
    on d2 by more than 1000 x on every record, and those that change Sigma_loo its bound as well"""
    n, w = 40, 0.37
    m, T, Sigma, ev, refs = chain_records(n, 3)
    rng = np.random.default_rng(6)
    worst = {}
    done = 0
    for e, r0 in zip(m, refs):
        if r0["pmin"] < 1e-3:
            continue
        done += 1
        i, j = int(e["p1"]), int(e["p2"])
        blocks = G.blocks_of(Sigma, i, j)
        Rm = np.asarray(e["R"]).reshape(3, 3) @ covref.exp_so3(0.3 * rng.standard_normal(3) / np.sqrt(3)).T
        tm = e["t"] + 0.1 * rng.standard_normal(3)
        r = A.audit(T, i, j, Rm, tm, KAPPA, TAU, w, *blocks)
        b = A.record_bounds(T, i, j, tm, *blocks, r)
        Sr, xi = np.asarray(r["sigma_rel"], dtype=F), np.asarray(r["xi"], dtype=F)
        Sji = G.sigma_rel(T, j, i, blocks[1], blocks[0], np.asarray(blocks[2]).T, F)
        readings = dict(w_as_1=wrong_d2(Sr, xi, KAPPA, TAU, 1.0), w_swapped=wrong_d2(Sr, xi, KAPPA, TAU, 1 - w),
                        a_plus=wrong_d2(Sr, xi, KAPPA, TAU, w, a_sign=1.0), b_dropped=wrong_d2(Sr, xi, KAPPA, TAU, w, drop_b=True),
                        kappa=wrong_d2(Sr, xi, KAPPA, TAU, w, half=1.0),
                        ij_swapped=wrong_d2(Sji, G.innovation(T, j, i, Rm, tm, F), KAPPA, TAU, w))
        # (the right reading in the same float64 arithmetic stays inside: the ratios below are not an artefact of wrong_d2)
        d2, sl = wrong_d2(Sr, xi, KAPPA, TAU, w)
        assert abs(d2 - float(r["d2"])) <= b["d2"] and (np.abs(sl - np.asarray(r["sigma_loo"], dtype=F)) <= b["sigma_loo"]).all()
        for k, (d2, sl) in readings.items():
            rd = abs(d2 - float(r["d2"])) / b["d2"]
            worst[k + "_d2"] = min(worst.get(k + "_d2", np.inf), rd)
            if k != "b_dropped":
                rs = (np.abs(sl - np.asarray(r["sigma_loo"], dtype=F)) / b["sigma_loo"]).max()
                worst[k + "_sigma_loo"] = min(worst.get(k + "_sigma_loo", np.inf), rs)
    assert done >= 30
    print("smallest error / bound of each wrong reading over %d records:" % done, {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v > 1e3, "the bound lets the reading '%s' pass (error / bound %.3g)" % (k, v)


def test_bridges_and_the_other_edges_are_far_apart():
    """banded_chain(40, 3), every edge at weight 1: p_min of a bridge is round-off (about u cond_2(H_red), either sign), that of
    every other edge well above it.  None lies in (1e-6, 1e-3): the GPU tests call the edges below 1e-6 untestable and hold
    the bounds on those above 1e-3.  The bridges are the edges whose removal disconnects the graph (union-find)."""
    n = 40
    m, T, Sigma, ev, refs = chain_records(n, 3)
    pm = np.array([float(r["pmin"]) for r in refs])
    print("n = %d, cond_2(H_red) = %.3g: p_min of the %d edges:" % (n, ev[-1] / ev[0], len(m)), " ".join("%.3g" % p for p in pm))
    assert not ((pm > 1e-6) & (pm < 1e-3)).any()

    def joined(skip):
        root = list(range(n))

        def find(a):
            while root[a] != a:
                a = root[a]
            return a
        for k, e in enumerate(m):
            if k != skip:
                root[find(int(e["p1"]))] = find(int(e["p2"]))
        return len({find(a) for a in range(n)}) == 1

    bridge = np.array([not joined(k) for k in range(len(m))])
    assert bridge.sum() >= 3 and (bridge == (pm <= 1e-6)).all()
    print("%d bridges, |p_min| <= %.3g; the other edges p_min >= %.3g" % (bridge.sum(), np.abs(pm[bridge]).max(), pm[~bridge].min()))

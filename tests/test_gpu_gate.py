"""GPU checks of the Mahalanobis gate of candidate measurements (csrc/gate.hip, Team.gate / Team.relative_covariances /
Team.zero_weight_measurements).

The graphs are covnested_ref.banded_chain(n, seed, window=8): noise-free, the ground truth is an exact minimum, no solve.

Bounds (u = 2.2e-16; the functions are in tests/gateref.py, and tests/test_gateref.py shows that they reject a swapped pair, a
transposed cross block, a flipped [t_ij]x and a wrong noise model):
  the kernel alone, against gateref in longdouble on the blocks the covariance call returns for the same pairs --
    |Sigma_rel - ref| <= 32 u (|J| |Sigma_12| |J|^T) elementwise: two 12-term products, gamma_24 and a third over;
    |xi_t - ref| <= 16 u (|t_i| + |t_j| + |t~|);  |xi_R - ref| <= 64 u / sin 3.0 for residual angles up to 3.0 rad, a zero
    residual gives |xi_R| <= 1e-15, the residual of exactly pi a finite vector with ||xi_R| - pi| <= 1e-6;
    d2: both bounds propagated to first order through xi^T S^-1 xi, plus 100 u cond_2(S) d2 for the 6 x 6 solve;
  end to end, against the numpy inverse of the dense reduced Hessian --
    B = 6 (n - 1) u cond_2(H_red) |Sigma|_F is what the covariance tests hold the blocks to; |Sigma_rel - ref|_F <= |[J_i J_j]|_2^2 B
    and |d2 - ref| <= |S^-1 xi|^2 |[J_i J_j]|_2^2 B + 100 u cond_2(S) d2.
Every test prints its largest error / bound."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests.test_gpu_covariance import BENCH
from tests.test_gpu_covariance_nested import team_of

pytestmark = pytest.mark.gpu

U = G.U
KAPPA, TAU = 100.0, 50.0
PI_AXIS = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
COUNTS = (1, 63, 64, 65, 255, 256, 257, 70001)
NESTED_BLOCK = 6


def offsets(n, N):
    rob = NR.robots_of(n, N)
    return rob, np.array([int(np.argmax(rob == a)) for a in range(N)] + [n])


def candidates(T, n, N, pairs, angles, seed, t_noise=0.05):
    """one candidate per pair (team poses i -> j): R~ = R_ij Exp(angle a)^T for a seeded unit axis a, so that the residual
    rotation R~^T R_ij is Exp(angle a); angle 0 is the exact relative pose (translation included), np.pi the rotation by
    exactly pi about PI_AXIS"""
    rng = np.random.default_rng(seed)
    rob, offs = offsets(n, N)
    c = np.zeros(len(pairs), dtype=capi.MEAS_DTYPE)
    for k, ((i, j), th) in enumerate(zip(pairs, angles)):
        Rij, tij = G.relative_pose(T, i, j, np.float64)
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        if th == np.pi:
            Rm = Rij @ (2.0 * np.outer(PI_AXIS, PI_AXIS) - np.eye(3))
        else:
            Rm = Rij @ covref.exp_so3(th * a).T if th else Rij
        tm = tij + (t_noise * rng.standard_normal(3) if th else 0.0)
        c[k]["r1"], c[k]["p1"], c[k]["r2"], c[k]["p2"] = rob[i], i - offs[rob[i]], rob[j], j - offs[rob[j]]
        c[k]["R"], c[k]["t"] = Rm.reshape(-1), tm
        c[k]["kappa"], c[k]["tau"] = KAPPA * rng.uniform(0.5, 2.0), TAU * rng.uniform(0.5, 2.0)
        c[k]["weight"] = rng.uniform()  # ignored
    return c


def blocks_call(t, T, pairs, method):
    if method == "nested":
        return t.covariances_nested(T, pairs, max_block=NESTED_BLOCK)
    return t.covariances(T, pairs, method=method)


def gate_call(t, cand, T, method, max_block=NESTED_BLOCK, **kw):
    return t.gate(cand, T, method=method, max_block=max_block if method == "nested" else None, **kw)


def base_pairs(n, N, block_of, seed):
    """the unique pairs of test 1: both orders, an endpoint that is pose 0 both ways round, two poses of one robot and of two,
    and under nested interior-separator (both ways) and separator-separator pairs"""
    rng = np.random.default_rng(seed)
    rob, offs = offsets(n, N)
    out = [(0, 5), (5, 0), (0, n - 1), (n - 1, 0), (3, 17), (17, 3), (1, 2), (2, 1)]
    out += [(offs[a] + 1, offs[a + 1] - 1) for a in range(N)]  # one robot
    out += [(offs[a] + 2, offs[a + 1] + 1) for a in range(N - 1)]  # two robots
    if block_of is not None:
        sep, inner = np.flatnonzero(block_of == -1), np.flatnonzero(block_of >= 0)
        assert len(sep) >= 2 and len(inner) >= 2
        out += [(inner[0], sep[0]), (sep[-1], inner[-1]), (sep[0], sep[-1]), (sep[1], sep[0])]
    while len(out) < 120:
        i, j = rng.integers(0, n, 2)
        if i != j:
            out.append((int(i), int(j)))
    seen, uniq = set(), []
    for p in out:
        p = (int(p[0]), int(p[1]))
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return np.array(uniq, dtype=np.int32)


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_kernel_against_the_reference_at_lane_and_launch_edges(N, method):
    n = 40
    m, T = NR.banded_chain(n, 3, window=8)
    t = team_of(m, n, N, T)
    block_of = None
    if method == "nested":
        block_of, info = t.covariance_plan(NESTED_BLOCK)
        assert info["promoted_poses"] > 0, info
    pairs = base_pairs(n, N, block_of, seed=7)
    P = len(pairs)
    angles = [(0.0, 1e-9, 0.3, 3.0)[k % 4] for k in range(P)]
    angles[8] = np.pi
    cand = candidates(T, n, N, pairs, angles, seed=11)
    # the reference, once: gateref in longdouble on the blocks the covariance call returns for the same pairs
    _, diag, cross = blocks_call(t, T, pairs, method)
    ref = []
    for k, (i, j) in enumerate(pairs):
        xi, d2, Sr, S = G.gate(T, i, j, cand[k]["R"], cand[k]["t"], cand[k]["kappa"], cand[k]["tau"], diag[i], diag[j], cross[k])
        b_s, b_x = G.sigma_rel_bound(T, i, j, diag[i], diag[j], cross[k]), G.xi_bound(T, i, j, cand[k]["t"])
        ref.append((np.asarray(xi, dtype=np.float64), float(d2), np.asarray(Sr, dtype=np.float64), b_s, b_x,
                    G.d2_bound(xi, S, d2, b_x, b_s), np.linalg.cond(np.asarray(S, dtype=np.float64))))
    rxi, rd2, rS = np.array([r[0] for r in ref]), np.array([r[1] for r in ref]), np.array([r[2] for r in ref])
    bS, bx, bd = np.array([r[3] for r in ref]), np.array([r[4] for r in ref]), np.array([r[5] for r in ref])
    ang = np.array(angles)
    print("%d robots, %s: %d unique pairs, cond_2(S) <= %.3g" % (N, method, P, max(r[6] for r in ref)))
    worst = dict(sigma_rel=0.0, xi_t=0.0, xi_R=0.0, d2=0.0, xi_R_zero=0.0, pi=0.0)
    rng = np.random.default_rng(5)
    for K in COUNTS:
        # every unique candidate as far as K reaches, then seeded repeats: duplicates at every count above P
        idx = np.r_[np.arange(min(K, P)), rng.integers(0, P, max(K - P, 0))]
        if K < P:
            idx = rng.permutation(P)[:K]
        res, xi, d2, accept, sg = gate_call(t, cand[idx], T, method, sigma_rel=True)
        assert xi.shape == (K, 6) and d2.shape == (K,) and sg.shape == (K, 6, 6) and accept.shape == (K,)
        assert res.n == 6 * (n - 1) and res.min_pivot > 0
        worst["sigma_rel"] = max(worst["sigma_rel"], (np.abs(sg - rS[idx]) / bS[idx]).max())
        assert (np.abs(sg - rS[idx]) <= bS[idx]).all()
        assert sg.tobytes() == np.ascontiguousarray(sg.transpose(0, 2, 1)).tobytes(), "sigma_rel is not bitwise symmetric"
        worst["xi_t"] = max(worst["xi_t"], (np.abs(xi[:, 3:] - rxi[idx, 3:]) / bx[idx, 3:]).max())
        assert (np.abs(xi[:, 3:] - rxi[idx, 3:]) <= bx[idx, 3:]).all()
        a = ang[idx]
        upto3, zero, pi = a <= 3.0, a == 0.0, a == np.pi
        worst["xi_R"] = max(worst["xi_R"], (np.abs(xi[upto3, :3] - rxi[idx][upto3, :3]) / bx[idx][upto3, :3]).max())
        assert (np.abs(xi[upto3, :3] - rxi[idx][upto3, :3]) <= bx[idx][upto3, :3]).all()
        if zero.any():
            worst["xi_R_zero"] = max(worst["xi_R_zero"], np.abs(xi[zero, :3]).max())
            assert np.abs(xi[zero, :3]).max() <= 1e-15
        if pi.any():
            assert np.isfinite(xi[pi]).all() and np.isfinite(d2[pi]).all()
            worst["pi"] = max(worst["pi"], np.abs(np.linalg.norm(xi[pi, :3], axis=1) - np.pi).max())
            assert np.abs(np.linalg.norm(xi[pi, :3], axis=1) - np.pi).max() <= 1e-6
        worst["d2"] = max(worst["d2"], (np.abs(d2[upto3] - rd2[idx][upto3]) / bd[idx][upto3]).max())
        assert (np.abs(d2[upto3] - rd2[idx][upto3]) <= bd[idx][upto3]).all()
        assert (accept == (np.sqrt(d2) <= capi.error_threshold_at_quantile(0.99, 6))).all()
        # duplicates: the bits of the first occurrence
        first = np.full(P, -1)
        first[idx[::-1]] = np.arange(K)[::-1]
        f = first[idx]
        if K > P:
            assert (f != np.arange(K)).any()
        assert xi.tobytes() == xi[f].tobytes() and d2.tobytes() == d2[f].tobytes() and sg.tobytes() == sg[f].tobytes()
        if K == 257:
            rel = t.relative_covariances(pairs[idx], T, method=method, max_block=NESTED_BLOCK if method == "nested" else None)
            assert rel.tobytes() == sg.tobytes()
    print("largest error / bound: sigma_rel %.3g, xi_t %.3g, xi_R %.3g, d2 %.3g; |xi_R| at zero residual %.3g, ||xi_R| - pi| %.3g"
          % (worst["sigma_rel"], worst["xi_t"], worst["xi_R"], worst["d2"], worst["xi_R_zero"], worst["pi"]))
    t.close()


def end_to_end_bounds(T, n, i, j, Hr_eigs, Sref, xi, S, d2):
    """(bound on |Sigma_rel - ref|_F, bound on |d2 - ref|)"""
    B = 6 * (n - 1) * U * (Hr_eigs[-1] / Hr_eigs[0]) * np.linalg.norm(Sref)
    Ji, Jj = G.jacobians(T, i, j, np.float64)
    J2 = np.linalg.norm(np.c_[Ji, Jj], 2) ** 2
    S = np.asarray(S, dtype=np.float64)
    w = np.linalg.solve(S, np.asarray(xi, dtype=np.float64))
    return J2 * B, (w @ w) * J2 * B + 100 * U * np.linalg.cond(S) * float(d2)


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_end_to_end_against_the_dense_numpy_inverse(method):
    n, N, K = 12, 2, 200
    m, T = NR.banded_chain(n, 4, window=8)
    Hr, Sref, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    rng = np.random.default_rng(9)
    pairs = []
    while len(pairs) < K:
        i, j = rng.integers(0, n, 2)
        if i != j:
            pairs.append((int(i), int(j)))
    cand = candidates(T, n, N, pairs, rng.uniform(0.01, 1.0, K), seed=13, t_noise=0.2)
    t = team_of(m, n, N, T)
    if method == "nested":
        assert t.covariance_plan(2)[1]["promoted_poses"] > 0
    res, xi, d2, accept, sg = gate_call(t, cand, T, method, max_block=2, sigma_rel=True)
    worst_s = worst_d = 0.0
    for k, (i, j) in enumerate(pairs):
        rxi, rd2, rS, S = G.gate(T, i, j, cand[k]["R"], cand[k]["t"], cand[k]["kappa"], cand[k]["tau"], *G.blocks_of(Sref, i, j))
        bs, bd = end_to_end_bounds(T, n, i, j, w, Sref, rxi, S, rd2)
        es, ed = np.linalg.norm(sg[k] - np.asarray(rS, dtype=np.float64)), abs(d2[k] - float(rd2))
        worst_s, worst_d = max(worst_s, es / bs), max(worst_d, ed / bd)
        assert es <= bs and ed <= bd, (k, i, j, es, bs, ed, bd)
    print("%s, n = %d, cond_2(H_red) = %.3e: largest error / bound: sigma_rel %.3g, d2 %.3g (d2 in [%.3g, %.3g], %d accepted)"
          % (method, n, w[-1] / w[0], worst_s, worst_d, d2.min(), d2.max(), accept.sum()))
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_a_leaf_edge_has_its_own_measurement_noise(method):
    """a pose joined to the graph by a single edge: the relative pose across that edge is known exactly as well as the edge
    says, Sigma_rel = Sigma_meas of the edge -- first principles, no reference code in the expected value"""
    n0, N = 12, 2
    m0, T0 = NR.banded_chain(n0, 6, window=8)
    _, Tx = NR.banded_chain(n0 + 1, 60, window=8)  # (a random extra pose)
    n = n0 + 1
    T = np.r_[T0, Tx[-12:]]
    Rij, tij = G.relative_pose(T, n0 - 1, n0, np.float64)
    e = np.zeros(1, dtype=capi.MEAS_DTYPE)
    e["p1"], e["p2"], e["R"], e["t"], e["kappa"], e["tau"], e["weight"] = n0 - 1, n0, Rij.reshape(-1), tij, 37.0, 11.0, 1.0
    m = np.concatenate([m0, e])
    _, Sref, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    t = team_of(m, n, N, T)
    rel = t.relative_covariances([(n0 - 1, n0)], T, method=method, max_block=2 if method == "nested" else None)
    want = np.asarray(G.sigma_meas(37.0, 11.0), dtype=np.float64)
    bound, _ = end_to_end_bounds(T, n, n0 - 1, n0, w, Sref, np.zeros(6), np.eye(6), 0.0)
    err = np.linalg.norm(rel[0] - want)
    print("%s: |Sigma_rel - Sigma_meas|_F = %.3e (bound %.3e, ratio %.3g)" % (method, err, bound, err / bound))
    assert err <= bound
    t.close()


def random_outliers(T, n, pairs, seed):
    """tests.util.add_outliers for given endpoints: R uniform on SO(3), t uniform in the bounding box of the trajectory"""
    rng = np.random.default_rng(seed)
    tr = np.asarray(T).reshape(n, 4, 3)[:, 3, :]
    lo, hi = tr.min(0), tr.max(0)
    out = np.zeros(len(pairs), dtype=capi.MEAS_DTYPE)
    for k, (i, j) in enumerate(pairs):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        Q *= np.sign(np.linalg.det(Q))
        out[k]["p1"], out[k]["p2"] = i, j
        out[k]["R"], out[k]["t"] = Q.reshape(-1), lo + rng.random(3) * (hi - lo)
        out[k]["kappa"], out[k]["tau"], out[k]["weight"] = KAPPA, TAU, 1.0
    return out


def test_planted_outliers_are_rejected_and_exact_closures_accepted():
    n, N = 40, 2
    m0, T = NR.banded_chain(n, 8, window=8)
    rng = np.random.default_rng(21)
    pairs = set()
    while len(pairs) < 20:  # longer than the window: no edge of the graph joins such a pair
        i, j = sorted(int(x) for x in rng.integers(0, n, 2))
        if j - i > 8:
            pairs.add((i, j))
    pairs = sorted(pairs)
    exact = np.zeros(10, dtype=capi.MEAS_DTYPE)
    for k, (i, j) in enumerate(pairs[:10]):
        Rij, tij = G.relative_pose(T, i, j, np.float64)
        exact[k]["p1"], exact[k]["p2"], exact[k]["R"], exact[k]["t"] = i, j, Rij.reshape(-1), tij
        exact[k]["kappa"], exact[k]["tau"], exact[k]["weight"] = KAPPA, TAU, 1.0
    planted = np.concatenate([exact, random_outliers(T, n, pairs[10:], seed=22)])
    m = np.concatenate([m0, planted])
    mp = capi.partition(m, n, N)
    t = team_of(m, n, N, T)
    for e in mp[len(m0):]:
        for a in {int(e["r1"]), int(e["r2"])}:
            assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
            t.agents[a].clear_data_matrices()
    zw = t.zero_weight_measurements()
    key = lambda q: sorted((int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"])) for e in q)
    assert len(zw) == 20 and key(zw) == key(mp[len(m0):])
    for method in ("dense", "schur"):
        res, xi, d2, accept = t.gate(zw, T, method=method)
        explicit = zw.copy()
        explicit["weight"], explicit["fixed_weight"] = 1.0, 0  # (ignored)
        _, xi2, d22, accept2 = t.gate(explicit, T, method=method)
        assert xi.tobytes() == xi2.tobytes() and d2.tobytes() == d22.tobytes() and (accept == accept2).all()
        rob, offs = offsets(n, N)
        is_exact = np.array([(int(offs[e["r1"]] + e["p1"]), int(offs[e["r2"]] + e["p2"])) in pairs[:10] for e in zw])
        assert is_exact.sum() == 10
        print("%s: d2 of the exact closures <= %.3g, of the outliers >= %.3g (threshold^2 %.3g)"
              % (method, d2[is_exact].max(), d2[~is_exact].min(), capi.error_threshold_at_quantile(0.99, 6) ** 2))
        assert (d2[is_exact] <= 1e-20).all() and accept[is_exact].all()
        assert not accept[~is_exact].any()
    t.close()


def raw_gate(t, T, method, max_block, cand, xi, d2, sg, res, num=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return capi.lib().dpgo_team_gate_candidates(t.h, p(T), method, max_block, len(cand) if num is None else num, p(cand), p(xi), p(d2),
                                                p(sg), C.byref(res))


def test_refusals_leave_the_outputs_untouched():
    n, N = 40, 2
    m, T = NR.banded_chain(n, 3, window=8)
    t = team_of(m, n, N, T)
    pairs = [(3, 17), (30, 2)]
    good = candidates(T, n, N, pairs, [0.3, 0.3], seed=1)
    xi, d2, sg, res = np.full((2, 6), 7.25), np.full(2, 7.25), np.full((2, 6, 6), 7.25), capi.Covariance()

    def refused(what, cand=good, method=capi.GATE_DENSE, T_=T, xi_=xi, d2_=d2, sg_=sg, num=None, max_block=0):
        res.n = 5
        rc = raw_gate(t, T_, method, max_block, cand, xi_, d2_, sg_, res, num)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg, (rc, msg)
        assert (xi == 7.25).all() and (d2 == 7.25).all() and (sg == 7.25).all()
        return msg

    refused("num must be positive", num=0)
    refused("num must be positive", num=-3)
    refused("no output requested", xi_=None, d2_=None, sg_=None)
    refused("exactly one of them is null", xi_=None)
    refused("exactly one of them is null", d2_=None)
    refused("method must be", method=3)
    refused("method must be", method=-1)

    def changed(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k][1] = v
        return c

    refused("candidate 1 names robot 2, which is not in the team", changed(r2=2))
    refused("candidate 1 names pose 20 of robot 0", changed(p2=20))
    refused("candidate 1 names pose -1 of robot 1", changed(p1=-1))
    refused("candidate 1 joins a pose to itself", changed(r2=good["r1"][1], p2=good["p1"][1]))
    refused("both must be positive", changed(kappa=0.0))
    refused("both must be positive", changed(tau=-1.0))
    bad = good.copy()
    bad["R"][1][0] *= 1.001
    refused("the measurement of candidate 1 is not in SE(3)", bad)
    # the relative-covariance query reads the endpoints alone: the same records pass
    sg2, res2 = np.zeros((2, 6, 6)), capi.Covariance()
    assert raw_gate(t, T, capi.GATE_DENSE, 0, changed(kappa=0.0), None, None, sg2, res2) == capi.OK and sg2.any() and res2.n == 6 * (n - 1)
    assert raw_gate(t, T, capi.GATE_DENSE, 0, bad, None, None, sg2, res2) == capi.OK
    # carried over from the covariance path, with its own message: T outside SE(3), and per method a T that is no minimum
    Tb = T.copy()
    Tb[12 * 17] *= 1.001
    refused("pose 17 of T is not in SE", T_=Tb)
    Ts = NR.spoil_rotations(T, n, [9, 10, 11, 28, 29], 50)
    w = np.linalg.eigvalsh(covref.reduced(covref.hessian(covref.q_full(m, n), Ts, n)).toarray())
    assert w[0] < -1e-3 * w[-1], "the spoiled trajectory is still a minimum"
    for method, mb in ((capi.GATE_DENSE, 0), (capi.GATE_SCHUR, 0), (capi.GATE_NESTED, NESTED_BLOCK)):
        msg = refused("non-positive pivot", T_=Ts, method=method, max_block=mb)
        assert "not a minimum" in msg and msg.startswith("marginal_covariances"), msg
        assert bytes(res) == bytes(capi.Covariance())
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.gate(good, Ts)
    with pytest.raises(ValueError, match="method must be"):
        t.gate(good, T, method="sparse")
    t.close()


def test_two_calls_give_the_same_bits_and_no_solver_state_changes():
    """two calls give the same bits under every method; a gate in front of the first run and another after 20 iterations leave
    X, Y and V after 50 more iterations bitwise those of the run without them.  The form of the other side-effect tests
    (test_gpu_covariance.py): the bench configuration, one team after the other, each closed before the next.  Two RTR runs
    are not comparable bit for bit: a team whose one-launch RTR solve nobody has waited for yet holds the device's lock
    (solve.hip, acquire_fused_rtr_lock), and another team -- or another process on the same GPU -- then takes the
    launch-per-step sequence, whose sums are ordered differently"""
    n, N = 40, 2
    m, T = NR.banded_chain(n, 3, window=8)
    rng = np.random.default_rng(2)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, n, (300, 2)) if i != j]
    cand = candidates(T, n, N, pairs, rng.uniform(0.0, 3.0, len(pairs)), seed=3)
    # a start away from the minimum, so that the runs move
    T0 = covref.perturb(T, 0.05 * np.random.default_rng(4).standard_normal(6 * n), n)
    mp = capi.partition(m, n, N)

    def gate_twice(t):
        for method in ("dense", "schur", "nested"):
            one = gate_call(t, cand, T, method, sigma_rel=True)
            two = gate_call(t, cand, T, method, sigma_rel=True)
            for x, y in zip(one[1:], two[1:]):
                assert x.tobytes() == y.tobytes()
            assert (one[0].logdet, one[0].min_pivot, one[0].max_pivot) == (two[0].logdet, two[0].min_pivot, two[0].max_pivot)

    outs = []
    for with_gate in (False, True):
        t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **BENCH))
        t.set_initial(T0, capi.fixed_stiefel(5))
        if with_gate:
            gate_twice(t)
        t.run(20)
        if with_gate:
            gate_twice(t)
        t.run(50)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()

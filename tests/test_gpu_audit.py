"""GPU checks of the leave-one-out audit of measurements that are in the graph (csrc/audit.hip, Team.audit /
Team.measurements_once).

The graphs are covnested_ref.banded_chain(n, seed, window=8): noise-free, the ground truth is an exact minimum, no solve.
banded_chain(40, 3) has 49 edges, 11 of them bridges; tests/test_auditref.py shows that p_min of a bridge at full weight is
round-off (|p_min| <= 4.1e-12 in the dense reference) and that of every other edge >= 0.0077, so "p_min < 1e-6" and
"p_min > 1e-3" of the reference name the two kinds, and nothing lies between.

Bounds (u = 2.2e-16; the functions are in tests/auditref.py with their derivation, and tests/test_auditref.py shows that they
reject a wrong weight, w and 1 - w swapped, a wrong sign in A, a dropped B^-1, a wrong noise model and a swapped pair):
  the kernel alone, against auditref in longdouble on the blocks the covariance call returns for the same pairs --
    xi as the gate's (gateref.xi_bound); xi_loo, d2, rho, p_min, Sigma_loo by auditref.record_bounds on the records with
    p_min > 1e-3; on the bridges testable is False, d2 = +inf, xi_loo = 0, Sigma_loo = 0 and rho within auditref.rho_bound of the
    reference, and |rho| itself within the end-to-end bound max(2 kappa, tau) |[J_i J_j]|_2^2 B of zero;
  end to end -- B = 6 (n - 1) u cond_2(H_red) |Sigma|_F is what the covariance tests hold the blocks of a graph to;
    Sigma_loo against the relative covariance of a second team without the edge: tests.test_auditref.loo_bound (B of both
    graphs through |[J_i J_j]|_2^2 and the amplification |D^-1 A^-1 D|_2^2, which grows like 1 / p_min);
    sum_e w_e 6 (1 - rho_e) = 6 (n - 1) within sum_e w_e^2 max(2 kappa, tau) |[J_i J_j]|_2^2 B.
Every test prints its largest error / bound."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import auditref as A
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests.test_auditref import loo_bound
from tests.test_gpu_covariance_nested import RTR_NESTEROV, team_of
from tests.test_gpu_gate import COUNTS, NESTED_BLOCK, blocks_call, offsets
from tests.util import DATA

pytestmark = pytest.mark.gpu

F = np.float64
U = G.U
WEIGHTS = (1.0, 0.37, 0.0, 1e-3, 1.0)
ANGLES = (0.0, 1e-9, 0.3, 3.0)
SCALES = ((1.0, 1.0), (1.0, 1.0), (0.5, 0.25), (0.25, 0.5), (1.0, 1.0))  # (kappa, tau) by round; at most 1: see records()


@functools.lru_cache(maxsize=None)
def dense(n, seed):
    """(m, T, Sigma, eigenvalues of H_red) of banded_chain(n, seed, window=8), once"""
    m, T = NR.banded_chain(n, seed, window=8)
    _, Sigma, ev = covref.dense_reference(covref.q_full(m, n), T, n)
    assert ev[0] > 0
    return m, T, Sigma, ev


def team_pairs(t, meas, n, N):
    """the team-order poses (i, j) of records in the robots' numbering"""
    _, offs = offsets(n, N)
    return np.array([(int(offs[e["r1"]] + e["p1"]), int(offs[e["r2"]] + e["p2"])) for e in meas], dtype=np.int32)


def records(base, rounds, seed):
    """len(base) * rounds records: the team's own measurements over and over with R~ turned by a residual angle of ANGLES about
    a seeded axis, t~ moved, kappa and tau scaled by SCALES and the weight taken from WEIGHTS, so that every edge meets every
    weight.  The scales are at most 1: a record that claims more information than the graph holds for its edge has no PSD A.
    Changing the record does not change T, and the kernel does not care.  Returns (records, angles, index into base)"""
    rng = np.random.default_rng(seed)
    L = len(base)
    rec = np.tile(base, rounds)
    ang = np.zeros(len(rec))
    for k in range(len(rec)):
        r, q = divmod(k, L)
        th = ANGLES[k % 4]
        a = rng.standard_normal(3)
        R = np.asarray(rec[k]["R"]).reshape(3, 3)
        if th:
            rec[k]["R"] = (R @ covref.exp_so3(th * a / np.linalg.norm(a)).T).reshape(-1)
            rec[k]["t"] = rec[k]["t"] + 0.05 * rng.standard_normal(3)
        rec[k]["kappa"], rec[k]["tau"] = rec[k]["kappa"] * SCALES[r % 5][0], rec[k]["tau"] * SCALES[r % 5][1]
        rec[k]["weight"] = WEIGHTS[(r + q) % 5]
        rec[k]["fixed_weight"], rec[k]["is_known_inlier"] = k % 2, k % 3 == 0  # ignored
        ang[k] = th
    return rec, ang, np.arange(len(rec)) % L


def audit_call(t, rec, T, method, max_block=NESTED_BLOCK, **kw):
    return t.audit(rec, T, method=method, max_block=max_block if method == "nested" else None, **kw)


def reference(T, pr, rec, diag, cross_of):
    """per record: (the longdouble reference, its bounds or None where the reference is not testable above 1e-3, the bound on xi,
    the bound on rho)"""
    out = []
    for (i, j), e, blk in zip(pr, rec, cross_of):
        blocks = (diag[i], diag[j], blk)
        r = A.audit(T, i, j, e["R"], e["t"], e["kappa"], e["tau"], e["weight"], *blocks)
        b_s, b_x = G.sigma_rel_bound(T, i, j, *blocks), G.xi_bound(T, i, j, e["t"])
        out.append((r, A.bounds(r, b_s, b_x) if float(r["pmin"]) > 1e-3 else None, b_x, A.rho_bound(r, b_s)))
    return out


def e2e_rho_bound(T, n, i, j, kappa, tau, ev, Sigma):
    Ji, Jj = G.jacobians(T, i, j, F)
    B = 6 * (n - 1) * U * (ev[-1] / ev[0]) * np.linalg.norm(Sigma)
    return max(2 * kappa, tau) * np.linalg.norm(np.c_[Ji, Jj], 2) ** 2 * B


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_kernel_against_the_reference_at_lane_and_launch_edges(N, method):
    n = 40
    m, T, Sigma, ev = dense(n, 3)
    t = team_of(m, n, N, T)
    if method == "nested":
        assert t.covariance_plan(NESTED_BLOCK)[1]["promoted_poses"] > 0
    base = t.measurements_once()
    assert len(base) == len(m)
    bp = team_pairs(t, base, n, N)
    rec, ang, of_base = records(base, 5, seed=11)
    P = len(rec)
    assert P < 255
    # the reference, once: auditref in longdouble on the blocks the covariance call returns for the same pairs
    _, diag, cross = blocks_call(t, T, bp, method)
    ref = reference(T, bp[of_base], rec, diag, cross[of_base])
    held = np.array([b is not None for _, b, _, _ in ref])
    bridge = np.array([float(r["pmin"]) < 1e-6 for r, _, _, _ in ref])
    assert (held | bridge).all() and held.sum() >= 200 and bridge.sum() >= 1, (held.sum(), bridge.sum())
    assert all(r["testable"] for (r, _, _, _), h in zip(ref, held) if h)
    f64 = lambda key: np.array([np.asarray(r[key], dtype=F) for r, _, _, _ in ref])
    rxi, rxl, rd2, rrho, rpm, rsl = (f64(k) for k in ("xi", "xi_loo", "d2", "rho", "pmin", "sigma_loo"))
    bound = lambda key, shape: np.array([np.broadcast_to(b[key], shape) if b is not None else np.full(shape, np.inf) for _, b, _, _ in ref])
    bxl, bd2, brho_h, bpm, bsl = bound("xi_loo", (6,)), bound("d2", ()), bound("rho", ()), bound("pmin", ()), bound("sigma_loo", (6, 6))
    bx, brho = np.array([b for _, _, b, _ in ref]), np.array([b for _, _, _, b in ref])
    rho0 = np.array([e2e_rho_bound(T, n, i, j, e["kappa"], e["tau"], ev, Sigma) for (i, j), e in zip(bp[of_base], rec)])
    thr = capi.error_threshold_at_quantile(0.99, 6)
    print("%d robots, %s: %d unique records, %d held to the bounds (p_min >= %.3g), %d on bridges at full weight (|p_min| <= %.3g)"
          % (N, method, P, held.sum(), rpm[held].min(), bridge.sum(), np.abs(rpm[bridge]).max()))
    worst = dict(xi=0.0, xi_loo=0.0, d2=0.0, rho=0.0, pmin=0.0, sigma_loo=0.0, rho_bridge=0.0, rho_bridge_zero=0.0)
    rng = np.random.default_rng(5)
    for K in COUNTS:
        # every unique record as far as K reaches, then seeded repeats: duplicates at every count above P
        idx = np.r_[np.arange(min(K, P)), rng.integers(0, P, max(K - P, 0))]
        if K < P:
            idx = rng.permutation(P)[:K]
        out = audit_call(t, rec[idx], T, method, sigma_loo=True)
        xi, xl, d2, rho, pm, sl = (out[k] for k in ("xi", "xi_loo", "d2", "redundancy", "pivot_min", "sigma_loo"))
        assert xi.shape == (K, 6) and xl.shape == (K, 6) and sl.shape == (K, 6, 6)
        assert d2.shape == rho.shape == pm.shape == out["testable"].shape == out["accept"].shape == (K,)
        assert out["covariance"].n == 6 * (n - 1) and out["covariance"].min_pivot > 0
        assert out["measurements"].tobytes() == rec[idx].tobytes()
        assert sl.tobytes() == np.ascontiguousarray(sl.transpose(0, 2, 1)).tobytes(), "sigma_loo is not bitwise symmetric"
        h, b = held[idx], bridge[idx]
        ratios = dict(xi=np.abs(xi - rxi[idx]) / bx[idx], xi_loo=np.abs(xl[h] - rxl[idx][h]) / bxl[idx][h],
                      d2=np.abs(d2[h] - rd2[idx][h]) / bd2[idx][h], rho=np.abs(rho[h] - rrho[idx][h]) / brho_h[idx][h],
                      pmin=np.abs(pm[h] - rpm[idx][h]) / bpm[idx][h], sigma_loo=np.abs(sl[h] - rsl[idx][h]) / bsl[idx][h],
                      rho_bridge=np.abs(rho[b] - rrho[idx][b]) / brho[idx][b], rho_bridge_zero=np.abs(rho[b]) / rho0[idx][b])
        for key, v in ratios.items():
            if v.size:
                worst[key] = max(worst[key], v.max())
                assert v.max() <= 1.0, (K, key, v.max())
        assert out["testable"][h].all() and np.isfinite(d2[h]).all()
        assert not out["testable"][b].any() and (d2[b] == np.inf).all() and not xl[b].any() and not sl[b].any()
        assert (out["accept"] == (out["testable"] & (np.sqrt(d2) <= thr))).all() and not out["accept"][b].any()
        zero_w = rec[idx]["weight"] == 0.0
        assert (rho[zero_w] == 1.0).all() and (pm[zero_w] == 1.0).all()
        # duplicates: the bits of the first occurrence
        first = np.full(P, -1)
        first[idx[::-1]] = np.arange(K)[::-1]
        f = first[idx]
        if K > P:
            assert (f != np.arange(K)).any()
        for a in (xi, xl, d2, rho, pm, sl):
            assert a.tobytes() == a[f].tobytes()
        if K == 257:  # a second call, and the call without Sigma_loo: the same bits
            for kw in (dict(sigma_loo=True), dict()):
                two = audit_call(t, rec[idx], T, method, **kw)
                for key in ("xi", "xi_loo", "d2", "redundancy", "pivot_min", "testable", "accept") + (("sigma_loo",) if kw else ()):
                    assert two[key].tobytes() == out[key].tobytes(), key
                assert ("sigma_loo" in two) == bool(kw)
    print("largest error / bound: " + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_weight_zero_is_the_gate(method):
    """the records of test 1 at weight 0: A = I exactly, so rho = 1 and p_min = 1 to the bit and xi_loo = xi within 4 u (one
    product with s and one with 1 / s, each with a rounded square root); d2 and xi agree with Team.gate within the sum of the
    two tests' bounds"""
    n, N = 40, 2
    m, T, _, _ = dense(n, 3)
    t = team_of(m, n, N, T)
    base = t.measurements_once()
    bp = team_pairs(t, base, n, N)
    rec, ang, of_base = records(base, 2, seed=12)
    rec["weight"] = 0.0
    _, diag, cross = blocks_call(t, T, bp, method)
    out = audit_call(t, rec, T, method)
    _, gxi, gd2, _ = t.gate(rec, T, method=method, max_block=NESTED_BLOCK if method == "nested" else None)
    assert (out["redundancy"] == 1.0).all() and (out["pivot_min"] == 1.0).all() and out["testable"].all()
    worst = dict(d2=0.0, xi=0.0, xi_loo=0.0)
    for k, ((i, j), e) in enumerate(zip(bp[of_base], rec)):
        blocks = (diag[i], diag[j], cross[of_base[k]])
        r = A.audit(T, i, j, e["R"], e["t"], e["kappa"], e["tau"], 0.0, *blocks)
        b_s, b_x = G.sigma_rel_bound(T, i, j, *blocks), G.xi_bound(T, i, j, e["t"])
        xi, d2, _, S = G.gate(T, i, j, e["R"], e["t"], e["kappa"], e["tau"], *blocks)
        b = A.bounds(r, b_s, b_x)["d2"] + G.d2_bound(xi, S, d2, b_x, b_s)
        worst["d2"] = max(worst["d2"], abs(out["d2"][k] - gd2[k]) / b)
        worst["xi"] = max(worst["xi"], (np.abs(out["xi"][k] - gxi[k]) / (2 * b_x)).max())
        lim = 4 * U * np.abs(out["xi"][k])
        worst["xi_loo"] = max(worst["xi_loo"], (np.abs(out["xi_loo"][k] - out["xi"][k])[lim > 0] / lim[lim > 0]).max(initial=0.0))
        assert abs(out["d2"][k] - gd2[k]) <= b and (np.abs(out["xi"][k] - gxi[k]) <= 2 * b_x).all()
        assert (np.abs(out["xi_loo"][k] - out["xi"][k]) <= lim).all()
    print("%s, %d records at weight 0: largest |audit - gate| / bound: " % (method, len(rec)) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_sigma_loo_is_the_relative_covariance_of_the_team_without_the_edge(method):
    """first principles: for five testable edges -- one shared between the two robots, one odometry edge among them -- a second
    team is built without the edge, and relative_covariances of that team is what sigma_loo of the full team must be"""
    n, N = 12, 2
    m, T, Sigma, ev = dense(n, 2)
    mb = 2 if method == "nested" else None
    t = team_of(m, n, N, T)
    base = t.measurements_once()
    bp = team_pairs(t, base, n, N)
    out = t.audit(base, T, method=method, max_block=mb, sigma_loo=True)
    ok = np.flatnonzero(out["pivot_min"] > 1e-3)
    assert not ((out["pivot_min"] > 1e-6) & (out["pivot_min"] <= 1e-3)).any()
    shared = [k for k in ok if base[k]["r1"] != base[k]["r2"]]
    odo = [k for k in ok if base[k]["r1"] == base[k]["r2"] and base[k]["p2"] == base[k]["p1"] + 1]
    assert shared and odo, "no testable shared edge or odometry edge: another seed"
    chosen = [shared[0], odo[0]] + [k for k in ok if k not in (shared[0], odo[0])][:3]
    worst = 0.0
    for k in chosen:
        i, j = bp[k]
        e = int(np.flatnonzero((m["p1"] == i) & (m["p2"] == j))[0])
        m1 = np.delete(m, e)
        _, Sigma1, ev1 = covref.dense_reference(covref.q_full(m1, n), T, n)
        assert ev1[0] > 0
        t1 = team_of(m1, n, N, T)
        want = t1.relative_covariances([(i, j)], T, method=method, max_block=mb)[0]
        t1.close()
        r = A.audit(T, i, j, base[k]["R"], base[k]["t"], base[k]["kappa"], base[k]["tau"], base[k]["weight"], *G.blocks_of(Sigma, i, j))
        err, b = np.linalg.norm(out["sigma_loo"][k] - want), loo_bound(T, n, i, j, ev, Sigma, ev1, Sigma1, r)
        worst = max(worst, err / b)
        assert err <= b, (k, i, j, err, b)
    print("%s: sigma_loo against the team without the edge, edges %s: largest error / bound %.3g"
          % (method, [tuple(int(x) for x in bp[k]) for k in chosen], worst))
    t.close()


def test_defaults_end_to_end():
    """Team.audit() with no arguments on the noise-free team: the team's own measurements at their weights, the rounding of the
    iterate.  Every testable edge passes with d2 <= 1e-18 (xi is the rounding's round-off, about 1e-14, whitened by at most
    sqrt(200) and divided by p_min >= 0.0077); the untestable edges are exactly the bridges of the graph (union-find on the
    host); the redundancy numbers sum to 6 (n - 1); solve_certified(audit=True) returns the audit of its final team, bit for bit"""
    n, N = 40, 2
    m, T, Sigma, ev = dense(n, 3)
    t = team_of(m, n, N, T)
    out = t.audit()
    meas = out["measurements"]
    assert meas.tobytes() == t.measurements_once().tobytes() and len(meas) == len(m) and (meas["weight"] == 1.0).all()
    assert sorted(out) == sorted(["measurements", "xi", "xi_loo", "d2", "redundancy", "pivot_min", "testable", "accept", "covariance"])
    pr = team_pairs(t, meas, n, N)

    def joined(skip):
        root = list(range(n))

        def find(a):
            while root[a] != a:
                a = root[a]
            return a
        for k, (i, j) in enumerate(pr):
            if k != skip:
                root[find(int(i))] = find(int(j))
        return len({find(a) for a in range(n)}) == 1

    bridge = np.array([not joined(k) for k in range(len(pr))])
    print("d2 of the testable edges <= %.3g, %d bridges, p_min of the others >= %.3g" % (out["d2"][~bridge].max(), bridge.sum(), out["pivot_min"][~bridge].min()))
    assert bridge.sum() >= 3 and (out["testable"] == ~bridge).all()
    assert (out["d2"][~bridge] <= 1e-18).all() and out["accept"][~bridge].all() and not out["accept"][bridge].any()
    total = float(np.sum(meas["weight"] * (1.0 - out["redundancy"]) * 6.0))
    bound = sum(e["weight"] ** 2 * e2e_rho_bound(T, n, i, j, e["kappa"], e["tau"], ev, Sigma) * 6 for (i, j), e in zip(pr, meas))
    print("sum w 6 (1 - rho) = %.15g, 6 (n - 1) = %d, difference / bound %.3g" % (total, 6 * (n - 1), abs(total - 6 * (n - 1)) / bound))
    assert abs(total - 6 * (n - 1)) <= bound
    t.close()
    # solve_certified on a small graph (the call of the covariance tests): the audit of its final team at its T
    ds = "smallGrid3D"
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    prm = capi.default_params(r=5, num_robots=N, **RTR_NESTEROV)
    res = capi.solve_certified(mp, prm, r0=5, T=capi.chordal_init(m, n), iters=300, audit=True, covariance_method="schur")
    assert sorted(res) == sorted(["T", "r", "ranks", "certificate", "rounding", "f_relaxed", "f_rounded", "gap_rel", "escape_costs", "audit"])
    t = capi.Team.from_measurements(mp, prm)
    t.set_initial(res["T"], capi.fixed_stiefel(5))
    want = t.audit(T=res["T"], method="schur")
    t.close()
    assert sorted(res["audit"]) == sorted(want) and len(want["d2"]) == len(m)
    for key, v in want.items():
        if key != "covariance":
            assert res["audit"][key].tobytes() == v.tobytes(), key
    assert res["audit"]["covariance"].logdet == want["covariance"].logdet
    print("solve_certified(audit=True) on %s: %d edges, %d testable, %d accepted at 0.99" % (ds, len(m), want["testable"].sum(), want["accept"].sum()))


def raw_audit(t, T, method, max_block, meas, min_redundancy, outs, res, num=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return capi.lib().dpgo_team_audit_measurements(t.h, p(T), method, max_block, len(meas) if num is None else num, p(meas),
                                                   C.c_double(min_redundancy), *[p(a) for a in outs], C.byref(res))


def test_refusals_leave_the_outputs_untouched():
    n, N = 40, 2
    m, T, _, _ = dense(n, 3)
    t = team_of(m, n, N, T)
    good = t.measurements_once()[[7, 30]].copy()
    good["weight"] = (1.0, 0.37)
    xi, xl, d2, rho, pm, sl = (np.full(s, 7.25) for s in ((2, 6), (2, 6), 2, 2, 2, (2, 6, 6)))
    outs = [xi, xl, d2, rho, pm, sl]
    res = capi.Covariance()

    def refused(what, meas=good, method=capi.GATE_DENSE, T_=T, num=None, max_block=0, min_redundancy=1e-6, null=None):
        res.n = 5
        o = [None if k == null else a for k, a in enumerate(outs)]
        rc = raw_audit(t, T_, method, max_block, meas, min_redundancy, o, res, num)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg, (rc, msg)
        assert all((a == 7.25).all() for a in outs)
        return msg

    for k in range(5):
        refused("null argument", null=k)
    refused("null argument", T_=None)
    refused("null argument", meas=None, num=2)
    refused("num must be positive", num=0)
    refused("num must be positive", num=-3)
    refused("method must be", method=3)
    refused("method must be", method=-1)
    for bad in (0.0, 1.0, -1e-3, 1.5, np.nan):
        refused("min_redundancy must lie in (0, 1)", min_redundancy=bad)

    def changed(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k][1] = v
        return c

    refused("record 1 names robot 2, which is not in the team", changed(r2=2))
    refused("record 1 names pose 20 of robot", changed(p2=20))
    refused("record 1 names pose -1 of robot", changed(p1=-1))
    refused("record 1 joins a pose to itself", changed(r2=good["r1"][1], p2=good["p1"][1]))
    refused("record 1 has kappa", changed(kappa=0.0))
    refused("record 1 has kappa", changed(tau=-1.0))
    refused("record 1 has kappa", changed(kappa=np.inf))
    refused("record 1 has kappa", changed(tau=np.nan))
    refused("record 1 has weight", changed(weight=-1e-300))
    refused("record 1 has weight", changed(weight=np.inf))
    refused("record 1 has weight", changed(weight=np.nan))
    bad = good.copy()
    bad["R"][1][0] *= 1.001
    refused("the measurement of record 1 is not in SE(3)", bad)
    bad = good.copy()
    bad["t"][1][2] = np.nan
    refused("the measurement of record 1 is not in SE(3)", bad)
    # carried over from the covariance path, with its own message: T outside SE(3), and per method a T that is no minimum
    Tb = T.copy()
    Tb[12 * 17] *= 1.001
    refused("pose 17 of T is not in SE", T_=Tb)
    Ts = NR.spoil_rotations(T, n, [9, 10, 11, 28, 29], 50)
    for method, mb in ((capi.GATE_DENSE, 0), (capi.GATE_SCHUR, 0), (capi.GATE_NESTED, NESTED_BLOCK)):
        res.n = 5
        rc = raw_audit(t, Ts, method, mb, good, 1e-6, outs, res)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and "non-positive pivot" in msg and "not a minimum" in msg and msg.startswith("marginal_covariances"), msg
        assert all((a == 7.25).all() for a in outs) and bytes(res) == bytes(capi.Covariance())
    # the same arguments pass once nothing is wrong, Sigma_loo left out included
    assert raw_audit(t, T, capi.GATE_DENSE, 0, good, 1e-6, outs[:5] + [None], res) == capi.OK and res.n == 6 * (n - 1)
    assert all(not (a == 7.25).any() for a in outs[:5]) and (sl == 7.25).all()
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.audit(good, Ts)
    with pytest.raises(capi.DpgoError, match="min_redundancy"):
        t.audit(good, T, min_redundancy=0.0)
    with pytest.raises(ValueError, match="method must be"):
        t.audit(good, T, method="sparse")
    t.close()

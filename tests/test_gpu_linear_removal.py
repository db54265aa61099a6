"""GPU checks of the first-order removal or down-weighting of measurements that are in the graph (csrc/linear_removal.hip,
Team.linear_removal).

The graph is covnested_ref.banded_chain(40, 3, window=8): noise-free, the ground truth T is an exact minimum, no solve; 49 edges,
10 of them closures, 38 not bridges, cyclomatic number 10.  Removing any subset of the closures leaves the odometry chain, so
such sets never disconnect the graph.  The record sets: K = 1, 2, 5, 10 closures removed fully; K = 11, 22, 43 distinct edges
(pose 0 among them) down-weighted to w / 2; one mixed set with w' in {0, 0.37 w}; one set with parallel records of different noise on one ordered pair.  6 K = 6, 12, 30, 60, 66, 132, 258 crosses the
64-lane stride of k_rem_finish and the 64- and 256-wide tiles; 6 N = 240 is no multiple of 64.  The measurements of the records
are moved so that |xi_k| = 0.05; the records are taken on trust, so T stays the minimum the team's own graph has.
Every set used for bounds has pivot_min_joint >= 1e-3 in the reference, which the test asserts.

Bounds (u = 2.2e-16; derived in tests/removalref.py, and tests/test_removalref.py shows that they reject a flipped sign of dx,
Sigma - ... for Sigma + ..., dw taken as w, a logdet_R without its dw term, N = R + A B and a scaling applied once, each by more
than 1000 x):
  the removal alone, against removalref in longdouble on the blocks covariances(pairs = the rectangular set) returns for the
    same method: every output within removalref.bounds;
  end to end, residual-free records removed fully: Sigma'_pp against the covariances of a team built without them, within
    6 (n - 1) u (cond_2(H_red) |Sigma|_F + cond_2(H'_red) |Sigma'|_F) in the Frobenius norm over all diagonal blocks.
Every test prints its largest error / bound."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import auditref as AR
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import removalref as V
from tests import updateref as R
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_gate import blocks_call
from tests.test_gpu_gate_joint import NESTED_BLOCK, records, setup
from tests.test_gpu_linear_update import check_rotations, closures, extended, update_call

pytestmark = pytest.mark.gpu

F = np.float64
U = V.U
N_POSES = 40
PAIRS = np.array([(0, 7), (12, 12), (13, 27), (27, 13), (5, 38), (39, 1)], dtype=np.int32)  # pose 0, a = b, across robots
OUTPUTS = ("xi", "delta", "T", "cov_diag", "cov_pairs", "xi_loo", "pivot_min", "d2_joint", "logdet_N", "logdet_R", "pivot_min_joint")


def edges_of(m):
    return [(int(a), int(b)) for a, b in zip(m["p1"], m["p2"])]


def closures_of(m):
    return [e for e, (i, j) in enumerate(edges_of(m)) if abs(i - j) != 1]


def record_sets(m):
    """[(name, edge indices, w'/w per record or None for a full removal, (kappa, tau) per record as multiples of the edge's or
    None)]"""
    clo = closures_of(m)
    order = [0] + [int(e) for e in np.random.default_rng(5).permutation(np.arange(1, len(m)))]  # distinct edges, the one at pose 0 first
    sets = [("%d closures removed" % K, clo[:K], None, None) for K in (1, 2, 5, 10)]
    sets += [("%d edges halved" % K, order[:K], np.full(K, 0.5), None) for K in (11, 22, 43)]
    # (the odometry edge 3 is a bridge: it can only be down-weighted)
    sets.append(("mixed", clo[:6] + [3, 17, 30], np.array([0.0, 0.37, 0.0, 0.37, 0.0, 0.37, 0.37, 0.37, 0.37]), None))
    # two and three parallel records on one ordered pair of poses whose noise is not proportional: together they claim less
    # than their edge holds (kappa 0.5 + 0.25, tau 0.8 + 0.1; 0.3 + 0.2 + 0.4, 0.5 + 0.1 + 0.3), and their blocks of N~ are
    # not symmetric
    sets.append(("parallel", [clo[0], clo[0], clo[4], 17, 17, 17], None,
                 np.array([(0.5, 0.8), (0.25, 0.1), (1.0, 1.0), (0.3, 0.5), (0.2, 0.1), (0.4, 0.3)])))
    return sets


def fma(a, b, c):
    """the correctly rounded a b + c (float(Fraction) rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def device_relative_pose(T, i, j):
    """(R_ij, t_ij) with the bits gate_jacobians forms: a measurement that is exactly this has an innovation of exactly zero --
    R~^T R_ij is then bitwise symmetric, so its logarithm is zero, and t_ij - t~ is zero"""
    P = np.asarray(T, dtype=F).reshape(-1, 4, 3)
    Ri, Rj, ti, tj = P[i, :3, :].T, P[j, :3, :].T, P[i, 3, :], P[j, 3, :]
    M, t = np.zeros((3, 3)), np.zeros(3)
    for a in range(3):
        for b in range(3):
            M[a, b] = fma(Ri[2, a], Rj[2, b], fma(Ri[1, a], Rj[1, b], Ri[0, a] * Rj[0, b]))
        t[a] = fma(Ri[2, a], tj[2] - ti[2], fma(Ri[1, a], tj[1] - ti[1], Ri[0, a] * (tj[0] - ti[0])))
    return M, t


def in_graph(m, T, n, N, idx, ratio=None, scale=0.05, seed=11, weight=1.0, noise=None):
    """the edges idx of the graph as records at `weight` whose measurements are moved so that the innovation of record k at T is
    scale x a seeded unit vector (0: exactly zero).  Returns (records in the team's numbering, ends, Rm, tm, kappa, tau, w, w')"""
    rng = np.random.default_rng(seed)
    E = edges_of(m)
    K = len(idx)
    ends = np.array([E[e] for e in idx], dtype=np.int64)
    Rm, tm = np.zeros((K, 3, 3)), np.zeros((K, 3))
    for k, (i, j) in enumerate(ends):
        if scale == 0:
            Rm[k], tm[k] = device_relative_pose(T, int(i), int(j))
            continue
        Rij, tij = G.relative_pose(T, int(i), int(j), F)
        x = rng.standard_normal(6)
        x = scale * x / np.linalg.norm(x)
        Rm[k], tm[k] = Rij @ covref.exp_so3(-x[:3]), tij - x[3:]
    kap, ta = np.array(m["kappa"][idx], dtype=F), np.array(m["tau"][idx], dtype=F)
    if noise is not None:
        kap, ta = kap * noise[:, 0], ta * noise[:, 1]
    rec = records(n, N, ends, Rm, tm, kap, ta)
    rec["weight"] = weight
    rec["fixed_weight"], rec["is_known_inlier"] = np.arange(K) % 2, np.arange(K) % 3 == 0  # ignored
    w = np.full(K, float(weight))
    return rec, ends, Rm, tm, kap, ta, w, (None if ratio is None else w * ratio)


def removal_call(t, rec, T, method, **kw):
    return t.linear_removal(rec, T=T, method=method, max_block=NESTED_BLOCK if method == "nested" else None, **kw)


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_the_removal_alone_at_tile_and_block_edges(N, method):
    n = N_POSES
    m, T, t = setup(n, N, method)
    X0 = t.global_X().copy()
    worst = {}
    for name, idx, ratio, noise in record_sets(m):
        K = len(idx)
        rec, ends, Rm, tm, kap, ta, w, w_new = in_graph(m, T, n, N, idx, ratio, noise=noise)
        out = removal_call(t, rec, T, method, new_weight=w_new, pairs=PAIRS)
        assert out["T"].shape == (12 * n,) and out["delta"].shape == (n, 6) and out["cov_diag"].shape == (n, 6, 6)
        assert out["cov_pairs"].shape == (len(PAIRS), 6, 6) and out["xi"].shape == out["xi_loo"].shape == (K, 6) and out["pivot_min"].shape == (K,)
        assert out["covariance"].n == 6 * (n - 1) and out["covariance"].min_pivot > 0
        assert abs(np.linalg.norm(out["xi"], axis=1) - 0.05).max() <= 1e-9
        # 1. against removalref on the blocks the covariance call returns for the rectangular set and the pairs
        poses = sorted(set(ends.reshape(-1).tolist()))
        _, diag, cross = blocks_call(t, T, np.r_[R.rect_pairs(poses, n), PAIRS], method)
        ref = V.removal(T, ends, Rm, tm, kap, ta, w, w_new, R.blocks_from_rect(poses, n, diag, cross), n, pairs=PAIRS)
        assert ref["testable"] and float(ref["pivot_min_joint"]) >= 1e-3, (name, float(ref["pivot_min_joint"]))
        b = V.bounds(ref, T, ends, tm, n, PAIRS)
        for key in OUTPUTS:
            r = V.ratio(np.asarray(out[key] - np.asarray(ref[key], dtype=F)), b[key])
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (name, key, r)
        worst["cond_N"] = max(worst.get("cond_N", 0.0), b["cond_N"])
        assert out["information_loss"] == 0.5 * (out["logdet_R"] - out["logdet_N"]) and out["information_loss"] > 0
        assert 0 < out["pivot_min_joint"] <= out["pivot_min"].min() * (1 + 1e-12) and out["pivot_min"].max() <= 1
        assert out["cov_diag"].tobytes() == np.ascontiguousarray(out["cov_diag"].transpose(0, 2, 1)).tobytes(), "not bitwise symmetric"
        assert (out["delta"][0] == 0).all() and (out["cov_diag"][0] == 0).all() and (out["cov_pairs"][0] == 0).all()
        assert out["T"][:12].tobytes() == T[:12].tobytes()
        assert (out["new_weight"] == (0.0 if w_new is None else w_new)).all() and out["measurements"].tobytes() == rec.tobytes()
        # the removal gives uncertainty back: every diagonal block grows
        assert (np.einsum("gaa->g", out["cov_diag"]) >= np.einsum("gaa->g", diag) * (1 - 1e-12)).all()
        # the verdict: 0.05 against sigmas of 0.07 and 0.14 is no outlier
        assert out["joint_accept"] == bool(np.sqrt(out["d2_joint"]) <= capi.error_threshold_at_quantile(0.99, 6 * K))
        # 5. T' is on SE(3)
        worst["rotations"] = max(worst.get("rotations", 0.0), check_rotations(out["T"], n))
        if K == 11:
            halved = out["T"]
        # 6. two calls: the same bytes
        if K in (10, 43):
            again = removal_call(t, rec, T, method, new_weight=w_new, pairs=PAIRS)
            for key in ("T", "delta", "cov_diag", "cov_pairs", "xi", "xi_loo", "pivot_min"):
                assert out[key].tobytes() == again[key].tobytes(), key
            for key in ("d2_joint", "logdet_N", "logdet_R", "pivot_min_joint"):
                assert out[key] == again[key], key
    # 5. a following call takes T'.  (That of the halved edges, where no pivot is below 1 / 2: the team's own graph still holds
    # every record at full weight, and where the removal of a closure moves the chain by 0.05 / pivot_min that graph has no
    # minimum near T'.)
    res = blocks_call(t, halved, None, method)[0]
    assert res.n == 6 * (n - 1)
    # and a team rebuilt without ten fully removed closures takes their T' (residuals of 1e-4, so that T' stays near the
    # minimum T of that noise-free graph)
    idx = closures_of(m)[:10]
    rec = in_graph(m, T, n, N, idx, scale=1e-4)[0]
    out = removal_call(t, rec, T, method)
    assert 1e-3 < np.abs(out["delta"]).max() < 0.05
    tx = team_of(np.delete(m, idx), n, N, out["T"])
    assert blocks_call(tx, out["T"], None, method)[0].n == 6 * (n - 1)
    tx.close()
    assert t.global_X().tobytes() == X0.tobytes()
    print("%d robots, %s: largest error / bound: " % (N, method) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_end_to_end_exact_records_against_the_graph_without_them(method):
    n, N = N_POSES, 2
    m, T, t = setup(n, N, method)
    idx = closures_of(m)[:5]
    rec, ends, Rm, tm, kap, ta, w, _ = in_graph(m, T, n, N, idx, scale=0)
    out = removal_call(t, rec, T, method)
    mx = np.delete(m, idx)
    tx = team_of(mx, n, N, T)
    res_x, diag_x, _ = blocks_call(tx, T, None, method)
    _, S0, w0 = covref.dense_reference(covref.q_full(m, n), T, n)
    _, S1, w1 = covref.dense_reference(covref.q_full(mx, n), T, n)
    assert w0[0] > 0 and w1[0] > 0
    bound = 6 * (n - 1) * U * (w0[-1] / w0[0] * np.linalg.norm(S0) + w1[-1] / w1[0] * np.linalg.norm(S1))
    err = np.linalg.norm(out["cov_diag"] - diag_x)
    # log det H from a Cholesky factor: the factor is exact for H + dH with |dH| <= gamma_n |L| |L|^T and d log det = tr(H^-1 dH),
    # at most n gamma_n cond_2(H) with n = 6 (n_poses - 1), for either graph
    loss, want = out["information_loss"], 0.5 * (out["covariance"].logdet - res_x.logdet)
    b_loss = 6 * (n - 1) * U * (w0[-1] / w0[0] + w1[-1] / w1[0]) * 6 * (n - 1)
    print("%s, exact records, cond_2(H_red) %.3g -> %.3g: |Sigma'_diag - without|_F / bound %.3g, max |xi| %.3g, max |dx| %.3g, "
          "information_loss %.12g against half the difference of the log dets %.12g (%.3g of its bound)"
          % (method, w0[-1] / w0[0], w1[-1] / w1[0], err / bound, np.abs(out["xi"]).max(), np.abs(out["delta"]).max(), loss, want,
             abs(loss - want) / b_loss))
    assert err <= bound
    assert (out["xi"] == 0).all() and (out["delta"] == 0).all() and out["T"].tobytes() == T.tobytes() and out["d2_joint"] == 0
    assert abs(loss - want) <= b_loss
    t.close()
    tx.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_round_trip_with_the_update_is_right_to_second_order(method):
    n, N, K = N_POSES, 2, 11
    m, T, t = setup(n, N, method)
    errs = []
    for s in (1.0, 0.25, 0.0625):
        ends, Rm, tm, kap, ta = closures(T, n, K, seed=29, scale=0.05 * s, normal=5)
        cand = records(n, N, ends, Rm, tm, kap, ta)
        up = update_call(t, cand, T, method)
        tx = team_of(extended(m, ends, Rm, tm, kap, ta), n, N, up["T"])
        cand["weight"] = 1.0
        back = removal_call(tx, cand, up["T"], method)
        errs.append(np.abs(back["T"] - T).max())
        tx.close()
    print("%s: max |T'' - T| %.3g, %.3g, %.3g (ratios %.3g, %.3g)" % (method, errs[0], errs[1], errs[2], errs[0] / errs[1], errs[1] / errs[2]))
    assert errs[0] / errs[1] >= 8 and errs[1] / errs[2] >= 8  # theory 16; a sign mistake 4
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_one_record_is_the_audit(method):
    n, N = N_POSES, 2
    m, T, t = setup(n, N, method)
    worst = {}
    for e, weight in ((closures_of(m)[0], 1.0), (closures_of(m)[3], 0.37), (20, 1.0)):
        rec, ends, Rm, tm, kap, ta, w, _ = in_graph(m, T, n, N, [e], weight=weight)
        out = removal_call(t, rec, T, method)
        aud = t.audit(rec, T, method=method, max_block=NESTED_BLOCK if method == "nested" else None)
        i, j = int(ends[0][0]), int(ends[0][1])
        _, diag, cross = blocks_call(t, T, np.array([(i, j)], dtype=np.int32), method)
        a = AR.audit(T, i, j, Rm[0], tm[0], kap[0], ta[0], weight, diag[i], diag[j], cross[0])
        ba = AR.record_bounds(T, i, j, tm[0], diag[i], diag[j], cross[0], a)
        poses = sorted((i, j))
        _, diag, cross = blocks_call(t, T, R.rect_pairs(poses, n), method)
        ref = V.removal(T, ends, Rm, tm, kap, ta, w, None, R.blocks_from_rect(poses, n, diag, cross), n)
        b = V.bounds(ref, T, ends, tm, n)
        assert float(ref["pivot_min_joint"]) >= 1e-3 and aud["testable"][0]
        r = dict(xi_loo=V.ratio(out["xi_loo"][0] - aud["xi_loo"][0], b["xi_loo"][0] + ba["xi_loo"]),
                 pivot_min=abs(out["pivot_min"][0] - aud["pivot_min"][0]) / (b["pivot_min"][0] + ba["pmin"]))
        if weight == 1.0:
            r["d2"] = abs(out["d2_joint"] - aud["d2"][0]) / (b["d2_joint"] + ba["d2"])
        assert np.abs(out["xi"] - aud["xi"]).max() <= 2 * b["xi"].max()
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (e, weight, k, v)
    print("%s, K = 1 against audit: largest |difference| / (sum of the bounds): " % method + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


def raw_removal(t, T, method, max_block, rec, new_weight, min_redundancy, pairs, bufs, res, num=None, num_pairs=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    Tn, dx, diag, cross, xi, xl, pm, sc = bufs
    return capi.lib().dpgo_team_linear_removal(t.h, p(T), method, max_block, len(rec) if num is None else num, p(rec), p(new_weight),
                                               C.c_double(min_redundancy), (0 if pairs is None else len(pairs)) if num_pairs is None else num_pairs,
                                               p(pairs), p(Tn), p(dx), p(diag), p(cross), p(xi), p(xl), p(pm), p(sc), C.byref(res))


def test_refusals_leave_the_outputs_untouched():
    n, N = N_POSES, 2
    m, T = NR.banded_chain(n, 3, window=8)
    t = team_of(m, n, N, T)
    clo = closures_of(m)
    good = in_graph(m, T, n, N, clo[:2])[0]
    pairs = np.array([(1, 2), (30, 4)], dtype=np.int32)
    fresh = lambda K=2, P=2: [np.full(12 * n, 7.25), np.full((n, 6), 7.25), np.full((n, 6, 6), 7.25), np.full((P, 6, 6), 7.25),
                              np.full((K, 6), 7.25), np.full((K, 6), 7.25), np.full(K, 7.25), np.full(4, 7.25)]
    bufs, res = fresh(), capi.Covariance()

    def refused(what, rec=good, method=capi.GATE_DENSE, T_=T, pairs_=pairs, num=None, num_pairs=None, max_block=0, null=None, bufs_=None,
                new_weight=None, min_redundancy=1e-6):
        res.n = 5
        b = list(bufs_ or bufs)
        if null is not None:
            b[null] = None
        rc = raw_removal(t, T_, method, max_block, rec, new_weight, min_redundancy, pairs_, b, res, num, num_pairs)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg, (rc, msg)
        for a in (bufs_ or bufs):
            assert (a == 7.25).all()
        return msg

    # ---- every refusal linear_update has
    assert refused("num must be positive", num=0).startswith("linear_removal:")
    refused("num must be positive", num=-3)
    refused("num_pairs must not be negative", num_pairs=-1)
    for q in range(8):
        if q != 3:
            assert refused("null argument", null=q).startswith("linear_removal:")
    refused("null argument", null=3)
    refused("null argument", pairs_=None, num_pairs=2)
    refused("method must be", method=3)
    refused("method must be", method=-1)

    def changed(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k][1] = v
        return c

    refused("record 1 names robot 2, which is not in the team", changed(r2=2))
    refused("record 1 names pose 20 of robot 0", changed(r1=0, p1=20))
    refused("record 1 names pose -1 of robot 1", changed(r1=1, p1=-1))
    refused("record 1 joins a pose to itself", changed(r2=good["r1"][1], p2=good["p1"][1]))
    refused("both must be positive", changed(kappa=0.0))
    refused("both must be positive", changed(tau=-1.0))
    refused("both must be positive", changed(tau=float("inf")))
    bad = good.copy()
    bad["R"][1][0] *= 1.001
    refused("the measurement of record 1 is not in SE(3)", bad)
    assert refused("pair 1 names pose 40, outside [0, 40)", pairs_=np.array([(1, 2), (30, 40)], dtype=np.int32)).startswith("linear_removal:")
    refused("pair 0 names pose -1", pairs_=np.array([(-1, 2), (30, 4)], dtype=np.int32))
    # ---- the call's own: the weights and min_redundancy
    refused("record 1 has weight = -1: it must be finite and not negative", changed(weight=-1.0))
    refused("record 1 has weight = inf", changed(weight=float("inf")))
    refused("record 1 has weight = nan", changed(weight=float("nan")))
    refused("record 1 has weight = 0: a record must be in the graph at a positive weight", changed(weight=0.0))
    for nw in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert "below its weight = 1" in refused("record 1 has new_weight = ", new_weight=np.array([0.0, nw]))
    for mr in (0.0, 1.0, -1e-6, float("nan")):
        refused("min_redundancy must lie in (0, 1)", min_redundancy=mr)
    # 30000 records: three matrices of order 180000, 288 K^2 bytes each, beyond any device
    many = np.repeat(good, 15000)
    big = fresh(len(many))
    msg = refused("bytes", many, bufs_=big)
    assert "30000 records on 4 of 40 poses" in msg and "3 x 259200000000" in msg and "are available on the device" in msg, msg
    # ---- behind the covariance path: a bridge alone, with the record named; three edges that cut the graph together
    bridge = in_graph(m, T, n, N, [clo[0], 0])[0]
    msg = refused("record 1 is not testable", bridge)
    assert msg.startswith("linear_removal:") and "min_redundancy = 1e-06" in msg and bytes(res) == bytes(capi.Covariance()), msg
    triple = V.cut_triple(m, n)
    cut = in_graph(m, T, n, N, list(triple))[0]
    three = fresh(3)
    msg = refused("the records together leave no redundancy", cut, bufs_=three)
    assert msg.startswith("linear_removal:") and bytes(res) == bytes(capi.Covariance()), msg
    for drop in range(3):  # (any two of them go through)
        ok = fresh()
        assert raw_removal(t, T, capi.GATE_DENSE, 0, np.delete(cut, drop), None, 1e-6, pairs, ok, res) == capi.OK and ok[7][3] >= 1e-3
    # halved, the bridge and the cut leave half of every pivot
    ok = fresh(3)
    assert raw_removal(t, T, capi.GATE_DENSE, 0, cut, np.full(3, 0.5), 1e-6, pairs, ok, res) == capi.OK and ok[7][3] >= 0.4
    with pytest.raises(capi.DpgoError, match="record 1 is not testable"):
        t.linear_removal(bridge, T=T)
    with pytest.raises(capi.DpgoError, match="leave no redundancy"):
        t.linear_removal(cut, T=T, method="schur")
    # carried over from the covariance path, with its own message: T outside SE(3), and per method a T that is no minimum
    Tb = T.copy()
    Tb[12 * 17] *= 1.001
    refused("pose 17 of T is not in SE", T_=Tb)
    Ts = NR.spoil_rotations(T, n, [9, 10, 11, 28, 29], 50)
    for method, mb in ((capi.GATE_DENSE, 0), (capi.GATE_SCHUR, 0), (capi.GATE_NESTED, NESTED_BLOCK)):
        msg = refused("non-positive pivot", T_=Ts, method=method, max_block=mb)
        assert "not a minimum" in msg and msg.startswith("marginal_covariances"), msg
        assert bytes(res) == bytes(capi.Covariance())
    with pytest.raises(ValueError, match="method must be"):
        t.linear_removal(good, T=T, method="sparse")
    with pytest.raises(ValueError, match="T holds"):
        t.linear_removal(good, T=T[:-12])
    # and the call goes through once nothing is wrong, with and without pairs
    ok = fresh()
    assert raw_removal(t, T, capi.GATE_DENSE, 0, good, None, 1e-6, pairs, ok, res) == capi.OK and res.n == 6 * (n - 1)
    assert all((a != 7.25).all() for a in ok)
    ok = fresh()
    assert raw_removal(t, T, capi.GATE_SCHUR, 0, good, np.array([0.5, 0.0]), 0.5e-3, None, ok, res) == capi.OK
    assert (ok[3] == 7.25).all() and (ok[0] != 7.25).all()
    t.close()

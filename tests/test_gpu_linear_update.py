"""GPU checks of the first-order update of a trajectory and its covariances for new closures (csrc/linear_update.hip,
Team.linear_update).

The graphs are covnested_ref.banded_chain(40, 3, window=8): noise-free, the ground truth T is an exact minimum, no solve.  The
closures are jointref.seeded_batch with outliers=0.0 on seeded pairs -- among the first of them pose 0 at either end, a pair and
its reverse, closures that share a pose, and from K = 22 on two exact duplicates --, their innovations rescaled to |xi_k| = 0.05.
K = 1, 2, 5, 11, 22, 43: the order 6 K = 6 .. 258 of M crosses the 32-slab and the 64-tile of the fp64 product and the blocks of
the dense inverse; 6 N = 240 is no multiple of 64.

Bounds (u = 2.2e-16; derived in tests/updateref.py, and tests/test_updateref.py shows that they reject swapped Jacobians, a
pose-0 block that is not zero, a Sigma_meas left out, a translation in the body frame and a missing mirror, each by more than
1000 x):
  the update alone, against updateref in longdouble on the blocks covariances(pairs = the rectangular set) returns for the same
    method: xi, dx, T', the blocks of Sigma', xi_post and the three figures within updateref.bounds;
  end to end, exact closures: Sigma'_pp against the covariances of a team built on the extended measurements, within
    6 (n - 1) u (cond_2(H_red) |Sigma|_F + cond_2(H'_red) |Sigma'|_F) in the Frobenius norm over all diagonal blocks.
Every test prints its largest error / bound."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import updateref as R
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_gate import blocks_call
from tests.test_gpu_gate_joint import NESTED_BLOCK, joint_call, records, setup

pytestmark = pytest.mark.gpu

F = np.float64
U = R.U
N_POSES = 40
FIXED = ((0, 5), (5, 0), (0, 39), (39, 0), (3, 17), (17, 3), (3, 20), (17, 21))
DUPLICATES = ((4, 20), (9, 21))  # (record, its exact copy further on)
PAIRS = np.array([(0, 7), (12, 12), (13, 27), (27, 13), (5, 38), (39, 1)], dtype=np.int32)  # pose 0, a = b, across robots
SIZES = (1, 2, 5, 11, 22, 43)


def closures(T, n, K, seed, scale=0.05, exact=False, normal=None):
    """K closures on seeded pairs: the relative poses of T moved so that the innovation of closure k is scale x the unit vector
    of seeded_batch's own noise draw (normal: scale x N(0, I) drawn with that seed instead; exact: zero)"""
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, K, seed, outliers=0.0, fixed=FIXED)
    rng = np.random.default_rng(normal) if normal is not None else None
    for k, (i, j) in enumerate(ends):
        Rij, tij = G.relative_pose(T, int(i), int(j), F)
        x = np.asarray(G.innovation(T, int(i), int(j), Rm[k], tm[k]), dtype=F)
        x = scale * (rng.standard_normal(6) if rng is not None else x / np.linalg.norm(x))
        if exact:
            x = np.zeros(6)
        Rm[k], tm[k] = Rij @ covref.exp_so3(-x[:3]), tij - x[3:]
    for src, dst in DUPLICATES:
        if dst < K:
            ends[dst], Rm[dst], tm[dst], kap[dst], ta[dst] = ends[src], Rm[src], tm[src], kap[src], ta[src]
    return ends, Rm, tm, kap, ta


def update_call(t, cand, T, method, **kw):
    return t.linear_update(cand, T, method=method, max_block=NESTED_BLOCK if method == "nested" else None, **kw)


def extended(m, ends, Rm, tm, kap, ta):
    """the measurements of the graph with the closures added, single-robot numbering"""
    c = np.zeros(len(ends), dtype=capi.MEAS_DTYPE)
    c["p1"], c["p2"] = ends[:, 0], ends[:, 1]
    c["R"], c["t"], c["kappa"], c["tau"], c["weight"] = Rm.reshape(-1, 9), tm, kap, ta, 1.0
    return np.concatenate([m, c])


def check_rotations(Tn, n):
    """|R'^T R' - I| <= 100 u and |det R' - 1| <= 100 u: the inputs are within about 4 u of orthonormal, Rodrigues adds about 8 u
    and the 3-term product about 3 u, so 100 u leaves a factor of five"""
    Rn = covref.rotations(Tn, n)
    orth = np.abs(np.einsum("gba,gbc->gac", Rn, Rn) - np.eye(3)).max()
    det = np.abs(np.linalg.det(Rn) - 1.0).max()
    assert orth <= 100 * U and det <= 100 * U, (orth, det)
    return max(orth, det) / (100 * U)


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_the_update_alone_at_tile_and_block_edges(N, method):
    n = N_POSES
    m, T, t = setup(n, N, method)
    X0 = t.global_X().copy()
    worst = {}
    for K in SIZES:
        ends, Rm, tm, kap, ta = closures(T, n, K, seed=17)
        cand = records(n, N, ends, Rm, tm, kap, ta)
        out = update_call(t, cand, T, method, pairs=PAIRS)
        assert out["T"].shape == (12 * n,) and out["delta"].shape == (n, 6) and out["cov_diag"].shape == (n, 6, 6)
        assert out["cov_pairs"].shape == (len(PAIRS), 6, 6) and out["xi"].shape == out["xi_post"].shape == (K, 6)
        assert out["covariance"].n == 6 * (n - 1) and out["covariance"].min_pivot > 0
        assert abs(np.linalg.norm(out["xi"], axis=1) - 0.05).max() <= 1e-9
        # 1. against updateref on the blocks the covariance call returns for the rectangular set and the pairs
        poses = sorted(set(ends.reshape(-1).tolist()))
        _, diag, cross = blocks_call(t, T, np.r_[R.rect_pairs(poses, n), PAIRS], method)
        ref = R.update(T, ends, Rm, tm, kap, ta, R.blocks_from_rect(poses, n, diag, cross), n, pairs=PAIRS)
        b = R.bounds(ref, T, ends, tm, n, PAIRS)
        for key in ("xi", "delta", "T", "cov_diag", "cov_pairs", "xi_post", "d2_joint", "logdet_M", "logdet_R"):
            r = R.ratio(np.asarray(out[key] - np.asarray(ref[key], dtype=F)), b[key])
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (K, key, r)
        assert out["information_gain"] == 0.5 * (out["logdet_M"] - out["logdet_R"]) and out["information_gain"] > 0
        assert out["cov_diag"].tobytes() == np.ascontiguousarray(out["cov_diag"].transpose(0, 2, 1)).tobytes(), "not bitwise symmetric"
        assert (out["delta"][0] == 0).all() and (out["cov_diag"][0] == 0).all() and (out["cov_pairs"][0] == 0).all()
        assert out["T"][:12].tobytes() == T[:12].tobytes()
        # the update takes uncertainty away: every diagonal block shrinks
        assert (np.einsum("gaa->g", out["cov_diag"]) <= np.einsum("gaa->g", diag) * (1 + 1e-12)).all()
        # 4. T' is on SE(3), and a following call takes it
        worst["rotations"] = max(worst.get("rotations", 0.0), check_rotations(out["T"], n))
        # 5. the joint gate's figures for the same set in the given order, all accepted
        g = joint_call(t, cand, T, method, order="given", quantile=0.999999)
        assert g["num_accepted"] == K
        tol = J.elimination_constant(K) * U * b["cond_M"] * 6 * K
        assert abs(out["d2_joint"] - g["d2_joint"]) <= tol * g["d2_joint"] and abs(out["logdet_M"] - g["logdet_joint"]) <= tol
        worst["joint"] = max(worst.get("joint", 0.0), abs(out["d2_joint"] - g["d2_joint"]) / (tol * g["d2_joint"]),
                             abs(out["logdet_M"] - g["logdet_joint"]) / tol)
        # 6. two calls: the same bytes
        if K in (11, 43):
            again = update_call(t, cand, T, method, pairs=PAIRS)
            for key in ("T", "delta", "cov_diag", "cov_pairs", "xi", "xi_post"):
                assert out[key].tobytes() == again[key].tobytes(), key
            assert (out["d2_joint"], out["logdet_M"], out["logdet_R"]) == (again["d2_joint"], again["logdet_M"], again["logdet_R"])
    res = blocks_call(t, out["T"], None, method)[0]
    assert res.n == 6 * (n - 1)
    assert t.global_X().tobytes() == X0.tobytes()
    print("%d robots, %s: largest error / bound: " % (N, method) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_end_to_end_exact_closures_against_the_extended_graph(method):
    n, N, K = N_POSES, 2, 11
    m, T, t = setup(n, N, method)
    ends, Rm, tm, kap, ta = closures(T, n, K, seed=23, exact=True)
    out = update_call(t, records(n, N, ends, Rm, tm, kap, ta), T, method)
    mx = extended(m, ends, Rm, tm, kap, ta)
    tx = team_of(mx, n, N, T)
    diag_x = blocks_call(tx, T, None, method)[1]
    _, S0, w0 = covref.dense_reference(covref.q_full(m, n), T, n)
    _, S1, w1 = covref.dense_reference(covref.q_full(mx, n), T, n)
    assert w0[0] > 0 and w1[0] > 0
    bound = 6 * (n - 1) * U * (w0[-1] / w0[0] * np.linalg.norm(S0) + w1[-1] / w1[0] * np.linalg.norm(S1))
    err = np.linalg.norm(out["cov_diag"] - diag_x)
    ref = R.update(T, ends, Rm, tm, kap, ta, R.blocks_from_sigma(0.5 * (S0 + S0.T)), n)
    b = R.bounds(ref, T, ends, tm, n)
    rd, rT = R.ratio(out["delta"], b["delta"]), R.ratio(out["T"] - T, b["T"])
    print("%s, exact closures, cond_2(H_red) %.3g -> %.3g: |Sigma'_diag - extended|_F / bound %.3g, |dx| / bound %.3g, |T' - T| / bound %.3g"
          % (method, w0[-1] / w0[0], w1[-1] / w1[0], err / bound, rd, rT))
    assert err <= bound and rd <= 1.0 and rT <= 1.0
    t.close()
    tx.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_second_order_on_the_returned_trajectory(method):
    n, N, K = N_POSES, 2, 11
    m, T, t = setup(n, N, method)
    errs, first = [], None
    for s in (1.0, 0.25, 0.0625):
        ends, Rm, tm, kap, ta = closures(T, n, K, seed=29, scale=0.05 * s, normal=5)
        out = update_call(t, records(n, N, ends, Rm, tm, kap, ta), T, method)
        xi_new = np.array([np.asarray(G.innovation(out["T"], int(i), int(j), Rm[k], tm[k]), dtype=F) for k, (i, j) in enumerate(ends)])
        errs.append(np.abs(xi_new - out["xi_post"]).max())
        first = first or (out, extended(m, ends, Rm, tm, kap, ta))
    out, mx = first
    Qx = covref.q_full(mx, n)
    f_T = covref.cost(covref.q_full(m, n), T, n)
    at_new, at_T, half = covref.cost(Qx, out["T"], n), covref.cost(Qx, T, n), 0.5 * out["d2_joint"]
    print("%s: max |xi(T') - xi_post| %.3g, %.3g, %.3g (ratios %.3g, %.3g); cost of the new graph at T' %.6g, f(T) + d2_joint / 2 = %.6g "
          "(%.3g relative), at T %.6g" % (method, errs[0], errs[1], errs[2], errs[0] / errs[1], errs[1] / errs[2], at_new, f_T + half,
                                          abs(at_new - f_T - half) / half, at_T))
    assert errs[0] / errs[1] >= 8 and errs[1] / errs[2] >= 8  # theory 16; a sign or frame mistake 4
    assert abs(at_new - f_T - half) <= 0.01 * half and at_new < at_T
    t.close()


def raw_update(t, T, method, max_block, cand, pairs, bufs, res, num=None, num_pairs=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    Tn, dx, diag, cross, xi, xp, sc = bufs
    return capi.lib().dpgo_team_linear_update(t.h, p(T), method, max_block, len(cand) if num is None else num, p(cand),
                                              (0 if pairs is None else len(pairs)) if num_pairs is None else num_pairs, p(pairs), p(Tn),
                                              p(dx), p(diag), p(cross), p(xi), p(xp), p(sc), C.byref(res))


def test_refusals_leave_the_outputs_untouched():
    n, N = N_POSES, 2
    m, T = NR.banded_chain(n, 3, window=8)
    t = team_of(m, n, N, T)
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, 2, 1, outliers=0.0, fixed=((3, 17), (30, 2)))
    good = records(n, N, ends, Rm, tm, kap, ta)
    pairs = np.array([(1, 2), (30, 4)], dtype=np.int32)
    fresh = lambda K=2, P=2: [np.full(12 * n, 7.25), np.full((n, 6), 7.25), np.full((n, 6, 6), 7.25), np.full((P, 6, 6), 7.25),
                              np.full((K, 6), 7.25), np.full((K, 6), 7.25), np.full(3, 7.25)]
    bufs, res = fresh(), capi.Covariance()

    def refused(what, cand=good, method=capi.GATE_DENSE, T_=T, pairs_=pairs, num=None, num_pairs=None, max_block=0, null=None, bufs_=None):
        res.n = 5
        b = list(bufs_ or bufs)
        if null is not None:
            b[null] = None
        rc = raw_update(t, T_, method, max_block, cand, pairs_, b, res, num, num_pairs)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg, (rc, msg)
        for a in (bufs_ or bufs):
            assert (a == 7.25).all()
        return msg

    assert refused("num must be positive", num=0).startswith("linear_update:")
    refused("num must be positive", num=-3)
    refused("num_pairs must not be negative", num_pairs=-1)
    for q in range(7):
        assert refused("null argument", null=q).startswith("linear_update:")
    refused("null argument", pairs_=None, num_pairs=2)
    refused("method must be", method=3)
    refused("method must be", method=-1)

    def changed(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k][1] = v
        return c

    refused("closure 1 names robot 2, which is not in the team", changed(r2=2))
    refused("closure 1 names pose 20 of robot 0", changed(p2=20))
    refused("closure 1 names pose -1 of robot 1", changed(p1=-1))
    refused("closure 1 joins a pose to itself", changed(r2=good["r1"][1], p2=good["p1"][1]))
    refused("both must be positive", changed(kappa=0.0))
    refused("both must be positive", changed(tau=-1.0))
    refused("both must be positive", changed(tau=float("inf")))
    bad = good.copy()
    bad["R"][1][0] *= 1.001
    refused("the measurement of closure 1 is not in SE(3)", bad)
    assert refused("pair 1 names pose 40, outside [0, 40)", pairs_=np.array([(1, 2), (30, 40)], dtype=np.int32)).startswith("linear_update:")
    refused("pair 0 names pose -1", pairs_=np.array([(-1, 2), (30, 4)], dtype=np.int32))
    # 30000 closures: three matrices of order 180000, 288 K^2 bytes each, beyond any device
    many = np.repeat(good, 15000)
    big = fresh(len(many))
    msg = refused("bytes", many, bufs_=big)
    assert "30000 closures on 4 of 40 poses" in msg and "3 x 259200000000" in msg and "are available on the device" in msg, msg
    # carried over from the covariance path, with its own message: T outside SE(3), and per method a T that is no minimum
    Tb = T.copy()
    Tb[12 * 17] *= 1.001
    refused("pose 17 of T is not in SE", T_=Tb)
    Ts = NR.spoil_rotations(T, n, [9, 10, 11, 28, 29], 50)
    for method, mb in ((capi.GATE_DENSE, 0), (capi.GATE_SCHUR, 0), (capi.GATE_NESTED, NESTED_BLOCK)):
        msg = refused("non-positive pivot", T_=Ts, method=method, max_block=mb)
        assert "not a minimum" in msg and msg.startswith("marginal_covariances"), msg
        assert bytes(res) == bytes(capi.Covariance())
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.linear_update(good, Ts)
    with pytest.raises(ValueError, match="method must be"):
        t.linear_update(good, T, method="sparse")
    with pytest.raises(ValueError, match="T holds"):
        t.linear_update(good, T[:-12])
    # and the call goes through once nothing is wrong, with and without pairs
    ok = fresh()
    assert raw_update(t, T, capi.GATE_DENSE, 0, good, pairs, ok, res) == capi.OK and res.n == 6 * (n - 1)
    assert all((a != 7.25).all() for a in ok)
    ok = fresh()
    assert raw_update(t, T, capi.GATE_SCHUR, 0, good, None, ok, res) == capi.OK
    assert (ok[3] == 7.25).all() and (ok[0] != 7.25).all()
    t.close()

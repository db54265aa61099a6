"""GPU checks of the selection of candidate closures under a budget (csrc/select.hip, Team.select_closures).

The graphs are covnested_ref.banded_chain(40, 3, window=8): noise-free, the ground truth T is an exact minimum, no solve.  The
pools are jointref.seeded_batch with the fixed pairs and duplicates of tests/test_gpu_gate_joint.py: pose 0 at either end, a
pair and its reverse, candidates that share a pose, and two exact duplicates.  Only the endpoints, kappa and tau are read.

Bounds (u = 2.2e-16; derived in tests/selectref.py, and tests/test_selectref.py shows that they reject a log det R or a factor
1/2 left out, a pivot chosen by marginal gain, a Sigma_meas left out of D and the smallest gain taken, each by more than 1000 x):
  D_k within jointref.m_block_bound; S_k|A within that and 16 (|A| + 1) u cond_2(M_AA) mag_D; a gain within half of
  sum |S^-1| b_S + 100 u cond_2(S) + 16 u (|log det S| + |log det Sigma_meas|), against selectref in longdouble on the blocks
  covariances(pairs = all pairs) returns for the same method, the device's own selection order replayed there.
Every test prints its largest error / bound."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import selectref as S
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_gate import blocks_call
from tests.test_gpu_gate_joint import DUPLICATES, NESTED_BLOCK, batch, joint_call, records, setup
from tests.test_gpu_linear_update import closures, extended, update_call

pytestmark = pytest.mark.gpu

F = np.float64
U = S.U
N_POSES = 40


def select_call(t, cand, budget, T, method, **kw):
    return t.select_closures(cand, budget, T, method=method, max_block=NESTED_BLOCK if method == "nested" else None, **kw)


def reference(t, T, n, ends, kap, ta, method):
    """(M in longdouble, its diagonal blocks' bounds, log det Sigma_meas) on the blocks the covariance call returns for all pairs
    of the endpoints, once per pool"""
    poses = sorted(set(ends.reshape(-1).tolist()))
    _, diag, cross = blocks_call(t, T, J.all_pairs(poses), method)
    M, bM = J.joint_M_dense(T, ends, kap, ta, J.blocks_from_pairs(poses, diag, cross), n)
    return M, [bM[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(len(ends))], S.logdet_meas(kap, ta)


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_selection_at_wave_and_workgroup_edges(N, method):
    n = N_POSES
    m, T, t = setup(n, N, method)
    ends, Rm, tm, kap, ta, _ = batch(T, n, 129, seed=17)
    cand = records(n, N, ends, Rm, tm, kap, ta)
    M, bD, ldR = reference(t, T, n, ends, kap, ta, method)
    X0 = t.global_X().copy()
    worst = {}
    for P in (1, 2, 63, 64, 65, 129):
        for budget in sorted(set(b for b in (1, 2, P) if b <= P)):
            out = select_call(t, cand[:P], budget, T, method)
            assert out["gain"].shape == out["gain_cond"].shape == out["rank"].shape == (P,)
            assert out["covariance"].n == 6 * (n - 1) and out["covariance"].min_pivot > 0
            assert out["num_selected"] == budget and (out["gain"] > 0).all()
            if budget == 1:
                S.check_marginal(out, M[:6 * P, :6 * P], ldR[:P], bD[:P], worst)
                assert out["selected"][0] == S.argmax_lower_index(out["gain"], np.ones(P, dtype=bool))
            S.check_replay(out, M[:6 * P, :6 * P], ldR[:P], bD[:P], "greedy", budget, worst, every=16)
            # what is not selected is worth no more than it was on its own; duplicated records: the lower index first
            assert (out["gain_cond"] <= out["gain"] * (1 + 1e-12)).all()
            for a, b in DUPLICATES:
                if b < P:
                    assert out["gain"][a] == out["gain"][b]
                    assert not (out["rank"][b] >= 0 and (out["rank"][a] < 0 or out["rank"][a] > out["rank"][b]))
    assert t.global_X().tobytes() == X0.tobytes()
    print("%d robots, %s: largest error / bound: " % (N, method) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_against_the_calls_the_device_already_has(method):
    n, N, P, b = N_POSES, 2, 65, 8
    m, T, t = setup(n, N, method)
    # R~ and t~ are T's own relative poses: the other calls read them, this one does not
    ends, Rm, tm, kap, ta = closures(T, n, P, seed=17, exact=True)
    pool = records(n, N, ends, Rm, tm, kap, ta)
    out = select_call(t, pool, b, T, method)
    sel = out["selected"]
    # the marginal gain from the gate's own relative covariance: both form S from the same blocks, each within m_block_bound
    M, bD, ldR = reference(t, T, n, ends, kap, ta, method)
    sg = t.gate(pool, T, method=method, max_block=NESTED_BLOCK if method == "nested" else None, sigma_rel=True)[4]
    worst = dict(gate=0.0)
    for k in range(P):
        Sk = sg[k] + np.asarray(G.sigma_meas(kap[k], ta[k]), dtype=F)
        g = 0.5 * (np.linalg.slogdet(Sk)[1] - float(ldR[k]))
        bound = S.gain_bound(dict(S=Sk, gain=g), 2 * bD[k], ldR[k]) + 16 * U * abs(g)  # (and slogdet's own rounding in float64)
        worst["gate"] = max(worst["gate"], abs(out["gain"][k] - g) / bound)
        assert abs(out["gain"][k] - g) <= bound, k
    # the information the update reports for the same set, and the joint gate's log det M_AA: three eliminations of the same
    # M_AA, each within jointref's elimination bound
    upd = update_call(t, pool[sel], T, method)
    jnt = joint_call(t, pool[sel], T, method, order="given", quantile=0.999999, innovation_covariance=True)
    assert jnt["num_accepted"] == b
    w = np.linalg.eigvalsh(jnt["M"])
    tol = J.elimination_constant(b) * U * (w[-1] / w[0]) * 6 * b
    worst["information_gain"] = abs(out["gain_total"] - upd["information_gain"]) / (0.5 * tol + 16 * U * b * abs(0.5 * upd["logdet_R"]))
    worst["logdet_update"] = abs(out["logdet_joint"] - upd["logdet_M"]) / tol
    worst["logdet_joint"] = abs(out["logdet_joint"] - jnt["logdet_joint"]) / tol
    print("%s: gain_total %.12g, information_gain %.12g, logdet_joint %.12g / %.12g; largest error / bound: "
          % (method, out["gain_total"], upd["information_gain"], out["logdet_joint"], jnt["logdet_joint"])
          + ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    t.close()


@pytest.mark.parametrize("method", ["dense", "schur", "nested"])
def test_end_to_end_against_the_log_det_of_the_extended_graph(method):
    n, N, P, b = N_POSES, 2, 30, 11
    m, T, t = setup(n, N, method)
    ends, Rm, tm, kap, ta = closures(T, n, P, seed=23, exact=True)
    out = select_call(t, records(n, N, ends, Rm, tm, kap, ta), b, T, method)
    sel = out["selected"]
    mx = extended(m, ends[sel], Rm[sel], tm[sel], kap[sel], ta[sel])
    tx = team_of(mx, n, N, T)
    res_x = blocks_call(tx, T, None, method)[0]
    want = 0.5 * (res_x.logdet - out["covariance"].logdet)
    _, S0, w0 = covref.dense_reference(covref.q_full(m, n), T, n)
    _, S1, w1 = covref.dense_reference(covref.q_full(mx, n), T, n)
    assert w0[0] > 0 and w1[0] > 0
    bound = 6 * (n - 1) * U * (w0[-1] / w0[0] * np.linalg.norm(S0) + w1[-1] / w1[0] * np.linalg.norm(S1))
    err = abs(out["gain_total"] - want)
    host = 0.5 * (np.sum(np.log(w1)) - np.sum(np.log(w0)))
    print("%s, exact closures, cond_2(H_red) %.3g -> %.3g: gain_total %.12g, (log det H' - log det H) / 2 = %.12g on the device, %.12g "
          "by numpy; error / bound %.3g" % (method, w0[-1] / w0[0], w1[-1] / w1[0], out["gain_total"], want, host, err / bound))
    assert want > 0 and err <= bound and abs(out["gain_total"] - host) <= bound
    t.close()
    tx.close()


@pytest.mark.parametrize("method", ["dense", "nested"])
def test_stopping_and_both_orders(method):
    n, N, P = N_POSES, 2, 65
    m, T, t = setup(n, N, method)
    ends, Rm, tm, kap, ta, _ = batch(T, n, P, seed=17)
    pool = records(n, N, ends, Rm, tm, kap, ta)
    full = select_call(t, pool, P, T, method)
    sel = full["selected"]
    at = full["gain_cond"][sel]
    assert full["num_selected"] == P and sorted(sel.tolist()) == list(range(P))
    # a threshold between two consecutive gains at selection stops the call at that step
    s = next(q for q in range(7, P - 1) if at[q] > at[q + 1])
    cut = select_call(t, pool, P, T, method, min_gain=0.5 * (at[s] + at[s + 1]))
    assert cut["num_selected"] == s + 1 and list(cut["selected"]) == list(sel[:s + 1])
    assert cut["gain_cond"][sel[:s + 1]].tobytes() == at[:s + 1].tobytes()
    assert cut["gain_total"] == float(np.cumsum(at[:s + 1])[-1])
    assert (cut["rank"][sel[s + 1:]] == -1).all() and (cut["gain_cond"][sel[s + 1:]] <= 0.5 * (at[s] + at[s + 1])).all()
    # a threshold above every gain selects nothing
    none = select_call(t, pool, 5, T, method, min_gain=float(full["gain"].max()))
    assert none["num_selected"] == 0 and len(none["selected"]) == 0 and none["gain_total"] == 0.0 and none["logdet_joint"] == 0.0
    assert none["gain_cond"].tobytes() == none["gain"].tobytes() == full["gain"].tobytes() and (none["rank"] == -1).all()
    # order="given" on greedy's own sequence: the same gains, bit for bit
    b = 20
    g = select_call(t, pool, b, T, method)
    perm = np.r_[g["selected"], np.setdiff1d(np.arange(P), g["selected"])]
    v = select_call(t, pool[perm], b, T, method, order="given")
    assert list(v["selected"]) == list(range(b)) and (v["rank"][:b] == np.arange(b)).all() and (v["rank"][b:] == -1).all()
    assert v["gain_cond"].tobytes() == g["gain_cond"][perm].tobytes() and v["gain"].tobytes() == g["gain"][perm].tobytes()
    assert (v["gain_total"], v["logdet_joint"]) == (g["gain_total"], g["logdet_joint"])
    # order="given" with budget b takes candidates 0 .. b - 1, and prices a plan that is not greedy's no higher in total
    plain = select_call(t, pool, b, T, method, order="given")
    assert list(plain["selected"]) == list(range(b)) and plain["gain_total"] < g["gain_total"]
    M, bD, ldR = reference(t, T, n, ends, kap, ta, method)
    worst = {}
    S.check_replay(plain, M, ldR, bD, "given", b, worst, every=16)
    print("%s: greedy %.9g, candidates 0 .. %d as given %.9g; the given order: largest error / bound: " % (method, g["gain_total"], b - 1, plain["gain_total"])
          + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


def test_two_calls_give_the_same_bytes():
    n, N, P, b = N_POSES, 3, 129, 40
    m, T, t = setup(n, N, "schur")
    ends, Rm, tm, kap, ta, _ = batch(T, n, P, seed=26)
    pool = records(n, N, ends, Rm, tm, kap, ta)
    X0 = t.global_X().copy()
    one, two = select_call(t, pool, b, T, "schur"), select_call(t, pool, b, T, "schur")
    for key in ("gain", "gain_cond", "rank", "selected"):
        assert one[key].tobytes() == two[key].tobytes(), key
    assert (one["num_selected"], one["gain_total"], one["logdet_joint"]) == (two["num_selected"], two["gain_total"], two["logdet_joint"])
    # R~, t~ and the weight are not read: records built from the pairs alone give the same bytes
    bare = t.candidates_from_pairs(ends, kap, ta)
    assert bare["r1"].tobytes() == pool["r1"].tobytes() and bare["p2"].tobytes() == pool["p2"].tobytes()
    three = select_call(t, bare, b, T, "schur")
    for key in ("gain", "gain_cond", "rank"):
        assert one[key].tobytes() == three[key].tobytes(), key
    assert t.global_X().tobytes() == X0.tobytes()
    t.close()


def raw_select(t, T, method, max_block, cand, order, budget, min_gain, bufs, res, num=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    gain, gc, rk, ns, gt, lj = bufs
    return capi.lib().dpgo_team_select_candidates(t.h, p(T), method, max_block, len(cand) if num is None else num, p(cand), order, budget,
                                                  C.c_double(min_gain), p(gain), p(gc), p(rk), p(ns), p(gt), p(lj),
                                                  C.byref(res) if res is not None else None)


def test_refusals_leave_the_outputs_untouched():
    import torch
    n, N = N_POSES, 2
    m, T = NR.banded_chain(n, 3, window=8)
    t = team_of(m, n, N, T)
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, 2, 1, fixed=((3, 17), (30, 2)))
    good = records(n, N, ends, Rm, tm, kap, ta)
    fresh = lambda P=2: [np.full(P, 7.25), np.full(P, 7.25), np.full(P, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32),
                         np.full(1, 7.25), np.full(1, 7.25)]
    bufs, res = fresh(), capi.Covariance()

    def refused(what, cand=good, method=capi.GATE_DENSE, T_=T, order=capi.JOINT_GREEDY, budget=1, min_gain=-np.inf, num=None, max_block=0,
                null=None, bufs_=None, res_=res):
        res.n = 5
        b = list(bufs_ or bufs)
        if null is not None:
            b[null] = None
        rc = raw_select(t, T_, method, max_block, cand, order, budget, min_gain, b, res_, num)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg, (rc, msg)
        for a in (bufs_ or bufs):
            assert (a == (7 if a.dtype == np.int32 else 7.25)).all()
        return msg

    assert refused("num must be positive", num=0).startswith("select_candidates:")
    refused("num must be positive", num=-3)
    for q in range(6):
        assert refused("null argument", null=q).startswith("select_candidates:")
    refused("null argument", T_=None)
    refused("null argument", res_=None)
    refused("null argument", cand=None, num=2)
    assert refused("budget must lie in [1, 2], not 0", budget=0).startswith("select_candidates:")
    refused("budget must lie in [1, 2], not 3", budget=3)
    refused("budget must lie in [1, 2], not -1", budget=-1)
    refused("method must be", method=3)
    refused("method must be", method=-1)
    refused("order must be DPGO_JOINT_GREEDY or DPGO_JOINT_GIVEN, not 2", order=2)
    refused("order must be", order=-1)
    assert refused("min_gain must not be NaN", min_gain=float("nan")).startswith("select_candidates:")

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
    refused("both must be positive", changed(tau=float("inf")))
    assert refused("both must be positive", changed(kappa=float("nan"))).startswith("select_candidates: candidate 1 has kappa")
    # a pool of 30000 with budget 30000: a factor of 288 x 30000^2 bytes.  A device with more than that free is first filled
    # up to half of it, so that the case is the same on every device
    many = np.repeat(good, 15000)
    big = fresh(len(many))
    need = 288 * 30000 * 30000
    free = torch.cuda.mem_get_info()[0]
    ballast = torch.empty(int(free - need // 2), dtype=torch.uint8, device="cuda") if free >= need // 2 else None
    msg = refused("bytes", many, budget=30000, bufs_=big)
    del ballast
    torch.cuda.empty_cache()
    assert "30000 candidates on 4 poses, budget 30000" in msg and "the factor of 30000 x 30000 blocks" in msg, msg
    assert "+ 259200000000 +" in msg and "are available on the device" in msg, msg
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
        t.select_closures(good, 1, Ts)
    with pytest.raises(ValueError, match="method must be"):
        t.select_closures(good, 1, T, method="sparse")
    with pytest.raises(ValueError, match="order must be"):
        t.select_closures(good, 1, T, order="random")
    with pytest.raises(capi.DpgoError, match="budget must lie in"):
        t.select_closures(good, 3, T)
    with pytest.raises(ValueError, match="T holds"):
        t.select_closures(good, 1, T[:-12])
    # R~ and t~ are not read: a record whose R~ is no rotation goes through, and the call goes through once nothing is wrong
    bad = good.copy()
    bad["R"][1][0] *= 1.5
    ok = fresh()
    assert raw_select(t, T, capi.GATE_DENSE, 0, bad, capi.JOINT_GIVEN, 2, -np.inf, ok, res) == capi.OK and res.n == 6 * (n - 1)
    assert (ok[0] != 7.25).all() and (ok[1] != 7.25).all() and list(ok[2]) == [0, 1] and ok[3][0] == 2 and ok[4][0] != 7.25 and ok[5][0] != 7.25
    t.close()

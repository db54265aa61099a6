"""CPU checks of tests/removalref.py, the numpy statement of the first-order removal or down-weighting of measurements that are
in the graph: the covariance form against the information form, the exact round trip with updateref, an actual
re-solve of a linear Gaussian graph, K = 1 against auditref, the second-order behaviour of the round trip, the bounds of the
GPU tests (tests/test_gpu_linear_removal.py) against the mistakes the conventions invite, and a cut of three edges that only the
joint pivot sees.  The last test is the one that fails where the call does not exist.

The graphs are banded_chain(12, seed, window=8), seeds 1 - 3: 14 / 14 / 13 edges with cyclomatic numbers 3 / 3 / 2, so a full
removal takes at most two closures and the larger sets are down-weighted by half."""
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import auditref as AR
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import removalref as V
from tests import updateref as R
from tests import test_updateref as TU
from tests.test_auditref import linear_graph, linear_solve
from tests.util import ROOT

F = np.float64
U = V.U
N_POSES = 12


def problem(seed, weights=None):
    n = N_POSES
    m, T = NR.banded_chain(n, seed, window=8)
    if weights is not None:
        m = m.copy()
        m["weight"] = weights(len(m))
    Hr, Sigma, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    return dict(n=n, m=m, T=T, Hr=0.5 * (Hr + Hr.T), Sigma=0.5 * (Sigma + Sigma.T), cond=w[-1] / w[0])


def records_of(P, idx, scale=0.05, seed=11):
    """the edges idx of the graph as records whose measurements are moved so that the innovation of record k at T is scale x a
    seeded unit vector (0: the exact relative pose)"""
    rng = np.random.default_rng(seed)
    m, T = P["m"], P["T"]
    ends = np.array([(int(m["p1"][e]), int(m["p2"][e])) for e in idx], dtype=np.int64)
    Rm, tm = np.zeros((len(idx), 3, 3)), np.zeros((len(idx), 3))
    for k, (i, j) in enumerate(ends):
        Rij, tij = G.relative_pose(T, int(i), int(j), F)
        x = rng.standard_normal(6)
        x = scale * x / np.linalg.norm(x)
        Rm[k], tm[k] = Rij @ covref.exp_so3(-x[:3]), tij - x[3:]
    return dict(ends=ends, Rm=Rm, tm=tm, kappa=np.array(m["kappa"][idx], dtype=F), tau=np.array(m["tau"][idx], dtype=F),
                w=np.array(m["weight"][idx], dtype=F))


def closures_of(P):
    return [e for e in range(len(P["m"])) if abs(int(P["m"]["p2"][e]) - int(P["m"]["p1"][e])) != 1]


def run(P, rec, w_new=None, Sigma=None, T=None, **kw):
    blocks = R.blocks_from_sigma(P["Sigma"] if Sigma is None else Sigma, kw.get("pairs", ()))
    return V.removal(P["T"] if T is None else T, rec["ends"], rec["Rm"], rec["tm"], rec["kappa"], rec["tau"], rec["w"], w_new, blocks, P["n"], **kw)


def full_sigma(ref, Sigma):
    """Sigma' of the free poses, 6 (n - 1) square, from B~ and U~"""
    Sp = ref["U"] @ ref["Bt"].T
    return Sigma + 0.5 * (Sp + Sp.T)[6:, 6:]


def mixed_set(P):
    """two closures removed fully and four other edges down-weighted by half, among them the first odometry edge (pose 0)"""
    clo = closures_of(P)[:2]
    rest = [e for e in range(len(P["m"])) if e not in clo]
    idx = clo + [rest[0], rest[3], rest[6], rest[9]]
    w_new = np.array([0.0, 0.0, 0.5, 0.5, 0.5, 0.5])
    return idx, w_new


def test_covariance_form_against_information_form():
    """tolerance 100 u cond_2(H) relative, H the reduced Hessian of the graph whose Sigma is given, as in test_updateref.py"""
    for seed in (1, 2, 3):
        P = problem(seed)
        idx, w_new = mixed_set(P)
        rec = records_of(P, idx)
        ref = run(P, rec, w_new)
        assert ref["testable"] and float(ref["pivot_min_joint"]) > 1e-3
        Sp, dx, Hp = V.information_form(P["Hr"], P["T"], rec["ends"], rec["kappa"], rec["tau"], ref["dw"], ref["xi"], P["n"])
        wp = np.linalg.eigvalsh(Hp)
        assert wp[0] > 0
        tol = 100 * U * P["cond"]
        eS = np.abs(np.asarray(full_sigma(ref, P["Sigma"]), dtype=F) - Sp).max() / np.abs(Sp).max()
        ed = np.abs(np.asarray(ref["delta"], dtype=F).reshape(-1)[6:] - dx).max() / np.abs(dx).max()
        for p in range(P["n"]):
            want = Sp[6 * p - 6:6 * p, 6 * p - 6:6 * p] if p else np.zeros((6, 6))
            assert np.abs(np.asarray(ref["cov_diag"][p], dtype=F) - want).max() <= tol * np.abs(Sp).max()
        # log det H' - log det H = log det N - log det R, and the fully removed pair alone is the graph without those edges
        ld = np.linalg.slogdet(Hp)[1] - np.linalg.slogdet(P["Hr"])[1]
        eL = abs(float(ref["logdet_N"] - ref["logdet_R"]) - ld)
        print("seed %d, cond_2(H) = %.3g, cond_2(H') = %.3g, smallest pivot of N~ %.3g: Sigma' %.3g, dx %.3g relative (tolerance %.3g), log det %.3g"
              % (seed, P["cond"], wp[-1] / wp[0], float(ref["pivot_min_joint"]), eS, ed, tol, eL))
        assert eS <= tol and ed <= tol and eL <= tol * abs(ld)
        assert float(ref["information_loss"]) > 0
        assert (np.asarray(ref["delta"][0], dtype=F) == 0).all() and (np.asarray(ref["cov_diag"][0], dtype=F) == 0).all()
        # xi_loo = R N^-1 xi is xi + A dx
        lhs = np.asarray(ref["xi"].reshape(-1) + ref["A"] @ ref["delta"].reshape(-1), dtype=F)
        assert np.abs(lhs - np.asarray(ref["xi_loo"], dtype=F).reshape(-1)).max() <= 1e-12 * np.abs(lhs).max()
        full = run(P, records_of(P, idx[:2]))
        _, Sx, wx = covref.dense_reference(covref.q_full(np.delete(P["m"], idx[:2]), P["n"]), P["T"], P["n"])
        assert np.abs(np.asarray(full_sigma(full, P["Sigma"]), dtype=F) - Sx).max() <= tol * np.abs(Sx).max()


def test_exact_round_trip_with_the_update():
    """updateref adds ten exact closures; the removal of the same ten at weight 1 from its Sigma' returns Sigma within the sum
    of the two bounds, and dx = 0 within its bound"""
    for seed in (1, 2, 3):
        Pu = TU.problem(seed)
        Rm, tm = TU.exact(Pu)
        up = TU.run(Pu, Rm, tm)
        b_up = R.bounds(up, Pu["T"], Pu["ends"], tm, Pu["n"])
        Sx = Pu["Sigma"] - (0.5 * (up["U"] @ up["B"].T + (up["U"] @ up["B"].T).T))[6:, 6:]  # (longdouble)
        rec = dict(ends=Pu["ends"], Rm=Rm, tm=tm, kappa=Pu["kappa"], tau=Pu["tau"], w=np.ones(len(Rm)))
        back = run(Pu, rec, Sigma=Sx)
        b = V.bounds(back, Pu["T"], Pu["ends"], tm, Pu["n"])
        worst = 0.0
        for p in range(Pu["n"]):
            want = Pu["Sigma"][6 * p - 6:6 * p, 6 * p - 6:6 * p] if p else np.zeros((6, 6))
            worst = max(worst, V.ratio(np.asarray(back["cov_diag"][p], dtype=F) - want, b["cov_diag"][p] + b_up["cov_diag"][p]))
        rd = V.ratio(back["delta"], b["delta"])
        print("seed %d: round trip, cond_2(N~) = %.3g: |Sigma'' - Sigma| / (sum of the bounds) %.3g, |dx| / bound %.3g"
              % (seed, b["cond_N"], worst, rd))
        assert worst <= 1.0 and rd <= 1.0
        # what the update gained the removal loses
        assert abs(float(back["information_loss"] - up["information_gain"])) <= 1e-12 * abs(float(up["information_gain"]))


def test_against_a_real_re_solve_of_a_linear_gaussian_graph():
    """test_auditref's 8-node ring with chords, two chords taken out jointly (one fully, one to 0.37 of its weight): for a
    linear graph the formulas are exact, and the two sides are float64 inverses of H and H' and a division by N~:
    64 u (cond_2(H) + cond_2(H')) cond_2(N~) relative"""
    n, edges, kap, tau, w, y = linear_graph(1)
    w = w.copy()
    w[9], w[10] = 1.0, 0.6
    take, w_new = [9, 10], np.array([0.0, 0.6 * 0.37])
    x, S, cH = linear_solve(n, edges, kap, tau, w, y)
    w1 = w.copy()
    w1[take] = w_new
    x1, S1, cH1 = linear_solve(n, edges, kap, tau, w1, y)
    A = np.zeros((12, 6 * (n - 1)))
    for k, e in enumerate(take):
        i, j = edges[e]
        for p, sgn in ((i, -1.0), (j, 1.0)):
            if p > 0:
                A[6 * k:6 * k + 6, 6 * (p - 1):6 * p] = sgn * np.eye(6)
    s = np.concatenate([np.asarray(AR.scaling(kap[e], tau[e], F)) * np.sqrt(w[e] - w_new[k]) for k, e in enumerate(take)])
    xi = np.concatenate([x[edges[e][1]] - x[edges[e][0]] - y[e] for e in take])
    out = V.core(A, S, s, xi, dtype=F)
    cost = lambda xx, ww: 0.5 * sum(ww[e] * np.sum((np.asarray(AR.scaling(kap[e], tau[e], F)) * (xx[j] - xx[i] - y[e])) ** 2)
                                    for e, (i, j) in enumerate(edges))
    ev = np.linalg.eigvalsh(out["Nt"])
    tol = 64 * U * (cH + cH1) * ev[-1] / ev[0]
    xi1 = np.concatenate([x1[edges[e][1]] - x1[edges[e][0]] - y[e] for e in take])
    errs = dict(Sigma=np.abs(out["Sigma"] - S1).max() / np.abs(S1).max(),
                x=np.abs(x.reshape(-1)[6:] + out["dx"] - x1.reshape(-1)[6:]).max() / np.abs(x1).max(),
                xi_loo=np.abs(out["xi_loo"] - xi1).max() / np.abs(xi1).max(),
                cost=abs(cost(x, w) - 0.5 * out["d2_joint"] - cost(x1, w1)) / cost(x1, w1))
    print("linear re-solve, cond_2(H) %.3g, cond_2(H') %.3g, cond_2(N~) %.3g, smallest pivot %.3g: " % (cH, cH1, ev[-1] / ev[0], out["pivot_min_joint"])
          + ", ".join("%s %.3g" % kv for kv in errs.items()) + " relative (tolerance %.3g)" % tol)
    assert all(v <= tol for v in errs.values()), errs
    assert 0 < out["pivot_min_joint"] <= 1


@pytest.mark.parametrize("w", [1.0, 0.37, 1e-3])
def test_one_record_is_the_audit(w):
    """K = 1, the edge in the graph at weight w and removed: xi_loo and pivot_min are the audit's, and at w = 1 d2_joint is its d2,
    within the sum of the two references' bounds"""
    worst = dict(xi_loo=0.0, pivot_min=0.0, d2=0.0)
    for seed in (1, 2, 3):
        P0 = problem(seed)
        e = closures_of(P0)[0]
        P = problem(seed, lambda L: np.where(np.arange(L) == e, w, 1.0))
        rec = records_of(P, [e])
        (i, j), Rm, tm = rec["ends"][0], rec["Rm"][0], rec["tm"][0]
        i, j = int(i), int(j)
        blocks = G.blocks_of(P["Sigma"], i, j)
        a = AR.audit(P["T"], i, j, Rm, tm, rec["kappa"][0], rec["tau"][0], w, *blocks)
        assert a["testable"] and float(a["pmin"]) > 1e-3
        ba = AR.record_bounds(P["T"], i, j, tm, *blocks, a)
        ref = run(P, rec)
        b = V.bounds(ref, P["T"], rec["ends"], rec["tm"], P["n"])
        worst["xi_loo"] = max(worst["xi_loo"], V.ratio(np.asarray(ref["xi_loo"][0] - a["xi_loo"], dtype=F), b["xi_loo"][0] + ba["xi_loo"]))
        worst["pivot_min"] = max(worst["pivot_min"], abs(float(ref["pivot_min"][0] - a["pmin"])) / (b["pivot_min"][0] + ba["pmin"]))
        assert abs(float(ref["pivot_min_joint"] - a["pmin"])) <= b["pivot_min_joint"] + ba["pmin"]
        if w == 1.0:
            worst["d2"] = max(worst["d2"], abs(float(ref["d2_joint"] - a["d2"])) / (b["d2_joint"] + ba["d2"]))
        else:
            assert abs(float(ref["d2_joint"] - a["d2"])) > 1000 * (b["d2_joint"] + ba["d2"])  # with a fractional weight it is NOT the audit's d2
    print("w = %g: |removal - audit| / (sum of the bounds): " % w + ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def round_trip(P, closures, s, remove):
    """at the ground truth updateref adds the closures off by 0.05 s, giving T'; `remove` at T' from the dense reference of the
    extended graph gives T'': max |T'' - T|"""
    Rm, tm = TU.off_by(P, s)
    up = TU.run(P, Rm, tm)
    T1 = np.asarray(up["T"], dtype=F)
    _, Sx, wx = covref.dense_reference(covref.q_full(TU.extended(P, Rm, tm), P["n"]), T1, P["n"])
    assert wx[0] > 0
    rec = dict(ends=P["ends"], Rm=Rm, tm=tm, kappa=P["kappa"], tau=P["tau"], w=np.ones(len(Rm)))
    T2 = remove(rec, 0.5 * (Sx + Sx.T), T1)
    return np.abs(np.asarray(T2, dtype=F) - P["T"]).max()


def test_the_round_trip_is_right_to_second_order():
    for seed in (1, 2, 3):
        P = TU.problem(seed)
        errs = [round_trip(P, None, s, lambda rec, Sx, T1: run(P, rec, Sigma=Sx, T=T1)["T"]) for s in (1.0, 0.25, 0.0625)]
        print("seed %d: max |T'' - T| %.3g, %.3g, %.3g (ratios %.3g, %.3g)" % (seed, errs[0], errs[1], errs[2], errs[0] / errs[1], errs[1] / errs[2]))
        assert errs[0] / errs[1] >= 8 and errs[1] / errs[2] >= 8, errs  # theory 16; a sign mistake 4
    P = TU.problem(1)
    errs = [round_trip(P, None, s, lambda rec, Sx, T1: run(P, rec, Sigma=Sx, T=T1, mistake="dx_sign")["T"]) for s in (1.0, 0.25, 0.0625)]
    assert errs[0] / errs[1] < 8


def test_the_bounds_reject_the_mistakes_the_conventions_invite():
    """each of them moves a figure by more than 1000 x the bound the GPU test holds that figure to"""
    P = problem(2, lambda L: np.where(np.arange(L) % 3 == 0, 0.8, 1.0))
    idx, w_new = mixed_set(P)
    w_new = w_new * P["m"]["weight"][idx]
    rec = records_of(P, idx)
    pairs = [(3, 9)]
    ref = run(P, rec, w_new, pairs=pairs)
    b = V.bounds(ref, P["T"], rec["ends"], rec["tm"], P["n"], pairs)
    # (float64 itself stays inside)
    f64 = run(P, rec, w_new, pairs=pairs, dtype=F)
    for key in ("Bt", "Nt", "delta", "cov_diag", "cov_pairs", "xi_loo", "T", "pivot_min"):
        assert V.ratio(np.asarray(f64[key], dtype=F) - np.asarray(ref[key], dtype=F), b[key]) <= 1.0, key
    for key in ("d2_joint", "logdet_N", "logdet_R", "pivot_min_joint"):
        assert abs(float(f64[key] - ref[key])) <= b[key], key

    def worst(key, mistake):
        other = run(P, rec, w_new, pairs=pairs, mistake=mistake)
        err = np.abs(np.asarray(other[key], dtype=F) - np.asarray(ref[key], dtype=F))
        bound = np.broadcast_to(b[key], np.shape(err))
        return float((err[bound > 0] / bound[bound > 0]).max())

    ratios = dict(dx_sign=worst("delta", "dx_sign"), sigma_minus=worst("cov_diag", "sigma_minus"), dw_as_w=worst("Nt", "dw_as_w"),
                  logdet_dw_left_out=worst("logdet_R", "logdet_dw_left_out"), n_plus=worst("Nt", "n_plus"),
                  scaled_once=worst("Nt", "scaled_once"))
    assert set(ratios) == set(V.MISTAKES)
    print("cond_2(N~) = %.3g; mistake -> error / bound: " % b["cond_N"] + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    assert all(v > 1000.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("n,seed", [(12, 1), (12, 2), (40, 3)])
def test_a_cut_of_three_edges_shows_in_the_joint_pivot_alone(n, seed):
    """two closures around one loop are each testable alone, and so is the odometry edge between them; together the three cut
    the graph, which no per-record figure shows: pivot_min >= 1e-3 for each, pivot_min_joint <= 1e-6.  (banded_chain(12, 3) has two loops that share no
    edge, and so no such triple; the 40-pose graph is the one the GPU test refuses on.)"""
    m, T = NR.banded_chain(n, seed, window=8)
    triple = V.cut_triple(m, n)
    assert triple is not None
    _, Sigma, ev = covref.dense_reference(covref.q_full(m, n), T, n)
    P = dict(n=n, m=m, T=T, Sigma=0.5 * (Sigma + Sigma.T))
    ref = run(P, records_of(P, list(triple)))
    pm, pj = np.asarray(ref["pivot_min"], dtype=F), float(ref["pivot_min_joint"])
    print("banded_chain(%d, %d): the edges %s cut the graph together: pivot_min %s, pivot_min_joint %.3g"
          % (n, seed, [(int(m["p1"][e]), int(m["p2"][e])) for e in triple], pm, pj))
    assert (pm >= 1e-3).all() and pj <= 1e-6
    # any two of them leave redundancy
    for drop in range(3):
        two = [e for k, e in enumerate(triple) if k != drop]
        assert float(run(P, records_of(P, two))["pivot_min_joint"]) >= 1e-3


def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+dpgo_team_linear_removal\s*\(", header)
    assert "dpgo_team_linear_removal" in capi.EXPORTS
    assert hasattr(capi.lib(), "dpgo_team_linear_removal")
    assert callable(getattr(capi.Team, "linear_removal", None))

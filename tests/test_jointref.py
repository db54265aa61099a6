"""CPU checks of tests/jointref.py, the numpy statement of the joint gate of a set of candidates: the conditional
test against its information form and against the 12 x 12 closed form, the order-independence of the joint figures, and the
bounds of the GPU tests (tests/test_gpu_gate_joint.py) against the mistakes the conventions invite.  The last test is the one
that fails where the call does not exist."""
import os
import re

import numpy as np

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests.util import ROOT

F = np.float64
THR2 = capi.error_threshold_at_quantile(0.99, 6) ** 2


def problem(seed, K=24, n=12, fixed=((0, 5), (5, 0), (3, 9), (9, 3), (3, 7), (2, 3))):
    m, T = NR.banded_chain(n, seed, window=8)
    Hr, Sigma, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    Sigma = 0.5 * (Sigma + Sigma.T)  # (the inverse LAPACK returns is symmetric to rounding only)
    ends, Rm, tm, kap, ta, inl = J.seeded_batch(T, n, K, seed + 100, fixed=fixed)
    blk = J.blocks_from_sigma(Sigma)
    M = J.joint_M(T, ends, kap, ta, blk)
    xi = J.innovations(T, ends, Rm, tm)
    return dict(n=n, T=T, Hr=Hr, Sigma=Sigma, ends=ends, Rm=Rm, tm=tm, kappa=kap, tau=ta, inlier=inl, blk=blk, M=M, xi=xi)


def test_the_conditional_test_is_the_gate_after_the_accepted_set_joined_the_graph():
    """the information form: with Sigma' = (H + A_A^T R_A^-1 A_A)^-1 and dx = -Sigma' A_A^T R_A^-1 xi_A, the pair
    (xi_k + A_k dx, A_k Sigma' A_k^T + R_k) is (xi_k|A, S_k|A)"""
    worst = 0.0
    for seed in (1, 2):
        P = problem(seed)
        K, n = len(P["ends"]), P["n"]
        A = np.asarray(J.a_matrix(P["T"], P["ends"], n), dtype=F)
        M, xi = np.asarray(P["M"], dtype=F), np.asarray(P["xi"], dtype=F).reshape(-1)
        Rb = np.zeros_like(M)
        for k in range(K):
            Rb[6 * k:6 * k + 6, 6 * k:6 * k + 6] = np.asarray(G.sigma_meas(P["kappa"][k], P["tau"][k]), dtype=F)
        assert np.abs(A @ P["Sigma"] @ A.T + Rb - M).max() <= 1e-13 * np.abs(M).max()  # M from the blocks is A Sigma A^T + R
        for acc in ([0], [3, 1], [5, 4, 0, 7, 2], list(range(0, K, 2))):
            E = J.Elimination(P["M"], P["xi"])
            for p in acc:
                E.pivot(p)
            rows = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in acc])
            AA = A[rows]
            Rinv = np.zeros((len(rows), len(rows)))
            for q, k in enumerate(acc):
                Rinv[6 * q:6 * q + 6, 6 * q:6 * q + 6] = np.linalg.inv(np.asarray(G.sigma_meas(P["kappa"][k], P["tau"][k]), dtype=F))
            Sp = np.linalg.inv(P["Hr"] + AA.T @ Rinv @ AA)
            dx = -Sp @ AA.T @ Rinv @ xi[rows]
            for k in np.flatnonzero(E.open):
                Ak = A[6 * k:6 * k + 6]
                x_info = xi[6 * k:6 * k + 6] + Ak @ dx
                S_info = Ak @ Sp @ Ak.T + np.asarray(G.sigma_meas(P["kappa"][k], P["tau"][k]), dtype=F)
                ex = np.abs(x_info - np.asarray(E.x[k], dtype=F)).max() / max(np.abs(xi[6 * k:6 * k + 6]).max(), 1e-300)
                eS = np.abs(S_info - np.asarray(E.D[k], dtype=F)).max() / np.abs(M[6 * k:6 * k + 6, 6 * k:6 * k + 6]).max()
                worst = max(worst, ex, eS)
    print("information form against the elimination: largest relative difference %.3g" % worst)
    assert worst <= 1e-9


def test_joint_figures_do_not_depend_on_the_order():
    for seed in (1, 2, 3):
        P = problem(seed)
        M, xi = np.asarray(P["M"], dtype=F), np.asarray(P["xi"], dtype=F).reshape(-1)
        g, v = J.run(P["M"], P["xi"], THR2, "greedy"), J.run(P["M"], P["xi"], THR2, "given")
        for r in (g, v):
            acc = r["accepted"]
            assert len(acc) >= 4 and len(acc) < len(P["ends"])
            rows = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in acc])
            MA = M[np.ix_(rows, rows)]
            dj = xi[rows] @ np.linalg.solve(MA, xi[rows])
            assert abs(float(r["d2_joint"]) - dj) <= 1e-10 * dj
            assert abs(float(sum(r["d2_cond"][acc])) - dj) <= 1e-10 * dj
            assert abs(float(r["logdet_joint"]) - np.linalg.slogdet(MA)[1]) <= 1e-10 * abs(np.linalg.slogdet(MA)[1])
            assert (np.sort(r["rank"][acc]) == np.arange(len(acc))).all() and (r["rank"][~r["accept"]] == -1).all()
        # the same set in another order: the same joint figures
        same = J.run(P["M"], P["xi"], THR2, "given", pivots=g["accepted"])
        assert sorted(same["accepted"]) == sorted(g["accepted"]) and list(same["accepted"]) != list(g["accepted"])
        assert abs(float(same["d2_joint"] - g["d2_joint"])) <= 1e-14 * float(g["d2_joint"])
        assert abs(float(same["logdet_joint"] - g["logdet_joint"])) <= 1e-14 * abs(float(g["logdet_joint"]))


def closed_form_pair(T, Sigma, i=3, j=9, kappa=100.0, tau=50.0):
    """two candidates on the pair (i, j) whose measurements differ by far more than their noise (0.6 rad, 0.8 m), each within
    Sigma_rel of the estimate -- the fixture of the closed-form test, here and on the GPU"""
    Rij, tij = G.relative_pose(T, i, j, F)
    Sr = np.asarray(G.sigma_rel(T, i, j, *G.blocks_of(Sigma, i, j)), dtype=F)
    w, V = np.linalg.eigh(Sr)
    step = 1.2 * np.sqrt(w[-1]) * V[:, -1]  # 1.2 sigma along the widest direction of Sigma_rel, either way
    ends = np.array([(i, j), (i, j)])
    Rm = np.array([Rij @ covref.exp_so3(-step[:3]), Rij @ covref.exp_so3(step[:3])])
    tm = np.array([tij - step[3:], tij + step[3:]])
    return ends, Rm, tm, np.full(2, kappa), np.full(2, tau), Sr


def test_two_contradicting_candidates_on_one_pair_against_the_closed_form():
    n = 12
    m, T = NR.banded_chain(n, 5, window=8)
    _, Sigma, _ = covref.dense_reference(covref.q_full(m, n), T, n)
    Sigma = 0.5 * (Sigma + Sigma.T)
    ends, Rm, tm, kap, ta, Sr = closed_form_pair(T, Sigma)
    R1 = np.asarray(G.sigma_meas(kap[0], ta[0]), dtype=F)
    xi = np.asarray(J.innovations(T, ends, Rm, tm), dtype=F)
    apart = np.sqrt((xi[0] - xi[1]) @ np.linalg.solve(2 * R1, xi[0] - xi[1]))  # in standard deviations of their difference's noise
    assert apart > 10, "the two do not contradict each other"
    M = J.joint_M(T, ends, kap, ta, J.blocks_from_sigma(Sigma))
    for order in ("greedy", "given"):
        r = J.run(M, xi, THR2, order)
        d2 = [float(G.gate(T, 3, 9, Rm[k], tm[k], kap[k], ta[k], *G.blocks_of(Sigma, 3, 9))[1]) for k in range(2)]
        assert max(d2) <= THR2, "both pass the gate on their own"
        assert r["accept"].sum() == 1
        a, b = int(r["accepted"][0]), int(np.flatnonzero(~r["accept"])[0])
        # the 12 x 12 closed form [[P + R, P], [P, P + R]] with P = Sigma_rel
        x_c = xi[b] - Sr @ np.linalg.solve(Sr + R1, xi[a])
        S_c = Sr + R1 - Sr @ np.linalg.solve(Sr + R1, Sr)
        assert np.abs(np.asarray(r["xi_cond"][b], dtype=F) - x_c).max() <= 1e-12 * np.abs(xi).max()
        st = r["steps"][-1]
        assert st["k"] == b and np.abs(st["rows"][b]["S"] - S_c).max() <= 1e-12 * np.abs(Sr + R1).max()
        assert float(r["d2_cond"][b]) > THR2 and abs(float(r["d2_cond"][b]) - x_c @ np.linalg.solve(S_c, x_c)) <= 1e-9 * float(r["d2_cond"][b])


def test_the_bounds_reject_the_mistakes_the_conventions_invite():
    """each of them moves a figure by more than 1000 x the bound the GPU test holds that figure to"""
    P = problem(4, K=24)
    T, ends, blk, K = P["T"], P["ends"], P["blk"], len(P["ends"])
    Mref = np.asarray(P["M"], dtype=F)
    bound = np.zeros_like(Mref)
    for k, (ik, jk) in enumerate(ends):
        for l, (il, jl) in enumerate(ends):
            bound[6 * k:6 * k + 6, 6 * l:6 * l + 6] = J.m_block_bound(T, ik, jk, il, jl, blk)

    def worst(Mw):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.abs(np.asarray(Mw, dtype=F) - Mref) / bound
        return np.nanmax(r)

    assert worst(J.joint_M(T, ends, P["kappa"], P["tau"], blk, dtype=F)) <= 1.0  # (float64 itself stays inside)
    Md, bd = J.joint_M_dense(T, ends, P["kappa"], P["tau"], blk, P["n"])  # the one-product form: the same M, the same bound
    assert np.abs(np.asarray(Md - P["M"], dtype=F)).max() <= 1e-17 * np.abs(Mref).max() and np.abs(bd - bound).max() <= 1e-12 * bound.max()
    # a missing transposition for a block with b < a
    no_t = lambda a, b: blk(min(a, b), max(a, b))
    # Sigma_meas added to off-diagonal blocks
    Moff = np.array(P["M"])
    for k in range(K):
        for l in range(K):
            if k != l:
                Moff[6 * k:6 * k + 6, 6 * l:6 * l + 6] += G.sigma_meas(P["kappa"][k], P["tau"][k])
    # a pose-0 block that is not zero
    not_zero = lambda a, b: blk(max(a, 1), max(b, 1))
    ratios = dict(transposition=worst(J.joint_M(T, ends, P["kappa"], P["tau"], no_t)), sigma_meas_off_diagonal=worst(Moff),
                  pose0=worst(J.joint_M(T, ends, P["kappa"], P["tau"], not_zero)))
    # xi not updated after a pivot; a tie broken towards the higher index (an exact duplicate of candidate 2 behind it)
    dup = np.r_[np.arange(K), 2]
    Md = J.joint_M(T, ends[dup], P["kappa"][dup], P["tau"][dup], blk)
    xd = P["xi"][dup]
    ref = J.run(Md, xd, THR2, "greedy")
    assert ref["accept"][2] and ref["rank"][2] < ref["rank"][K] and ref["accept"][K]
    conds = J.prefix_conditions(Md, ref["accepted"])
    by_k = {s["k"]: s for s in ref["steps"]}
    # (the step that decides k holds its magnitudes; greedy's rejected are decided by the last step recorded)

    def ratio_against(other, ks):
        out = 0.0
        for k in ks:
            s = by_k[k]
            b_x, b_d = J.conditional_bounds(s, conds[s["n_acc"]])
            out = max(out, (np.abs(np.asarray(other["xi_cond"][k] - ref["xi_cond"][k], dtype=F)) / b_x).max(),
                      abs(float(other["d2_cond"][k] - ref["d2_cond"][k])) / b_d)
        return out

    class Frozen(J.Elimination):  # xi_k|A left at xi_k
        def pivot(self, p):
            x = self.x.copy()
            super().pivot(p)
            self.x = x

    E = Frozen(Md, xd)
    frozen = dict(xi_cond=np.zeros((K + 1, 6), dtype=J.LD), d2_cond=np.zeros(K + 1, dtype=J.LD))
    for k in ref["accepted"]:
        frozen["xi_cond"][k], frozen["d2_cond"][k] = E.x[k], E.d2()[k]
        E.pivot(k)
    ratios["xi_not_updated"] = ratio_against(frozen, ref["accepted"][1:])
    acc = list(ref["accepted"])
    a, b = acc.index(2), acc.index(K)
    acc[a], acc[b] = K, 2
    swapped = J.run(Md, xd, THR2, "greedy", pivots=acc)
    ratios["tie_towards_the_higher_index"] = ratio_against(swapped, [2, K])
    print("mistake -> error / bound: " + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    assert all(v > 1000.0 for v in ratios.values()), ratios


def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+dpgo_team_gate_candidates_jointly\s*\(", header)
    assert "dpgo_team_gate_candidates_jointly" in capi.EXPORTS
    assert callable(getattr(capi.Team, "gate_jointly", None))
    assert (capi.JOINT_GREEDY, capi.JOINT_GIVEN) == (0, 1) and "DPGO_JOINT_GREEDY = 0, DPGO_JOINT_GIVEN = 1" in header

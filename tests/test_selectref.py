"""CPU checks of tests/selectref.py, the numpy statement of the selection of candidate closures under a budget:
gain_total against the log-determinants of the Hessians with and without the selected closures, the (1 - 1 / e) guarantee
against brute force, order="given" on greedy's own sequence, and the bounds of the GPU tests (tests/test_gpu_select.py) against
the mistakes the conventions invite.  The last test is the one that fails where the call does not exist."""
import itertools
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import selectref as S
from tests.util import ROOT

F = np.float64
U = S.U
FIXED = ((0, 5), (5, 0), (3, 9), (9, 3), (3, 7), (2, 3))


def problem(seed, P=12, n=12):
    m, T = NR.banded_chain(n, seed, window=8)
    Hr, Sigma, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    Sigma = 0.5 * (Sigma + Sigma.T)  # (the inverse LAPACK returns is symmetric to rounding only)
    ends, kap, ta = S.seeded_pool(T, n, P, seed + 100, fixed=FIXED)
    blk = J.blocks_from_sigma(Sigma)
    return dict(n=n, m=m, T=T, Hr=Hr, w=w, Sigma=Sigma, ends=ends, kappa=kap, tau=ta, blk=blk, M=J.joint_M(T, ends, kap, ta, blk),
                ldR=S.logdet_meas(kap, ta))


def exact_closures(m, T, ends, kap, ta):
    """the measurements of the graph with the candidates added as the relative poses of T itself, at weight 1"""
    c = np.zeros(len(ends), dtype=capi.MEAS_DTYPE)
    for k, (i, j) in enumerate(ends):
        Rij, tij = G.relative_pose(T, int(i), int(j), F)
        c[k]["p1"], c[k]["p2"], c[k]["R"], c[k]["t"] = i, j, np.asarray(Rij).reshape(-1), tij
    c["kappa"], c["tau"], c["weight"] = kap, ta, 1.0
    return np.concatenate([m, c])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gain_total_is_half_the_growth_of_log_det_H(seed):
    """Bound, in the idiom of the project's end-to-end bounds (6 (n - 1) u cond_2(H_red)): slogdet of H in float64 is the log det
    of a matrix within that relative distance of H, and d log det H = tr(H^-1 dH) is of that size; the same for H'.  Sigma =
    inv(H) carries the same relative error into M_AA, and through tr(M_AA^-1 dM_AA) over its 6 |A| rows into log det M_AA:
    6 (n - 1) u (cond_2(H) (1 + 6 |A|) + cond_2(H')), halved as the gain halves the log-determinants."""
    P = problem(seed)
    n, b = P["n"], 5
    r = S.run(P["M"], P["ldR"], b)
    sel = r["selected"]
    assert r["num_selected"] == b == len(set(sel.tolist()))
    mx = exact_closures(P["m"], P["T"], P["ends"][sel], P["kappa"][sel], P["tau"][sel])
    Hx, _, wx = covref.dense_reference(covref.q_full(mx, n), P["T"], n)
    want = 0.5 * (np.linalg.slogdet(Hx)[1] - np.linalg.slogdet(P["Hr"])[1])
    bound = 0.5 * 6 * (n - 1) * U * (P["w"][-1] / P["w"][0] * (1 + 6 * b) + wx[-1] / wx[0])
    err = abs(float(r["gain_total"]) - want)
    print("seed %d: gain_total %.12g, (log det H' - log det H) / 2 = %.12g, error / bound %.3g" % (seed, float(r["gain_total"]), want, err / bound))
    assert want > 0 and err <= bound
    # the same figure straight from the definition, and the joint log-determinant
    assert abs(float(r["gain_total"] - S.set_value(P["M"], P["ldR"], sel))) <= 1e-15 * want
    rows = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in sel])
    ld = np.linalg.slogdet(np.asarray(P["M"], dtype=F)[np.ix_(rows, rows)])[1]
    assert abs(float(r["logdet_joint"]) - ld) <= 1e-10 * abs(ld)
    assert (np.sort(r["rank"][sel]) == np.arange(b)).all() and (np.delete(r["rank"], sel) == -1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_greedy_against_brute_force_and_its_gains_do_not_increase(seed):
    P = problem(seed)
    M10, ld10 = P["M"][:60, :60], P["ldR"][:10]
    g = S.run(M10, ld10, 3)
    best, arg = max((float(S.set_value(M10, ld10, c)), c) for c in itertools.combinations(range(10), 3))
    val = float(g["gain_total"])
    print("seed %d: greedy %s %.9g, the best of 120 subsets %s %.9g (ratio %.4f)" % (seed, list(g["selected"]), val, list(arg), best, val / best))
    assert val >= (1 - 1 / np.e) * best and val <= best * (1 + 1e-15)
    # submodularity along greedy's own path, all twelve steps; the marginal gain is the largest a candidate ever has
    full = S.run(P["M"], P["ldR"], 12)
    at = full["gain_cond"][full["selected"]]
    assert full["num_selected"] == 12 and (np.diff(at) <= 1e-15 * at[:-1]).all() and (at > 0).all()
    assert (full["gain_cond"] <= full["gain"] * (1 + 1e-15)).all()
    # a threshold between two consecutive gains stops the call there
    cut = S.run(P["M"], P["ldR"], 12, min_gain=0.5 * float(at[4] + at[5]))
    assert at[4] > at[5] and cut["num_selected"] == 5 and list(cut["selected"]) == list(full["selected"][:5])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_given_on_the_sequence_of_greedy_reproduces_its_gains(seed):
    P = problem(seed)
    b = 6
    g = S.run(P["M"], P["ldR"], b)
    perm = np.r_[g["selected"], np.setdiff1d(np.arange(12), g["selected"])]
    rows = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in perm])
    v = S.run(P["M"][np.ix_(rows, rows)], P["ldR"][perm], b, order="given")
    assert list(v["selected"]) == list(range(b))
    tol = 1e-17 * np.abs(np.asarray(g["gain_cond"][perm], dtype=F)) + 1e-18
    assert (np.abs(v["gain_cond"] - g["gain_cond"][perm]) <= tol).all() and (np.abs(v["gain"] - g["gain"][perm]) <= tol).all()
    assert abs(v["gain_total"] - g["gain_total"]) <= 1e-17 * abs(g["gain_total"])
    # any other order of the same set: the same total
    w = S.run(P["M"], P["ldR"], b, pivots=g["selected"][::-1])
    assert abs(float(w["gain_total"] - g["gain_total"])) <= 1e-15 * float(g["gain_total"])


def test_the_bounds_reject_the_mistakes_the_conventions_invite():
    """each of them moves a figure by more than 1000 x the bound the GPU test holds that figure to"""
    P = problem(4)
    T, ends, blk, M, ldR, b = P["T"], P["ends"], P["blk"], P["M"], P["ldR"], 6
    bD = [S.d_bound(T, int(i), int(j), blk) for i, j in ends]
    ref = S.run(M, ldR, b)
    conds = J.prefix_conditions(M, ref["selected"])
    bound_at = {s["k"]: S.step_bound(s, s["k"], conds[s["n_acc"]], bD[s["k"]], ldR[s["k"]]) for s in ref["steps"] if not s["stop"]}
    sel = ref["selected"]
    at = np.asarray(ref["gain_cond"][sel], dtype=F)
    bnd = np.array([bound_at[k] for k in sel])
    # float64 itself stays inside
    f64 = S.run(np.asarray(M, dtype=F), np.asarray(ldR, dtype=F), b, pivots=sel, dtype=F)
    assert (np.abs(np.asarray(f64["gain_cond"][sel], dtype=F) - at) <= bnd).all()
    ratios = {}
    # log det R left out; the factor 1/2 left out
    ratios["logdet_R_left_out"] = (np.abs(0.5 * np.asarray(ldR[sel], dtype=F)) / bnd).min()
    ratios["half_left_out"] = (np.abs(at) / bnd).min()
    # Sigma_meas left out of D: on the diagonal blocks, against d_bound
    ratios["sigma_meas_left_out"] = min((np.diag(np.asarray(G.sigma_meas(P["kappa"][k], P["tau"][k]), dtype=F)) / np.diag(bD[k])).min()
                                        for k in range(len(ends)))

    def rule_ratio(pivots):
        """a recorded order that is not the rule's: by how many bounds the pick's gain falls short of the rule's own choice"""
        rep = S.run(M, ldR, b, pivots=pivots)
        cA = J.prefix_conditions(M, rep["selected"])
        out = 0.0
        for s in rep["steps"]:
            if s["stop"] or s["k"] == s["choice"]:
                continue
            k, c = s["k"], s["choice"]
            two = S.step_bound(s, k, cA[s["n_acc"]], bD[k], ldR[k]) + S.step_bound(s, c, cA[s["n_acc"]], bD[c], ldR[c])
            out = max(out, float(s["gain"][c] - s["gain"][k]) / two)
        return out

    assert rule_ratio(sel) == 0.0
    # the pivot chosen by marginal gain in the place of conditional gain
    by_marginal = np.argsort(-np.asarray(ref["gain"], dtype=F), kind="stable")[:b]
    assert list(by_marginal) != list(sel)
    ratios["pivot_by_marginal_gain"] = rule_ratio(by_marginal)
    # the smallest gain taken in the place of the largest
    E = J.Elimination(M, np.zeros(len(M)))
    smallest = []
    for _ in range(b):
        g = S.gains(E, ldR)
        k = int(np.flatnonzero(E.open)[np.argmin(g[E.open])])
        smallest.append(k)
        E.pivot(k)
    ratios["smallest_gain_taken"] = rule_ratio(smallest)
    print("mistake -> error / bound: " + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    assert all(v > 1000.0 for v in ratios.values()), ratios


def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+dpgo_team_select_candidates\s*\(", header)
    assert "dpgo_team_select_candidates" in capi.EXPORTS
    assert hasattr(capi.lib(), "dpgo_team_select_candidates")
    assert callable(getattr(capi.Team, "select_closures", None)) and callable(getattr(capi.Team, "candidates_from_pairs", None))

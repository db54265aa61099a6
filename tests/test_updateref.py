"""CPU checks of tests/updateref.py, the numpy statement of the first-order update of a trajectory and its covariances for new
closures: the covariance form against the information form, exact closures against the dense reference of the
extended graph, the second-order behaviour of the updated innovations, and the bounds of the GPU tests
(tests/test_gpu_linear_update.py) against the mistakes the conventions invite.  The last test is the one that fails where the
call does not exist."""
import os
import re

import numpy as np

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import updateref as R
from tests.util import ROOT

F = np.float64
U = R.U
N_POSES, K_CLOSURES = 12, 10
FIXED = ((0, 5), (5, 0), (3, 9), (9, 3))


def problem(seed):
    n = N_POSES
    m, T = NR.banded_chain(n, seed, window=8)
    Hr, Sigma, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    Sigma = 0.5 * (Sigma + Sigma.T)
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, K_CLOSURES, seed + 100, outliers=0.0, fixed=FIXED)
    return dict(n=n, m=m, T=T, Hr=Hr, Sigma=Sigma, cond=w[-1] / w[0], ends=ends, Rm=Rm, tm=tm, kappa=kap, tau=ta)


def exact(P):
    """the closures set exactly to T's relative poses"""
    rel = [G.relative_pose(P["T"], int(i), int(j), F) for i, j in P["ends"]]
    return np.array([r[0] for r in rel]), np.array([r[1] for r in rel])


def off_by(P, s, seed=7):
    """the closures off by 0.05 s N(0, I) in rotation vector and translation"""
    rng = np.random.default_rng(seed)
    Rm, tm = exact(P)
    w, d = 0.05 * s * rng.standard_normal((len(Rm), 3)), 0.05 * s * rng.standard_normal((len(Rm), 3))
    return np.array([Rm[k] @ covref.exp_so3(w[k]) for k in range(len(Rm))]), tm + d


def extended(P, Rm, tm):
    """the measurements of the graph with the closures added, single-robot numbering"""
    c = np.zeros(len(P["ends"]), dtype=capi.MEAS_DTYPE)
    c["p1"], c["p2"] = P["ends"][:, 0], P["ends"][:, 1]
    c["R"], c["t"], c["kappa"], c["tau"], c["weight"] = Rm.reshape(-1, 9), tm, P["kappa"], P["tau"], 1.0
    return np.concatenate([P["m"], c])


def run(P, Rm, tm, **kw):
    return R.update(P["T"], P["ends"], Rm, tm, P["kappa"], P["tau"], R.blocks_from_sigma(P["Sigma"], kw.get("pairs", ())), P["n"], **kw)


def full_sigma(ref, P):
    """Sigma' of the free poses, 6 (n - 1) square, from B and U"""
    Sp = np.asarray(ref["U"] @ ref["B"].T, dtype=F)
    return P["Sigma"] - 0.5 * (Sp + Sp.T)[6:, 6:]


def test_covariance_form_against_information_form():
    for seed in (1, 2, 3):
        P = problem(seed)
        ref = run(P, P["Rm"], P["tm"])
        Sp, dx = R.information_form(P["Hr"], P["T"], P["ends"], P["kappa"], P["tau"], ref["xi"], P["n"])
        tol = 100 * U * P["cond"]
        eS = np.abs(full_sigma(ref, P) - Sp).max() / np.abs(Sp).max()
        ed = np.abs(np.asarray(ref["delta"], dtype=F).reshape(-1)[6:] - dx).max() / np.abs(dx).max()
        # the stored blocks are those of the full matrix
        for p in range(P["n"]):
            want = Sp[6 * p - 6:6 * p, 6 * p - 6:6 * p] if p else np.zeros((6, 6))
            assert np.abs(np.asarray(ref["cov_diag"][p], dtype=F) - want).max() <= tol * np.abs(Sp).max()
        print("seed %d, cond_2(H_red) = %.3g: Sigma' %.3g, dx %.3g relative (tolerance %.3g)" % (seed, P["cond"], eS, ed, tol))
        assert eS <= tol and ed <= tol
        assert (np.asarray(ref["delta"][0], dtype=F) == 0).all()
        # xi_post = R z is xi + A dx
        lhs = np.asarray(ref["xi"].reshape(-1) + ref["A"] @ ref["delta"].reshape(-1), dtype=F)
        assert np.abs(lhs - np.asarray(ref["xi_post"], dtype=F).reshape(-1)).max() <= 1e-12 * np.abs(lhs).max()


def test_exact_closures_leave_T_and_give_the_covariance_of_the_extended_graph():
    for seed in (1, 2, 3):
        P = problem(seed)
        Rm, tm = exact(P)
        pairs = [(3, 9), (0, 4), (7, 7)]
        ref = run(P, Rm, tm, pairs=pairs)
        b = R.bounds(ref, P["T"], P["ends"], tm, P["n"], pairs)
        assert (np.abs(np.asarray(ref["delta"], dtype=F)) <= b["delta"]).all()
        assert (np.abs(np.asarray(ref["T"], dtype=F) - P["T"]) <= b["T"]).all()
        Hx, Sx, wx = covref.dense_reference(covref.q_full(extended(P, Rm, tm), P["n"]), P["T"], P["n"])
        tol = 100 * U * P["cond"]
        eS = np.abs(full_sigma(ref, P) - Sx).max() / np.abs(Sx).max()
        print("seed %d: exact closures, Sigma' against the dense reference of the extended graph %.3g relative (tolerance %.3g)"
              % (seed, eS, tol))
        assert eS <= tol
        for q, (a, c) in enumerate(pairs):
            want = Sx[6 * a - 6:6 * a, 6 * c - 6:6 * c] if a and c else np.zeros((6, 6))
            assert np.abs(np.asarray(ref["cov_pairs"][q], dtype=F) - want).max() <= tol * np.abs(Sx).max()
        # the information the batch brings: log det of the Hessians
        gain = 0.5 * (np.linalg.slogdet(Hx)[1] - np.linalg.slogdet(P["Hr"])[1])
        assert abs(float(ref["information_gain"]) - gain) <= 1e-9 * abs(gain)


def second_order(P, update_of):
    """(max |xi(T') - xi_post| at s = 1, 1/4, 1/16; the update at s = 1 with its closures)"""
    errs, first = [], None
    for s in (1.0, 0.25, 0.0625):
        Rm, tm = off_by(P, s)
        out = update_of(Rm, tm)
        xi_new = np.asarray(J.innovations(out["T"], P["ends"], Rm, tm), dtype=F)
        errs.append(np.abs(xi_new - np.asarray(out["xi_post"], dtype=F)).max())
        first = first or (out, Rm, tm)
    return errs, first


def check_second_order(P, errs, first):
    out, Rm, tm = first
    assert errs[0] / errs[1] >= 8 and errs[1] / errs[2] >= 8, errs  # theory 16; a sign or frame mistake 4
    Qx = covref.q_full(extended(P, Rm, tm), P["n"])
    f_T = covref.cost(covref.q_full(P["m"], P["n"]), P["T"], P["n"])
    at_new, at_T = covref.cost(Qx, np.asarray(out["T"], dtype=F), P["n"]), covref.cost(Qx, P["T"], P["n"])
    half = 0.5 * float(out["d2_joint"])
    assert abs(at_new - f_T - half) <= 0.01 * half, (at_new, f_T, half)
    assert at_new < at_T
    return at_new, at_T, half


def test_the_updated_innovations_are_right_to_second_order():
    for seed in (1, 2, 3):
        P = problem(seed)
        errs, first = second_order(P, lambda Rm, tm: run(P, Rm, tm))
        at_new, at_T, half = check_second_order(P, errs, first)
        print("seed %d: max |xi(T') - xi_post| %.3g, %.3g, %.3g (ratios %.3g, %.3g); cost of the new graph at T' %.6g = f(T) + %.6g "
              "to %.3g relative, at T %.6g" % (seed, errs[0], errs[1], errs[2], errs[0] / errs[1], errs[1] / errs[2], at_new, half,
                                               abs(at_new - half) / half, at_T))
    # a retraction with the wrong sign is first order only
    P = problem(1)

    def wrong(Rm, tm):
        out = run(P, Rm, tm)
        out["T"] = R.retract(P["T"], -out["delta"])
        return out

    errs, _ = second_order(P, wrong)
    assert errs[0] / errs[1] < 8


def test_the_bounds_reject_the_mistakes_the_conventions_invite():
    """each of them moves a figure by more than 1000 x the bound the GPU test holds that figure to"""
    P = problem(2)
    Rm, tm = off_by(P, 1.0)
    pairs = [(3, 9)]
    ref = run(P, Rm, tm, pairs=pairs)
    b = R.bounds(ref, P["T"], P["ends"], tm, P["n"], pairs)
    # (float64 itself stays inside)
    f64 = R.update(P["T"], P["ends"], Rm, tm, P["kappa"], P["tau"], R.blocks_from_sigma(P["Sigma"], pairs), P["n"], pairs=pairs, dtype=F)
    for key in ("B", "M", "delta", "cov_diag", "cov_pairs", "xi_post", "T"):
        assert R.ratio(np.asarray(f64[key], dtype=F) - np.asarray(ref[key], dtype=F), b[key]) <= 1.0, key
    for key in ("d2_joint", "logdet_M", "logdet_R"):
        assert abs(float(f64[key] - ref[key])) <= b[key], key

    def worst(key, other):
        err, bound = np.abs(np.asarray(other[key], dtype=F) - np.asarray(ref[key], dtype=F)), np.broadcast_to(b[key], np.shape(ref[key]))
        return float((err[bound > 0] / bound[bound > 0]).max())

    blk = J.blocks_from_sigma(P["Sigma"])
    not_zero = lambda a, c: blk(max(a, 1), max(c, 1))
    pose0 = R.update(P["T"], P["ends"], Rm, tm, P["kappa"], P["tau"], R.Blocks(not_zero, lambda p: not_zero(p, p), lambda q: blk(3, 9)),
                     P["n"], pairs=pairs)
    ratios = dict(jacobians_swapped=worst("B", run(P, Rm, tm, pairs=pairs, mistake="jacobians_swapped")),
                  pose0_block_not_zero=worst("B", pose0),
                  sigma_meas_left_out=worst("M", run(P, Rm, tm, pairs=pairs, mistake="sigma_meas_left_out")),
                  translation_in_body_frame=worst("T", run(P, Rm, tm, pairs=pairs, mistake="translation_in_body_frame")),
                  no_mirror=worst("cov_diag", run(P, Rm, tm, pairs=pairs, mistake="no_mirror")))
    print("mistake -> error / bound: " + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    assert all(v > 1000.0 for v in ratios.values()), ratios


def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+dpgo_team_linear_update\s*\(", header)
    assert "dpgo_team_linear_update" in capi.EXPORTS
    assert hasattr(capi.lib(), "dpgo_team_linear_update")
    assert callable(getattr(capi.Team, "linear_update", None))

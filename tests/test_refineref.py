"""CPU checks of tests/refineref.py, the reference of the Newton refinement on SE(3), and of the call's presence:
  1. the longdouble gradient against central differences of covref.cost
  2. the reference iteration on the inputs of tests/test_gpu_refine.py -- banded_chain(12, 1, window=8) with noise (0.02, 0.05)
     from T* perturbed by s = 1e-4, 1e-3, 1e-2 and banded_chain(40, 3, window=8) with noise (0.05, 0.1) from s = 1e-4, noise at
     seed 7, starts at seed 11 -- reaches |g|_inf <= 1e-9 within 6 steps with a positive smallest eigenvalue of H_red at every
     iterate; s = 3e-2 on the 12 poses is indefinite at the start
  3. the bounds used on the GPU reject the wrong sign of the step, pose 0's rows read, a body-frame translation update and the
     factor 1/2 of the antisymmetric part kept in the rotation rows
  4. dpgo_team_refine is declared in include/dpgo_hip.h, exported by the library and bound in capi"""
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covref
from tests import refineref as RR
from tests.util import ROOT

F = np.float64
CASES = (("chain12", 1e-4), ("chain12", 1e-3), ("chain12", 1e-2), ("chain40", 1e-4))
GRAD_TOL = 1e-9
_runs = {}


def run(name, s):
    """the reference iteration from the start (name, s), computed once"""
    if (name, s) not in _runs:
        c = RR.case(name)
        _runs[(name, s)] = RR.newton(c["m"], c["n"], RR.start(c["Tstar"], c["n"], s, 11), grad_tol=GRAD_TOL)
    return _runs[(name, s)]


def test_gradient_against_central_differences():
    c = RR.case("chain12")
    n, Q = c["n"], c["Q"]
    T = RR.start(c["Tstar"], n, 1e-2, 11)
    g = np.asarray(RR.gradient(Q, T, n), dtype=F)
    assert (g[:6] == 0).all()
    h, worst = 1e-5, 0.0
    for k in range(6, 6 * n):
        e = np.zeros(6 * n)
        e[k] = h
        fd = (covref.cost(Q, covref.perturb(T, e, n), n) - covref.cost(Q, covref.perturb(T, -e, n), n)) / (2 * h)
        # the truncation of the central difference (third derivative of the order of the largest curvature) and its rounding
        tol = 1e4 * h * h + 1e-15 * abs(covref.cost(Q, T, n)) * 1e4 / h + 1e-7 * abs(g[k])
        worst = max(worst, abs(fd - g[k]) / tol)
    print("longdouble gradient against central differences: largest error / tolerance %.3g" % worst)
    assert worst <= 1.0
    # and the cost by edges is the cost by Q
    assert abs(float(RR.edge_cost(c["m"], T, n)) - covref.cost(Q, T, n)) <= 1e-9 * covref.cost(Q, T, n)


@pytest.mark.parametrize("name,s", CASES)
def test_reference_iteration_converges_inside_the_basin(name, s):
    c = RR.case(name)
    gs = float(np.abs(np.asarray(RR.gradient(c["Q"], c["Tstar"], c["n"]), dtype=F)).max())
    assert gs <= 1e-11, gs
    r = run(name, s)
    print("%s, s = %g: %s in %d steps, alpha %s, |g|_inf %s, smallest eigenvalues %s" %
          (name, s, r["status"], r["iterations"], r["history"]["alpha"], ["%.3g" % v for v in r["history"]["grad_inf"]],
           ["%.3g" % v for v in r["history"]["eig_min"]]))
    assert r["status"] == "converged" and r["iterations"] <= 6 and r["grad_inf"] <= GRAD_TOL
    assert all(w > 0 for w in r["history"]["eig_min"]) and len(r["history"]["eig_min"]) == r["iterations"]
    assert np.abs(r["T"] - c["Tstar"]).max() <= RR.final_bound(c["Q"], c["Tstar"], c["n"], GRAD_TOL)


def test_the_start_outside_the_basin_is_indefinite():
    c = RR.case("chain12")
    r = RR.newton(c["m"], c["n"], RR.start(c["Tstar"], c["n"], 3e-2, 11), grad_tol=GRAD_TOL)
    assert r["status"] == "indefinite" and r["iterations"] == 0 and r["history"]["eig_min"][0] < -0.1
    # the noise-free graph at its ground truth has a zero gradient and a zero cost
    assert float(RR.edge_cost(c["clean"], c["truth"], c["n"])) <= 1e-25


def test_the_bounds_reject_planted_mistakes():
    c = RR.case("chain12")
    n, Q, m = c["n"], c["Q"], c["m"]
    T0 = RR.start(c["Tstar"], n, 1e-2, 11)
    g, gb = RR.gradient(Q, T0, n), RR.gradient_bound(Q, T0, n)
    for mistake in ("half", "pose0"):
        err = np.abs(np.asarray(RR.gradient(Q, T0, n, mistake=mistake) - g, dtype=F))
        print("%s: the gradient leaves its bound at %d entries" % (mistake, int((err > gb).sum())))
        assert (err > gb).any()
    good = run("chain12", 1e-2)
    fb = RR.final_bound(Q, c["Tstar"], n, GRAD_TOL)
    assert np.abs(good["T"] - c["Tstar"]).max() <= fb
    for mistake in ("sign", "body"):
        r = RR.newton(m, n, T0, max_iters=good["iterations"] + 1, grad_tol=GRAD_TOL, mistake=mistake)
        err = np.abs(r["T"] - c["Tstar"]).max()
        print("%s: status %s after %d steps, alpha %s, |T - T*|_inf %.3g of the bound" %
              (mistake, r["status"], r["iterations"], r["history"]["alpha"], err / fb))
        assert r["status"] != "converged" or err > fb
    # the first accepted step length is what the GPU test compares: with the wrong sign no entry of the ladder passes
    assert RR.newton(m, n, T0, max_iters=1, grad_tol=GRAD_TOL, mistake="sign")["status"] == "no_descent"


def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+dpgo_team_refine\s*\(", header)
    assert "dpgo_team_refine" in capi.EXPORTS
    assert hasattr(capi.lib(), "dpgo_team_refine")
    assert callable(getattr(capi.Team, "refine", None))
    assert capi.REFINE_STATUS == RR.STATUS

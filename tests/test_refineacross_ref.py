"""CPU checks of tests/refineacross_ref.py, the float64 statement of the refinement over a split team (DESIGN.md 5n "Across
teams"), against the measuring sticks of tests/refineref.py on the whole problem; and that the call is declared, exported and
bound with the signatures the documents give.
  1. the inputs are what the GPU tests take them for (public / interior poses and owned measurements per robot), the across
     iteration takes the iterations listed below from every start and ends within refineref.final_bound of T*; the starts
     outside the basin are indefinite at once; armijo = 0.7 takes alpha = 1/2 four times
  2. the robots' sums equal refineref.edge_cost within refineref.cost_bound, at the start and at a trial point
  3. each planted mistake of refineacross_ref.MISTAKES is rejected by those bounds
  4. dpgo_team_refine_across is declared, exported and bound; Team.refine, distributed.refine and
     distributed.certify_and_round have the documented signatures"""
import inspect
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyacross_ref as XR
from tests import refineacross_ref as XF
from tests import refineref as RR
from tests.util import ROOT

F = np.float64
LD = np.longdouble
GRAD_TOL = 1e-9
# (case, robots, (public, interior) per robot with pose 0 among robot 0's interior, measurements owned per robot or None)
SETS = [("chain12", 3, [(1, 3), (4, 0), (2, 2)], None),
        ("chain40", 3, [(2, 11), (5, 8), (4, 10)], None),
        ("chain40", 8, XR.GRAPHS[2][3], None),
        ("chain40", 1, [(0, 40)], None),
        ("band40", 2, None, [320, 184]),
        ("band40", 1, [(0, 40)], [504])]
# (case, start, iterations of the reference)
RUNS = [("chain12", 1e-4, 2), ("chain12", 1e-3, 3), ("chain12", 1e-2, 5), ("chain40", 1e-4, 3), ("chain40", 1e-3, 3),
        ("band40", 1e-3, 3), ("band40", 1e-2, 4)]
LADDER = [("chain12", 1e-3), ("chain40", 1e-3), ("band40", 1e-2)]
INDEFINITE = [("chain12", 3e-2), ("chain40", 1e-2)]
ROBOTS = dict(chain12=(3,), chain40=(3, 8, 1), band40=(2, 1))


@pytest.mark.parametrize("name,N,sets,owned", SETS)
def test_the_inputs_are_what_the_gpu_tests_take_them_for(name, N, sets, owned):
    c, sp = XF.case(name), XF.split(name, N)
    if (name, N) == ("chain40", 8):
        assert (5, 0) in XR.counts(sp["robot_of"], sp["public"])  # a robot with no interior pose
    if sets is not None:
        assert XR.counts(sp["robot_of"], sp["public"]) == [tuple(s) for s in sets]
    if owned is not None:
        assert list(sp["owned"]) == owned
    assert int(sp["owned"].sum()) == len(c["m"]) and (len(c["m"]) == 504 if name == "band40" else True)
    if name == "band40":
        w = np.linalg.eigvalsh(RR.hessian_red(c["Q"], c["Tstar"], c["n"]))
        gs = float(np.abs(np.asarray(RR.gradient(c["Q"], c["Tstar"], c["n"]), dtype=F)).max())
        print("band40: eigenvalues of H_red at T* from %.4g to %.4g, |g(T*)|_inf %.3g" % (w[0], w[-1], gs))
        assert 14.0 < w[0] < 15.0 and 5e4 < w[-1] < 6e4 and gs < 1e-10


@pytest.mark.parametrize("name,s,its", RUNS)
def test_the_across_reference_converges_as_listed(name, s, its):
    c = XF.case(name)
    n, Q = c["n"], c["Q"]
    T0 = RR.start(c["Tstar"], n, s, 11)
    fb = RR.final_bound(Q, c["Tstar"], n, GRAD_TOL)
    for N in ROBOTS[name]:
        out = XF.newton(name, N, T0, grad_tol=GRAD_TOL)
        err = float(np.abs(out["T"] - c["Tstar"]).max())
        print("%s as %d robots, s = %g: %s in %d iterations, alpha %s, |g|_inf %s, smallest eigenvalues %s, |T - T*|_inf %.3g of the "
              "bound" % (name, N, s, out["status"], out["iterations"], out["history"]["alpha"],
                         ["%.3g" % v for v in out["history"]["grad_inf"]], ["%.3g" % v for v in out["history"]["eig_min"]], err / fb))
        assert out["status"] == "converged" and out["iterations"] == its
        assert out["history"]["alpha"] == [1.0] * its and min(out["history"]["eig_min"]) > 0
        assert err <= fb
        assert out["iterations"] == RR.newton(c["m"], n, T0, grad_tol=GRAD_TOL)["iterations"]


@pytest.mark.parametrize("name,s", LADDER)
def test_a_strict_armijo_halves_the_step_four_times(name, s):
    c = XF.case(name)
    T0 = RR.start(c["Tstar"], c["n"], s, 11)
    for N in ROBOTS[name]:
        out = XF.newton(name, N, T0, max_iters=4, grad_tol=GRAD_TOL, armijo=0.7)
        g = out["history"]["grad_inf"]
        print("%s as %d robots, s = %g, armijo 0.7: alpha %s, |g|_inf %s" % (name, N, s, out["history"]["alpha"], ["%.3g" % v for v in g]))
        assert out["status"] == "max_iters" and out["history"]["alpha"] == [0.5] * 4
        assert all(0.4 < g[k + 1] / g[k] < 0.6 for k in range(4))


@pytest.mark.parametrize("name,s", INDEFINITE)
def test_the_refusal_cases_are_indefinite_at_the_start(name, s):
    c = XF.case(name)
    out = XF.newton(name, ROBOTS[name][0], RR.start(c["Tstar"], c["n"], s, 11), grad_tol=GRAD_TOL)
    assert out["status"] == "indefinite" and out["iterations"] == 0 and out["history"]["eig_min"][0] < 0


def _first_step(name, N, s):
    c, sp = XF.case(name), XF.split(name, N)
    m, n, Q = c["m"], c["n"], c["Q"]
    T0 = RR.start(c["Tstar"], n, s, 11)
    g = XF.gradient(Q, T0, sp, n)
    X = XR.eliminate(RR.hessian_red(Q, T0, n), sp["robot_of"], sp["public"], g.reshape(-1, 1))[:, 0]
    return c, sp, m, n, Q, T0, g, X


@pytest.mark.parametrize("name,N", [("chain12", 3), ("chain40", 3), ("chain40", 8), ("band40", 2)])
def test_robot_sums_equal_the_edge_cost_and_mistakes_are_rejected(name, N):
    c, sp, m, n, Q, T0, g, X = _first_step(name, N, 1e-3)
    alpha = 0.5  # (entry l = 1 of the ladder)
    Tl = RR.trial(T0, X, alpha, n)
    f0, fl = RR.edge_cost(m, T0, n, LD), RR.edge_cost(m, Tl, n, LD)
    b0, bl = RR.cost_bound(m, T0, n), RR.cost_bound(m, Tl, n)
    gb = RR.gradient_bound(Q, T0, n)
    gref = np.asarray(RR.gradient(Q, T0, n), dtype=F)

    def figures(mistake):
        e0 = abs(float(LD(XF.total(XF.robot_costs(m, sp, [T0] * N, n, mistake))) - f0)) / b0
        el = abs(float(LD(XF.total(XF.robot_costs(m, sp, XF.trial_views(sp, T0, X, alpha, n, mistake), n, mistake))) - fl)) / bl
        eg = float((np.abs(XF.gradient(Q, T0, sp, n, mistake) - gref)[6:] / gb[6:]).max())
        return e0, el, eg

    e0, el, eg = figures(None)
    print("%s as %d robots: the robots' sums against edge_cost: %.3g of the bound at the start, %.3g at the trial point" % (name, N, e0, el))
    assert e0 <= 1.0 and el <= 1.0 and eg <= 1.0
    for mistake in XF.MISTAKES:
        w = max(figures(mistake))
        print("%s as %d robots, mistake %s: %.3g times the bound" % (name, N, mistake, w))
        assert w > 1.0, (mistake, w)


def test_the_call_is_declared_exported_and_bound():
    sym = "dpgo_team_refine_across"
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    assert sym in capi.EXPORTS, sym
    assert hasattr(capi.lib(), sym), sym
    sig = inspect.signature(capi.Team.refine)
    assert list(sig.parameters)[1:] == ["T", "method", "max_block", "max_iters", "grad_tol", "armijo", "ladder", "transport",
                                        "owner_of_robot"]
    assert [sig.parameters[k].default for k in ("max_iters", "grad_tol", "armijo", "ladder")] == [10, 1e-8, 1e-4, 8]
    from dpgo_ros_amd import distributed
    assert list(inspect.signature(distributed.refine).parameters) == ["backend_or_team", "dist", "owner_of_robot", "T", "gather", "kw"]
    assert inspect.signature(distributed.certify_and_round).parameters["refine"].default is False

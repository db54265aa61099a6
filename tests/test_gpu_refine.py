"""GPU checks of Team.refine, the Newton refinement of a trajectory on SE(3) (csrc/refine.hip, refine_block.h),
against tests/refineref.py.

Inputs (tests/test_refineref.py asserts that the float64 reference converges on each with a positive smallest eigenvalue at every
iterate): covnested_ref.banded_chain(12, 1, window=8) with noise (0.02, 0.05) as one robot, from T* perturbed by s = 1e-4, 1e-3,
1e-2; banded_chain(40, 3, window=8) with noise (0.05, 0.1) as 1, 2 and 3 robots, from s = 1e-4 (noise at seed 7, starts at seed
11).  The dense path, the nested path at max_block = 6 and at the default.  grad_tol = 1e-9 throughout: the reference's second
iterate on the 40 poses has |g|_inf = 1.07e-8, too close to the default 1e-8 for the count of iterations to be compared.
  1. after one iteration (max_iters = 1): grad_inf0 within the gradient's bound, f0 within the cost's, the step -- recovered as
     Log(T_0^-1 T_1) / -alpha -- within 5m's column bound 6 (n - 1) u cond_2(H_red) |Sigma|_2 |g|_2 of the longdouble solve, the
     decrement within what that bound and the gradient's allow, alpha the reference's
  2. the full call: converged in the reference's iterations or one more; the longdouble gradient at the returned T is below
     grad_tol; every R_i in SO(3) to 100 u; pose 0 bit for bit
  3. |T - T*|_inf within refineref.final_bound
  4. the noise-free ground truth comes back bit for bit with iterations = 0
  5. the start s = 3e-2 is refused with the path's pivot message behind "refine:", T_out untouched
  6. two calls give the same bytes; the iterate, the weights and the cost are untouched
  7. every host refusal with its message, and a good call behind them
  8. solve_certified(refine=True) on tinyGrid3D
Each test prints its largest error / bound (DESIGN.md 5n records them)."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from dpgo_ros_amd import capi
from tests import applyref as AR
from tests import covref
from tests import refineref as RR
from tests.test_gpu_certificate import RTR_NESTEROV
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_gate_joint import NESTED_BLOCK
from tests.util import DATA

pytestmark = pytest.mark.gpu

F = np.float64
LD = np.longdouble
GRAD_TOL = 1e-9
METHODS = (("dense", None), ("nested", NESTED_BLOCK), ("nested", None))
TEAMS = (("chain12", 1, (1e-4, 1e-3, 1e-2)), ("chain40", 1, (1e-4,)), ("chain40", 2, (1e-4,)), ("chain40", 3, (1e-4,)))
_ref = {}


def reference(name, s):
    """the start, the reference's iteration from it and the figures of its first step, computed once"""
    if (name, s) not in _ref:
        c = RR.case(name)
        n, Q = c["n"], c["Q"]
        T0 = RR.start(c["Tstar"], n, s, 11)
        g = RR.gradient(Q, T0, n)
        Hr = RR.hessian_red(Q, T0, n)
        X = AR.reference(Hr, np.asarray(g, dtype=F).reshape(-1, 1))[:, 0]  # (longdouble)
        w = np.linalg.eigvalsh(Hr)
        gb = RR.gradient_bound(Q, T0, n)
        sb = float(AR.bound(Hr, np.asarray(g, dtype=F).reshape(-1, 1))[0])  # 5m's column bound
        g64, X64 = np.asarray(g, dtype=F), np.asarray(X, dtype=F)
        _ref[(name, s)] = dict(T0=T0, g=g, X=X, gb=gb, step_bound=sb, f0=RR.edge_cost(c["m"], T0, n, LD),
                               f0_bound=RR.cost_bound(c["m"], T0, n), dec=float(g @ X),
                               dec_bound=float(np.linalg.norm(g64)) * (sb + float(np.linalg.norm(gb)) / w[0])
                               + float(np.linalg.norm(gb) * np.linalg.norm(X64))
                               + 6 * n * RR.U * float(np.abs(g64) @ np.abs(X64)),
                               run=RR.newton(c["m"], n, T0, grad_tol=GRAD_TOL))
    return _ref[(name, s)]


def recovered_step(T0, T1, alpha, n):
    """xi with T1 = T0 [+] (-alpha xi)"""
    A, B = np.asarray(T0).reshape(n, 4, 3), np.asarray(T1).reshape(n, 4, 3)
    xi = np.zeros((n, 6))
    for g in range(n):
        xi[g, :3] = Rotation.from_matrix(A[g, :3, :] @ B[g, :3, :].T).as_rotvec()  # (R0^T R1; the rows of the layout are columns)
        xi[g, 3:] = B[g, 3, :] - A[g, 3, :]
    return xi.reshape(-1) / -alpha


def state(t):
    return t.global_X().tobytes(), b"".join(t.agents[i].measurements().tobytes() for i in t.ids), t.cost()


@pytest.mark.parametrize("method,max_block", METHODS)
@pytest.mark.parametrize("name,N,starts", TEAMS)
def test_first_iteration_against_the_reference(name, N, starts, method, max_block):
    c = RR.case(name)
    n = c["n"]
    t = team_of(c["m"], n, N, c["truth"])
    for s in starts:
        r = reference(name, s)
        out = t.refine(r["T0"], method=method, max_block=max_block, max_iters=1, grad_tol=GRAD_TOL)
        h = out["history"]
        assert out["status"] == "max_iters" and out["iterations"] == 1 and len(h["alpha"]) == 1
        eg = abs(out["grad_inf0"] - float(np.abs(r["g"]).max())) / r["gb"].max()
        ef = abs(float(LD(out["f0"]) - r["f0"])) / r["f0_bound"]
        ed = abs(h["decrement"][0] - r["dec"]) / r["dec_bound"]
        X = recovered_step(r["T0"], out["T"], h["alpha"][0], n)
        ex = float(np.linalg.norm(np.asarray(X - r["X"], dtype=F))) / r["step_bound"]
        print("%s, %d robots, %s max_block %s, s = %g: grad_inf0 %.3g, f0 %.3g, step %.3g, decrement %.3g of their bounds; alpha %g, "
              "pivot_min %.3g" % (name, N, method, max_block, s, eg, ef, ex, ed, h["alpha"][0], h["pivot_min"][0]))
        assert eg <= 1.0 and ef <= 1.0 and ex <= 1.0 and ed <= 1.0
        assert h["alpha"][0] == r["run"]["history"]["alpha"][0]
        assert h["pivot_min"][0] > 0 and out["covariance"].n == 6 * (n - 1) and out["covariance"].min_pivot == h["pivot_min"][0]
        assert out["f0"] == h["f"][0] and out["f"] == h["f"][1] and out["grad_inf"] == h["grad_inf"][1]
    t.close()


@pytest.mark.parametrize("method,max_block", METHODS)
@pytest.mark.parametrize("name,N,starts", TEAMS)
def test_full_call_converges_as_the_reference_does(name, N, starts, method, max_block):
    c = RR.case(name)
    n, Q = c["n"], c["Q"]
    t = team_of(c["m"], n, N, c["truth"])
    before = state(t)
    fb = RR.final_bound(Q, c["Tstar"], n, GRAD_TOL)
    for s in starts:
        r = reference(name, s)
        out = t.refine(r["T0"], method=method, max_block=max_block, grad_tol=GRAD_TOL)
        its = r["run"]["iterations"]
        g = float(np.abs(np.asarray(RR.gradient(Q, out["T"], n), dtype=F)).max())
        P = out["T"].reshape(n, 4, 3)[:, :3, :]
        orth = float(np.abs(np.einsum("gcb,gdb->gcd", P, P) - np.eye(3)).max())
        det = float(np.abs(np.linalg.det(P) - 1.0).max())
        err = float(np.abs(out["T"] - c["Tstar"]).max())
        print("%s, %d robots, %s max_block %s, s = %g: %s in %d iterations (reference %d), alpha %s, |g|_inf %s, longdouble |g|_inf "
              "%.3g, |R^T R - I| %.3g u, |T - T*|_inf %.3g = %.3g of the bound" %
              (name, N, method, max_block, s, out["status"], out["iterations"], its, out["history"]["alpha"],
               ["%.3g" % v for v in out["history"]["grad_inf"]], g, orth / RR.U, err, err / fb))
        assert out["status"] == "converged" and out["iterations"] in (its, its + 1)
        assert out["grad_inf"] <= GRAD_TOL and g <= GRAD_TOL
        assert orth <= 100 * RR.U and det <= 100 * RR.U
        assert out["T"][:12].tobytes() == r["T0"][:12].tobytes(), "pose 0 moved"
        assert err <= fb
        assert len(out["history"]["f"]) == out["iterations"] + 1 == len(out["history"]["alpha"]) + 1
        # 6. the same bytes
        again = t.refine(r["T0"], method=method, max_block=max_block, grad_tol=GRAD_TOL)
        assert again["T"].tobytes() == out["T"].tobytes() and again["iterations"] == out["iterations"]
        for key in out["history"]:
            assert again["history"][key].tobytes() == out["history"][key].tobytes(), key
    assert state(t) == before
    t.close()


@pytest.mark.parametrize("method,max_block", METHODS)
def test_noise_free_ground_truth_comes_back_bit_for_bit(method, max_block):
    c = RR.case("chain40")
    n = c["n"]
    t = team_of(c["clean"], n, 2, c["truth"])
    out = t.refine(c["truth"], method=method, max_block=max_block)
    print("noise-free ground truth, %s max_block %s: f %.3g, |g|_inf %.3g" % (method, max_block, out["f"], out["grad_inf"]))
    assert out["status"] == "converged" and out["iterations"] == 0 and out["T"].tobytes() == c["truth"].tobytes()
    assert out["covariance"].n == 0 and len(out["history"]["alpha"]) == 0 and out["f0"] == out["f"]
    t.close()


def raw_refine(t, T, method, max_block, max_iters, grad_tol, armijo, ladder, T_out, hist, out, res):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return capi.lib().dpgo_team_refine(None if t is None else t.h, p(T), method, max_block, max_iters, C.c_double(grad_tol),
                                       C.c_double(armijo), ladder, p(T_out), p(hist), None if out is None else C.byref(out),
                                       None if res is None else C.byref(res))


@pytest.mark.parametrize("method,max_block", METHODS)
def test_a_start_outside_the_basin_is_refused_with_the_pivot_message(method, max_block):
    c = RR.case("chain12")
    n = c["n"]
    t = team_of(c["m"], n, 1, c["truth"])
    Tb = RR.start(c["Tstar"], n, 3e-2, 11)
    T_out, hist, out, res = np.full(12 * n, 7.25), np.full((11, 5), 7.25), capi.Refine(), capi.Covariance()
    out.iterations = res.n = 5
    code = capi.GATE_NESTED if method == "nested" else capi.GATE_DENSE
    assert raw_refine(t, Tb, code, max_block or 0, 10, 1e-8, 1e-4, 8, T_out, hist, out, res) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    assert msg.startswith("refine: ") and "non-positive pivot" in msg and "the Hessian is not positive definite at this T: not a minimum" in msg, msg
    assert (T_out == 7.25).all() and (hist == 7.25).all()
    assert bytes(out) == bytes(capi.Refine()) and bytes(res) == bytes(capi.Covariance())
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.refine(Tb, method=method, max_block=max_block)
    assert t.refine(RR.start(c["Tstar"], n, 1e-4, 11), method=method, max_block=max_block, grad_tol=GRAD_TOL)["status"] == "converged"
    t.close()


def test_refusals_leave_the_outputs_untouched():
    c = RR.case("chain40")
    n = c["n"]
    t = team_of(c["m"], n, 2, c["truth"])
    T0 = reference("chain40", 1e-4)["T0"]
    T_out, hist, out, res = np.full(12 * n, 7.25), np.full((11, 5), 7.25), capi.Refine(), capi.Covariance()

    def refused(what, t_=t, T_=T0, method=capi.GATE_DENSE, max_block=0, max_iters=10, grad_tol=1e-8, armijo=1e-4, ladder=8, T_out_=T_out,
                hist_=hist, out_=out, res_=res):
        out.iterations = res.n = 5
        rc = raw_refine(t_, T_, method, max_block, max_iters, grad_tol, armijo, ladder, T_out_, hist_, out_, res_)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg and msg.startswith("refine:"), (rc, msg)
        assert (T_out == 7.25).all() and (hist == 7.25).all()
        if out_ is not None:
            assert bytes(out) == bytes(capi.Refine())
        if res_ is not None:
            assert bytes(res) == bytes(capi.Covariance())
        return msg

    for kw in (dict(t_=None), dict(T_=None), dict(T_out_=None), dict(hist_=None), dict(out_=None), dict(res_=None)):
        refused("null argument", **kw)
    refused("max_iters must not be negative, not -1", max_iters=-1)
    refused("ladder must lie in [1, 32], not 0", ladder=0)
    refused("ladder must lie in [1, 32], not 33", ladder=33)
    for bad in (0.0, -1e-8, np.nan, np.inf):
        refused("grad_tol must be positive", grad_tol=bad)
    for bad in (0.0, 1.0, -0.5, 2.0, np.nan):
        refused("armijo must lie in (0, 1)", armijo=bad)
    refused("method must be", method=3)
    msg = refused("DPGO_GATE_NESTED", method=capi.GATE_SCHUR)
    assert "no robot split has the Schur path's sets" in msg
    Tb = T0.copy()
    Tb[12 * 17] *= 1.001
    refused("pose 17 of T is not in SE(3)", T_=Tb)
    with pytest.raises(capi.DpgoError, match="Schur path's sets"):
        t.refine(T0, method="schur")
    with pytest.raises(ValueError, match="method must be"):
        t.refine(T0, method="sparse")
    with pytest.raises(ValueError, match="T holds"):
        t.refine(T0[:-12])
    # and a good call runs behind them, also with a ladder of one entry, with T_out = T and with max_iters = 0
    want = reference("chain40", 1e-4)["run"]
    for code, mb in ((capi.GATE_DENSE, 0), (capi.GATE_NESTED, NESTED_BLOCK)):
        Tio = T0.copy()
        assert raw_refine(t, Tio, code, mb, 10, GRAD_TOL, 1e-4, 1, Tio, hist, out, res) == capi.OK
        assert out.status == 0 and out.iterations in (want["iterations"], want["iterations"] + 1) and res.n == 6 * (n - 1)
        assert np.isnan(hist[out.iterations, 2:]).all() and not np.isnan(hist[:out.iterations]).any()
    z = t.refine(T0, max_iters=0, grad_tol=GRAD_TOL)
    assert z["status"] == "max_iters" and z["iterations"] == 0 and z["T"].tobytes() == T0.tobytes() and z["covariance"].n == 0
    t.close()


def test_solve_certified_refines_on_request():
    ds = "tinyGrid3D"
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    prm = capi.default_params(r=5, num_robots=1, **RTR_NESTEROV)
    Tc = capi.chordal_init(m, n)
    plain = capi.solve_certified(m, prm, r0=5, T=Tc, iters=300)
    out = capi.solve_certified(m, prm, r0=5, T=Tc, iters=300, refine=True, covariances=True)
    assert sorted(out) == sorted(list(plain) + ["refine", "covariances"])
    r = out["refine"]
    print("solve_certified(refine=True) on %s: %s in %d iterations, |g|_inf %.3g -> %.3g, f %.15g -> %.15g, f_rounded %.15g" %
          (ds, r["status"], r["iterations"], r["grad_inf0"], r["grad_inf"], r["f0"], r["f"], out["f_rounded"]))
    assert r["status"] == "converged" and r["grad_inf"] <= 1e-8
    assert out["T"].tobytes() == r["T"].tobytes() and out["f_rounded"] == plain["f_rounded"]
    # the descent is checked within ONE summation, the call's own sum of the measurements' terms
    assert r["f"] <= r["f0"] + r["iterations"] * RR.eps_f(r["f0"], len(m))
    # f_rounded is another summation of the cost at the rounded point, 1/2 <T, T Q>, whose terms cancel: it is known to
    # (4 d + 16) u / 2 |T| |Q| |T|^T, d the most blocks in a row of Q (the rounding of Q's entries and of the row sums)
    Qa = abs(covref.q_full(m, n)).tocsr()
    Ta = np.abs(covref.as_matrix(plain["T"], 3, n))
    d = int(np.diff(Qa[::4].indptr).max() // 4) + 1
    slack = (4 * d + 16) * RR.U * 0.5 * float(np.sum(Ta * (Qa @ Ta.T).T))
    print("f - f_rounded = %.3g, the cancellation bound of f_rounded %.3g" % (r["f"] - out["f_rounded"], slack))
    assert r["f"] <= out["f_rounded"] + slack
    t = capi.Team.from_measurements(m, prm)
    t.set_initial(out["T"], capi.fixed_stiefel(5))
    assert t.covariances(out["T"])[1].tobytes() == out["covariances"][1].tobytes()  # taken at the refined T
    t.close()

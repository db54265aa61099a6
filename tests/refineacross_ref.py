"""numpy statement of the Newton refinement of a trajectory over a team split across participants (DESIGN.md 5n "Across teams",
csrc/refine.hip), on top of tests/refineref.py and tests/applyacross_ref.py.

What the split changes of refineref.newton, restated here in float64:
    owners        a measurement belongs to one robot: a private one to its own, a shared one to the lower robot id
    robot_costs   every robot sums the terms of its own measurements; the robots' totals are added in robot order from 0.  A robot
                  evaluates its terms on ITS view of the trajectory: its own poses and the remote end points of its shared
                  measurements (the halo)
    trial_views   the trial point T [+] (-alpha X) as each robot sees it: the rows of X of a halo pose are read out of x_S, the
                  separator's part of X, at the pose's place there (robot after robot, each robot's public poses in order)
    decrement     every robot's g_a^T X_a over its own rows, the robots' shares in robot order
    eps_f         (24 + max_a ceil(E_a / 256) + R) u f: refineref's chain, the workgroup partials of the largest robot, and the R
                  robots' totals added one after another
    the step      applyacross_ref.eliminate on covschur_ref.partition's sets with V = g
The measuring sticks are refineref's (gradient, gradient_bound, edge_cost, cost_bound, final_bound) and applyref.bound on the whole
problem; none of them is the code under test.

MISTAKES, each rejected by those bounds (tests/test_refineacross_ref.py): "both": a shared measurement counted by both of its
robots; "unstepped": the remote end point of a shared measurement left where it was in the trials; "local0": every robot holds
its own first pose fixed; "swap": the halo rows of X read from x_S with the public blocks of the first two robots that have
any changed over."""
import numpy as np

from tests import applyacross_ref as XR
from tests import covref
from tests import covschur_ref as SR
from tests import refineref as RR

F = np.float64
LD = np.longdouble
U = RR.U
MISTAKES = ("both", "unstepped", "local0", "swap")

_cases = {}
_splits = {}


def case(name):
    """refineref.case for "chain12" and "chain40"; "band40": the ground truth of banded_chain(40, 3, window=8) with a measurement
    for every pair i < j <= min(i + 16, 39) (504 of them), noise (0.05, 0.1) at seed 7 through refineref.noisy"""
    if name != "band40":
        return RR.case(name)
    if name not in _cases:
        from dpgo_ros_amd import capi
        from tests.covnested_ref import banded_chain
        n = 40
        _, truth = banded_chain(n, 3, window=8)
        P = truth.reshape(n, 4, 3)
        Rg, tg = P[:, :3, :].transpose(0, 2, 1), P[:, 3, :]
        src, dst = np.array([(i, j) for i in range(n) for j in range(i + 1, min(i + 16, n - 1) + 1)]).T
        clean = np.zeros(len(src), dtype=capi.MEAS_DTYPE)
        clean["p1"], clean["p2"] = src, dst
        clean["R"] = np.einsum("eji,ejk->eik", Rg[src], Rg[dst]).reshape(len(src), 9)
        clean["t"] = np.einsum("eji,ej->ei", Rg[src], tg[dst] - tg[src])
        clean["kappa"], clean["tau"], clean["weight"] = 100.0, 50.0, 1.0
        m = RR.noisy(clean, 0.05, 0.1, 7)
        Tstar = RR.optimum(m, n, truth)
        _cases[name] = dict(m=m, n=n, truth=truth, Tstar=Tstar, Q=covref.q_full(m, n), clean=clean)
    return _cases[name]


def split(name, N):
    """dict(mp: the measurements split over N robots by capi.partition, robot_of, public, owner: the robot every measurement of
    the single-robot list belongs to, owned: their number per robot), computed once"""
    from dpgo_ros_amd import capi
    if (name, N) not in _splits:
        c = case(name)
        m, n = c["m"], c["n"]
        mp = capi.partition(m, n, N) if N > 1 else m
        robot_of, public = SR.partition(mp, n, N)
        owner = np.minimum(robot_of[m["p1"]], robot_of[m["p2"]])
        _splits[(name, N)] = dict(mp=mp, robot_of=robot_of, public=public, owner=owner, owned=np.bincount(owner, minlength=N), N=N)
    return _splits[(name, N)]


def eps_f(f, owned):
    return (RR.EPS_CHAIN + int(max((int(e) + 255) // 256 for e in owned)) + len(owned)) * U * abs(f)


def robot_costs(m, sp, views, n, mistake=None):
    """the robots' totals of the cost, robot a's measurements evaluated on views[a] (a trajectory of n poses: what a sees)"""
    r1, r2 = sp["robot_of"][m["p1"]], sp["robot_of"][m["p2"]]
    out = np.zeros(sp["N"])
    for a in range(sp["N"]):
        mine = (sp["owner"] == a) | (((r1 == a) | (r2 == a)) if mistake == "both" else False)
        out[a] = RR.edge_terms(m[mine], views[a], n).sum() if mine.any() else 0.0
    return out


def total(parts):
    """the robots' totals added in robot order from 0"""
    v = 0.0
    for p in parts:
        v = v + float(p)
    return v


def trial_views(sp, T, X, alpha, n, mistake=None):
    """per robot, the trial trajectory as it sees it: its own poses stepped by their rows of X, every other pose by the rows the
    robot reads out of x_S (a pose that is not public is never read by another robot: left where it is)"""
    robot_of, public = sp["robot_of"], sp["public"]
    X6 = np.asarray(X, dtype=F).reshape(n, 6)
    sep = [g for g in range(1, n) if public[g]]  # (robot after robot: the poses are numbered by robot)
    xS = X6[sep].copy() if sep else np.zeros((0, 6))
    place = {g: k for k, g in enumerate(sep)}
    if mistake == "swap":
        have = [a for a in range(sp["N"]) if any(robot_of[g] == a for g in sep)][:2]
        ia, ib = ([k for k, g in enumerate(sep) if robot_of[g] == a] for a in have)
        order = [k for k in range(len(sep)) if k < ia[0]] + ib + [k for k in range(len(sep)) if ia[-1] < k < ib[0]] + ia + \
                [k for k in range(len(sep)) if k > ib[-1]]
        xS = xS[order]
    views = []
    for a in range(sp["N"]):
        Xa = np.zeros((n, 6))
        for g in range(n):
            if robot_of[g] == a:
                Xa[g] = X6[g]
            elif g in place and mistake != "unstepped":
                Xa[g] = xS[place[g]]
        if mistake == "local0":
            Xa[np.flatnonzero(robot_of == a)[0]] = 0.0
        Xa[0] = 0.0
        views.append(covref.perturb(T, -alpha * Xa.reshape(-1), n))
    return views


def gradient(Q, T, sp, n, mistake=None):
    """refineref.gradient in float64; "local0": the rows of every robot's first pose zero"""
    g = np.asarray(RR.gradient(Q, T, n), dtype=F).reshape(n, 6).copy()
    if mistake == "local0":
        for a in range(sp["N"]):
            g[np.flatnonzero(sp["robot_of"] == a)[0]] = 0.0
    return g.reshape(-1)


def decrement(sp, g, X, n):
    g6, X6 = np.asarray(g, dtype=F).reshape(n, 6), np.asarray(X, dtype=F).reshape(n, 6)
    return total(float(np.sum(g6[sp["robot_of"] == a] * X6[sp["robot_of"] == a])) for a in range(sp["N"]))


def newton(name, N, T0, max_iters=10, grad_tol=1e-8, armijo=1e-4, ladder=8, mistake=None):
    """the iteration of dpgo_team_refine_across in float64: a dict in the shape of Team.refine's, with `X` (the steps) and
    `eig_min` in its history.  "indefinite" also at the start: the library refuses that"""
    c, sp = case(name), split(name, N)
    m, n, Q = c["m"], c["n"], c["Q"]
    T = np.array(T0, dtype=F)
    hist = dict(f=[], grad_inf=[], alpha=[], decrement=[], eig_min=[], X=[])
    k, status = 0, None
    while True:
        g = gradient(Q, T, sp, n, mistake)
        f = total(robot_costs(m, sp, [T] * N, n, mistake))
        hist["f"].append(f)
        hist["grad_inf"].append(float(np.abs(g).max()))
        if hist["grad_inf"][-1] <= grad_tol:
            status = "converged"
            break
        if k == max_iters:
            status = "max_iters"
            break
        Hr = RR.hessian_red(Q, T, n)
        w = np.linalg.eigvalsh(Hr)
        hist["eig_min"].append(float(w[0]))
        if not w[0] > 0:
            status = "indefinite"
            break
        X = XR.eliminate(Hr, sp["robot_of"], sp["public"], g.reshape(-1, 1))[:, 0]
        dec = decrement(sp, g, X, n)
        hist["decrement"].append(dec)
        hist["X"].append(X)
        took = None
        for l in range(ladder):
            a = 2.0 ** -l
            views = trial_views(sp, T, X, a, n, mistake)
            fl = total(robot_costs(m, sp, views, n, mistake))
            if fl <= f - armijo * a * dec + eps_f(f, sp["owned"]):
                took = a
                break
        if took is None:
            status = "no_descent"
            break
        hist["alpha"].append(took)
        T = RR.trial(T, X, took, n)
        k += 1
    return dict(T=T, status=status, iterations=k, f0=hist["f"][0], f=hist["f"][-1], grad_inf0=hist["grad_inf"][0],
                grad_inf=hist["grad_inf"][-1], history=hist)

"""numpy statement of X = Sigma V over a team split across participants (DESIGN.md 5m "across teams",
csrc/covariance_schur.hip, csrc/covariance_apply.hip), written from the definitions.

Two parts.
    eliminate   the elimination in the device's order, in float64, on covschur_ref.partition's robot-wise sets: for robot a
                with interior poses I_a and public poses S_a, v_a = V[I_a],
                    u_a = C_a v_a,  r_a = v_{S_a} - W_a^T v_a  (no interior pose: r_a = v_{S_a}),
                    r_S = the r_a of every robot at the robot's place in the separator,
                    x_S = Sigma_SS r_S,  x_a = u_a - W_a x_S[S_a],  X[I_a] = x_a,  X[S_a] = x_S[S_a].
                Which participant holds a robot changes nothing of it: the split does not appear.
    the measuring stick is tests/applyref.py's: applyref.reference (the longdouble dense solve on covref's H_red of the whole
                problem) and applyref.bound, 6 (n - 1) u cond_2(H_red) |Sigma_red|_2 |v_red|_2 per column.  It is not the
                code under test and shares nothing with the elimination but H_red."""
import numpy as np

from tests import applyref as AR
from tests import covref
from tests import covschur_ref as SR
from tests.covnested_ref import banded_chain

F = np.float64

# (poses, seed, robots, (public, interior) per robot with pose 0 among robot 0's interior; window = 8): a robot with no
# interior pose; the plain case; a robot with no interior pose among seven with interior poses; an empty separator
GRAPHS = [(12, 1, 3, [(1, 3), (4, 0), (2, 2)]),
          (40, 3, 3, [(2, 11), (5, 8), (4, 10)]),
          (40, 3, 8, [(1, 4), (2, 3), (2, 3), (4, 1), (3, 2), (5, 0), (4, 1), (1, 4)]),
          (40, 3, 1, [(0, 40)])]
MISTAKES = ("sign", "no_wtv", "swap", "pose0")

_graphs = {}


def graph(n, seed, N):
    """dict(m: the measurements in single-robot numbering, mp: split over N robots, T: the ground truth, Hr, robot_of, public),
    computed once"""
    from dpgo_ros_amd import capi
    key = (n, seed, N)
    if key not in _graphs:
        m, T = banded_chain(n, seed, window=8)
        mp = capi.partition(m, n, N) if N > 1 else m
        robot_of, public = SR.partition(mp, n, N)
        Hr = covref.dense_reference(covref.q_full(m, n), T, n)[0]
        _graphs[key] = dict(m=m, mp=mp, T=T, Hr=Hr, robot_of=robot_of, public=public, n=n, N=N)
    return _graphs[key]


def counts(robot_of, public):
    """(public, interior) poses per robot, pose 0 counted among robot 0's interior"""
    A = int(robot_of.max()) + 1
    return [(int(public[robot_of == a].sum()), int((~public[robot_of == a]).sum())) for a in range(A)]


def eliminate(Hr, robot_of, public, V, mistake=None):
    """X (6 n x m, float64) by the robot-wise elimination.  mistake: one of MISTAKES -- "sign": + W_a x_S; "no_wtv": r_a
    without its W_a^T v_a term; "swap": the r_a of the first two robots that have public poses change places in r_S;
    "pose0": pose 0's rows of V added into the first rows that are read"""
    assert mistake is None or mistake in MISTAKES
    info = SR.sets(robot_of, public)
    sep, interior, sep_of = info["separator"], info["interior"], info["sep_of"]
    Hr, V = np.asarray(Hr, dtype=F), np.asarray(V, dtype=F)
    Vr = V[6:].copy()
    if mistake == "pose0":
        Vr[:6] += V[:6]
    m = V.shape[1]
    rS = SR.rows(sep) if sep else np.zeros(0, dtype=np.int64)
    Sc = Hr[np.ix_(rS, rS)].copy()
    Xr = np.zeros((Hr.shape[0], m))
    W, loc, rI, r_parts = {}, {}, {}, []
    for a in range(len(interior)):
        la = (6 * np.asarray(sep_of[a], dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)  # inside the separator
        loc[a] = la
        r_a = Vr[rS[la]].copy()
        if interior[a]:
            r = SR.rows(interior[a])
            B = Hr[np.ix_(r, rS[la])]
            C = np.linalg.inv(Hr[np.ix_(r, r)])
            W[a], rI[a] = C @ B, r
            Sc[np.ix_(la, la)] -= B.T @ W[a]
            Xr[r] = C @ Vr[r]  # u_a
            if mistake != "no_wtv":
                r_a = r_a - W[a].T @ Vr[r]
        r_parts.append(r_a)
    if mistake == "swap":
        i, j = [a for a in range(len(r_parts)) if len(r_parts[a])][:2]
        r_parts[i], r_parts[j] = r_parts[j], r_parts[i]
    if sep:
        r_S = np.concatenate(r_parts, axis=0)
        Sc = 0.5 * (Sc + Sc.T)
        x_S = np.linalg.inv(Sc) @ r_S
        Xr[rS] = x_S
        for a in W:
            Xr[rI[a]] = Xr[rI[a]] + W[a] @ x_S[loc[a]] if mistake == "sign" else Xr[rI[a]] - W[a] @ x_S[loc[a]]
    return AR.full(Xr)


def reference(Hr, V):
    """the measuring stick: (X by the longdouble dense solve, the per-column bound)"""
    return AR.reference(Hr, V), AR.bound(Hr, V)

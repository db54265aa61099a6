"""GPU checks of the SE-Sync rounding (csrc/round.hip, Team.round, solve_certified) against the numpy statement of
tests/test_rounding.py: lifted exact points, random manifold points, weights, the SE-Sync optima, the end-to-end
certified solve, the translation entry point against chordal's, determinism, no side effects and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests.test_certificate import as_matrix, q_full, random_manifold_point
from tests.test_gpu_certificate import ETA, OPTIMA, converge, team_at
from tests.test_rounding import anchored, cost_numpy, from_T, refine_translations, round_numpy
from tests.util import DATA, ROOT

pytestmark = pytest.mark.gpu

_CHORDAL = {}


def chordal(ds):
    if ds not in _CHORDAL:
        m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
        _CHORDAL[ds] = (m, n, capi.chordal_init(m, n))
    return _CHORDAL[ds]


def relerr(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


@pytest.mark.parametrize("ds,N", [("smallGrid3D", 2), ("sphere2500", 5)])
def test_lifted_chordal_point_rounds_to_chordal(ds, N):
    m, n, T = chordal(ds)
    ref = anchored(T)
    for r in range(3, 9):
        t, _, _ = team_at(ds, N, T=T, r=r)
        f = t.cost()
        rd0, T0 = t.round(refine_translations=False)
        rd1, T1 = t.round()
        print("%s / %d, r = %d: unrefined %.3e, refined %.3e, %r" % (ds, N, r, relerr(T0, ref), relerr(T1, ref), rd1))
        assert rd0.r == r and rd0.refined == 0 and rd1.refined == 1 and rd0.num_degenerate == 0
        assert relerr(T0, ref) <= 1e-12
        assert relerr(T1, ref) <= 1e-12
        s = np.array(rd0.sigma)
        assert (s[3:r] <= 1e-12 * s[0]).all() and (s[r:] == 0).all()
        assert abs(rd0.f_rounded - rd0.f_relaxed) <= 1e-12 * rd0.f_relaxed
        assert abs(rd1.f_rounded - rd1.f_relaxed) <= 1e-12 * rd1.f_relaxed
        assert abs(rd0.f_relaxed - f) <= 1e-12 * f
        t.close()


@pytest.mark.parametrize("ds,N", [("smallGrid3D", 3), ("sphere2500", 5)])
@pytest.mark.parametrize("r", [5, 7, 8])
def test_random_point_matches_numpy(ds, N, r):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    X = random_manifold_point(np.random.default_rng(20 + r), r, n)
    t, _, _ = team_at(ds, N, X=X, r=r)
    rd0, T0 = t.round(refine_translations=False)
    ref, _, sigma = round_numpy(X, r, n)
    assert np.abs(T0 - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())
    # (`reflected` is relative to the eigensolver's signs of U, so it is not compared with numpy's; T does not depend on them)
    assert rd0.num_degenerate == 0
    assert np.abs(np.array(rd0.sigma[:r]) - sigma).max() <= 1e-10 * sigma[0]
    Xm = as_matrix(X, r, n)
    f_x = 0.5 * float(np.sum(Xm * (q_full(m, n) @ Xm.T).T))
    assert abs(rd0.f_relaxed - f_x) <= 1e-12 * f_x
    assert abs(rd0.f_relaxed - t.cost()) <= 1e-12 * f_x
    assert abs(rd0.f_rounded - cost_numpy(m, n, T0)) <= 1e-10 * rd0.f_rounded
    rd1, T1 = t.round()
    R0, _ = from_T(T0)
    R1, t1 = from_T(T1)
    assert np.array_equal(R0, R1)
    _, ts = from_T(refine_translations(m, n, T0))
    assert relerr(t1, ts) <= 1e-8
    assert rd1.f_rounded <= rd0.f_rounded * (1 + 1e-12), (rd0, rd1)
    assert abs(rd1.f_rounded - cost_numpy(m, n, T1)) <= 1e-10 * rd1.f_rounded
    t.close()


def test_current_weights_enter_the_refinement_and_the_cost():
    ds, N, r = "smallGrid3D", 2, 5
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    X = random_manifold_point(np.random.default_rng(8), r, n)
    t, _, _ = team_at(ds, N, X=X, r=r)
    shared = np.nonzero(mp["r1"] != mp["r2"])[0]
    own = np.nonzero(mp["r1"] == mp["r2"])[0]
    pick = list(own[[3, 40, 77, 150]]) + list(shared[:3])
    mw = m.copy()
    for k, w in zip(pick, [0.25, 3.0, 0.5, 1.7, 0.1, 2.5, 0.6]):
        e = mp[k]
        for a in {int(e["r1"]), int(e["r2"])}:
            assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), w)
            t.agents[a].clear_data_matrices()
        mw["weight"][k] = w
    rd0, T0 = t.round(refine_translations=False)
    rd1, T1 = t.round()
    Xm = as_matrix(X, r, n)
    f_x = 0.5 * float(np.sum(Xm * (q_full(mw, n) @ Xm.T).T))
    assert abs(rd0.f_relaxed - f_x) <= 1e-12 * f_x
    assert abs(rd0.f_rounded - cost_numpy(mw, n, T0)) <= 1e-10 * rd0.f_rounded
    _, ts = from_T(refine_translations(mw, n, T0))
    assert relerr(from_T(T1)[1], ts) <= 1e-8
    _, ts_unweighted = from_T(refine_translations(m, n, T0))
    assert relerr(ts, ts_unweighted) > 1e-6  # (the weights matter)
    assert abs(rd1.f_rounded - cost_numpy(mw, n, T1)) <= 1e-10 * rd1.f_rounded
    t.close()


@pytest.mark.parametrize("ds,N,at_optimum,kw", OPTIMA, ids=[o[0] for o in OPTIMA])
def test_sesync_optima_round_tight(ds, N, at_optimum, kw):
    t, m, n = team_at(ds, N, **kw)
    k = converge(t, at_optimum)
    assert k > 0, "the pinned optimum was not reached in %d iterations (cost %.12g)" % (-k, t.cost())
    rd0, _ = t.round(refine_translations=False)
    rd, T = t.round()
    print("%s / %d: %r, gap %.3e unrefined, %.3e refined" % (ds, N, rd, (rd0.f_rounded - rd0.f_relaxed) / rd0.f_relaxed,
                                                             (rd.f_rounded - rd.f_relaxed) / rd.f_relaxed))
    assert abs(rd0.f_rounded - rd0.f_relaxed) <= 1e-6 * rd0.f_relaxed
    # the refinement may land BELOW f_relaxed: the iterate is only as close to the optimum as the pinned tolerance (torus3D:
    # 2e-5 of 2f), and the translations re-solved for its rounded rotations are optimal.  As a bound the gap is one-sided.
    assert rd.f_rounded - rd.f_relaxed <= 1e-6 * rd.f_relaxed
    assert at_optimum(rd.f_rounded) and at_optimum(rd0.f_rounded), (rd0, rd)
    assert T[:12].tolist() == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]
    t.close()


def test_solve_certified_end_to_end():
    ds = "smallGrid3D"
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    prm = capi.default_params(r=3, num_robots=1, method=capi.METHOD_RTR, rtr_iterations=10, rtr_tcg_iterations=100,
                              gradnorm_tol=1e-9)
    X0 = random_manifold_point(np.random.default_rng(1), 3, n)
    out = capi.solve_certified(m, prm, r0=3, r_max=8, eta=ETA, X0=X0, iters=40, first_iters=0)
    rd = out["rounding"]
    print("solve_certified: ranks %s, %r, gap_rel %s" % (out["ranks"], rd, out["gap_rel"]))
    assert out["certificate"].certified == 1 and out["r"] >= 4
    assert out["gap_rel"] is not None and abs(out["gap_rel"]) <= 1e-6
    assert out["f_relaxed"] == rd.f_relaxed and out["f_rounded"] == rd.f_rounded and rd.refined == 1
    assert out["T"].size == 12 * n
    ref, _, _ = team_at(ds, 1, method=capi.METHOD_RTR, rtr_iterations=10, rtr_tcg_iterations=100, gradnorm_tol=1e-9)
    ref.run(40)
    f5 = ref.cost()
    ref.close()
    assert abs(out["f_rounded"] - f5) <= 1e-6 * f5, (out["f_rounded"], f5)
    # the staircase's own result is untouched: rounding on the final team leaves its X bitwise as riemannian_staircase has it
    st = capi.riemannian_staircase(m, prm, r0=3, r_max=8, eta=ETA, X0=X0, iters=40, first_iters=0)
    seen = {}

    def after_round(team, o):
        team.round()
        seen["X"] = [team.agents[i].get_X() for i in team.ids]

    capi._staircase(m, prm, 3, 8, ETA, None, X0, 40, 0, None, 30, None, 0, on_final=after_round)
    assert st["ranks"] == out["ranks"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(st["X"], seen["X"]))


@pytest.mark.parametrize("ds", ["tinyGrid3D", "smallGrid3D", "sphere2500", "torus3D", "cubicle", "parking-garage"])
def test_translations_given_rotations_reproduce_chordal(ds):
    m, n, T = chordal(ds)
    Tz = T.copy().reshape(n, 12)
    Tz[:, 9:] = 0.0
    got = capi.translations_given_rotations(m, n, Tz)
    assert np.array_equal(got.reshape(n, 12)[:, :9], T.reshape(n, 12)[:, :9])
    assert relerr(got.reshape(n, 12)[:, 9:], T.reshape(n, 12)[:, 9:]) <= 1e-12


def test_translations_given_rotations_dense_path():
    """DPGO_CHORDAL_DENSE=1 sends dpgo_chordal_init to its dense path; the entry point follows it there"""
    code = ("import numpy as np, os; from dpgo_ros_amd import capi; "
            "m, n = capi.read_g2o(os.path.join(%r, 'smallGrid3D.g2o')); T = capi.chordal_init(m, n); "
            "Tz = T.copy().reshape(n, 12); Tz[:, 9:] = 0; g = capi.translations_given_rotations(m, n, Tz).reshape(n, 12); "
            "t = T.reshape(n, 12)[:, 9:]; print('REL', np.abs(g[:, 9:] - t).max() / np.abs(t).max())" % DATA)
    env = dict(os.environ, DPGO_CHORDAL_DENSE="1")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    rel = float(res.stdout.split("REL")[1].split()[0])
    assert rel <= 1e-12, rel


def test_round_is_deterministic_and_has_no_side_effects():
    """two calls give the same bits; 100 + 100 iterations of the bench configuration with a round (refined) in between leave
    X, Y and V bitwise those of a run without it"""
    kw = dict(method=capi.METHOD_RGD, acceleration=1, rgd_stepsize=0.2, rgd_use_preconditioner=1, restart_interval=20)
    outs = []
    for with_round in (False, True):
        t, m, n = team_at("sphere2500", 5, **kw)
        t.run(100)
        if with_round:
            a1, T1 = t.round()
            a2, T2 = t.round()
            assert bytes(a1) == bytes(a2) and T1.tobytes() == T2.tobytes()
            b1, U1 = t.round(refine_translations=False)
            b2, U2 = t.round(refine_translations=False)
            assert bytes(b1) == bytes(b2) and U1.tobytes() == U2.tobytes()
        t.run(100)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_refusals():
    m, n = capi.read_g2o(os.path.join(DATA, "smallGrid3D.g2o"))
    mp = capi.partition(m, n, 2)
    part = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=2), local_ids=[0])
    part.agents[0].set_X(random_manifold_point(np.random.default_rng(2), 5, part.agents[0].n))
    with pytest.raises(capi.DpgoError, match="every robot"):
        part.round()
    part.close()
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=2))
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.round()
    t.close()

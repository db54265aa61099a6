"""GPU checks of the marginal covariances by nested dissection inside each robot (csrc/covariance_nested.hip,
Team.covariances(method="nested") / Team.covariances_nested, DESIGN.md 5e "nested").

Bounds, as in tests/test_gpu_covariance.py and tests/test_gpu_covariance_schur.py: an inverse through Cholesky has the forward
error n eps cond_2(H_red) (n = 6 (N - 1), eps = 2.2e-16).  Against the numpy inverse the nested path is held to that bound,
and so is log det; against another path of the library to twice it, because both lie within it of the truth; a column block
C_p to |H_red C_p - E_p|_F <= n eps cond_est against scipy's sparse Hessian.  Nothing in them is tuned; the measured ratios
are in profiles/r12_covariance_nested.md."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests import covnested_ref as NR
from tests import covref
from tests.test_certificate import random_manifold_point
from tests.test_gpu_certificate import OPTIMA, RTR_NESTEROV, converge, team_at
from tests.test_gpu_covariance import BENCH, all_pairs, gather
from tests.test_gpu_covariance_schur import pair_cases
from tests.util import DATA, add_outliers

pytestmark = pytest.mark.gpu

EPS = covref.EPS


def team_of(m, n, N, T, **kw):
    """a team of N robots on the measurements m (single-robot numbering), initialised at the trajectory T"""
    mp = capi.partition(m, n, N) if N > 1 else m
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **dict(RTR_NESTEROV, **kw)))
    t.set_initial(T, capi.fixed_stiefel(5))
    return t


def plan_of(t, m, n, N, max_block):
    """the team's plan, which must be the host-only plan of the same pattern; returns (block_of, info, sets)"""
    rowptr, col = NR.pattern(m, n)
    block_of, info = t.covariance_plan(max_block)
    host, hinfo = capi.covariance_nested_plan(NR.robots_of(n, N), rowptr, col, max_block)
    assert block_of.tobytes() == host.tobytes() and info == hinfo
    return block_of, info, NR.sets(block_of, rowptr, col)


def check_against_numpy(tag, t, m, n, T, max_block, ref=None):
    """every diagonal block and all N^2 pairs against the numpy inverse (ref: covref.dense_reference of the same point)"""
    Hr, Sref, w = ref if ref is not None else covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0, "%s: the reference H_red is not positive definite (%.3e)" % (tag, w[0])
    cond, nn = w[-1] / w[0], 6 * (n - 1)
    bound = nn * EPS * cond
    pairs = all_pairs(n)
    res, diag, cross = t.covariances_nested(T, pairs, max_block=max_block)
    S = covref.full_sigma(diag, cross, pairs, n)
    err = np.linalg.norm(S - Sref) / np.linalg.norm(Sref)
    sign, logdet = np.linalg.slogdet(Hr)
    lerr = abs(res.logdet - logdet) / abs(logdet)
    print("%s, max_block %s: n = %d, cond_2 = %.3e, |Sigma - ref|_F / |ref|_F = %.3e (bound %.3e, ratio %.3e), logdet %.12g "
          "(rel %.3e), %r" % (tag, max_block, nn, cond, err, bound, err / bound, res.logdet, lerr, res))
    assert res.n == nn
    assert err <= bound
    assert sign > 0 and lerr <= bound
    assert res.min_pivot > 0 and res.max_pivot >= res.min_pivot
    # the diagonal block of a pose is the pair (i, i), symmetrised, bit for bit
    for g in range(n):
        Bc = cross[g * n + g]
        assert np.abs(diag[g] - 0.5 * (Bc + Bc.T)).max() == 0.0
    # pose 0: exactly zero, alone and in every pair
    assert not diag[0].any()
    zero = (pairs[:, 0] == 0) | (pairs[:, 1] == 0)
    assert not cross[zero].any() and cross[~zero].any()
    for g in range(1, n):
        assert diag[g].tobytes() == np.ascontiguousarray(diag[g].T).tobytes()
        assert np.linalg.eigvalsh(diag[g])[0] > 0
    return res


@pytest.mark.parametrize("ds,N,blocks", [("tinyGrid3D", 1, (1, 2, 3)), ("smallGrid3D", 1, (4, 16, 40)),
                                         ("smallGrid3D", 2, (4, 16, 40)), ("smallGrid3D", 3, (4, 16, 40))])
def test_small_graphs_match_the_numpy_inverse(ds, N, blocks):
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    t, _, _ = team_at(ds, N, T=capi.chordal_init(m, n), **RTR_NESTEROV)
    t.run(300)
    rd, T = t.round()
    ref = covref.dense_reference(covref.q_full(m, n), T, n)
    split = 0
    for max_block in blocks:
        _, info, _ = plan_of(t, m, n, N, max_block)
        split += info["promoted_poses"] > 0
        check_against_numpy("%s / %d, rounded T (f %.9g), %r" % (ds, N, rd.f_rounded, info), t, m, n, T, max_block, ref)
    assert split >= 2, "the block sizes do not split a robot"
    # method="nested" is the call at the default block size; T = None rounds the current iterate first
    a, d0, _ = t.covariances(method="nested")
    b, d1, _ = t.covariances_nested(T, max_block=capi.COV_NESTED_DEFAULT_BLOCK)
    assert d0.tobytes() == d1.tobytes() and a.logdet == b.logdet
    t.close()


def seeded_pairs(sets_, n, count, seed):
    """about `count` pairs that cover every case: two poses of one block, of two blocks, a block's pose with a separator pose
    both ways round, two separator poses, the same pose twice, a pair that names pose 0"""
    rng = np.random.default_rng(seed)
    blocks, sep = sets_["blocks"], sets_["separator"]
    big = [b for b in range(len(blocks)) if len(blocks[b]) > 1]
    out = [(0, blocks[0][0]), (sep[0], 0), (blocks[1][0], blocks[1][0]), (sep[1], sep[1])]
    for _ in range((count - len(out)) // 5):
        b, c = rng.choice(len(blocks), 2, replace=False)
        out.append(tuple(rng.choice(blocks[rng.choice(big)], 2)))
        out.append((rng.choice(blocks[b]), rng.choice(blocks[c])))
        out.append((rng.choice(blocks[b]), rng.choice(sep)))
        out.append((rng.choice(sep), rng.choice(blocks[c])))
        out.append(tuple(rng.choice(sep, 2)))
    return np.array(out, dtype=np.int32)


def test_tile_and_block_edges_on_banded_chains():
    """block orders 6 |I_b| on both sides of the Cholesky's NB = 32, of the 64-tiles and of the K slabs of 32, and several widths
    6 |N_b|.  Case A: all 360^2 pairs, more pairs across blocks than one launch indexes; case B: seeded pairs of every case"""
    cases = [(360, 0, 11), (600, 2, 43)]
    made, orders, widths = [], set(), set()
    for n, longs, max_block in cases:
        m, T = NR.banded_chain(n, 5, longs=longs)
        rowptr, col = NR.pattern(m, n)
        block_of, info = capi.covariance_nested_plan(np.zeros(n, dtype=np.int32), rowptr, col, max_block)
        s = NR.sets(block_of, rowptr, col)
        orders |= {6 * len(I) for I in s["blocks"]}
        widths |= {6 * len(N) for N in s["coupled"]}
        made.append((n, max_block, m, T, s, info))
    print("block orders %s, widths %s" % (sorted(orders), sorted(widths)))
    assert any(o < 32 for o in orders) and any(33 <= o <= 64 for o in orders) and any(o > 64 and o % 32 for o in orders)
    assert len(widths) >= 2
    # case A
    n, max_block, m, T, s, info = made[0]
    assert sum(len(I) for I in s["blocks"]) ** 2 > 65535
    t = team_of(m, n, 1, T)
    plan_of(t, m, n, 1, max_block)
    check_against_numpy("banded chain %d, all pairs, %r" % (n, info), t, m, n, T, max_block)
    t.close()
    # case B
    n, max_block, m, T, s, info = made[1]
    Hr, Sref, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    nn = 6 * (n - 1)
    bound = nn * EPS * w[-1] / w[0]
    pairs = seeded_pairs(s, n, 300, seed=11)
    t = team_of(m, n, 1, T)
    res, diag, cross = t.covariances_nested(T, pairs, max_block=max_block)
    t.close()
    full = np.zeros((6 * n, 6 * n))
    full[6:, 6:] = Sref
    want_d = np.stack([full[6 * g:6 * g + 6, 6 * g:6 * g + 6] for g in range(n)])
    want_c = np.stack([full[6 * a:6 * a + 6, 6 * b:6 * b + 6] for a, b in pairs])
    err = np.sqrt(np.linalg.norm(diag - want_d) ** 2 + np.linalg.norm(cross - want_c) ** 2) / np.linalg.norm(Sref)
    perr = np.linalg.norm(cross - want_c) / np.linalg.norm(want_c)
    sign, logdet = np.linalg.slogdet(Hr)
    lerr = abs(res.logdet - logdet) / abs(logdet)
    print("banded chain %d, %d pairs, %r: cond_2 %.3e, error of the blocks over |ref|_F %.3e, pairs alone %.3e (bound %.3e), "
          "logdet rel %.3e, %r" % (n, len(pairs), info, w[-1] / w[0], err, perr, bound, lerr, res))
    assert err <= bound and perr <= bound and lerr <= bound
    assert not cross[:2].any() and cross[2:].any()
    same = pairs[:, 0] == pairs[:, 1]
    for (a, _), Bc in zip(pairs[same], cross[same]):
        assert np.abs(diag[a] - 0.5 * (Bc + Bc.T)).max() == 0.0


def test_degenerate_plans():
    ds = "smallGrid3D"
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    Tc = capi.chordal_init(m, n)
    pairs = all_pairs(n)
    # a block size at or above every interior, and a team in which every pose is public: the call IS method="schur"
    for N, max_block in ((2, 2500), (5, 4)):
        t, _, _ = team_at(ds, N, T=Tc, **RTR_NESTEROV)
        _, info, _ = plan_of(t, m, n, N, max_block)
        assert info["promoted_poses"] == 0
        if N == 5:
            assert info["blocks"] == 0 and info["separator_poses"] == n - 1
        a, da, ca = t.covariances_nested(Tc, pairs, max_block=max_block)
        b, db, cb = t.covariances(Tc, pairs, method="schur")
        assert da.tobytes() == db.tobytes() and ca.tobytes() == cb.tobytes()
        assert (a.n, a.logdet, a.min_pivot, a.max_pivot) == (b.n, b.logdet, b.min_pivot, b.max_pivot)
        t.close()
    # blocks of one pose
    t, _, _ = team_at(ds, 2, T=Tc, **RTR_NESTEROV)
    _, info, _ = plan_of(t, m, n, 2, 1)
    assert info["largest_block"] == 1 and info["promoted_poses"] > 0
    check_against_numpy("%s / 2, chordal T, %r" % (ds, info), t, m, n, Tc, 1)
    t.close()


def test_sphere2500_at_the_optimum_against_the_other_paths():
    """one robot at the default block size against method="dense" on the same team, five robots at max_block = 128 against
    method="schur": all diagonal blocks and about 200 pairs, |a - b|_F / |b|_F <= 2 n eps cond_est"""
    ds, N, at_optimum, kw = OPTIMA[0]
    assert ds == "sphere2500"
    t, m, n = team_at(ds, N, **kw)
    it = converge(t, at_optimum)
    assert it > 0, "the pinned optimum was not reached in %d iterations (cost %.12g)" % (-it, t.cost())
    rd, T = t.round()
    lo, hi = covref.extreme_eigenvalues(covref.reduced(covref.hessian(covref.q_full(m, n), T, n)))
    assert lo > 0
    nn = 6 * (n - 1)
    bound = 2 * nn * EPS * hi / lo
    pairs = pair_cases(m, n, N, 200, seed=7)

    def compare(tag, team, other, max_block):
        _, info = team.covariance_plan(max_block)
        assert info["promoted_poses"] > 0
        rn, dn, cn = team.covariances_nested(T, pairs, max_block=max_block)
        ro, do, co = team.covariances(T, pairs, method=other)
        a, b = np.concatenate([dn.ravel(), cn.ravel()]), np.concatenate([do.ravel(), co.ravel()])
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        perr = np.linalg.norm(cn - co) / np.linalg.norm(co)
        lerr = abs(rn.logdet - ro.logdet) / abs(ro.logdet)
        print("%s, %r: n = %d, cond_est %.3e, |nested - %s|_F / |%s|_F = %.3e (pairs alone %.3e; bound %.3e, ratio %.3e), logdet "
              "%.12g against %.12g (rel %.3e)\n  nested %r\n  %s %r" % (tag, info, nn, hi / lo, other, other, err, perr, bound,
                                                                          err / bound, rn.logdet, ro.logdet, lerr, rn, other, ro))
        assert rn.n == nn == ro.n
        assert err <= bound and perr <= bound and lerr <= bound
        assert cn[2:].any() and not cn[:2].any() and not dn[0].any()
        for g in range(1, n):
            assert dn[g].tobytes() == np.ascontiguousarray(dn[g].T).tobytes()

    compare("%s / %d" % (ds, N), t, "schur", 128)
    t.close()
    one = team_of(m, n, 1, T)
    compare("%s / 1" % ds, one, "dense", None)
    one.close()


def column_block_residual(tag, t, Hr, n, T, p, max_block=None):
    """the pairs (i, p) for all i, stacked into C_p; |H_red C_p - E_p|_F"""
    pairs = np.stack([np.arange(n), np.full(n, p)], axis=1)
    res, diag, cross = t.covariances_nested(T, pairs, max_block=max_block)
    Cp = cross[1:].reshape(6 * (n - 1), 6)
    E = np.zeros_like(Cp)
    E[6 * (p - 1):6 * p] = np.eye(6)
    rr = np.linalg.norm(Hr @ Cp - E)
    assert np.abs(0.5 * (cross[p] + cross[p].T) - diag[p]).max() == 0.0
    print("%s: p = %d, |H_red C_p - E_p|_F = %.3e, %r" % (tag, p, rr, res))
    return rr, res


def test_a_graph_both_other_paths_refuse():
    """one robot, the pose count taken from the device's memory so that three dense matrices of order 6 (N - 1) exceed it: "dense"
    refuses, "schur" (one robot: no separator, the same three matrices) refuses, "nested" answers within its own formula and
    its column blocks pass the residual check for an interior and a promoted pose"""
    free_b, total_b = torch.cuda.mem_get_info()
    n = int(np.ceil(1.05 * np.sqrt(total_b / 24.0) / 6.0)) + 1
    m, T = NR.banded_chain(n, 3, longs=n // 200)
    t = team_of(m, n, 1, T, precond_mode=capi.PRECOND_BLOCK_JACOBI)  # (the solver does not run: no preconditioner to set up)
    rowptr, col = NR.pattern(m, n)
    block_of, info = t.covariance_plan()
    s = NR.sets(block_of, rowptr, col)
    need_dense, need_nested = 3.0 * (6.0 * (n - 1)) ** 2 * 8.0, NR.nested_bytes(s)
    print("%d poses on one robot: %r; dense %.3e bytes, nested %.3e bytes, device %.3e (free %.3e)"
          % (n, info, need_dense, need_nested, total_b, free_b))
    assert need_dense > total_b and need_nested < 0.5 * free_b
    Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
    lo, hi = covref.extreme_eigenvalues(Hr)
    nn = 6 * (n - 1)
    bound = nn * EPS * hi / lo
    print("eigenvalues %.3e .. %.3e, bound %.3e" % (lo, hi, bound))
    assert lo > 0
    assert bound < 1e-2 * np.sqrt(6.0)  # (of the graph: the bound must be one that a wrong block, |E_p|_F = 2.4, cannot meet)
    with pytest.raises(capi.DpgoError) as e:
        t.covariances(T, method="dense")
    assert "%.0f bytes" % need_dense in str(e.value), str(e.value)
    with pytest.raises(capi.DpgoError, match="the Schur path needs"):
        t.covariances(T, method="schur")
    p_int = [g for g in range(n // 2, n) if block_of[g] >= 0][0]
    p_sep = [g for g in range(n // 2, n) if block_of[g] == -1][0]
    for p in (p_int, p_sep):
        rr, res = column_block_residual("banded chain %d / 1 (%s)" % (n, "interior" if p == p_int else "promoted"), t, Hr, n, T, p)
        assert res.n == nn and res.min_pivot > 0 and rr <= bound, (rr, bound)
    t.close()


def raw_call(t, T, pairs, diag, cross, res, max_block):
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return capi.lib().dpgo_team_marginal_covariances_nested(t.h, capi._d(np.ascontiguousarray(T)), int(max_block), len(pr),
                                                            capi._d(pr) if len(pr) else None, capi._d(diag),
                                                            capi._d(cross) if len(pr) else None, C.byref(res))


MARGIN = 1e-6  # (of first_failing_factor: every pivot up to the failing one this far from 0, against a round-off of 1e-13)


def refused_pivot(t, T, pairs, max_block, n):
    """the raw call on outputs filled with 7.25: refused, outputs untouched; returns the message"""
    diag, cross, res = np.full((n, 6, 6), 7.25), np.full((len(pairs), 6, 6), 7.25), capi.Covariance()
    res.n = 5
    assert raw_call(t, T, pairs, diag, cross, res, max_block) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    print(msg)
    assert "not positive definite at this T: not a minimum" in msg, msg
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    return msg


def pivot_message(f, robot):
    """what the call says of the factor f (covnested_ref.first_failing_factor)"""
    where = "block %d of robot %d" % (f["block"], robot) if f["kind"] == "block" else "the Schur complement on the separator"
    return "non-positive pivot at row %d of %s (pose %d)" % (f["row"], where, f["pose"])


def test_refusals_leave_the_outputs_untouched():
    ds, N, max_block = "smallGrid3D", 2, 16
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    Q = covref.q_full(m, n)
    rowptr, col = NR.pattern(m, n)
    robot_of = NR.robots_of(n, N)
    s = NR.sets(capi.covariance_nested_plan(robot_of, rowptr, col, max_block)[0], rowptr, col)
    Tc = capi.chordal_init(m, n)
    assert NR.first_failing_factor(covref.reduced(covref.hessian(Q, Tc, n)).toarray(), s) is None
    # a random trajectory is not a minimum.  The seed is picked on the CPU so that the reference H_red has an eigenvalue below
    # -1e-6 of the largest and the elimination, factor by factor in the order of the call, meets its first non-positive
    # pivot in a BLOCK, every pivot up to it MARGIN away from 0: the message must name that block, its robot and that pose
    for seed in range(20):
        T = random_manifold_point(np.random.default_rng(100 + seed), 3, n)
        R = covref.rotations(T, n)
        if (np.linalg.det(R) < 0).any():  # (the Stiefel projection gives O(3): flip the reflected ones)
            P = T.reshape(n, 4, 3).copy()
            P[np.linalg.det(R) < 0, 2, :] *= -1.0
            T = P.reshape(-1)
        Hr = covref.reduced(covref.hessian(Q, T, n)).toarray()
        w = np.linalg.eigvalsh(Hr)
        fb = NR.first_failing_factor(Hr, s)
        if w[0] < -1e-6 * w[-1] and fb["kind"] == "block" and fb["margin"] > MARGIN:
            break
    else:
        raise AssertionError("no seed gave an indefinite reference Hessian that fails in a block")
    print("random T (seed %d): eigenvalues %.3e .. %.3e, %r" % (seed, w[0], w[-1], fb))
    # the chordal point with the rotations of a few SEPARATOR poses replaced: again picked on the CPU, so that every block
    # stays positive definite and the first non-positive pivot is one of the Schur complement on the separator
    for sseed in range(20):
        spoiled = np.random.default_rng(sseed).choice(s["separator"], 2, replace=False)
        Ts = NR.spoil_rotations(Tc, n, spoiled, 50 + sseed)
        fs = NR.first_failing_factor(covref.reduced(covref.hessian(Q, Ts, n)).toarray(), s)
        if fs is not None and fs["kind"] == "separator" and fs["margin"] > MARGIN:
            break
    else:
        raise AssertionError("no seed gave a Hessian that fails on the separator alone")
    print("chordal T, poses %s spoiled (seed %d): %r" % (sorted(spoiled), sseed, fs))
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    block_of, info, s_team = plan_of(t, m, n, N, max_block)
    assert info["promoted_poses"] > 0 and s_team == s
    pairs = np.array([[1, 2], [5, 100]])
    msg = refused_pivot(t, T, pairs, max_block, n)
    assert block_of[fb["pose"]] == fb["block"] and pivot_message(fb, robot_of[fb["pose"]]) in msg, (msg, fb)
    msg = refused_pivot(t, Ts, pairs, max_block, n)
    assert block_of[fs["pose"]] == -1 and pivot_message(fs, -1) in msg, (msg, fs)
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.covariances_nested(T, max_block=max_block)
    diag, cross, res = np.full((n, 6, 6), 7.25), np.full((2, 6, 6), 7.25), capi.Covariance()
    # a pair index N
    assert raw_call(t, Tc, np.array([[1, n]]), diag, cross, res, max_block) == capi.ERR
    assert "outside" in capi.lib().dpgo_last_error().decode()
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    # T outside SE(3)
    Tb = Tc.copy()
    Tb[12 * 17] *= 1.001
    assert raw_call(t, Tb, pairs, diag, cross, res, max_block) == capi.ERR
    assert "pose 17 of T is not in SE" in capi.lib().dpgo_last_error().decode()
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    # a graph cut in two by zero weights: every edge between the two robots
    mp = capi.partition(m, n, N)
    for e in mp[mp["r1"] != mp["r2"]]:
        for a in (int(e["r1"]), int(e["r2"])):
            assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
    for a in t.ids:
        t.agents[a].clear_data_matrices()
    res.n = 5
    assert raw_call(t, Tc, pairs, diag, cross, res, max_block) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    assert "is not joined to pose 0 by edges of positive weight" in msg and msg.startswith("marginal_covariances_nested"), msg
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    t.close()
    # an incomplete team
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N))
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.covariances_nested(Tc, max_block=max_block)
    t.close()


def test_a_failing_block_late_in_a_large_batch_is_named():
    """a chain of 1200 poses on one robot at max_block = 3: 388 blocks of at most 3 poses, whose workspaces (at most
    3 x 18^2 + 18 K + K^2 doubles each, K <= 42) are under 2 MB together -- one batch.  The ground truth is a minimum; the
    rotations of ONE block's poses are replaced, which changes H in that block and in its separator poses only, so every
    block before it stays positive definite and the first failing factor is that block.  Its index in the batch is past what
    the batched inverse's return code can hold (128) in the first case and past 256 in the second: the message must still
    name the block, the robot and the pose that the CPU elimination finds"""
    n, max_block = 1200, 3
    m, Tg = NR.banded_chain(n, 7)
    Q = covref.q_full(m, n)
    rowptr, col = NR.pattern(m, n)
    t = team_of(m, n, 1, Tg, precond_mode=capi.PRECOND_BLOCK_JACOBI)  # (the solver does not run)
    block_of, info, s = plan_of(t, m, n, 1, max_block)
    nblk = len(s["blocks"])
    assert nblk > 300
    pairs = np.array([[1, 2]])
    for lo in (128, 256):
        b = [k for k in range(lo + 2, nblk) if len(s["blocks"][k]) >= 2][0]
        T = NR.spoil_rotations(Tg, n, s["blocks"][b], b)
        f = NR.first_failing_factor(covref.reduced(covref.hessian(Q, T, n)).tocsr(), s)
        print("block %d (poses %s) spoiled: %r" % (b, s["blocks"][b], f))
        assert f is not None and f["kind"] == "block" and f["block"] == b and f["margin"] > MARGIN
        msg = refused_pivot(t, T, pairs, max_block, n)
        assert pivot_message(f, 0) in msg, (msg, f)
    # and the team still answers at the minimum
    res, diag, _ = t.covariances_nested(Tg, max_block=max_block)
    assert res.min_pivot > 0 and diag[1:].any()
    t.close()


def test_a_block_size_that_does_not_fit_the_device_is_refused_with_the_figure():
    """blocks of one pose put six tenths of a banded chain into the separator (measured on the CPU: 0.61 at 6 000 and at 36 000
    poses).  The pose count is taken from the device's memory so that three matrices of that order exceed it together with
    everything the library's pool can hold idle (4 GiB), while the default block size asks for less than half of what is free
    (about 1 GB here) -- the criterion of test_a_graph_both_other_paths_refuse"""
    free_b, total_b = torch.cuda.mem_get_info()
    n = int(np.ceil(1.1 * np.sqrt((total_b + (4 << 30)) / 24.0) / (6 * 0.6)))
    m, T = NR.banded_chain(n, 5)
    t = team_of(m, n, 1, T, precond_mode=capi.PRECOND_BLOCK_JACOBI)  # (the solver does not run: no preconditioner to set up)
    rowptr, col = NR.pattern(m, n)
    block_of, info = t.covariance_plan(1)
    need = NR.nested_bytes(NR.sets(block_of, rowptr, col))
    block_of, dinfo = t.covariance_plan()
    need_default = NR.nested_bytes(NR.sets(block_of, rowptr, col))
    print("%d poses, max_block 1: %r, %.0f bytes; default: %r, %.0f bytes; device %.0f" % (n, info, need, dinfo, need_default, total_b))
    assert need > total_b + (4 << 30) and need_default < 0.5 * free_b
    pairs = np.array([[1, 2]])
    diag, cross, res = np.full((n, 6, 6), 7.25), np.full((1, 6, 6), 7.25), capi.Covariance()
    res.n = 5
    assert raw_call(t, T, pairs, diag, cross, res, 1) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    print(msg)
    assert "needs %.0f bytes for its large buffers" % need in msg and "set by the separator of %d poses" % info["separator_poses"] in msg
    assert "another max_block changes the figure" in msg and "are available on the device" in msg
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    t.close()


def test_two_calls_give_the_same_bits_and_the_solver_is_untouched():
    """100 iterations of the bench configuration, two calls, 200 more iterations: X, Y and V bitwise those of the run
    without the calls"""
    outs = []
    for with_call in (False, True):
        t, m, n = team_at("sphere2500", 5, **BENCH)
        t.run(100)
        if with_call:
            pairs = pair_cases(m, n, 5, 60, seed=1)
            T = capi.chordal_init(m, n)
            assert t.covariance_plan(128)[1]["promoted_poses"] > 0
            a1, d1, c1 = t.covariances_nested(T, pairs, max_block=128)
            a2, d2, c2 = t.covariances_nested(T, pairs, max_block=128)
            assert d1.tobytes() == d2.tobytes() and c1.tobytes() == c2.tobytes()
            assert (a1.logdet, a1.min_pivot, a1.max_pivot, a1.n) == (a2.logdet, a2.min_pivot, a2.max_pivot, a2.n)
            print("sphere2500 / 5 at the chordal T: %r" % a1)
        t.run(200)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_current_weights_are_honoured():
    ds, N, max_block = "smallGrid3D", 2, 16
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    t.run(300)
    _, T = t.round()
    _, d_before, _ = t.covariances_nested(T, max_block=max_block)
    lc = [k for k in range(len(mp)) if not (mp["r1"][k] == mp["r2"][k] and mp["p1"][k] + 1 == mp["p2"][k])]
    e = mp[lc[len(lc) // 2]]
    for a in {int(e["r1"]), int(e["r2"])}:
        assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
        t.agents[a].clear_data_matrices()
    mw, nw = gather(t)
    assert nw == n and len(mw) == len(m) and (mw["weight"] == 0).sum() == 1
    plan_of(t, m, n, N, max_block)  # (an edge of weight 0 counts: the sets do not move)
    check_against_numpy("%s / %d, one loop closure at weight 0" % (ds, N), t, mw, n, T, max_block)
    _, d_after, _ = t.covariances_nested(T, max_block=max_block)
    assert np.abs(d_after - d_before).max() > 1e-9 * np.abs(d_before).max()  # (the weight matters)
    t.close()


def test_weights_after_an_update_round_are_honoured():
    ds, N, max_block = "smallGrid3D", 2, 16
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mo = add_outliers(m.view(O.MEAS_DTYPE), n, frac=0.1, seed=0).view(capi.MEAS_DTYPE)
    mp = capi.partition(mo, n, N)
    kw = dict(RTR_NESTEROV, robust_cost_type=capi.COST_GNC_TLS, gnc_barc=3.0, gnc_mu_step=2.0, gnc_init_mu=1e-2)
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **kw))
    t.set_initial(capi.chordal_init(m, n), capi.fixed_stiefel(5))
    t.run(100)
    t.update_weights()
    t.run(300)
    mw, nw = gather(t)
    w = mw["weight"]
    print("after one update round: %d of %d weights changed, range %.3g .. %.3g" % ((w != 1.0).sum(), len(w), w.min(), w.max()))
    assert nw == n and (w != 1.0).any()
    _, T = t.round()
    assert t.covariance_plan(max_block)[1]["promoted_poses"] > 0
    check_against_numpy("%s / %d + 10 %% outliers, one update round" % (ds, N), t, mw, n, T, max_block)
    t.close()


def test_solve_certified_returns_the_covariances_on_request():
    ds, N, max_block = "smallGrid3D", 2, 16
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    prm = capi.default_params(r=5, num_robots=N, **RTR_NESTEROV)
    Tc = capi.chordal_init(m, n)
    out = capi.solve_certified(mp, prm, r0=5, T=Tc, iters=300, covariances=True, covariance_method="nested",
                               covariance_max_block=max_block)
    res, diag = out["covariances"]
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    res2, diag2, _ = t.covariances_nested(out["T"], max_block=max_block)
    res3, diag3, _ = t.covariances(out["T"], method="schur")
    t.close()
    assert diag.shape == (n, 6, 6) and diag.tobytes() == diag2.tobytes() and res.logdet == res2.logdet
    assert diag.tobytes() != diag3.tobytes()  # (the block size was passed on: another elimination order, other round-off)

"""GPU checks of the marginal covariances by robot-wise Schur complement (csrc/covariance_schur.hip,
Team.covariances(method="schur")).

Bounds, as in tests/test_gpu_covariance.py: an inverse through Cholesky has the forward error n eps cond_2(H_red)
(n = 6 (N - 1), eps = 2.2e-16).  Against the numpy inverse the Schur path is held to that bound; against the dense path
of the library to twice it, because both lie within it of the truth; a column block C_p to |H_red C_p - E_p|_F <= n eps
cond_est against scipy's sparse Hessian.  Nothing in them is tuned; the measured ratios are in
profiles/r11_covariance_schur.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests import covref, covschur_ref
from tests.test_certificate import random_manifold_point
from tests.test_gpu_certificate import OPTIMA, RTR_NESTEROV, converge, team_at
from tests.test_gpu_covariance import BENCH, all_pairs, gather
from tests.util import DATA, add_outliers

pytestmark = pytest.mark.gpu

EPS = covref.EPS


def check_against_dense(tag, t, m, n, T):
    """the criterion of tests/test_gpu_covariance.py::check_against_dense for method="schur": every diagonal block and all
    N^2 pairs against the numpy inverse"""
    Q = covref.q_full(m, n)
    Hr, Sref, w = covref.dense_reference(Q, T, n)
    assert w[0] > 0, "%s: the reference H_red is not positive definite (%.3e)" % (tag, w[0])
    cond, nn = w[-1] / w[0], 6 * (n - 1)
    bound = nn * EPS * cond
    pairs = all_pairs(n)
    res, diag, cross = t.covariances(T, pairs, method="schur")
    S = covref.full_sigma(diag, cross, pairs, n)
    err = np.linalg.norm(S - Sref) / np.linalg.norm(Sref)
    # the diagonal blocks as returned (symmetrised) and as cross blocks (a, a) (not symmetrised) agree to round-off
    for g in range(n):
        Bc = cross[g * n + g]
        assert np.abs(diag[g] - 0.5 * (Bc + Bc.T)).max() == 0.0
    sign, logdet = np.linalg.slogdet(Hr)
    lerr = abs(res.logdet - logdet) / abs(logdet)
    print("%s: n = %d, cond_2 = %.3e, |Sigma - ref|_F / |ref|_F = %.3e (bound %.3e, ratio %.3e), logdet %.12g (rel %.3e), %r"
          % (tag, nn, cond, err, bound, err / bound, res.logdet, lerr, res))
    assert res.n == nn
    assert err <= bound
    assert sign > 0 and lerr <= bound
    assert res.min_pivot > 0 and res.max_pivot >= res.min_pivot
    # pose 0: exactly zero, alone and in every pair
    assert not diag[0].any()
    zero = (pairs[:, 0] == 0) | (pairs[:, 1] == 0)
    assert not cross[zero].any() and cross[~zero].any()
    for g in range(1, n):
        assert diag[g].tobytes() == np.ascontiguousarray(diag[g].T).tobytes()
        assert np.linalg.eigvalsh(diag[g])[0] > 0
    return res


@pytest.mark.parametrize("ds,N", [("tinyGrid3D", 1), ("tinyGrid3D", 2), ("smallGrid3D", 2), ("smallGrid3D", 3), ("smallGrid3D", 5)])
def test_blocks_match_dense_inverse(ds, N):
    """tinyGrid3D / 1 has no separator, smallGrid3D / 5 no interior pose: both ends of the path"""
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    Tc = capi.chordal_init(m, n)
    t, _, _ = team_at(ds, N, T=Tc, **RTR_NESTEROV)
    check_against_dense("%s / %d, chordal T" % (ds, N), t, m, n, Tc)
    t.run(300)
    rd, T = t.round()
    check_against_dense("%s / %d, rounded T (f %.9g)" % (ds, N, rd.f_rounded), t, m, n, T)
    # T = None rounds the current iterate first
    a, d0, _ = t.covariances(method="schur")
    b, d1, _ = t.covariances(T, method="schur")
    assert d0.tobytes() == d1.tobytes() and a.logdet == b.logdet
    t.close()


def pair_cases(m, n, N, count, seed):
    """about `count` seeded pairs that cover every case: interior-interior of one robot and of two, interior-public both
    ways round, public-public, the same pose twice, a pair that names pose 0"""
    mp = capi.partition(m, n, N)
    robot_of, public = covschur_ref.partition(mp, n, N)
    rng = np.random.default_rng(seed)
    interior = [g for g in range(1, n) if not public[g]]
    pub = [g for g in range(1, n) if public[g]]
    out = [(0, interior[0]), (pub[0], 0), (interior[3], interior[3]), (pub[1], pub[1])]
    per = (count - len(out)) // 5
    by_robot = [[g for g in interior if robot_of[g] == a] for a in range(N)]
    have = [a for a in range(N) if by_robot[a]]  # (smallGrid3D / 3: every pose of robot 1 is public)
    for _ in range(per):
        a, b = rng.choice(have, 2, replace=False)
        out.append(tuple(rng.choice(by_robot[a], 2)))                          # one robot
        out.append((rng.choice(by_robot[a]), rng.choice(by_robot[b])))          # two robots
        out.append((rng.choice(interior), rng.choice(pub)))
        out.append((rng.choice(pub), rng.choice(interior)))
        out.append(tuple(rng.choice(pub, 2)))
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("k", [0, 1], ids=["sphere2500", "torus3D"])
def test_schur_matches_the_dense_path_at_scale(k):
    """all diagonal blocks and about 200 pairs at the rounded optimum: |Sigma_schur - Sigma_dense|_F / |Sigma_dense|_F <= 2 n
    eps cond_est (cond_est as tests/test_gpu_covariance.py::at_scale takes it)"""
    ds, N, at_optimum, kw = OPTIMA[k]
    t, m, n = team_at(ds, N, **kw)
    it = converge(t, at_optimum)
    assert it > 0, "the pinned optimum was not reached in %d iterations (cost %.12g)" % (-it, t.cost())
    rd, T = t.round()
    Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
    lo, hi = covref.extreme_eigenvalues(Hr)
    assert lo > 0
    nn = 6 * (n - 1)
    bound = 2 * nn * EPS * hi / lo
    pairs = pair_cases(m, n, N, 200, seed=7)
    rs, ds_, cs = t.covariances(T, pairs, method="schur")
    rd_, dd, cd = t.covariances(T, pairs, method="dense")
    a, b = np.concatenate([ds_.ravel(), cs.ravel()]), np.concatenate([dd.ravel(), cd.ravel()])
    err = np.linalg.norm(a - b) / np.linalg.norm(b)
    perr = np.linalg.norm(cs - cd) / np.linalg.norm(cd)
    lerr = abs(rs.logdet - rd_.logdet) / abs(rd_.logdet)
    print("%s / %d: n = %d, cond_est %.3e, |schur - dense|_F / |dense|_F = %.3e (pairs alone %.3e; bound %.3e, ratio %.3e), "
          "logdet %.12g against %.12g (rel %.3e)\n  schur %r\n  dense %r" % (ds, N, nn, hi / lo, err, perr, bound, err / bound,
                                                                             rs.logdet, rd_.logdet, lerr, rs, rd_))
    assert rs.n == nn == rd_.n
    assert err <= bound and perr <= bound and lerr <= bound
    assert cs[2:].any() and not cs[:2].any() and not ds_[0].any()
    for g in range(1, n):
        assert ds_[g].tobytes() == np.ascontiguousarray(ds_[g].T).tobytes()
    t.close()


def column_block_residual(tag, t, Hr, n, T, p):
    """the pairs (i, p) for all i, stacked into C_p; |H_red C_p - E_p|_F"""
    pairs = np.stack([np.arange(n), np.full(n, p)], axis=1)
    res, diag, cross = t.covariances(T, pairs, method="schur")
    Cp = cross[1:].reshape(6 * (n - 1), 6)
    E = np.zeros_like(Cp)
    E[6 * (p - 1):6 * p] = np.eye(6)
    rr = np.linalg.norm(Hr @ Cp - E)
    assert np.abs(0.5 * (cross[p] + cross[p].T) - diag[p]).max() == 0.0
    print("%s: p = %d, |H_red C_p - E_p|_F = %.3e, %r" % (tag, p, rr, res))
    return rr, res


def test_cubicle_column_blocks_without_the_dense_path():
    """one interior and one public pose of cubicle / 4 (2044 public poses, the largest interior 1109)"""
    ds, N, at_optimum, kw = OPTIMA[2]
    assert ds == "cubicle"
    t, m, n = team_at(ds, N, **kw)
    it = converge(t, at_optimum)
    assert it > 0, "the pinned optimum was not reached in %d iterations (cost %.12g)" % (-it, t.cost())
    rd, T = t.round()
    Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
    lo, hi = covref.extreme_eigenvalues(Hr)
    nn = 6 * (n - 1)
    bound = nn * EPS * hi / lo
    print("%s / %d: n = %d, eigenvalues %.3e .. %.3e, bound %.3e" % (ds, N, nn, lo, hi, bound))
    assert lo > 0
    _, public = covschur_ref.partition(capi.partition(m, n, N), n, N)
    p_int = [g for g in range(n // 2, n) if not public[g]][0]
    p_pub = [g for g in range(n // 2, n) if public[g]][0]
    for p in (p_int, p_pub):
        rr, res = column_block_residual("%s / %d (%s)" % (ds, N, "interior" if p == p_int else "public"), t, Hr, n, T, p)
        assert res.n == nn and rr <= bound, (rr, bound)
    t.close()


def loop_chain(n, N, seed, between=True):
    """a noise-free pose graph of n poses split among N robots by the contiguous rule: the odometry chain i -> i + 1, seeded
    loop closures inside the robots (one for every 4 poses, random ends) and, with `between`, between them (one for every 60
    poses, random ends).  Rotations and positions are drawn at random (positions in a box of side 10), so the graph is compact
    and well joined and H_red at the ground truth is well conditioned for its size.  Returns (measurements in single-robot
    numbering, ground-truth trajectory in the layout of chordal_init)"""
    rng = np.random.default_rng(seed)

    def rot(w):
        th = np.linalg.norm(w, axis=-1, keepdims=True)
        k = w / np.maximum(th, 1e-12)
        K = np.zeros(w.shape[:-1] + (3, 3))
        K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
        K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
        s, c = np.sin(th)[..., None], (1 - np.cos(th))[..., None]
        return np.eye(3) + s * K + c * (K @ K)

    Rg = rot(rng.standard_normal((n, 3)))
    tg = rng.uniform(-5.0, 5.0, (n, 3))
    Rg[0], tg[0] = np.eye(3), 0.0
    per = n // N
    robot = np.minimum(np.arange(n) // per, N - 1)
    a = rng.integers(0, n, n // 4)
    b = np.minimum(per * robot[a] + rng.integers(0, per, n // 4), n - 1)
    keep = (robot[a] == robot[b]) & (a != b)
    src = np.r_[np.arange(n - 1), np.minimum(a[keep], b[keep])]
    dst = np.r_[np.arange(1, n), np.maximum(a[keep], b[keep])]
    if between:
        a, b = rng.integers(0, n, 4 * (n // 60)), rng.integers(0, n, 4 * (n // 60))
        keep = np.flatnonzero(robot[a] != robot[b])[:n // 60]
        src, dst = np.r_[src, np.minimum(a[keep], b[keep])], np.r_[dst, np.maximum(a[keep], b[keep])]
    m = np.zeros(len(src), dtype=capi.MEAS_DTYPE)
    m["p1"], m["p2"] = src, dst
    m["R"] = np.einsum("eji,ejk->eik", Rg[src], Rg[dst]).reshape(len(src), 9)
    m["t"] = np.einsum("eji,ej->ei", Rg[src], tg[dst] - tg[src])
    m["kappa"], m["tau"], m["weight"] = 100.0, 50.0, 1.0
    T = np.zeros((n, 4, 3))
    T[:, :3, :] = Rg.transpose(0, 2, 1)
    T[:, 3, :] = tg
    return m, T.reshape(-1)


def test_a_chain_split_among_robots_with_all_pairs():
    """no loop closure between the robots: only the poses at the cuts are public (at most 2 per robot), the ideal case of the
    path.  All 360^2 pairs, 86 400 of them between interiors of two robots -- more than one launch can index"""
    n, N = 360, 3
    m, T = loop_chain(n, N, seed=5, between=False)
    mp = capi.partition(m, n, N)
    robot_of, public = covschur_ref.partition(mp, n, N)
    info = covschur_ref.sets(robot_of, public)
    assert info["s"] == [1, 2, 1] and sum(len(i) for i in info["interior"]) == n - 5
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **RTR_NESTEROV))
    t.set_initial(T, capi.fixed_stiefel(5))
    check_against_dense("chain %d / %d, all pairs" % (n, N), t, m, n, T)
    t.close()


def test_a_robot_without_interior_between_two_with_one():
    """a chain of 9 poses on robots of 4, 2 and 3 poses: both poses of the middle robot are public (the cuts), so its set has
    an empty interior and two separator poses, next to two robots with interiors.  All 81 pairs against the dense path of
    the same team under n eps cond_2 (cond_2 of the reference H_red; in the Frobenius norm over all blocks and in the 2-norm
    block by block), the diagonal blocks bitwise the symmetrised pairs
    (g, g), and the same call over one participant per robot bitwise the single team's"""
    from tests.test_gpu_covariance_across import Split, bits, scalars
    n, N, sizes = 9, 3, [4, 2, 3]
    m, T = loop_chain(n, N, seed=5, between=False)
    first = np.concatenate([[0], np.cumsum(sizes)])
    robot_of = np.repeat(np.arange(N), sizes)
    mp = m.copy()
    for a, b in (("r1", "p1"), ("r2", "p2")):
        mp[a], mp[b] = robot_of[m[b]], m[b] - first[robot_of[m[b]]]
    public = np.zeros(n, dtype=bool)
    cross = mp["r1"] != mp["r2"]
    public[m["p1"][cross]] = public[m["p2"][cross]] = True
    public[0] = False
    info = covschur_ref.sets(robot_of, public)
    assert info["s"][1] == 2 and not info["interior"][1] and info["interior"][0] and info["interior"][2], info
    Hr, _, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    nn = 6 * (n - 1)
    bound = nn * EPS * w[-1] / w[0]
    pairs = all_pairs(n)
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **RTR_NESTEROV))
    t.set_initial(T, capi.fixed_stiefel(5))
    X = t.global_X()
    rs, ds_, cs = t.covariances(T, pairs, method="schur")
    rd, dd, cd = t.covariances(T, pairs, method="dense")
    t.close()
    derr = np.linalg.norm(ds_ - dd) / np.linalg.norm(dd)
    perr = np.linalg.norm(cs - cd) / np.linalg.norm(cd)
    lerr = abs(rs.logdet - rd.logdet) / abs(rd.logdet)
    print("chain %d on robots of %r: sets %r, cond_2 %.3e, |schur - dense|_F / |dense|_F: diagonal %.3e, pairs %.3e, logdet rel %.3e "
          "(bound %.3e)" % (n, sizes, info["s"], w[-1] / w[0], derr, perr, lerr, bound))
    assert rs.n == nn == rd.n
    assert derr <= bound and perr <= bound and lerr <= bound
    # block by block, so that an error confined to one block is not diluted: a block of a matrix has at most the matrix's
    # 2-norm, and |Sigma|_2 = 1 / lambda_min(H_red)
    worst = max(np.linalg.norm(a - b, 2) for a, b in zip(np.concatenate([ds_, cs]), np.concatenate([dd, cd])))
    print("largest |block_schur - block_dense|_2 = %.3e (bound %.3e)" % (worst, bound / w[0]))
    assert worst <= bound / w[0]
    zero = (pairs[:, 0] == 0) | (pairs[:, 1] == 0)
    assert not ds_[0].any() and not cs[zero].any() and cs[~zero].any()
    for g in range(n):
        Bc = cs[g * n + g]
        assert ds_[g].tobytes() == (0.5 * (Bc + Bc.T)).tobytes()
    sp = Split(mp, N, [[0], [1], [2]], X, **RTR_NESTEROV)
    out = sp.run(lambda tm, tr: tm.covariances(T[sp.cols(sp.teams.index(tm), 12)], pairs, transport=tr, owner_of_robot=sp.owner))
    for q, (r, d, c) in enumerate(out):
        assert scalars(r) == scalars(rs), (q, r, rs)
        assert bits(c) == bits(cs), q
        assert bits(d) == bits(ds_.reshape(-1)[sp.cols(q, 36)]), q
    sp.close()


def test_a_graph_the_dense_path_refuses():
    """8 robots, the pose count taken from the device's memory so that the three dense matrices exceed it while the Schur
    path's own formula fits: "dense" refuses with the bytes and the pointer to "schur", "schur" answers and its column blocks
    pass the residual check for an interior and a public pose"""
    N = 8
    free_b, total_b = torch.cuda.mem_get_info()
    # 3 (6 (n - 1))^2 8 > total, with a twentieth to spare
    n = int(np.ceil(1.05 * np.sqrt(total_b / 24.0) / 6.0)) + 1
    n += (-n) % N
    m, T = loop_chain(n, N, seed=3)
    mp = capi.partition(m, n, N)
    robot_of, public = covschur_ref.partition(mp, n, N)
    info = covschur_ref.sets(robot_of, public)
    need_dense, need_schur = 3.0 * (6.0 * (n - 1)) ** 2 * 8.0, covschur_ref.schur_bytes(info)
    print("%d poses on %d robots: %d public poses, largest interior %d; dense %.3e bytes, Schur %.3e bytes, device %.3e (free %.3e)"
          % (n, N, len(info["separator"]), info["largest_interior"], need_dense, need_schur, total_b, free_b))
    assert need_dense > total_b and need_schur < 0.5 * free_b  # (the large buffers; the small ones are 0.2 GB here)
    assert len(info["separator"]) > 100 and min(len(i) for i in info["interior"]) > 100
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N, **RTR_NESTEROV))
    t.set_initial(T, capi.fixed_stiefel(5))
    with pytest.raises(capi.DpgoError) as e:
        t.covariances(T, method="dense")
    msg = str(e.value)
    assert "%.0f bytes" % need_dense in msg and 'method="schur"' in msg and "are available on the device" in msg, msg
    Hr = covref.reduced(covref.hessian(covref.q_full(m, n), T, n))
    lo, hi = covref.extreme_eigenvalues(Hr)
    nn = 6 * (n - 1)
    bound = nn * EPS * hi / lo
    print("eigenvalues %.3e .. %.3e, bound %.3e" % (lo, hi, bound))
    assert lo > 0
    assert bound < 1e-2 * np.sqrt(6.0)  # (of the graph: the bound must be one that a wrong block, |E_p|_F = 2.4, cannot meet)
    p_int = [g for g in range(n // 2, n) if not public[g]][0]
    p_pub = [g for g in range(n // 2, n) if public[g]][0]
    for p in (p_int, p_pub):
        rr, res = column_block_residual("loop chain %d / %d (%s)" % (n, N, "interior" if p == p_int else "public"), t, Hr, n, T, p)
        assert res.n == nn and res.min_pivot > 0 and rr <= bound, (rr, bound)
    t.close()


def test_current_weights_are_honoured():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    t.run(300)
    _, T = t.round()
    _, d_before, _ = t.covariances(T, method="schur")
    lc = [k for k in range(len(mp)) if not (mp["r1"][k] == mp["r2"][k] and mp["p1"][k] + 1 == mp["p2"][k])]
    e = mp[lc[len(lc) // 2]]
    for a in {int(e["r1"]), int(e["r2"])}:
        assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
        t.agents[a].clear_data_matrices()
    mw, nw = gather(t)
    assert nw == n and len(mw) == len(m) and (mw["weight"] == 0).sum() == 1
    check_against_dense("%s / %d, one loop closure at weight 0" % (ds, N), t, mw, n, T)
    _, d_after, _ = t.covariances(T, method="schur")
    assert np.abs(d_after - d_before).max() > 1e-9 * np.abs(d_before).max()  # (the weight matters)
    t.close()


def test_weights_after_an_update_round_are_honoured():
    ds, N = "smallGrid3D", 2
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
    check_against_dense("%s / %d + 10 %% outliers, one update round" % (ds, N), t, mw, n, T)
    t.close()


def raw_call(t, T, pairs, diag, cross, res, flags=capi.COV_SCHUR):
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return capi.lib().dpgo_team_marginal_covariances(t.h, capi._d(np.ascontiguousarray(T)), flags, len(pr),
                                                     capi._d(pr) if len(pr) else None, capi._d(diag),
                                                     capi._d(cross) if len(pr) else None, C.byref(res))


def test_refusals_leave_the_outputs_untouched():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    Q = covref.q_full(m, n)
    robot_of, public = covschur_ref.partition(mp, n, N)
    # a random trajectory is not a minimum: the seed is picked on the CPU so that the reference H_red has an eigenvalue
    # below -1e-6 of the largest, far beyond the factorisation's own error
    for seed in range(20):
        T = random_manifold_point(np.random.default_rng(100 + seed), 3, n)
        R = covref.rotations(T, n)
        if (np.linalg.det(R) < 0).any():  # (the Stiefel projection gives O(3): flip the reflected ones)
            P = T.reshape(n, 4, 3).copy()
            P[np.linalg.det(R) < 0, 2, :] *= -1.0
            T = P.reshape(-1)
        w = np.linalg.eigvalsh(covref.reduced(covref.hessian(Q, T, n)).toarray())
        if w[0] < -1e-6 * w[-1]:
            break
    else:
        raise AssertionError("no seed gave an indefinite reference Hessian")
    print("random T (seed %d): eigenvalues %.3e .. %.3e" % (seed, w[0], w[-1]))
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    pairs = np.array([[1, 2], [5, 100]])
    diag, cross, res = np.full((n, 6, 6), 7.25), np.full((2, 6, 6), 7.25), capi.Covariance()
    assert raw_call(t, T, pairs, diag, cross, res) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    print(msg)
    assert "not positive definite at this T: not a minimum" in msg and "pivot" in msg, msg
    # the message names the factor (a robot's interior block or the separator) and the pose, which lies in that set
    import re
    mm = re.search(r"of (the interior Hessian of robot (\d+)|the Schur complement on the public poses) \(pose (\d+)\)", msg)
    assert mm, msg
    pose = int(mm.group(3))
    assert 1 <= pose < n
    if mm.group(2) is not None:
        assert not public[pose] and robot_of[pose] == int(mm.group(2))
    else:
        assert public[pose]
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    with pytest.raises(capi.DpgoError, match="not a minimum"):
        t.covariances(T, method="schur")
    # a pair index N
    Tc = capi.chordal_init(m, n)
    assert raw_call(t, Tc, np.array([[1, n]]), diag, cross, res) == capi.ERR
    assert "outside" in capi.lib().dpgo_last_error().decode()
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    # a flag the call does not know
    for flags in (2, 3, -1):
        assert raw_call(t, Tc, pairs, diag, cross, res, flags=flags) == capi.ERR
        assert "flags must be 0 or DPGO_COV_SCHUR" in capi.lib().dpgo_last_error().decode()
        assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    # T outside SE(3)
    Tb = Tc.copy()
    Tb[12 * 17] *= 1.001
    with pytest.raises(capi.DpgoError, match="pose 17 of T is not in SE"):
        t.covariances(Tb, method="schur")
    # a graph cut in two by zero weights: every edge between the two robots
    for e in mp[mp["r1"] != mp["r2"]]:
        for a in (int(e["r1"]), int(e["r2"])):
            assert t.agents[a].set_measurement_weight(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]), 0.0)
    for a in t.ids:
        t.agents[a].clear_data_matrices()
    res.n = 5
    assert raw_call(t, Tc, pairs, diag, cross, res) == capi.ERR
    msg = capi.lib().dpgo_last_error().decode()
    assert "is not joined to pose 0 by edges of positive weight" in msg and msg.startswith("marginal_covariances"), msg
    assert (diag == 7.25).all() and (cross == 7.25).all() and bytes(res) == bytes(capi.Covariance())
    t.close()
    t = capi.Team.from_measurements(mp, capi.default_params(r=5, num_robots=N))
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.covariances(Tc, method="schur")
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
            a1, d1, c1 = t.covariances(T, pairs, method="schur")
            a2, d2, c2 = t.covariances(T, pairs, method="schur")
            assert d1.tobytes() == d2.tobytes() and c1.tobytes() == c2.tobytes()
            assert (a1.logdet, a1.min_pivot, a1.max_pivot, a1.n) == (a2.logdet, a2.min_pivot, a2.max_pivot, a2.n)
            print("sphere2500 / 5 at the chordal T: %r" % a1)
        t.run(200)
        outs.append([np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)])
        t.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_solve_certified_returns_the_covariances_on_request():
    ds, N = "smallGrid3D", 2
    m, n = capi.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mp = capi.partition(m, n, N)
    prm = capi.default_params(r=5, num_robots=N, **RTR_NESTEROV)
    Tc = capi.chordal_init(m, n)
    out = capi.solve_certified(mp, prm, r0=5, T=Tc, iters=300, covariances=True, covariance_method="schur")
    res, diag = out["covariances"]
    t, _, _ = team_at(ds, N, **RTR_NESTEROV)
    res2, diag2, _ = t.covariances(out["T"], method="schur")
    t.close()
    assert diag.shape == (n, 6, 6) and diag.tobytes() == diag2.tobytes() and res.logdet == res2.logdet

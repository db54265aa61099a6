"""GPU checks of the certificate eigensolver (csrc/certify.hip) at every rank, block and team edge, against the long-double
reference and the contract of tests/certref.py (check_certificate): small seeded teams sized for the tiles of
k_cert_apply, k_cert_lambda, k_cert_gram and k_cert_precond, rank-deficient iterates, weights, the -eta decision on both
sides of the truth, the iteration cap, teams of one to three poses, a split across teams and determinism.  The spectral
gaps the iteration caps are derived from are asserted on the CPU (tests/test_certref.py)."""
import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import certref as CR
from tests.test_gpu_certify_across import Split, assemble, bits

pytestmark = pytest.mark.gpu

TOL = CR.TOL
CAP = CR.iteration_cap(CR.GAP_FLOOR)  # 753
TRUTH_CAP = CR.iteration_cap(CR.TRUTH_GAP_FLOOR)  # 2913
FAR = dict(eta=1e300, eta_relative=False)  # eta out of reach: the solver runs to convergence
_TEAMS = {}
RATIOS = {}  # family -> the largest error / bound ratio of each checked quantity (printed; DESIGN.md 5b records them)


def teardown_module(module):
    for t in _TEAMS.values():
        t.close()
    _TEAMS.clear()
    for fam, d in sorted(RATIOS.items()):
        print("largest error / bound, %s: %s" % (fam, ", ".join("%s %.3g" % kv for kv in sorted(d.items()))))


def make_team(mp, sizes, r, X=None, mode=capi.PRECOND_AUTO):
    t = capi.Team.from_measurements(mp.view(capi.MEAS_DTYPE), capi.default_params(r=r, num_robots=len(sizes), precond_mode=mode))
    if X is not None:
        off = np.r_[0, np.cumsum(sizes)]
        for a, n in enumerate(sizes):
            assert t.agents[a].n == n
            t.agents[a].set_X(X[4 * r * off[a]:4 * r * off[a + 1]])
    return t


def edge(r, mode=capi.PRECOND_DENSE):
    """the tile-edge team of rank r at its seeded point (kept for the module), and its reference"""
    mp, sizes, X = CR.edge_team(r)
    if (r, mode) not in _TEAMS:
        _TEAMS[r, mode] = make_team(mp, sizes, r, X, mode)
    return _TEAMS[r, mode], CR.reference("edge-r%d" % r, mp, sizes, r, X)


def run(family, t, ref, r, precondition=True, **kw):
    """one call through the contract; returns (Certificate, v)"""
    args = CR.Args(r, **kw)
    c, v = t.certify(precondition=precondition, **args.kw())
    out = CR.check_certificate(ref, args, c, v)
    worst = RATIOS.setdefault(family, {})
    for k, x in out.items():
        worst[k] = max(worst.get(k, 0.0), x)
    return c, v


@pytest.mark.parametrize("block", range(3, 9))
@pytest.mark.parametrize("r", range(3, 9))
def test_every_rank_and_block(r, block):
    """lambda_min(S) and the deflated lambda_min at a seeded random manifold point of the tile-edge team"""
    t, ref = edge(r)
    assert not t.agents[len(ref.sizes) - 1].neighbors() and all(t.agents[a].neighbors() for a in range(len(ref.sizes) - 1))
    for deflate in (False, True):
        c, _ = run("every r and block", t, ref, r, tol=TOL, max_iters=CAP, block=block, deflate=deflate, **FAR)
        print("r %d block %d deflate %d: %r" % (r, block, deflate, c))
        assert c.certified == 1, c


MODES = [("dense", capi.PRECOND_DENSE, True), ("block_jacobi", capi.PRECOND_BLOCK_JACOBI, True),
         ("two_level", capi.PRECOND_TWO_LEVEL, True), ("none", capi.PRECOND_DENSE, False)]


@pytest.mark.parametrize("r", [4, 7])
def test_preconditioner_forms(r):
    """dense inverses, the 4 x 4 diagonal inverses (k_cert_precond's Dinv branch), two-level agents (the preconditioner is
    switched off inside) and no preconditioner: every form meets the contract against the same truth"""
    for name, mode, pc in MODES:
        t, ref = edge(r, mode)
        assert all(t.agents[a].preconditioner() == mode for a in range(len(ref.sizes)))
        for deflate in (False, True):
            c, _ = run("preconditioner forms", t, ref, r, precondition=pc, tol=TOL, max_iters=CAP, deflate=deflate, **FAR)
            print("r %d %s deflate %d: %d iterations, %r" % (r, name, deflate, c.iterations, c))
            assert c.certified == 1, (name, c)


@pytest.mark.parametrize("name,mode", [(m[0], m[1]) for m in MODES[:2]], ids=[m[0] for m in MODES[:2]])
def test_preconditioner_product(name, mode):
    """k_cert_precond<K> itself, K = 3 .. 8, both branches, on the tile-edge team (agents of 1 .. 257 poses: N4 = 4, 256,
    260, 1028 around the 256-lane stride): T V against the long-double (Q_a + shift I)^-1 V, or the inverse of its 4 x 4
    diagonal blocks.  |z - z_ref|_2 <= 4n u kappa_2 |P^-1|_2 |v|_2 per agent, the bound of tests/test_gpu_shapes.py for an
    inverse formed by elimination over 4n unknowns (kappa_2 and |.|_2 of the 4 x 4 blocks for the block form)"""
    r = 5
    t, ref = edge(r, mode)
    mp, sizes, _ = CR.edge_team(r)
    off = np.r_[0, np.cumsum(sizes)]
    rng = np.random.default_rng(60 + mode)
    bj = mode == capi.PRECOND_BLOCK_JACOBI
    worst = 0.0
    for K in range(3, 9):
        V = rng.standard_normal(K * 4 * ref.N)
        out = t.certificate_precondition(V)
        for a, n in enumerate(sizes):
            assert t.agents[a].preconditioner() == mode
            P, D, cond, cond_d = CR.precond_reference("edge-r%d" % r, mp, sizes, a)
            sl = slice(4 * K * off[a], 4 * K * off[a + 1])
            Va = V[sl].reshape(4 * n, K)
            Z = CR.precond_apply(P, D, Va, bj)
            kappa, pinv = cond_d if bj else cond
            err = float(np.linalg.norm(np.asarray(out[sl].reshape(4 * n, K) - Z, dtype=np.float64)))
            bound = 4 * n * CR.U * kappa * pinv * np.linalg.norm(Va)
            worst = max(worst, err / bound)
            assert err <= bound, (name, K, a, n, err, bound)
    RATIOS.setdefault("preconditioner product", {})[name] = worst


def test_preconditioner_forms_at_the_noise_free_optimum():
    """where the Ritz values stay near 0 the preconditioner is applied in every iteration: all forms, deflated"""
    r = 4
    mp, sizes, m, _ = CR.truth_team()
    N = sum(sizes)
    ref = None
    for name, mode, pc in MODES:
        t = make_team(mp, sizes, r, mode=mode)
        t.set_initial(capi.odometry_init(m.view(capi.MEAS_DTYPE), N), capi.fixed_stiefel(r))
        assert all(t.agents[a].preconditioner() == mode for a in range(len(sizes)))
        ref = ref or CR.Reference(mp, sizes, r, t.global_X())
        c, _ = run("preconditioner forms", t, ref, r, precondition=pc, eta=1e-6, tol=TOL, max_iters=TRUTH_CAP)
        print("truth r %d %s: %d iterations, %r" % (r, name, c.iterations, c))
        assert c.certified == 1, (name, c)
        t.close()


@pytest.mark.parametrize("r", [4, 6, 8])
def test_rank_deficient_lifted_ground_truth(r):
    """a noise-free graph at its lifted ground truth: X has rank 3, Z = [X; e_t] rank 4 of r + 1, S is positive
    semidefinite with the null space Z.  Deflated, and undeflated with block 3 below the null space's dimension"""
    mp, sizes, m, _ = CR.truth_team()
    N = sum(sizes)
    t = make_team(mp, sizes, r, mode=capi.PRECOND_DENSE)
    t.set_initial(capi.odometry_init(m.view(capi.MEAS_DTYPE), N), capi.fixed_stiefel(r))
    ref = CR.Reference(mp, sizes, r, t.global_X())
    assert ref.nz == 4 and ref.gap(True) >= CR.TRUTH_GAP_FLOOR and ref.gap(False, 4) >= CR.TRUTH_GAP_FLOOR
    for kw in (dict(deflate=True), dict(deflate=False, block=3)):
        c, _ = run("rank-deficient iterates", t, ref, r, eta=1e-6, tol=TOL, max_iters=TRUTH_CAP, **kw)
        print("truth r %d %s: %r" % (r, kw, c))
        assert c.certified == 1, c
        assert abs(c.lambda_min) <= (TOL + CR.C_PROD * CR.U) * ref.s, c
    t.close()


@pytest.mark.parametrize("r", range(3, 8))
def test_rank_deficient_zero_row(r):
    """[X; 0] from the staircase's escape point at alpha = 0: the zero row is dropped from Z by the reference rule"""
    mp, sizes, X = CR.mini_team(r)
    N = sum(sizes)
    X1 = capi.escape_point(X, r, N, np.zeros(4 * N), 0.0)
    assert bits(X1) == bits(CR.lift_zero(X, r, N))
    ref = CR.reference("lifted-r%d" % r, mp, sizes, r + 1, X1)
    assert ref.nz == r + 1
    t = make_team(mp, sizes, r + 1, X1, capi.PRECOND_DENSE)
    for deflate in (False, True):
        c, _ = run("rank-deficient iterates", t, ref, r + 1, tol=TOL, max_iters=CAP, deflate=deflate, **FAR)
        print("[X; 0] r %d deflate %d: %r" % (r, deflate, c))
        assert c.certified == 1, c
    t.close()


@pytest.mark.parametrize("weights", ["mixed", "dead_pose"])
def test_weights(weights):
    """edge weights 0, 0.25 and 1; and a pose whose every edge has weight 0 (four zero rows of S)"""
    r = 5
    mp, sizes, X = CR.mini_team(r, weights)
    ref = CR.reference("weights-" + weights, mp, sizes, r, X)
    t = make_team(mp, sizes, r, X, capi.PRECOND_DENSE)
    for deflate in (False, True):
        c, _ = run("weights", t, ref, r, tol=TOL, max_iters=CAP, deflate=deflate, **FAR)
        print("weights %s deflate %d: %r" % (weights, deflate, c))
        assert c.certified == 1, c
    t.close()


@pytest.mark.parametrize("deflate", [False, True])
def test_decision_on_both_sides_of_the_truth(deflate):
    r = 6
    t, ref = edge(r)
    lo, hi = ref.truth(deflate)
    lam = abs(hi)
    assert hi < 0 and 0.1 * lam > 1e3 * ((hi - lo) + TOL * ref.s)  # the margin is far wider than bracket and tolerance
    for rel in (False, True):
        scale = ref.s if rel else 1.0
        c, _ = run("decision", t, ref, r, eta=0.9 * lam / scale, eta_relative=rel, tol=TOL, max_iters=CAP, deflate=deflate)
        assert c.certified == 0, c
        c, _ = run("decision", t, ref, r, eta=1.1 * lam / scale, eta_relative=rel, tol=TOL, max_iters=CAP, deflate=deflate)
        assert c.certified == 1 and lo - TOL * ref.s - CR.C_PROD * CR.U * ref.s <= c.lambda_min <= hi + 2 * TOL * ref.s, c
    # the iteration cap: one iteration cannot converge from random numbers, and its Ritz value is no lower than the truth
    c, _ = run("decision", t, ref, r, tol=TOL, max_iters=1, deflate=deflate, **FAR)
    assert c.certified == -1 and c.iterations == 1 and c.lambda_min >= lo - CR.C_PROD * CR.U * ref.s, c


def test_a_team_without_poses_is_refused():
    """one pose alone cannot be stated (a pose exists as the end of a measurement, self loops are refused): a robot without
    measurements has no pose and never becomes INITIALIZED"""
    t = capi.Team(capi.default_params(r=3, num_robots=1), [0])
    assert t.agents[0].n == 0
    with pytest.raises(capi.DpgoError, match="not initialized"):
        t.certify()
    t.close()


@pytest.mark.parametrize("one_agent", [True, False], ids=["one_agent", "one_pose_agents"])
@pytest.mark.parametrize("total", [2, 3])
def test_tiny_teams(total, one_agent):
    """4N - nz < K: the starting block cannot have rank K.  The call then meets the contract or refuses with the cause
    (d = 0 is always refused here; the checker's branch for it is exercised by the stand-in of tests/test_certref.py).
    Where d >= K the problem has at most 12 dimensions and the search space [X W P] spans it after at most d / K steps:
    the call converges"""
    mp, sizes = CR.tiny_team(total, one_agent)
    seen = {"solved": 0, "refused": 0}
    stalled = []
    for r in range(3, 9):
        X = CR.random_point(r, r, total)
        ref = CR.Reference(mp, sizes, r, X)
        t = make_team(mp, sizes, r, X)
        for deflate in (False, True):
            d = ref.d if deflate else ref.L
            for K in range(3, 9):
                kw = dict(tol=TOL, max_iters=100, block=K, deflate=deflate, **FAR)
                if d >= K:
                    c, _ = run("tiny teams", t, ref, r, **kw)
                    seen["solved"] += 1
                    seen["status %d" % c.certified] = seen.get("status %d" % c.certified, 0) + 1
                    if c.certified != 1:
                        stalled.append((r, K, deflate, d, repr(c)))
                    continue
                try:
                    c, _ = run("tiny teams", t, ref, r, **kw)
                    seen["solved"] += 1
                except capi.DpgoError as e:
                    assert "too small for the block size" in str(e) and "4N - nz = %d" % d in str(e), str(e)
                    seen["refused"] += 1
        t.close()
    print("tiny team of %d (%s): %r" % (total, "one agent" if one_agent else "one-pose agents", seen))
    print("not converged where d >= K:", stalled)
    assert seen["solved"] and seen["refused"]
    assert not stalled, stalled


def test_split_across_teams_is_bitwise_the_single_team():
    """One participant holds the 1-pose agent and the agent without shared edges, the other everything else: the split
    result meets the contract, every participant reports the same bytes, and they are the single team's (the eigensolver's
    Gram sums add per agent, then the agents in robot order, in one team and across teams alike: DESIGN.md 5d)"""
    r = 5
    mp, sizes, X = CR.edge_team(r)
    ref = CR.reference("edge-r%d" % r, mp, sizes, r, X)
    N = len(sizes)
    t = make_team(mp, sizes, r, X)
    kw = dict(tol=TOL, max_iters=CAP, **FAR)
    c0, v0 = run("across teams", t, ref, r, **kw)
    sp = Split(mp.view(capi.MEAS_DTYPE), N, [[0, N - 1], list(range(1, N - 1))], X, r=r)
    res = sp.run(lambda tm, tr: tm.certify(transport=tr, owner_of_robot=sp.owner, **CR.Args(r, **kw).kw()))
    c1 = res[0][0]
    v1 = assemble(sp, [v for _, v in res], 4)
    assert all(bytes(c) == bytes(c1) for c, _ in res)
    out = CR.check_certificate(ref, CR.Args(r, **kw), c1, v1)
    RATIOS["across teams"].update({k: max(RATIOS["across teams"].get(k, 0.0), x) for k, x in out.items()})
    sgn = np.sign(v1 @ v0)
    print("single %r\nsplit  %r\n|lambda_1 - lambda_0| / s = %.3g, |residual_1 - residual_0| / s = %.3g, max |v_1 -+ v_0| = %.3g" % (
        c0, c1, abs(c1.lambda_min - c0.lambda_min) / ref.s, abs(c1.residual - c0.residual) / ref.s, np.abs(sgn * v1 - v0).max()))
    sp.close()
    t.close()
    assert c1.certified == 1 and c0.certified == 1
    assert c1.norm_bound == c0.norm_bound and (c1.block, c1.deflated) == (c0.block, c0.deflated)
    assert bytes(c1) == bytes(c0) and bits(v1) == bits(v0)


@pytest.mark.parametrize("r", [3, 8])
def test_two_calls_give_the_same_bytes(r):
    t, ref = edge(r)
    for deflate in (False, True):
        kw = dict(tol=TOL, max_iters=CAP, deflate=deflate, **FAR)
        (c1, v1), (c2, v2) = run("determinism", t, ref, r, **kw), run("determinism", t, ref, r, **kw)
        assert c1.iterations > 10 and bytes(c1) == bytes(c2) and bits(v1) == bits(v2)

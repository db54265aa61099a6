"""No-GPU checks of the certificate reference (tests/certref.py) and of the fixtures the GPU module
tests/test_gpu_certificate_edges.py runs on: the long-double S agrees with the sparse statement of
tests/test_certificate.py, every fixture with an expectation of convergence has its spectral gap, the checker accepts a
dense eigen-solve standing in for the GPU solver and rejects planted wrong answers."""
import types

import numpy as np
import pytest

from tests import certref as CR
from tests import xref
from tests.test_certificate import certificate_matrix, q_full
from tests.test_xref import C_PROD, ratio

U = xref.U64
FIXTURES = CR.converging_fixtures()


def built(name):
    mp, sizes, r, X, modes = dict(FIXTURES)[name]()
    return mp, sizes, r, X, modes, CR.reference(name, mp, sizes, r, X)


def global_numbering(mp, sizes):
    off = np.r_[0, np.cumsum(sizes)]
    m = mp.copy()
    m["p1"], m["p2"] = mp["p1"] + off[mp["r1"]], mp["p2"] + off[mp["r2"]]
    m["r1"] = m["r2"] = 0
    return m


def stand_in(ref, args, v=None):
    """a dense eigen-solve in place of the GPU solver: the fp64 Rayleigh quotient and residual of the reference's
    eigenvector (or of v), the decision taken as certify_body takes it"""
    if args.deflate and ref.d == 0:
        return types.SimpleNamespace(lambda_min=0.0, residual=0.0, norm_bound=ref.s, certified=1, iterations=1,
                                     block=args.block, deflated=1), np.zeros(ref.L)
    if v is None:
        v = np.asarray(ref.vd if args.deflate else ref.v, dtype=np.float64)
    Sv = ref.S64 @ v
    if args.deflate:
        Zo = np.asarray(ref.Zo, dtype=np.float64)
        Sv = Sv - Zo.T @ (Zo @ Sv)
    theta = float(v @ Sv) / float(v @ v)
    res = float(np.linalg.norm(Sv - theta * v) / np.linalg.norm(v))
    eta_abs = args.eta * ref.s if args.eta_relative else args.eta
    status = 0 if theta < -eta_abs else 1 if res <= args.tol * ref.s else -1
    c = types.SimpleNamespace(lambda_min=min(0.0, theta) if args.deflate else theta, residual=res, norm_bound=ref.s,
                              certified=status, iterations=args.max_iters if status < 0 else 1, block=args.block,
                              deflated=int(args.deflate))
    return c, v


@pytest.mark.parametrize("name", ["edge-r3", "edge-r8", "lifted-r4", "weights-mixed", "weights-dead_pose", "truth-r6"])
def test_S_agrees_with_the_sparse_statement(name):
    mp, sizes, r, X, _, ref = built(name)
    n = sum(sizes)
    S = certificate_matrix(q_full(global_numbering(mp, sizes), n), X, r, n).toarray()
    assert np.abs(ref.S64 - S).max() <= C_PROD * U * ref.s
    # and with the operator of tests/xref.py, in long double
    V = np.random.default_rng(1).standard_normal(3 * 4 * n)
    want, mag = xref.Team(mp, sizes).certificate_apply(xref.blocks(X, r, n), xref.blocks(V, 3, n))
    got = (np.asarray(V, dtype=xref.LD).reshape(4 * n, 3).T @ ref.S).T.reshape(-1)
    assert ratio(got, xref.flat(want), xref.flat(mag), 1) <= 1  # (both long double: far inside one fp64 unit)


@pytest.mark.parametrize("name", [f[0] for f in FIXTURES])
def test_fixture_has_its_gap_and_the_checker_accepts_the_truth(name):
    mp, sizes, r, X, modes, ref = built(name)
    assert ref.s >= ref.rho and ref.s_err <= 1e-12 * ref.s
    for deflate, mult, floor in modes:
        gap = ref.gap(deflate, mult)
        lo, hi = ref.truth(deflate)
        print("%s deflate=%d: gap %.4f, lambda/s %.3e, bracket %.1e s, nz %d" % (name, deflate, gap, hi / ref.s,
                                                                                (hi - lo) / ref.s, ref.nz))
        assert gap >= floor, (name, deflate, gap)
        assert hi - lo <= C_PROD * U * ref.s
        if name.startswith("truth"):
            assert ref.nz == 4 and abs(hi) <= C_PROD * U * ref.s
        else:
            assert hi < -0.1 * ref.s  # indefinite at a random point, by far
            if name.startswith("lifted"):
                assert ref.nz == r  # (the zero row of [X; 0] is dropped: r - 1 rows of X and e_t)
        # dry run: eta out of reach (the solver runs to convergence), and the decision on both sides of the truth
        lam = abs(hi)
        cases = ((1e300, False, 1), (0.9 * lam, False, 0), (1.1 * lam, False, 1), (1.1 * lam / ref.s, True, 1))
        if name.startswith("truth"):
            cases = ((1e300, False, 1), (1e-6, True, 1))
        for eta, rel, want in cases:
            args = CR.Args(r, eta=eta, tol=CR.TOL, max_iters=10, deflate=deflate, eta_relative=rel)
            c, v = stand_in(ref, args)
            assert c.certified == want, (name, eta, c)
            out = CR.check_certificate(ref, args, c, v)
            assert all(x <= 1 for x in out.values()), out


@pytest.mark.parametrize("deflate", [False, True])
def test_checker_rejects_planted_wrong_answers(deflate):
    mp, sizes, r, X, _, ref = built("lifted-r4")
    s = ref.s
    lo, hi = ref.truth(deflate)
    conv = CR.Args(r, eta=1e300, tol=CR.TOL, max_iters=10, deflate=deflate, eta_relative=False)

    def rejected(args, c, v):
        with pytest.raises(AssertionError):
            CR.check_certificate(ref, args, c, v)

    c, v = stand_in(ref, conv)
    CR.check_certificate(ref, conv, c, v)
    for off in (1e-6 * s, -1e-6 * s):  # lambda off by 1e-6 s, either way
        c, v = stand_in(ref, conv)
        c.lambda_min += off
        rejected(conv, c, v)
    # status 1 where the truth is below -eta
    args = CR.Args(r, eta=0.5 * abs(hi), tol=CR.TOL, max_iters=10, deflate=deflate, eta_relative=False)
    c, v = stand_in(ref, args)
    assert c.certified == 0
    c.certified = 1
    rejected(args, c, v)
    # status 0 where the truth is above -eta
    args = CR.Args(r, eta=2 * abs(hi), tol=CR.TOL, max_iters=10, deflate=deflate, eta_relative=False)
    c, v = stand_in(ref, args)
    assert c.certified == 1
    c.certified = 0
    rejected(args, c, v)
    # a residual wrong by a factor of two (on a vector whose residual is well above round-off and below tol s)
    rng = np.random.default_rng(2)
    w = rng.standard_normal(ref.L)
    if deflate:
        Zo = np.asarray(ref.Zo, dtype=np.float64)
        w -= Zo.T @ (Zo @ w)
    v1 = np.asarray(ref.vd if deflate else ref.v, dtype=np.float64) + 1e-11 * w / np.linalg.norm(w)
    v1 /= np.linalg.norm(v1)
    c, v = stand_in(ref, conv, v1)
    assert c.certified == 1 and 100 * C_PROD * U * s < c.residual < CR.TOL * s
    CR.check_certificate(ref, conv, c, v)
    for f in (2.0, 0.5):
        c, v = stand_in(ref, conv, v1)
        c.residual *= f
        rejected(conv, c, v)
    # norm_bound below the spectral radius
    c, v = stand_in(ref, conv)
    c.norm_bound = 0.9 * ref.rho
    rejected(conv, c, v)
    # not converged, but fewer iterations than the cap
    c, v = stand_in(ref, conv)
    c.certified, c.iterations = -1, 5
    rejected(conv, c, v)
    # a Ritz value below the truth
    c, v = stand_in(ref, conv)
    c.certified, c.iterations, c.lambda_min = -1, 10, lo - 1e-9 * s
    rejected(conv, c, v)
    if deflate:
        # v with a component in Z
        c, v = stand_in(ref, conv)
        v2 = v + 1e-9 * np.asarray(ref.Zo[0], dtype=np.float64)
        rejected(conv, c, v2 / np.linalg.norm(v2))


@pytest.mark.parametrize("total", [2, 3])
@pytest.mark.parametrize("one_agent", [True, False], ids=["one_agent", "one_pose_agents"])
def test_tiny_team_reference(total, one_agent):
    """the dimension count of the tiny teams: nz = min(r + 1, 4N) at a random point, d = 4N - nz, lambda_defl = 0 at d = 0"""
    mp, sizes = CR.tiny_team(total, one_agent)
    for r in range(3, 9):
        X = CR.random_point(r, r, total)
        ref = CR.Reference(mp, sizes, r, X)
        assert ref.nz == min(r + 1, 4 * total) and ref.d == 4 * total - ref.nz
        for deflate in (False, True):
            args = CR.Args(r, eta=1e300, tol=CR.TOL, max_iters=10, deflate=deflate, eta_relative=False)
            c, v = stand_in(ref, args)
            CR.check_certificate(ref, args, c, v)
        if ref.d == 0:
            assert ref.truth(True) == (0.0, 0.0)

"""Reference of the certificate eigensolver (csrc/certify.hip): lambda_min(S(X)), its decision and norm_bound.  TEST
INFRASTRUCTURE ONLY, no capi call: it runs without a GPU.

S(X) = Q - Lambda(X) is assembled in long double block by block from the measurement list (weights included: the edge
cost of tests/xref.py), Lambda from xref.Team.vq.  A dense copy rounded to fp64 goes through LAPACK (scipy eigh).

Truth bracket.  For the eigenvector v LAPACK returns, theta_ref = v^T S v / v^T v and rho_ref = |S v - theta_ref v| / |v|
are recomputed in long double (deflated: with P S P, P the long-double projector onto Z-perp, and v projected first).  A
symmetric matrix has an eigenvalue within rho of every Rayleigh quotient and none of its Rayleigh quotients lies below
lambda_min, so an eigenvalue lies in [theta_ref - rho_ref, theta_ref]; eigh finds the smallest eigenvalue to n u |S|, which
makes that eigenvalue lambda_min.  Every comparison with "the truth" below uses this bracket [lo, hi], not a number.

Deflated truth.  Z = [rows of X; e_t]: rows unit-scaled, eigenvalues of the scaled Gram matrix below 1e-12 of the largest
dropped -> nz; B an orthonormal basis of Z-perp, d = 4N - nz, lambda_defl = min(0, lambda_min(B^T S B)), 0
when d = 0.

norm_bound.  k_cert_lambda takes, per column c of pose g, the sum of the magnitudes of (i) the stored 4 x 4 blocks of the
pose's row of its agent's Q -- one block per pose of the same agent it shares an edge with, parallel edges merged, and the
diagonal block, which also holds the local ends of the agent's shared edges --, (ii) the blocks of its shared edges, one
per edge, (iii) Lambda_g.  s is the largest of them.  The same expression evaluated on |T| and |X| gives the magnitude;
an fp64 evaluation in any order lies within count u magnitude of the long-double value, count = the rounding steps of one
sum (Reference.s_count).

Fixtures: seeded teams sized for the certificate kernels' tiles (edge_team), small teams for rank-deficient iterates and
weights (mini_team), teams of one to three poses (tiny_team)."""
import numpy as np
import scipy.linalg as sla

from oracle import np_crosscheck as NP
from oracle import oracle as O
from tests import xref
from tests.test_xref import C_PROD
from tests.util import synthetic_chain

LD = xref.LD
U = xref.U64
RANK_TOL = 1e-12  # directions of Z below this fraction of the largest are dropped
TOL = 1e-10  # the solver's tolerance in the GPU tests, relative to s
# Floors of the relative spectral gap (lambda_2 - lambda_1) / s of the fixtures a GPU test expects to converge on
# (asserted by tests/test_certref.py): the seeded random manifold points, and the noise-free optimum, where S is a
# connection Laplacian whose low end is dense
GAP_FLOOR = 0.015
TRUTH_GAP_FLOOR = 0.001


def iteration_cap(gap, tol=TOL):
    """max_iters for a fixture of relative gap `gap`: a Krylov eigensolver without preconditioner reduces the residual
    by exp(-2 sqrt(gap)) per iteration at the least (the Chebyshev rate; LOBPCG's three-term recurrence is of that
    class), so ln(1 / tol) / (2 sqrt(gap)) iterations reach tol; eight times that is the cap (the block's restarts and
    the start from random numbers)"""
    return int(np.ceil(4 * np.log(1 / tol) / np.sqrt(gap)))


# ----------------------------------------------------------------------------- graphs
def rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def team_graph(sizes, seed, closures, isolated_last=True, every_pose_shared=None, consistent=False):
    """Measurements in robot numbering of a team of len(sizes) agents cut from one odometry chain.  closures: the number of
    seeded loop closures between random poses (any two agents, or one); isolated_last: the last agent has no shared edge
    (the chain is cut in front of it and its closures stay inside); every_pose_shared = (a, b): every pose of agent a
    gets an edge to a pose of agent b; consistent: every measurement, odometry included, is taken without noise from a
    seeded random ground truth (rotations uniform, translations standard normal: the lifted truth is a global optimum of
    cost 0), else random closures on synthetic_chain's noisy odometry.  Returns (mp, m_global, truth (R, t) or None)."""
    rng = np.random.default_rng(seed)
    sizes = list(sizes)
    off = np.r_[0, np.cumsum(sizes)]
    total = int(off[-1])
    m, _ = synthetic_chain(total, seed=seed, lc_every=total + 1)
    truth = None
    if consistent:
        truth = (np.array([rotation(rng) for _ in range(total)]), rng.standard_normal((total, 3)))

    def measured(i, j):
        Rg, tg = truth
        return (Rg[i].T @ Rg[j]).reshape(-1), Rg[i].T @ (tg[j] - tg[i])
    if consistent:
        for e in m:
            e["R"], e["t"] = measured(int(e["p1"]), int(e["p2"]))
    robot = np.searchsorted(off, np.arange(total), side="right") - 1
    last = len(sizes) - 1
    if isolated_last:
        m = m[~((robot[m["p1"]] != last) & (robot[m["p2"]] == last))]
    pairs = set()
    if every_pose_shared is not None:
        a, b = every_pose_shared
        assert sizes[b] >= sizes[a] + 3
        pairs |= {(int(off[a]) + k, int(off[b]) + 3 + k) for k in range(sizes[a])}
    free = int(off[last]) if isolated_last else total
    want = len(pairs) + closures
    while len(pairs) < want and free >= 3:
        i, j = sorted(int(x) for x in rng.integers(0, free, 2))
        if j - i >= 2:
            pairs.add((i, j))
    if isolated_last and sizes[last] >= 3:
        want = len(pairs) + max(1, sizes[last] // 3)
        while len(pairs) < want:
            i, j = sorted(int(x) for x in rng.integers(int(off[last]), total, 2))
            if j - i >= 2:
                pairs.add((i, j))
    pairs = sorted(pairs)
    e = np.zeros(len(pairs), dtype=m.dtype)
    for k, (i, j) in enumerate(pairs):
        e[k]["p1"], e[k]["p2"] = i, j
        if consistent:
            e[k]["R"], e[k]["t"] = measured(i, j)
        else:
            e[k]["R"], e[k]["t"] = rotation(rng).reshape(-1), rng.standard_normal(3)
        e[k]["kappa"], e[k]["tau"], e[k]["weight"] = 20.0 + k % 7, 3.0 + k % 5, 1.0
    m = np.concatenate([m, e])
    mp = m.copy()
    mp["r1"], mp["p1"] = robot[m["p1"]], m["p1"] - off[robot[m["p1"]]]
    mp["r2"], mp["p2"] = robot[m["p2"]], m["p2"] - off[robot[m["p2"]]]
    return mp, m, truth


def edge_sizes(r):
    """agents at the tiles of the certificate kernels: 1, 2, PPB - 1, PPB, PPB + 1 poses (PPB = 64 / K poses per wave of
    k_cert_apply<K>, K = r by default), 31 / 33 (one 128-column Gram chunk: 4 n = 124, 132), 64 / 65 (N4 = 256, 260: the
    256-lane strides of k_cert_precond), 257 (two 256-pose tiles of k_cert_lambda); the last agent has no shared edge"""
    # (PPB follows r, the default block: a block K != r meets its own wave boundary PPB(K) - 1 / PPB(K) / PPB(K) + 1 only
    # in the team of rank K; the other (r, K) pairs run k_cert_apply<K> against the rank-r Lambda at the remaining edges)
    ppb = 64 // r
    return [1, 2, ppb - 1, ppb, ppb + 1, 31, 33, 64, 65, 257, ppb + 1]


MINI_SIZES = [1, 2, 7, 33, 31, 5]  # 79 poses
# seeds of the random manifold points: the first of 400 + r + 10 k (edge team) whose S has a relative gap >= GAP_FLOOR
# in both modes -- chosen on the reference's spectrum alone (tests/test_certref.py asserts the gaps)
EDGE_X_SEED = {3: 403, 4: 414, 5: 415, 6: 426, 7: 477, 8: 478}
MINI_X_SEED = {(3, None): 743, (4, None): 744, (5, None): 705, (6, None): 726, (7, None): 727, (5, "mixed"): 715,
               (5, "dead_pose"): 715}  # (the first of 700 + r + 10 k, as above)
_CACHE = {}


def random_point(seed, r, n):
    """a seeded random point of the manifold, flat iterate layout"""
    return NP.flat(NP.project_manifold(np.random.default_rng(seed).standard_normal((r, 4 * n)), n))


def edge_team(r):
    """(mp, sizes, X): the tile-edge team of rank r at a seeded random manifold point; agent 4 (PPB + 1 poses) has a shared
    edge at every pose (to agent 7), N / 4 random closures"""
    key = ("edge", r)
    if key not in _CACHE:
        sizes = edge_sizes(r)
        N = sum(sizes)
        assert N % 32 != 0
        mp, _, _ = team_graph(sizes, 300 + r, closures=N // 4, every_pose_shared=(4, 7))
        _CACHE[key] = (mp, sizes, random_point(EDGE_X_SEED[r], r, N))
    return _CACHE[key]


def mini_team(r, weights=None):
    """(mp, sizes, X): 79 poses at a random point.  weights "mixed": closures weighted 0 / 0.25 / 1 and odometry 0.25 / 1
    (still connected); "dead_pose": besides, every edge of one pose has weight 0"""
    key = ("mini", r, weights)
    if key not in _CACHE:
        sizes = MINI_SIZES
        N = sum(sizes)
        mp, _, _ = team_graph(sizes, 500 + r, closures=N // 2, every_pose_shared=(2, 3))
        if weights is not None:
            rng = np.random.default_rng(600 + r)
            odo = (mp["r1"] == mp["r2"]) & (mp["p2"] == mp["p1"] + 1)
            chain = odo | ((mp["r2"] == mp["r1"] + 1) & (mp["p2"] == 0))  # the cut chain: odometry and agent-to-agent links
            mp["weight"] = np.where(chain, rng.choice([0.25, 1.0], len(mp)), rng.choice([0.0, 0.25, 1.0], len(mp)))
            assert (mp["weight"] == 0).any() and (mp["weight"] == 0.25).any() and (mp["weight"] == 1).any()
            if weights == "dead_pose":
                a, p = 3, sizes[3] // 2
                dead = ((mp["r1"] == a) & (mp["p1"] == p)) | ((mp["r2"] == a) & (mp["p2"] == p))
                assert dead.sum() >= 2
                mp["weight"][dead] = 0.0
        _CACHE[key] = (mp, sizes, random_point(MINI_X_SEED[r, weights], r, N))
    return _CACHE[key]


def truth_team():
    """(mp, sizes, m_global, truth): a connected noise-free team (no isolated agent) whose lifted ground truth is a rank-3
    global optimum of cost 0: S is positive semidefinite with the 4-dimensional null space Z.  The odometry of m_global
    chains through every pose, so an odometry initialisation reproduces the truth up to the gauge"""
    key = ("truth",)
    if key not in _CACHE:
        sizes = MINI_SIZES[:-1]
        mp, m, truth = team_graph(sizes, 800, closures=3 * sum(sizes), isolated_last=False, every_pose_shared=(2, 3),
                                  consistent=True)
        _CACHE[key] = (mp, sizes, m, truth)
    return _CACHE[key]


def lifted_truth(truth, r):
    """[R_i | t_i] of a ground truth under the first three coordinate axes of R^r, flat iterate layout"""
    R, t = truth
    n = len(R)
    X = np.zeros((r, 4 * n))
    for i in range(n):
        X[:3, 4 * i:4 * i + 3] = R[i]
        X[:3, 4 * i + 3] = t[i]
    return NP.flat(X)


def tiny_team(total, one_agent, seed=0):
    """(mp, sizes) of a team of 2 or 3 poses: one agent (odometry, and a closure 0 -> 2 at three poses) or `total` one-pose
    agents (the same edges, all shared).  One pose alone cannot be stated: a pose exists as the end of a measurement"""
    assert total in (2, 3)
    rng = np.random.default_rng(900 + seed)
    pairs = [(0, 1)] if total == 2 else [(0, 1), (1, 2), (0, 2)]
    mp = np.zeros(len(pairs), dtype=O.MEAS_DTYPE)
    for k, (i, j) in enumerate(pairs):
        if one_agent:
            mp[k]["p1"], mp[k]["p2"] = i, j
        else:
            mp[k]["r1"], mp[k]["r2"] = i, j
        mp[k]["R"], mp[k]["t"] = rotation(rng).reshape(-1), rng.standard_normal(3)
        mp[k]["kappa"], mp[k]["tau"], mp[k]["weight"] = 20.0 + k, 3.0 + k, 1.0
    return mp, ([total] if one_agent else [1] * total)


def lift_zero(X, r, n):
    """[X; 0] at rank r + 1, flat iterate layout (what dpgo_escape_point returns at alpha = 0)"""
    return NP.flat(np.vstack([np.asarray(X).reshape(4 * n, r).T, np.zeros((1, 4 * n))]))


def converging_fixtures():
    """every fixture a GPU test expects convergence on: (name, build) with build() -> (mp, sizes, r, X, modes), modes =
    [(deflate, multiplicity of lambda_1, gap floor)].  At the noise-free optimum lambda_1 = 0 is the 4-dimensional null
    space Z undeflated: any vector of it is an eigenvector, the gap that counts is the one above it"""
    both = [(False, 1, GAP_FLOOR), (True, 1, GAP_FLOOR)]
    out = []
    for r in range(3, 9):
        out.append(("edge-r%d" % r, lambda r=r: edge_team(r)[:2] + (r, edge_team(r)[2], both)))
    for r in range(3, 8):
        def lifted(r=r):
            mp, sizes, X = mini_team(r)
            return mp, sizes, r + 1, lift_zero(X, r, sum(sizes)), both
        out.append(("lifted-r%d" % r, lifted))
    for w in ("mixed", "dead_pose"):
        out.append(("weights-" + w, lambda w=w: mini_team(5, w)[:2] + (5, mini_team(5, w)[2], both)))
    for r in (4, 6, 8):
        def truth(r=r):
            mp, sizes, _, tr = truth_team()
            return mp, sizes, r, lifted_truth(tr, r), [(False, 4, TRUTH_GAP_FLOOR), (True, 1, TRUTH_GAP_FLOOR)]
        out.append(("truth-r%d" % r, truth))
    return out


def reference(key, mp, sizes, r, X):
    """the Reference of a fixture, built once per process"""
    key = ("ref",) + tuple(key if isinstance(key, tuple) else (key,))
    if key not in _CACHE:
        _CACHE[key] = Reference(mp, sizes, r, X)
    return _CACHE[key]


# ----------------------------------------------------------------------------- the reference
def _mgs(rows):
    """rows orthonormalised in long double (modified Gram-Schmidt, twice)"""
    Z = np.array(rows, dtype=LD)
    for _ in range(2):
        for k in range(len(Z)):
            for l in range(k):
                Z[k] -= (Z[l] @ Z[k]) * Z[l]
            Z[k] /= np.sqrt(Z[k] @ Z[k])
    return Z


class Reference:
    """S(X) of a team (measurements mp in robot numbering, sizes per agent) at the iterate X (flat, team order, rank r)"""

    def __init__(self, mp, sizes, r, X):
        self.r, self.sizes = r, list(sizes)
        team = xref.Team(mp, sizes)
        N = self.N = team.N
        L = self.L = 4 * N
        Xb = xref.blocks(X, r, N)
        i, j, T, om = team.i, team.j, team.T, team.om
        aT = np.abs(T)
        TO, TOm = T * om[:, None, :], aT * om[:, None, :]
        TOT, TOTm = TO @ T.transpose(0, 2, 1), TOm @ aT.transpose(0, 2, 1)
        Om = np.eye(4, dtype=LD) * om[:, None, :]
        E, Em = team.vq(Xb)
        Y, aY = Xb[:, :, :3], np.abs(Xb[:, :, :3])
        lam = xref._sym(Y.transpose(0, 2, 1) @ E[:, :, :3])
        lamm = xref._sym(aY.transpose(0, 2, 1) @ Em[:, :, :3])
        # S, block (g, h) at S4[g, h]
        S4 = np.zeros((N, N, 4, 4), dtype=LD)
        np.add.at(S4, (i, i), TOT)
        np.add.at(S4, (j, j), Om)
        np.add.at(S4, (i, j), -TO)
        np.add.at(S4, (j, i), -TO.transpose(0, 2, 1))
        g = np.arange(N)
        S4[g, g, :3, :3] -= lam
        S = S4.transpose(0, 2, 1, 3).reshape(L, L)
        self.S = 0.5 * (S + S.T)
        self.S64 = self.S.astype(np.float64)
        # norm_bound: the stored blocks (same agent, merged; the diagonal block holds every edge's local end), the shared
        # edges one by one, Lambda
        same = np.asarray(mp["r1"] == mp["r2"])
        A4, M4 = np.zeros((N, N, 4, 4), dtype=LD), np.zeros((N, N, 4, 4), dtype=LD)
        for (a, b, blk, mag) in ((i, i, TOT, TOTm), (j, j, Om, Om),
                                 (i[same], j[same], -TO[same], TOm[same]),
                                 (j[same], i[same], -TO[same].transpose(0, 2, 1), TOm[same].transpose(0, 2, 1))):
            np.add.at(A4, (a, b), blk)
            np.add.at(M4, (a, b), mag)
        rs, rm = np.abs(A4).sum(axis=(1, 3)), M4.sum(axis=(1, 3))
        sh = ~same
        np.add.at(rs, i[sh], np.abs(TO[sh]).sum(axis=2))
        np.add.at(rm, i[sh], TOm[sh].sum(axis=2))
        np.add.at(rs, j[sh], np.abs(TO[sh]).transpose(0, 2, 1).sum(axis=2))
        np.add.at(rm, j[sh], TOm[sh].transpose(0, 2, 1).sum(axis=2))
        rs[:, :3] += np.abs(lam).sum(axis=2)
        rm[:, :3] += lamm.sum(axis=2)
        self.s = float(rs.max()) if N else 0.0
        deg = np.bincount(np.r_[i, j], minlength=N).max() if len(i) else 0
        # rounding steps of one column sum: an entry of a diagonal block accumulates up to deg edges of a 4-term product
        # with two multiplications each (6 deg); an entry of Lambda is an r-term product of X with the Euclidean gradient,
        # itself within C_PROD u of its magnitude, then halved and added (C_PROD + r + 2); the sum adds 4 entries per block
        # (deg + 1 blocks at the most) and 3 of Lambda
        self.s_count = 6 * int(deg) + C_PROD + r + 2 + 4 * (int(deg) + 1) + 3
        self.s_err = float(self.s_count * U * rm.max()) if N else 0.0
        # spectrum (fp64 LAPACK) and the bracket of lambda_min
        w, V = sla.eigh(self.S64, subset_by_index=[0, min(1, L - 1)])
        wmax = sla.eigvalsh(self.S64, subset_by_index=[L - 1, L - 1])[0]
        self.rho = float(max(abs(w[0]), abs(wmax)))  # spectral radius, to n u |S|
        self.w = w
        self.lo, self.hi, self.v = self._bracket(V[:, 0], None)
        # deflation
        Z = np.vstack([np.asarray(X, dtype=LD).reshape(L, r).T, np.tile(np.array([0, 0, 0, 1], dtype=LD), N)])
        G = (Z @ Z.T).astype(np.float64)
        dg = np.array([1.0 / np.sqrt(x) if x > 0 else 0.0 for x in np.diag(G)])
        mu, Vz = np.linalg.eigh(0.5 * (G + G.T) * dg[:, None] * dg[None, :])
        keep = mu > RANK_TOL * mu[-1]
        self.nz = int(keep.sum())
        self.d = L - self.nz
        self.Zrows = Z  # (for |Z v|: unit-scaled below)
        self.Zo = _mgs((Vz[:, keep].T * dg[None, :]).astype(LD) @ Z)
        if self.d > 0:
            Qf, _ = np.linalg.qr(np.asarray(self.Zo, dtype=np.float64).T, mode="complete")
            self.B = Qf[:, self.nz:]
            BSB = self.B.T @ self.S64 @ self.B
            BSB = 0.5 * (BSB + BSB.T)
            wd, Yd = sla.eigh(BSB, subset_by_index=[0, min(1, self.d - 1)])
            self.wd = wd
            lo, hi, self.vd = self._bracket(self.B @ Yd[:, 0], self.Zo)
            self.lo_d, self.hi_d = min(0.0, lo), min(0.0, hi)
        else:
            self.B, self.wd, self.vd = np.zeros((L, 0)), np.zeros(0), np.zeros(L, dtype=LD)
            self.lo_d = self.hi_d = 0.0

    # -- long-double operator
    def project(self, v, Zo):
        return v if Zo is None else v - Zo.T @ (Zo @ v)

    def rayleigh(self, v, deflate):
        """(theta, rho) of v in long double: v^T S v / v^T v and |P S v - theta v| / |v| (P = I undeflated)"""
        v = np.asarray(v, dtype=LD)
        Sv = self.project(self.S @ v, self.Zo if deflate else None)
        nn = v @ v
        theta = (v @ Sv) / nn
        res = Sv - theta * v
        return theta, np.sqrt((res @ res) / nn)

    def _bracket(self, v64, Zo):
        v = self.project(np.asarray(v64, dtype=LD), Zo)
        v = v / np.sqrt(v @ v)
        theta, rho = self.rayleigh(v, Zo is not None)
        return float(theta - rho), float(theta), v

    def truth(self, deflate):
        """the bracket [lo, hi] of what the call reports: lambda_min(S), or min(0, lambda_min on Z-perp)"""
        return (self.lo_d, self.hi_d) if deflate else (self.lo, self.hi)

    def gap(self, deflate, mult=1):
        """relative spectral gap (lambda_{mult+1} - lambda_1) / s of the operator the solver iterates on (mult = 1 needs
        the two eigenvalues kept above; a larger multiplicity solves the dense problem again)"""
        if mult == 1:
            w = self.wd if deflate else self.w
        else:
            A = self.B.T @ self.S64 @ self.B if deflate else self.S64
            w = sla.eigvalsh(0.5 * (A + A.T), subset_by_index=[0, mult])
        return float(w[mult] - w[0]) / self.s


class _Zeros(dict):
    """neighbour poses that do not matter (the preconditioner's operator has no linear term)"""

    def __missing__(self, key):
        return np.zeros(12)


def precond_reference(key, mp, sizes, a, shift=0.1):
    """(P, D, (kappa_2(P), |P^-1|_2), the same of D) of agent a: P = Q_a + shift I dense (fp64 copy of the long-double
    assembly of tests/xref.py), D its 4 x 4 diagonal blocks (n, 4, 4); built once per process"""
    key = ("precond", key, a)
    if key not in _CACHE:
        n = sizes[a]
        ag = xref.Agent(mp, a, n, 3, _Zeros({None: None}), shift=shift)
        P = ag.q_dense() + shift * np.eye(4 * n)
        D = (ag.block_diag_q() + shift * np.eye(4, dtype=LD)).astype(np.float64)
        ev, evd = np.linalg.eigvalsh(P), np.linalg.eigvalsh(D)
        _CACHE[key] = (P, D, (float(ev.max() / ev.min()), float(1 / ev.min())), (float(evd.max() / evd.min()), float(1 / evd.min())))
    return _CACHE[key]


def precond_apply(P, D, V, block_jacobi):
    """P^-1 V (or the block-diagonal D^-1 V) for V (4n, K): an fp64 solve and two refinement steps on the long-double residual"""
    n = len(D)
    if block_jacobi:
        def solve(R):
            return np.linalg.solve(D, np.asarray(R, dtype=np.float64).reshape(n, 4, -1)).reshape(4 * n, -1)

        def apply(Z):
            return (D.astype(LD) @ Z.reshape(n, 4, -1)).reshape(4 * n, -1)
    else:
        Pl = P.astype(LD)

        def solve(R):
            return np.linalg.solve(P, np.asarray(R, dtype=np.float64))

        def apply(Z):
            return Pl @ Z
    V = np.asarray(V, dtype=LD)
    Z = solve(V).astype(LD)
    for _ in range(2):
        Z = Z + solve(V - apply(Z))
    return Z


class Args:
    """the arguments of one call of Team.certify"""

    def __init__(self, r, eta=1e-6, tol=1e-8, max_iters=1000, block=0, deflate=True, eta_relative=True):
        self.eta, self.tol, self.max_iters, self.block = eta, tol, max_iters, block or r
        self.deflate, self.eta_relative = deflate, eta_relative

    def kw(self):
        return dict(eta=self.eta, tol=self.tol, max_iters=self.max_iters, block=self.block, deflate=self.deflate,
                    eta_relative=self.eta_relative)


def check_certificate(ref, args, cert, v):
    """The contract of dpgo_team_certify at every exit, against the reference's bracket [lo, hi] of the truth.

    Arithmetic bound (derived, not measured).  The solver reports the Ritz value theta of a vector of its block and the
    residual rho of that pair.  An eigenvalue lies within rho of theta and theta >= lambda_min, so a converged call
    (rho <= tol s) is within tol s of an eigenvalue -- that it is the smallest one is what the comparison with the truth
    checks.  On top comes the round-off of the operator products theta and rho are formed from: RO = C_PROD u s (C_PROD
    of tests/test_xref.py; s the reference's Gershgorin bound).  The reported residual is the root of a Gram entry summed
    over 4N terms: it agrees with the long-double one to RO + 4N u residual.  |v| = 1 and Z v = 0 hold to C_PROD u after
    two CholQR passes and the projection.

    Returns the error / bound ratios that were checked (all <= 1)."""
    s = ref.s
    RO = C_PROD * U * s
    out = {}
    assert all(np.isfinite(x) for x in (cert.lambda_min, cert.residual, cert.norm_bound)), cert
    assert cert.certified in (-1, 0, 1), cert
    assert cert.block == args.block and cert.deflated == int(args.deflate), cert
    assert 1 <= cert.iterations <= args.max_iters, cert
    # norm_bound: the reference's s within its rounding bound, and a bound on the spectral radius
    out["norm_bound"] = abs(cert.norm_bound - s) / ref.s_err if ref.s_err > 0 else float(cert.norm_bound != s)
    assert abs(cert.norm_bound - s) <= ref.s_err, (cert.norm_bound, s, ref.s_err)
    assert cert.norm_bound >= ref.rho * (1 - ref.L * U), (cert.norm_bound, ref.rho)
    eta_abs = args.eta * cert.norm_bound if args.eta_relative else args.eta
    tol_abs = args.tol * s
    lo, hi = ref.truth(args.deflate)
    lam = cert.lambda_min
    # a Rayleigh quotient cannot undershoot
    out["undershoot"] = max(0.0, lo - lam) / RO
    assert lam >= lo - RO, (lam, lo, RO)
    v = np.asarray(v, dtype=LD)
    nv = float(np.sqrt(v @ v))
    if ref.d == 0 and args.deflate:
        # nothing is left of R^{4N}: the only admissible answer is lambda_min 0, certified
        assert cert.certified == 1 and lam == 0.0, cert
        return out
    out["norm_v"] = abs(nv - 1) / (C_PROD * U)
    assert abs(nv - 1) <= C_PROD * U, nv
    if args.deflate:
        zv = float(np.abs(ref.Zo @ v).max())
        out["Zv"] = zv / (C_PROD * U)
        assert zv <= C_PROD * U, zv
    theta_v, res_v = (float(x) for x in ref.rayleigh(v, args.deflate))
    if cert.certified == 1:
        assert res_v <= tol_abs + RO, (res_v, tol_abs)
        agree = RO + ref.L * U * res_v
        out["residual"] = abs(cert.residual - res_v) / agree
        assert abs(cert.residual - res_v) <= agree, (cert.residual, res_v, agree)
        out["lambda"] = max(lam - hi, lo - lam, 0.0) / (tol_abs + RO)
        assert lo - tol_abs - RO <= lam <= hi + tol_abs + RO, (lam, lo, hi, tol_abs)
        assert hi >= -eta_abs - tol_abs, (hi, eta_abs)
    elif cert.certified == 0:
        assert lam < -eta_abs, (lam, eta_abs)
        assert hi < -eta_abs, (hi, eta_abs)
        assert theta_v < -eta_abs + RO, (theta_v, eta_abs)
    else:
        assert cert.iterations == args.max_iters, cert
    return out

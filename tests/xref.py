"""Extended-precision reference of the per-agent operations and of the team's certificate operator and rounding.  TEST
INFRASTRUCTURE ONLY: written from the measurement list (the edge cost w/2 |(X_j - X_i T) Omega^(1/2)|^2, T = [[R, t], [0, 1]],
Omega = diag(kappa, kappa, kappa, tau)), not from the oracle.

Arithmetic is np.longdouble (64-bit significand on x86-64: u = 2^-64, 2^11 below fp64's), 3 x 3 SVDs and nearest
rotations are mpmath at 40 digits.  Every product also returns its componentwise magnitude: the same expression evaluated
on |a| and |b| (sum |a||b|), pushed through the later steps the same way.  A kernel that forms the product in fp64 with any
summation order then satisfies |gpu - ref| <= c 2^-53 mag, c a small multiple of the number of terms; a missing term, pose
or lane is of the order of mag itself.

Layout: an agent's iterate is r x 4n, flat column-major over the poses ([(4 j + c) r + a]); here it is held as blocks
B[j] = the r x 4 matrix [Y_j | p_j], shape (n, r, 4)."""
import mpmath
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended long double (x86-64: 80-bit)"
U64 = 2.0 ** -53
mpmath.mp.dps = 40
F = np.diag([1.0, 1.0, -1.0])


def blocks(x, r, n):
    """flat iterate layout -> (n, r, 4) long double blocks"""
    return np.asarray(x, dtype=LD).reshape(n, 4, r).transpose(0, 2, 1).copy()


def flat(B):
    """(n, r, 4) blocks -> flat iterate layout, fp64"""
    return np.ascontiguousarray(np.asarray(B).transpose(0, 2, 1), dtype=np.float64).reshape(-1)


def edge_arrays(m):
    """T (e, 4, 4) and Omega diagonals (e, 4) of every measurement row, long double"""
    e = len(m)
    T = np.zeros((e, 4, 4), dtype=LD)
    T[:, :3, :3] = np.asarray(m["R"], dtype=LD).reshape(e, 3, 3)
    T[:, :3, 3] = np.asarray(m["t"], dtype=LD)
    T[:, 3, 3] = 1
    w = np.asarray(m["weight"], dtype=LD)
    om = np.zeros((e, 4), dtype=LD)
    om[:, :3] = (np.asarray(m["kappa"], dtype=LD) * w)[:, None]
    om[:, 3] = np.asarray(m["tau"], dtype=LD) * w
    return T, om


def _sym(S):
    return 0.5 * (S + S.transpose(0, 2, 1))


def tangent_project(X, V, Vm=None):
    """P_X(V): rotation block W - Y Sym(Y^T W), translation column unchanged.  (value, magnitude)"""
    Vm = np.abs(V) if Vm is None else Vm
    Y, W = X[:, :, :3], V[:, :, :3]
    out, mag = V.copy(), Vm.copy()
    out[:, :, :3] = W - Y @ _sym(Y.transpose(0, 2, 1) @ W)
    aY = np.abs(Y)
    mag[:, :, :3] = Vm[:, :, :3] + aY @ _sym(aY.transpose(0, 2, 1) @ Vm[:, :, :3])
    return out, mag


class Agent:
    """one robot's problem: its measurements, its size n and the neighbour poses ((robot, pose) -> r x 4n flat block of
    4 r doubles, the layout of update_neighbor_poses) that the shared edges read"""

    def __init__(self, m, aid, n, r, nbr_poses=None, shift=0.1):
        self.aid, self.n, self.r, self.shift = aid, n, r, shift
        mine = m[(m["r1"] == aid) | (m["r2"] == aid)]
        self.m = mine
        loc1, loc2 = mine["r1"] == aid, mine["r2"] == aid
        T, om = edge_arrays(mine)
        both = loc1 & loc2
        self.priv = (mine["p1"][both].astype(int), mine["p2"][both].astype(int), T[both], om[both])
        s1 = loc1 & ~loc2  # local tail i, neighbour head j
        s2 = loc2 & ~loc1  # neighbour tail i, local head j
        nbr_poses = nbr_poses or {}

        def nb(rows):
            return np.array([blocks(nbr_poses[(int(a), int(b))], r, 1)[0] for a, b in rows], dtype=LD).reshape(-1, r, 4)
        self.sh1 = (mine["p1"][s1].astype(int), T[s1], om[s1], nb(zip(mine["r2"][s1], mine["p2"][s1])))
        self.sh2 = (mine["p2"][s2].astype(int), T[s2], om[s2], nb(zip(mine["r1"][s2], mine["p1"][s2])))

    # -- products, edge by edge
    def xq(self, X, Xm=None):
        """X Q (value, magnitude): Q the agent's data matrix, private edges and the local ends of shared edges"""
        Xm = np.abs(X) if Xm is None else Xm
        out, mag = np.zeros_like(X), np.zeros_like(X)
        i, j, T, om = self.priv
        aT = np.abs(T)
        Tt, aTt = T.transpose(0, 2, 1), aT.transpose(0, 2, 1)
        res = (X[j] - X[i] @ T) * om[:, None, :]
        resm = (Xm[j] + Xm[i] @ aT) * om[:, None, :]
        np.add.at(out, j, res)
        np.add.at(out, i, -res @ Tt)
        np.add.at(mag, j, resm)
        np.add.at(mag, i, resm @ aTt)
        i, T, om, _ = self.sh1
        np.add.at(out, i, ((X[i] @ T) * om[:, None, :]) @ T.transpose(0, 2, 1))
        np.add.at(mag, i, ((Xm[i] @ np.abs(T)) * om[:, None, :]) @ np.abs(T).transpose(0, 2, 1))
        j, T, om, _ = self.sh2
        np.add.at(out, j, X[j] * om[:, None, :])
        np.add.at(mag, j, Xm[j] * om[:, None, :])
        return out, mag

    def G(self):
        """the linear term from the neighbour poses (value, magnitude)"""
        G = np.zeros((self.n, self.r, 4), dtype=LD)
        Gm = np.zeros_like(G)
        i, T, om, Z = self.sh1
        np.add.at(G, i, -(Z * om[:, None, :]) @ T.transpose(0, 2, 1))
        np.add.at(Gm, i, (np.abs(Z) * om[:, None, :]) @ np.abs(T).transpose(0, 2, 1))
        j, T, om, Z = self.sh2
        np.add.at(G, j, -(Z @ T) * om[:, None, :])
        np.add.at(Gm, j, (np.abs(Z) @ np.abs(T)) * om[:, None, :])
        return G, Gm

    def egrad(self, X):
        q, qm = self.xq(X)
        G, Gm = self.G()
        return q + G, qm + Gm

    def f(self, X):
        q, qm = self.xq(X)
        G, Gm = self.G()
        aX = np.abs(X)
        return 0.5 * np.sum(X * q) + np.sum(G * X), 0.5 * np.sum(aX * qm) + np.sum(Gm * aX)

    def rgrad(self, X):
        E, Em = self.egrad(X)
        return tangent_project(X, E, Em)

    def hessvec(self, X, eta):
        """P_X(eta Q - eta_rot Sym(Y^T E_rot)), E the Euclidean gradient (value, magnitude)"""
        E, Em = self.egrad(X)
        H, Hm = self.xq(eta)
        Y, aY = X[:, :, :3], np.abs(X[:, :, :3])
        H[:, :, :3] -= eta[:, :, :3] @ _sym(Y.transpose(0, 2, 1) @ E[:, :, :3])
        Hm[:, :, :3] += np.abs(eta[:, :, :3]) @ _sym(aY.transpose(0, 2, 1) @ Em[:, :, :3])
        return tangent_project(X, H, Hm)

    # -- the preconditioner's operator
    def q_dense(self):
        """Q as a dense 4n x 4n fp64 matrix (for the fp64 solve and the conditioning only): I Q, the 4n rows of the identity
        taken as one iterate"""
        n = self.n
        E = np.eye(4 * n, dtype=LD).reshape(4 * n, n, 4).transpose(1, 0, 2)
        return np.ascontiguousarray(self.xq(E)[0].transpose(1, 0, 2).reshape(4 * n, 4 * n), dtype=np.float64)

    def block_diag_q(self):
        """the 4 x 4 diagonal blocks of Q, long double"""
        D = np.zeros((self.n, 4, 4), dtype=LD)
        i, j, T, om = self.priv
        np.add.at(D, i, (T * om[:, None, :]) @ T.transpose(0, 2, 1))
        np.add.at(D, j, np.eye(4, dtype=LD) * om[:, None, :])
        i, T, om, _ = self.sh1
        np.add.at(D, i, (T * om[:, None, :]) @ T.transpose(0, 2, 1))
        j, T, om, _ = self.sh2
        np.add.at(D, j, np.eye(4, dtype=LD) * om[:, None, :])
        return D

    def precondition(self, X, V, block_jacobi=False):
        """P_X((Q + shift I)^-1 V) row by row (block_jacobi: the inverse of the 4 x 4 diagonal blocks of Q + shift I): an
        fp64 solve, then two refinement steps with the residual in long double.  Returns (value, Z, kappa_2, |P^-1|_2) with
        Z the unprojected solve."""
        n, r, s = self.n, self.r, self.shift
        if block_jacobi:
            D = self.block_diag_q() + s * np.eye(4, dtype=LD)
            D64 = D.astype(np.float64)

            def apply(Z):
                return Z @ D  # D symmetric

            def solve(Rh):
                return np.linalg.solve(D64, Rh.astype(np.float64).transpose(0, 2, 1)).transpose(0, 2, 1).astype(LD)
            ev = np.linalg.eigvalsh(D64)
        else:
            P = self.q_dense() + s * np.eye(4 * n)

            def apply(Z):
                return self.xq(Z)[0] + s * Z

            def solve(Rh):
                Rf = flat(Rh).reshape(4 * n, r)  # [(4 j + c), a]
                return blocks(np.linalg.solve(P, Rf).reshape(-1), r, n)
            ev = np.linalg.eigvalsh(P)
        Z = solve(V)
        for _ in range(2):
            Z = Z + solve(V - apply(Z))
        out, _ = tangent_project(X, Z)
        return out, Z, float(ev.max() / ev.min()), float(1.0 / ev.min())

    def public_pose_ids(self, nbr):
        m = self.m
        ids = np.r_[m["p1"][(m["r1"] == self.aid) & (m["r2"] == nbr)], m["p2"][(m["r2"] == self.aid) & (m["r1"] == nbr)]]
        return np.unique(ids.astype(np.int32))


# ----------------------------------------------------------------------------- manifold maps
def _inv3(M):
    """3 x 3 inverses by the adjugate, long double, batched"""
    a, b, c = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    d, e, f = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    g, h, i = M[..., 2, 0], M[..., 2, 1], M[..., 2, 2]
    A = np.stack([np.stack([e * i - f * h, c * h - b * i, b * f - c * e], -1),
                  np.stack([f * g - d * i, a * i - c * g, c * d - a * f], -1),
                  np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    det = a * A[..., 0, 0] + b * A[..., 1, 0] + c * A[..., 2, 0]
    return A / det[..., None, None]


def polar(X):
    """rotation blocks -> their polar factors Y (Y^T Y)^-1/2 (Denman-Beavers on the 3 x 3 Gram matrix, long double);
    translations unchanged.  Also returns cond(Y_i) per pose."""
    Y = X[:, :, :3]
    M = Y.transpose(0, 2, 1) @ Y
    sc = np.trace(M, axis1=1, axis2=2)[:, None, None] / 3
    A, Zi = M / sc, np.broadcast_to(np.eye(3, dtype=LD), M.shape).copy()
    for _ in range(60):
        A, Zi = 0.5 * (A + _inv3(Zi)), 0.5 * (Zi + _inv3(A))
    out = X.copy()
    out[:, :, :3] = Y @ (Zi / np.sqrt(sc))
    s = np.linalg.svd(Y.astype(np.float64), compute_uv=False)
    return out, s[:, 0] / s[:, -1]


def retract_qf(X, eta):
    """QF retraction: the Q factor (positive diagonal of R) of every rotation block of X + eta, long double (modified
    Gram-Schmidt, twice); translations X + eta.  Also returns cond(A_i) and the deviation |A^T A - I|_F^2 per pose."""
    A = X + eta
    Y = A[:, :, :3].copy()
    for _ in range(2):
        for j in range(3):
            for i in range(j):
                Y[:, :, j] -= np.sum(Y[:, :, i] * Y[:, :, j], axis=1)[:, None] * Y[:, :, i]
            Y[:, :, j] /= np.sqrt(np.sum(Y[:, :, j] * Y[:, :, j], axis=1))[:, None]
    out = A.copy()
    out[:, :, :3] = Y
    A64 = A[:, :, :3].astype(np.float64)
    s = np.linalg.svd(A64, compute_uv=False)
    dev = np.sum((A64.transpose(0, 2, 1) @ A64 - np.eye(3)) ** 2, axis=(1, 2))
    return out, s[:, 0] / s[:, -1], dev


# ----------------------------------------------------------------------------- team level
class Team:
    """the whole problem (every robot local), poses in team order: robot by robot, offsets off[robot]"""

    def __init__(self, m, sizes):
        self.sizes = list(sizes)
        self.off = np.r_[0, np.cumsum(self.sizes)].astype(int)
        self.N = int(self.off[-1])
        self.i = self.off[m["r1"].astype(int)] + m["p1"].astype(int)
        self.j = self.off[m["r2"].astype(int)] + m["p2"].astype(int)
        self.T, self.om = edge_arrays(m)

    def vq(self, V, Vm=None):
        """V Q_full for K x 4N blocks V (N, K, 4) (value, magnitude)"""
        Vm = np.abs(V) if Vm is None else Vm
        out, mag = np.zeros_like(V), np.zeros_like(V)
        i, j, T, om = self.i, self.j, self.T, self.om
        res = (V[j] - V[i] @ T) * om[:, None, :]
        resm = (Vm[j] + Vm[i] @ np.abs(T)) * om[:, None, :]
        np.add.at(out, j, res)
        np.add.at(out, i, -res @ T.transpose(0, 2, 1))
        np.add.at(mag, j, resm)
        np.add.at(mag, i, resm @ np.abs(T).transpose(0, 2, 1))
        return out, mag

    def certificate_apply(self, X, V):
        """S(X) V = V Q - V Lambda(X), Lambda_i = [[Sym(Y_i^T (X Q)_i,rot), 0], [0, 0]] (value, magnitude)"""
        E, Em = self.vq(X)
        Y, aY = X[:, :, :3], np.abs(X[:, :, :3])
        lam = _sym(Y.transpose(0, 2, 1) @ E[:, :, :3])
        lamm = _sym(aY.transpose(0, 2, 1) @ Em[:, :, :3])
        out, mag = self.vq(V)
        out[:, :, :3] -= V[:, :, :3] @ lam
        mag[:, :, :3] += np.abs(V[:, :, :3]) @ lamm
        return out, mag


def _mp(x):
    """a long double as an mpf, exactly (two fp64 parts)"""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(x) - LD(hi)))


def nearest_rotation(A):
    """the nearest rotation to a 3 x 3 block and its singular values, mpmath at 40 digits"""
    M = mpmath.matrix([[_mp(A[k][c]) for c in range(3)] for k in range(3)])
    U, S, Vt = mpmath.svd_r(M)
    d = mpmath.det(U * Vt)
    D = mpmath.diag([1, 1, 1 if d > 0 else -1])
    R = U * D * Vt
    return np.array([[float(R[k, c]) for c in range(3)] for k in range(3)]), np.array([float(S[k]) for k in range(3)])


def round_team(X, U=None, reflect=None):
    """SE-Sync rounding of the (N, r, 4) iterate: U = the top-3 eigenvectors of the Gram matrix of the rotation block
    (mpmath), the determinant vote (a tie keeps U), nearest rotations (mpmath) and anchoring at the first pose.  U or the
    vote may be given.  Returns (T flat 12 per pose, reflected, singular values of every block, Gram eigenvalues)."""
    N, r = X.shape[0], X.shape[1]
    Y = X[:, :, :3]
    if U is None:
        Gm = np.einsum("nac,nbc->ab", Y, Y)
        E, Q = mpmath.eigsy(mpmath.matrix([[_mp(Gm[a, b]) for b in range(r)] for a in range(r)]))
        ev = np.array([float(E[k]) for k in range(r)])
        order = np.argsort(-ev)[:3]
        U = np.array([[float(Q[a, k]) for k in order] for a in range(r)], dtype=LD)
        gram_ev = ev[np.argsort(-ev)]
    else:
        U, gram_ev = np.asarray(U, dtype=LD), None
    B = np.einsum("ak,nac->nkc", U, X)  # U^T [Y_i | p_i]
    dets = np.array([float(np.linalg.det(b[:, :3].astype(np.float64))) for b in B])
    if reflect is None:
        reflect = int((dets < 0).sum() > (dets > 0).sum())
    if reflect:
        B[:, 2, :] *= -1
    Rs, sv = np.zeros((N, 3, 3)), np.zeros((N, 3))
    for g in range(N):
        Rs[g], sv[g] = nearest_rotation(B[g, :, :3])
    t = B[:, :, 3]
    R0, t0 = Rs[0].astype(LD), t[0]
    Ra = np.einsum("mk,nmc->nkc", R0, Rs.astype(LD))
    ta = np.einsum("mk,nm->nk", R0, t - t0)
    T = np.concatenate([Ra.transpose(0, 2, 1).reshape(N, 9), ta], axis=1)
    return T.astype(np.float64).reshape(-1), reflect, sv, gram_ev

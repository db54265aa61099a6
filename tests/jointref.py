"""numpy statement of the joint gate of a set of candidate measurements, in longdouble by default, written from
the definitions and not from csrc/gate_joint.hip.

Conventions of tests/gateref.py.  K candidates, candidate k joining the team poses i_k != j_k; A the 6 K x 6 N matrix whose
row block k holds J_i^k at pose i_k and J_j^k at pose j_k; R the block diagonal of the Sigma_meas,k.
    M = A Sigma A^T + R;  block (k, l) = sum over a in {i_k, j_k}, b in {i_l, j_l} of J_a^k Sigma_ab J_b^l^T + delta_kl Sigma_meas,k,
    a block Sigma_ab that names pose 0 is zero, Sigma_ba = Sigma_ab^T;
    given an accepted set A:  xi_k|A = xi_k - M_kA M_AA^-1 xi_A,  S_k|A = M_kk - M_kA M_AA^-1 M_Ak,  d2_k|A = xi_k|A^T S_k|A^-1 xi_k|A,
    +inf where S_k|A has a non-positive pivot;
    greedy: the open candidate of smallest d2_k|A, the lower index on ties, accepted when d2 <= thr2, else stop;
    given:  k = 0 .. K - 1 in turn, accepted when d2_k|A <= thr2, else skipped;
    d2_joint = sum of the d2 at acceptance = xi_A^T M_AA^-1 xi_A,  logdet_joint = log det M_AA."""
import numpy as np

from tests import gateref as G

LD = np.longdouble
U = G.U


# ---- M from given blocks

def blocks_from_sigma(Sigma):
    """blk(a, b) = Sigma_ab of the full 6 (n - 1) square Sigma of the reduced problem; what names pose 0 is zero"""
    def blk(a, b):
        if a == 0 or b == 0:
            return np.zeros((6, 6))
        return Sigma[6 * (a - 1):6 * a, 6 * (b - 1):6 * b]
    return blk


def blocks_from_pairs(poses, diag, cross):
    """blk(a, b) from what a covariance call returns: diag[pose] and cross[q] = Sigma_ab for the q-th of the pairs a < b of the
    sorted poses (all_pairs below)"""
    where = {(int(a), int(b)): q for q, (a, b) in enumerate(all_pairs(poses))}

    def blk(a, b):
        if a == b:
            return diag[a]
        return cross[where[(a, b)]] if a < b else cross[where[(b, a)]].T
    return blk


def all_pairs(poses):
    """every unordered pair a < b of the sorted distinct poses, in sorted order"""
    p = sorted(set(int(x) for x in poses))
    return np.array([(p[a], p[b]) for a in range(len(p)) for b in range(a + 1, len(p))], dtype=np.int32).reshape(-1, 2)


def row_blocks(T, ends, dtype=LD):
    """[(i, J_i, j, J_j)] per candidate"""
    return [(int(i),) + (G.jacobians(T, int(i), int(j), dtype)[0],) + (int(j),) + (G.jacobians(T, int(i), int(j), dtype)[1],)
            for i, j in ends]


def joint_M(T, ends, kappa, tau, blk, dtype=LD):
    """M (6 K x 6 K) from the blocks blk(a, b); symmetric as the blocks are"""
    K = len(ends)
    rows = row_blocks(T, ends, dtype)
    M = np.zeros((6 * K, 6 * K), dtype=dtype)
    for k, (ik, Jik, jk, Jjk) in enumerate(rows):
        for l, (il, Jil, jl, Jjl) in enumerate(rows):
            B = np.zeros((6, 6), dtype=dtype)
            for a, Ja in ((ik, Jik), (jk, Jjk)):
                for b, Jb in ((il, Jil), (jl, Jjl)):
                    B += Ja @ np.asarray(blk(a, b), dtype=dtype) @ Jb.T
            if k == l:
                B += G.sigma_meas(kappa[k], tau[k], dtype)
            M[6 * k:6 * k + 6, 6 * l:6 * l + 6] = B
    return M


def joint_M_dense(T, ends, kappa, tau, blk, n, dtype=LD):
    """the same M as one product A Sigma A^T + R with the 6 n square Sigma of all n poses assembled from blk (the rows and
    columns of pose 0 zero), and beside it |A| |Sigma| |A|^T in float64 -- block (k, l) of which is the |J^k| |Sigma_kl| |J^l|^T
    of m_block_bound, since the two endpoints of a candidate differ"""
    K = len(ends)
    poses = sorted(set(int(x) for x in np.asarray(ends).reshape(-1)))
    S = np.zeros((6 * n, 6 * n), dtype=dtype)
    for a in poses:
        for b in poses:
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = np.asarray(blk(a, b), dtype=dtype)
    A = np.zeros((6 * K, 6 * n), dtype=dtype)
    for k, (i, Ji, j, Jj) in enumerate(row_blocks(T, ends, dtype)):
        A[6 * k:6 * k + 6, 6 * i:6 * i + 6], A[6 * k:6 * k + 6, 6 * j:6 * j + 6] = Ji, Jj
    M = A @ S @ A.T
    for k in range(K):
        M[6 * k:6 * k + 6, 6 * k:6 * k + 6] += G.sigma_meas(kappa[k], tau[k], dtype)
    Af = np.abs(np.asarray(A, dtype=np.float64))
    return M, 32 * U * (Af @ np.abs(np.asarray(S, dtype=np.float64)) @ Af.T)


def innovations(T, ends, Rm, tm, dtype=LD):
    return np.array([G.innovation(T, int(i), int(j), Rm[k], tm[k], dtype) for k, (i, j) in enumerate(ends)], dtype=dtype)


def a_matrix(T, ends, n, dtype=LD):
    """A restricted to the free poses 1 .. n - 1 (6 K x 6 (n - 1)): what multiplies the reduced Sigma"""
    A = np.zeros((6 * len(ends), 6 * (n - 1)), dtype=dtype)
    for k, (i, Ji, j, Jj) in enumerate(row_blocks(T, ends, dtype)):
        for p, J in ((i, Ji), (j, Jj)):
            if p > 0:
                A[6 * k:6 * k + 6, 6 * (p - 1):6 * p] += J
    return A


# ---- the elimination under a given pivot order

def _chol6(S):
    """batched Cholesky of S[K, 6, 6] (numpy's LAPACK takes no longdouble): (L, ok[K])"""
    L = np.zeros_like(S)
    ok = np.ones(len(S), dtype=bool)
    for c in range(6):
        p = S[:, c, c] - np.einsum("kq,kq->k", L[:, c, :c], L[:, c, :c])
        ok &= p > 0
        d = np.sqrt(np.where(p > 0, p, 1))
        L[:, c, c] = d
        for r in range(c + 1, 6):
            L[:, r, c] = (S[:, r, c] - np.einsum("kq,kq->k", L[:, r, :c], L[:, c, :c])) / d
    return L, ok


def _forward(L, x):
    """y = L^-1 x, batched"""
    y = np.zeros_like(x)
    for c in range(6):
        y[:, c] = (x[:, c] - np.einsum("kq,kq->k", L[:, c, :c], y[:, :c])) / L[:, c, c]
    return y


class Elimination:
    """Left-looking block Cholesky of M in the order the pivots are taken.  D[k], x[k]: S_k|A and xi_k|A of every candidate
    that is still open; mag_x, mag_D: the sums of the absolute values of the terms they were formed from (the magnitudes the
    error bounds multiply)."""

    def __init__(self, M, xi, dtype=LD):
        self.M = np.asarray(M, dtype=dtype)
        self.K = len(self.M) // 6
        K = self.K
        self.x = np.asarray(xi, dtype=dtype).reshape(K, 6).copy()
        self.D = np.array([self.M[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(K)], dtype=dtype)
        self.mag_x, self.mag_D = np.abs(self.x), np.abs(self.D)
        self.W = np.zeros((6 * K, 0), dtype=dtype)
        self.open = np.ones(K, dtype=bool)
        self.accepted, self.d2_at, self.logdet = [], [], dtype(0)
        self.dtype = dtype

    def d2(self):
        """d2_k|A of every candidate (meaningful where open); +inf for a non-positive pivot"""
        L, ok = _chol6(self.D)
        y = _forward(L, self.x)
        return np.where(ok, np.einsum("kc,kc->k", y, y), self.dtype(np.inf))

    def close(self, k):
        self.open[k] = False

    def pivot(self, p):
        """accept p: every open candidate is conditioned on it"""
        K = self.K
        L, ok = _chol6(self.D[p:p + 1])
        assert ok[0], "the pivot's block is not positive definite"
        L = L[0]
        y = _forward(L[None], self.x[p:p + 1])[0]
        self.accepted.append(int(p))
        self.d2_at.append(y @ y)
        self.logdet = self.logdet + 2 * np.sum(np.log(np.diag(L)))
        self.open[p] = False
        Gm = self.M[:, 6 * p:6 * p + 6] - self.W @ self.W[6 * p:6 * p + 6, :].T
        Wn = np.zeros_like(Gm)
        for c in range(6):  # w L^T = g
            Wn[:, c] = (Gm[:, c] - Wn[:, :c] @ L[c, :c]) / L[c, c]
        self.W = np.c_[self.W, Wn]
        Wb = Wn.reshape(K, 6, 6)
        o = self.open
        self.x[o] -= Wb[o] @ y
        self.D[o] -= Wb[o] @ Wb[o].transpose(0, 2, 1)
        self.mag_x[o] += np.abs(Wb[o]) @ np.abs(y)
        self.mag_D[o] += np.abs(Wb[o]) @ np.abs(Wb[o]).transpose(0, 2, 1)


def argmin_lower_index(d2, open_mask):
    """the open candidate of smallest d2, the lower index on ties; -1 when none is open"""
    idx = np.flatnonzero(open_mask)
    if not len(idx):
        return -1
    return int(idx[np.argmin(d2[idx])])  # (argmin returns the first of equal values)


def run(M, xi, thr2, order="greedy", pivots=None, dtype=LD):
    """Both selection rules, or (pivots given) the replay of a recorded order of acceptance under the same rule: at every
    step the recorded pivot is taken in the place of the rule's own choice, and the rule's choice is kept beside it.
    Returns a dict: accept[K], rank[K], accepted, xi_cond[K, 6], d2_cond[K] (at the moment k was decided; greedy's rejected:
    given the final set), d2_joint, logdet_joint, and steps: one record per decision with
        k (the candidate decided), n_acc (|A| before), d2 (of all K given A), open (mask before), choice (the rule's own
        candidate), near (the up to four open candidates of smallest d2), stop (greedy: this step rejects all that is left), rows
        (for k, choice and near, at the stop for every open candidate: mag_x, mag_D, S, x, d2 in float64)."""
    E = Elimination(M, xi, dtype)
    K = E.K
    rank = np.full(K, -1)
    xi_cond, d2_cond = np.zeros((K, 6), dtype=dtype), np.zeros(K, dtype=dtype)
    steps = []

    def record(k, d2, choice, every_open=False):
        idx = np.flatnonzero(E.open)
        near = idx[np.argsort(d2[idx], kind="stable")[:4]]  # the smallest among the open ones
        rows = {int(r): dict(mag_x=np.asarray(E.mag_x[r], dtype=np.float64), mag_D=np.asarray(E.mag_D[r], dtype=np.float64),
                             S=np.asarray(E.D[r], dtype=np.float64), x=np.asarray(E.x[r], dtype=np.float64), d2=float(d2[r]))
                for r in set([int(k), int(choice)] + [int(r) for r in (idx if every_open else near)])}
        steps.append(dict(k=int(k), n_acc=len(E.accepted), d2=d2.copy(), open=E.open.copy(), choice=int(choice),
                          near=[int(r) for r in near], rows=rows, stop=every_open))

    if order == "greedy":
        s = 0
        while E.open.any():
            d2 = E.d2()
            choice = argmin_lower_index(d2, E.open)
            k = choice if pivots is None else (int(pivots[s]) if s < len(pivots) else choice)
            stop = not d2[k] <= thr2 if pivots is None else s >= len(pivots)
            record(k, d2, choice, every_open=stop)
            if stop:
                break
            xi_cond[k], d2_cond[k], rank[k] = E.x[k], d2[k], s
            E.pivot(k)
            s += 1
        rest = E.open.copy()
        if rest.any():
            d2 = E.d2()
            xi_cond[rest], d2_cond[rest] = E.x[rest], d2[rest]
    elif order == "given":
        taken = None if pivots is None else set(int(p) for p in pivots)
        for k in range(K):
            d2 = E.d2()
            record(k, d2, k)
            xi_cond[k], d2_cond[k] = E.x[k], d2[k]
            if (d2[k] <= thr2) if taken is None else (k in taken):
                rank[k] = len(E.accepted)
                E.pivot(k)
            else:
                E.close(k)
    else:
        raise ValueError(order)
    return dict(accept=rank >= 0, rank=rank, accepted=np.array(E.accepted, dtype=int), xi_cond=xi_cond, d2_cond=d2_cond,
                d2_joint=sum(E.d2_at, dtype(0)), logdet_joint=E.logdet, steps=steps)


# ---- the error bounds the tests hold csrc/gate_joint.hip to; u = 2.2e-16.  tests/test_jointref.py shows that each of them
# rejects the mistakes the conventions invite.

def m_block_bound(T, ik, jk, il, jl, blk):
    """elementwise on the block (k, l) of M: 32 u |J^k| |Sigma_kl| |J^l|^T with J^k = [J_i^k J_j^k] and Sigma_kl the 12 x 12
    cross block of the two endpoint sets -- gateref.sigma_rel_bound carried to off-diagonal blocks: two 12-term products,
    gamma_24 and a third over"""
    Jk = np.abs(np.c_[G.jacobians(T, ik, jk, np.float64)])
    Jl = np.abs(np.c_[G.jacobians(T, il, jl, np.float64)])
    S = np.abs(np.block([[np.asarray(blk(a, b), dtype=np.float64) for b in (il, jl)] for a in (ik, jk)]))
    return 32 * U * (Jk @ S @ Jl.T)


def elimination_constant(n_acc):
    """c of the elimination bound c u cond_2(M_AA) x magnitude, from the operation count of |A| = n_acc block steps, as the
    gamma-constants of gateref.py are derived.  An entry of row k of the factor's column q is an accumulation of 6 q products
    and a 6-term substitution against the pivot's factor; xi_k|A and S_k|A are then one more accumulation of 6 |A| products
    of those entries.  Two accumulations in a row of at most 6 (|A| + 1) terms each: gamma_{12 (|A| + 1)}, and a third over:
    c = 16 (|A| + 1).  The entries of the factor carry the relative error of a Cholesky factor, which the condition number
    of what has been factored -- M_AA -- multiplies.  With A empty nothing has been eliminated and the term stands for the
    rounding of the inputs alone."""
    return 16 * (n_acc + 1)


def prefix_conditions(M, accepted, every=1):
    """cond_2(M_AA) of the prefixes A = accepted[:a], a = 0 .. len(accepted) (1 for the empty set).  every > 1: computed at
    every `every`-th prefix and at those up to `every`, the last computed value standing for the ones behind it -- by
    interlacing the condition number of a principal submatrix is no larger, so the stand-in only tightens the bound."""
    M = np.asarray(M, dtype=np.float64)
    out, last = np.ones(len(accepted) + 1), 1.0
    for a in range(1, len(accepted) + 1):
        if a <= every or a % every == 0:
            idx = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in accepted[:a]])
            w = np.linalg.eigvalsh(M[np.ix_(idx, idx)])
            last = w[-1] / w[0]
        out[a] = last
    return out


def conditional_bounds(step, cond_A, k=None):
    """(b_xi[6], b_d2) for candidate k of a step's rows (None: the one it decides), given cond_A = cond_2(M_AA): e = c u cond_A;
    the innovation within e x mag_x elementwise, the block within e x mag_D, both carried through d2 = xi^T S^-1 xi by
    gateref.d2_bound, which adds 100 u cond_2(S) d2 for the 6 x 6 solve itself"""
    row = step["rows"][step["k"] if k is None else int(k)]
    e = elimination_constant(step["n_acc"]) * U * cond_A
    b_x, b_S = e * row["mag_x"], e * row["mag_D"]
    if not np.isfinite(row["d2"]):
        return b_x, np.inf
    return b_x, G.d2_bound(row["x"], row["S"], row["d2"], b_x, b_S)


# ---- seeded batches of candidates

def seeded_batch(T, n, K, seed, outliers=0.3, kappa=100.0, tau=50.0, fixed=()):
    """K candidates on seeded pairs of the n poses of T: ends[K, 2], Rm[K, 3, 3], tm[K, 3], kappa[K], tau[K], inlier[K].
    The first len(fixed) pairs are `fixed`.  A candidate is the relative pose of T with noise drawn from its own noise model,
    rotation N(0, I / (2 kappa)) as a rotation vector on the right and translation N(0, I / tau); an outlier (probability
    `outliers`) is off by 0.3 rad about a seeded axis and 0.3 m along a seeded direction on top of that."""
    rng = np.random.default_rng(seed)
    ends = [tuple(p) for p in fixed]
    while len(ends) < K:
        i, j = rng.integers(0, n, 2)
        if i != j:
            ends.append((int(i), int(j)))
    ends = np.array(ends[:K], dtype=np.int64)
    Rm, tm = np.zeros((K, 3, 3)), np.zeros((K, 3))
    kap, ta = kappa * rng.uniform(0.5, 2.0, K), tau * rng.uniform(0.5, 2.0, K)
    inlier = rng.uniform(size=K) >= outliers
    for k, (i, j) in enumerate(ends):
        Rij, tij = G.relative_pose(T, int(i), int(j), np.float64)
        w = rng.standard_normal(3) / np.sqrt(2 * kap[k])
        d = rng.standard_normal(3) / np.sqrt(ta[k])
        if not inlier[k]:
            a, b = rng.standard_normal(3), rng.standard_normal(3)
            w = w + 0.3 * a / np.linalg.norm(a)
            d = d + 0.3 * b / np.linalg.norm(b)
        Rm[k], tm[k] = Rij @ _exp_so3(w), tij + d
    return ends, Rm, tm, kap, ta, inlier


def _exp_so3(w):
    th = np.linalg.norm(w)
    Kx = np.asarray(G.skew(w, np.float64))
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx

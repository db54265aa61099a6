"""numpy statement of the first-order removal or down-weighting of measurements that are in the graph, in
longdouble by default, written from the definitions and not from csrc/linear_removal.hip.

Conventions of tests/gateref.py, tests/jointref.py and tests/updateref.py.  K records, record k joining the poses i_k != j_k of
the n poses, in the weighted graph at weight w_k > 0 and going to w'_k with 0 <= w'_k < w_k; T a minimum of that graph.
dw_k = w_k - w'_k, R the block diagonal of the Sigma_meas,k / dw_k, A and B = Sigma A^T the update's.
    H' = H - A^T R^-1 A,  N = R - A B,  Sigma' = Sigma + B N^-1 B^T,  dx = +B N^-1 xi,  T' = T [+] dx,
    xi_loo = xi + A dx = R N^-1 xi,  d2_joint = xi^T N^-1 xi,  log det H' - log det H = log det N - log det R.
Whitened: s_k = (sqrt(2 kappa_k dw_k) x 3, sqrt(tau_k dw_k) x 3), D = diag(s), R = D^-2,
    B~ = B D,  xi~ = D xi,  N~ = D N D = I - (D A) B~,  G~ = N~^-1,  z~ = G~ xi~,  U~ = B~ G~,
    dx = B~ z~,  Sigma'_pq = Sigma_pq + U~_p B~_q^T,  xi_loo = z~ / s,  d2_joint = xi~^T z~,
    logdet_R = sum_k -3 log(2 kappa_k) - 3 log tau_k - 6 log dw_k,  logdet_N = log det N~ + logdet_R,
    pivot_min_k the smallest Cholesky pivot of the block (k, k) of N~ (the audit's at weight dw_k), pivot_min_joint the smallest
    pivot of the Cholesky factor of N~.
The information form of the same removal: Sigma' = (H_red - A^T R^-1 A)^-1, dx = +Sigma' A^T R^-1 xi."""
import numpy as np

from tests import auditref as AR
from tests import gateref as G
from tests import jointref as J
from tests import updateref as R

LD = np.longdouble
U = G.U
F = np.float64

MISTAKES = ("dx_sign", "sigma_minus", "dw_as_w", "logdet_dw_left_out", "n_plus", "scaled_once")


def scales(kappa, tau, dw, dtype=LD):
    """s, 6 K: (sqrt(2 kappa_k dw_k) x 3, sqrt(tau_k dw_k) x 3) per record"""
    return np.concatenate([np.r_[np.full(3, np.sqrt(2 * dtype(kappa[k]) * dtype(dw[k]))), np.full(3, np.sqrt(dtype(tau[k]) * dtype(dw[k])))]
                           for k in range(len(kappa))]).astype(dtype)


def pivots(M):
    """the pivots of the Cholesky factorisation of M before the square root, up to and with the first that is not positive"""
    M = np.asarray(M)
    n = len(M)
    L = np.zeros_like(M)
    out = []
    for c in range(n):
        p = M[c, c] - L[c, :c] @ L[c, :c]
        out.append(p)
        if not p > 0:
            break
        L[c, c] = np.sqrt(p)
        L[c + 1:, c] = (M[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return np.array(out, dtype=M.dtype)


def removal(T, ends, Rm, tm, kappa, tau, w, w_new, blocks, n, pairs=(), dtype=LD, mistake=None):
    """the removal from given blocks; a dict of everything formed on the way.  w_new None: all zero.  mistake: one of MISTAKES,
    the planted mistakes of tests/test_removalref.py (None: the definitions).  A set without redundancy (a pivot of N~ that is
    not positive) gives the dict up to pivot_min_joint, with testable False."""
    K = len(ends)
    w = np.asarray(w, dtype=dtype).reshape(K)
    wn = np.zeros(K, dtype=dtype) if w_new is None else np.asarray(w_new, dtype=dtype).reshape(K)
    dw = w - wn
    assert (w > 0).all() and (wn >= 0).all() and (dw > 0).all()
    if mistake == "dw_as_w":
        dw = w.copy()
    A = R.a_full(T, ends, n, dtype)
    S = R.sigma_columns(ends, blocks, n, dtype)
    B = S @ A.T
    s = scales(kappa, tau, dw, dtype)
    Bt = B * s[None, :]
    AB = (A if mistake == "scaled_once" else s[:, None] * A) @ Bt
    Nt = np.eye(6 * K, dtype=dtype) + AB if mistake == "n_plus" else np.eye(6 * K, dtype=dtype) - AB
    Nt = (Nt + Nt.T) / 2
    xi = np.asarray(J.innovations(T, ends, Rm, tm, dtype), dtype=dtype).reshape(-1)
    xit = s * xi
    pivot_min = np.array([AR.cholesky(Nt[6 * k:6 * k + 6, 6 * k:6 * k + 6], 0, dtype)[1] for k in range(K)], dtype=dtype)
    pj = pivots(Nt).min()
    logdet_R = sum((-3 * np.log(2 * dtype(kappa[k])) - 3 * np.log(dtype(tau[k])) - (0 if mistake == "logdet_dw_left_out" else 6 * np.log(dw[k]))
                    for k in range(K)), dtype(0))
    out = dict(A=A, S=S, B=B, s=s, dw=dw, Bt=Bt, Nt=Nt, xi=xi.reshape(K, 6), xit=xit, pivot_min=pivot_min, pivot_min_joint=pj,
               logdet_R=logdet_R, testable=bool(pj > 0), kappa=np.asarray(kappa, dtype=F), tau=np.asarray(tau, dtype=F))
    if not pj > 0:
        return out
    Gt, logdet_Nt = R.spd_inverse(Nt)
    zt = Gt @ xit
    Ut = Bt @ Gt
    sign = -1 if mistake == "dx_sign" else 1
    dx = sign * (Bt @ zt)
    ssig = -1 if mistake == "sigma_minus" else 1
    rows = lambda p: slice(6 * p, 6 * p + 6)
    diag = np.zeros((n, 6, 6), dtype=dtype)
    for p in range(n):
        D = np.asarray(blocks.diag(p), dtype=dtype) + ssig * (Ut[rows(p)] @ Bt[rows(p)].T)
        diag[p] = (D + D.T) / 2
    cross = np.array([np.asarray(blocks.pair(q), dtype=dtype) + ssig * (Ut[rows(int(a))] @ Bt[rows(int(b))].T) for q, (a, b) in enumerate(pairs)],
                     dtype=dtype).reshape(-1, 6, 6)
    out.update(G=Gt, z=zt, U=Ut, delta=dx.reshape(n, 6), xi_loo=(zt / s).reshape(K, 6), cov_diag=diag, cov_pairs=cross, T=R.retract(T, dx, dtype),
               d2_joint=xit @ zt, logdet_Nt=logdet_Nt, logdet_N=logdet_Nt + logdet_R, information_loss=-logdet_Nt / 2)
    return out


def core(A, Sigma, s, xi, dtype=LD):
    """the whitened algebra alone, on any linear(ised) graph: A (6 K x d) the rows of the records, Sigma (d x d) the covariance
    of the estimate, s (6 K) with R^-1 = diag(s)^2, xi (6 K) the residuals.  A dict: Sigma' (full), dx, xi_loo, d2_joint,
    logdet_Nt, Nt, pivot_min_joint"""
    A, Sigma, s, xi = (np.asarray(a, dtype=dtype) for a in (A, Sigma, s, xi))
    Bt = (Sigma @ A.T) * s[None, :]
    Nt = np.eye(len(s), dtype=dtype) - (s[:, None] * A) @ Bt
    Nt = (Nt + Nt.T) / 2
    Gt, ld = R.spd_inverse(Nt)
    zt = Gt @ (s * xi)
    Sp = Sigma + Bt @ Gt @ Bt.T
    return dict(Sigma=(Sp + Sp.T) / 2, dx=Bt @ zt, xi_loo=zt / s, d2_joint=(s * xi) @ zt, logdet_Nt=ld, Nt=Nt, pivot_min_joint=pivots(Nt).min())


def connected(n, edges):
    """whether the graph of the n nodes and the edges (i, j) is connected"""
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for i, j in edges:
        root[find(int(i))] = find(int(j))
    return len(set(find(a) for a in range(n))) == 1


def cut_triple(m, n):
    """the first (c1, o, c2) in index order -- two closures c1 < c2 and one odometry edge o of the measurements m on n poses --
    none of which is a bridge and no two of which cut the graph, but which cut it together: two closures around one loop and
    the odometry edge between them.  None when there is none."""
    e = [(int(a["p1"]), int(a["p2"])) for a in m]
    odo = [k for k, (i, j) in enumerate(e) if abs(i - j) == 1]
    clo = [k for k, (i, j) in enumerate(e) if abs(i - j) != 1]
    without = lambda drop: connected(n, [e[k] for k in range(len(e)) if k not in drop])
    for a, c1 in enumerate(clo):
        for c2 in clo[a + 1:]:
            for o in odo:
                if (not without((c1, o, c2)) and without((c1, o)) and without((c2, o)) and without((c1, c2))):
                    return c1, o, c2
    return None


def information_form(Hr, T, ends, kappa, tau, dw, xi, n):
    """(Sigma', dx, H') = ((H_red - A^T R^-1 A)^-1, +Sigma' A^T R^-1 xi, H') in float64, R^-1 = diag(s)^2; dx of the free poses
    1 .. n - 1"""
    A = np.asarray(J.a_matrix(T, ends, n), dtype=F)
    Ri = np.asarray(scales(kappa, tau, dw), dtype=F) ** 2
    Hp = Hr - A.T @ (Ri[:, None] * A)
    Hp = 0.5 * (Hp + Hp.T)
    Sp = np.linalg.inv(Hp)
    Sp = 0.5 * (Sp + Sp.T)
    return Sp, Sp @ (A.T @ (Ri * np.asarray(xi, dtype=F).reshape(-1))), Hp


# ---- the error bounds the tests hold csrc/linear_removal.hip to; u = 2.2e-16, elementwise unless said otherwise.
# tests/test_removalref.py shows that they reject the mistakes the conventions invite.  Every constant is updateref's or
# auditref's; what the scaling adds is counted here.
#
# s.  One product 2 kappa dw (or tau dw) of a difference dw = w - w' that is itself rounded, and one square root: three
# roundings, of which the square root halves the two in front of it: |s - ref| <= 2 u s.
# B~ and N~, in front of the inverse.  B~ = B D is updateref's B (|B - ref| <= 24 u |Sigma| |A|^T) times s, one more product
# with an operand that carries 2 u:
#     |B~ - ref| <= (b_B + 3 u |B|) s^T                                 column c scaled by s_c
# An element of (D A) B~ is updateref's 12-term sum J[a][y] B~[y][c] (24 u |A| |B~| + |A| b_B~) times s_k, one more product with an
# operand that carries 2 u; the subtraction from the identity and the symmetrisation are two more roundings of a figure that
# is at most 1 + |D A B~| in size:
#     |N~ - ref| <= s o (24 u |A| |B~| + |A| b_B~) + 3 u |D A| |B~| + 2 u (I + |D A| |B~|)
#     xi~        s o b_xi + 3 u |xi~|                                    b_xi = gateref.xi_bound
# Everything behind G~, as in updateref with N~ in M's place: e = 16 (K + 1) u cond_2(N~) times the sum of the absolute values
# of the terms, the errors of the inputs carried to first order (delta G~ = -G~ delta N~ G~):
#     z~         e |G~| |xi~| + |G~| (b_N |z~| + b_xi~)
#     U~         e |B~| |G~| + b_B~ |G~| + |B~| |G~| b_N |G~|
#     dx         e |B~| |z~| + b_B~ |z~| + |B~| b_z
#     xi_loo     b_z / s + 4 u |xi_loo|                                  one division by an s that carries 2 u
#     Sigma'     e |U~_p| |B~_q|^T + b_U,p |B~_q|^T + |U~_p| b_B~,q^T + 2 u |Sigma'_pq|; a diagonal block: the larger of the bound
#                and its transpose
#     d2_joint   e |xi~|^T |z~| + |xi~|^T b_z + b_xi~^T |z~|
#     logdet_N   updateref's logdet_M for N~ -- sum(|G~| o (b_N + 8 K u |L| |L|^T)) + 8 K u sum |log L_kk^2| + 16 u 6 K -- plus
#                logdet_R's own bound and 2 u (|log det N~| + |logdet_R|) for the sum
#     logdet_R   updateref's (2 K + 8) u sum_k over the 3 + 3 + 6 logarithms of a record; the argument dw of the last carries
#                one rounding, which moves its logarithm by u whatever its size: + 6 K u
#     T'         updateref's
#     pivot_min  auditref's pivot bound on the block (k, k) of N~ with b_A = its block of b_N
#     pivot_min_joint  the same perturbation argument for the whole factor: the pivot c moves by h^T dN h with
#                h = (-N_{c-1}^-1 n_c, 1), the computed factor is the exact factor of N~ + dN' with |dN'| <= 8 K u |L| |L|^T (the
#                gamma_{6 K + 1} updateref uses for logdet_M): max_c 2 |h|^T (b_N + 8 K u |L| |L|^T) |h|

def bounds(ref, T, ends, tm, n, pairs=()):
    """the bounds above for a reference removal (a dict of removal()), in float64: a dict with the keys of the outputs and of
    Bt, Nt"""
    K = len(ends)
    f = lambda a: np.abs(np.asarray(a, dtype=F))
    A, S, B, Bt, Gm, Um = f(ref["A"]), f(ref["S"]), f(ref["B"]), f(ref["Bt"]), f(ref["G"]), f(ref["U"])
    Nt = np.asarray(ref["Nt"], dtype=F)
    s, xit, z = np.asarray(ref["s"], dtype=F), f(ref["xit"]), f(ref["z"])
    DA = s[:, None] * A
    b_B = (24 * U * (S @ A.T) + 3 * U * B) * s[None, :]
    b_N = s[:, None] * (24 * U * (A @ Bt) + A @ b_B) + 3 * U * (DA @ Bt) + 2 * U * (np.eye(6 * K) + DA @ Bt)
    b_N = np.maximum(b_N, b_N.T)  # (a block may be formed as the transpose of its mirror image)
    b_xi = np.array([G.xi_bound(T, int(i), int(j), tm[k]) for k, (i, j) in enumerate(ends)]).reshape(-1)
    b_xit = s * b_xi + 3 * U * xit
    w = np.linalg.eigvalsh(Nt)
    cond = w[-1] / w[0]
    e = 16 * (K + 1) * U * cond
    b_z = e * (Gm @ xit) + Gm @ (b_N @ z + b_xit)
    b_U = e * (Bt @ Gm) + b_B @ Gm + Bt @ (Gm @ b_N @ Gm)
    b_dx = (e * (Bt @ z) + b_B @ z + Bt @ b_z).reshape(n, 6)
    rows = lambda p: slice(6 * p, 6 * p + 6)

    def sig(p, q, Spq):
        return e * (Um[rows(p)] @ Bt[rows(q)].T) + b_U[rows(p)] @ Bt[rows(q)].T + Um[rows(p)] @ b_B[rows(q)].T + 2 * U * f(Spq)

    b_diag = np.array([np.maximum(sig(p, p, ref["cov_diag"][p]), sig(p, p, ref["cov_diag"][p]).T) for p in range(n)])
    b_pairs = np.array([sig(int(a), int(b), ref["cov_pairs"][q]) for q, (a, b) in enumerate(pairs)]).reshape(-1, 6, 6)
    L = np.abs(np.linalg.cholesky(Nt))
    LL = 8 * K * U * (L @ L.T)
    kap, ta, dw = np.asarray(ref["kappa"], dtype=F), np.asarray(ref["tau"], dtype=F), np.asarray(ref["dw"], dtype=F)
    b_ldR = (2 * K + 8) * U * float(np.sum(3 * np.abs(np.log(2 * kap)) + 3 * np.abs(np.log(ta)) + 6 * np.abs(np.log(dw)))) + 6 * K * U
    b_ldN = (np.sum(Gm * (b_N + LL)) + 8 * K * U * np.sum(np.abs(2 * np.log(np.diag(L)))) + 16 * U * 6 * K + b_ldR
             + 2 * U * (abs(float(ref["logdet_Nt"])) + abs(float(ref["logdet_R"]))))
    # the pivots: every record's own block, and the whole factor
    b_pm = np.zeros(K)
    for k in range(K):
        blk = slice(6 * k, 6 * k + 6)
        Ak = Nt[blk, blk]
        Lk = np.abs(np.linalg.cholesky(Ak))
        dA = b_N[blk, blk] + 8 * U * (Lk @ Lk.T)
        for c in range(6):
            h = np.r_[-np.linalg.solve(Ak[:c, :c], Ak[:c, c]), 1.0] if c else np.ones(1)
            b_pm[k] = max(b_pm[k], 2 * (np.abs(h) @ dA[:c + 1, :c + 1] @ np.abs(h)))
    dN = b_N + LL
    Lf = np.linalg.cholesky(Nt)
    b_pj = 0.0
    for c in range(6 * K):
        # h = (-N_{c-1}^-1 n_c, 1) through the leading factor: N_{c-1}^-1 n_c = L^-T (L^-1 n_c)
        h = np.r_[-np.linalg.solve(Lf[:c, :c].T, np.linalg.solve(Lf[:c, :c], Nt[:c, c])), 1.0] if c else np.ones(1)
        b_pj = max(b_pj, 2 * (np.abs(h) @ dN[:c + 1, :c + 1] @ np.abs(h)))
    Tn = np.asarray(ref["T"], dtype=F).reshape(n, 4, 3)
    b_T = np.zeros((n, 4, 3))
    b_T[:, :3, :] = (np.sqrt(3.0) * (2 * b_dx[:, :3].max(axis=1) + 16 * U))[:, None, None]
    b_T[:, 3, :] = b_dx[:, 3:] + 2 * U * np.abs(Tn[:, 3, :])
    return dict(Bt=b_B, Nt=b_N, xi=b_xi.reshape(K, 6), xit=b_xit, z=b_z, delta=b_dx,
                xi_loo=(b_z / s + 4 * U * f(ref["xi_loo"]).reshape(-1)).reshape(K, 6), cov_diag=b_diag, cov_pairs=b_pairs,
                d2_joint=e * (xit @ z) + xit @ b_z + b_xit @ z, logdet_N=b_ldN, logdet_R=b_ldR, pivot_min=b_pm, pivot_min_joint=b_pj,
                T=b_T.reshape(-1), cond_N=cond, e=e)


ratio = R.ratio

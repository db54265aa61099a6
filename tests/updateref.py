"""numpy statement of the first-order update of a trajectory and its covariances for a set of new closures, in
longdouble by default, written from the definitions and not from csrc/linear_update.hip.

Conventions of tests/gateref.py and tests/jointref.py.  K closures, closure k joining the poses i_k != j_k of the n poses; A
the 6 K x 6 n matrix whose row block k holds J_i^k at pose i_k and J_j^k at pose j_k; R the block diagonal of the Sigma_meas,k;
a block Sigma_ab that names pose 0 is zero.
    B = Sigma A^T (6 n x 6 K; B_0 = 0),  M = A B + R,  G = M^-1,  z = G xi,  U = B G,
    dx = -B z,  xi_post = R z = xi + A dx,  Sigma'_pq = Sigma_pq - U_p B_q^T,  T'_p = (R_p Exp(phi_p), t_p + delta_p),
    d2_joint = xi^T z,  logdet_M = log det M,  logdet_R = sum_k -3 log(2 kappa_k) - 3 log tau_k.
The information form of the same update: Sigma' = (H_red + A^T R^-1 A)^-1, dx = -Sigma' A^T R^-1 xi."""
import numpy as np

from tests import gateref as G
from tests import jointref as J

LD = np.longdouble
U = G.U
F = np.float64


# ---- the blocks of Sigma an update reads: sigma(p, e) = Sigma_{p,e} for an endpoint e, diag(p) = Sigma_pp, pair(q) = the q-th
# requested pair block

class Blocks:
    def __init__(self, sigma, diag, pair):
        self.sigma, self.diag, self.pair = sigma, diag, pair


def blocks_from_sigma(Sigma, pairs=()):
    """from the full 6 (n - 1) square Sigma of the reduced problem"""
    blk = J.blocks_from_sigma(Sigma)
    pr = [(int(a), int(b)) for a, b in pairs]
    return Blocks(blk, lambda p: blk(p, p), lambda q: blk(*pr[q]))


def rect_pairs(poses, n):
    """the rectangular set an update asks of the covariance path: for each endpoint rank a and each pose p the pair (p, e_a),
    block number a n + p"""
    e = sorted(set(int(x) for x in poses))
    return np.array([(p, ea) for ea in e for p in range(n)], dtype=np.int32).reshape(-1, 2)


def blocks_from_rect(poses, n, diag, cross):
    """from what a covariance call returns for rect_pairs(poses, n) with the requested pairs appended: the rectangular
    analogue of jointref.blocks_from_pairs"""
    e = sorted(set(int(x) for x in poses))
    rank = {ea: a for a, ea in enumerate(e)}
    return Blocks(lambda p, ea: cross[rank[int(ea)] * n + int(p)], lambda p: diag[int(p)], lambda q: cross[len(e) * n + q])


# ---- longdouble linear algebra (numpy's LAPACK wrappers take no longdouble)

def cholesky(M):
    M = np.asarray(M)
    n = len(M)
    L = np.zeros_like(M)
    for c in range(n):
        p = M[c, c] - L[c, :c] @ L[c, :c]
        assert p > 0, "not positive definite at row %d" % c
        L[c, c] = np.sqrt(p)
        L[c + 1:, c] = (M[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return L


def spd_inverse(M):
    """(M^-1, log det M) of a symmetric positive definite M through its Cholesky factor"""
    L = cholesky(M)
    n = len(L)
    Li = np.zeros_like(L)
    I = np.eye(n, dtype=L.dtype)
    for r in range(n):
        Li[r] = (I[r] - L[r, :r] @ Li[:r]) / L[r, r]
    return Li.T @ Li, 2 * np.sum(np.log(np.diag(L)))


def exp_so3(w, dtype=LD):
    w = np.asarray(w, dtype=dtype)
    th = np.sqrt(w @ w)
    K = G.skew(w, dtype)
    if th < 1e-6:
        return np.eye(3, dtype=dtype) + K + K @ K / 2
    return np.eye(3, dtype=dtype) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def retract(T, dx, dtype=LD, translation_in_body_frame=False):
    """T [+] dx: R_p <- R_p Exp(phi_p), t_p <- t_p + delta_p (the world frame); flat, the layout of T"""
    P = np.array(T, dtype=dtype).reshape(-1, 4, 3)
    X = np.asarray(dx, dtype=dtype).reshape(-1, 6)
    for g in range(len(P)):
        R = P[g, :3, :].T
        P[g, 3, :] += R @ X[g, 3:] if translation_in_body_frame else X[g, 3:]  # (the mistake of test_updateref)
        P[g, :3, :] = (R @ exp_so3(X[g, :3], dtype)).T
    return P.reshape(-1)


def a_full(T, ends, n, dtype=LD, swap=False):
    """A with the columns of all n poses (pose 0 included: what multiplies it is zero)"""
    A = np.zeros((6 * len(ends), 6 * n), dtype=dtype)
    for k, (i, Ji, j, Jj) in enumerate(J.row_blocks(T, ends, dtype)):
        if swap:
            Ji, Jj = Jj, Ji
        A[6 * k:6 * k + 6, 6 * i:6 * i + 6], A[6 * k:6 * k + 6, 6 * j:6 * j + 6] = Ji, Jj
    return A


def r_diagonal(kappa, tau, dtype=LD):
    """the diagonal of R"""
    return np.concatenate([np.diag(G.sigma_meas(kappa[k], tau[k], dtype)) for k in range(len(kappa))])


def sigma_columns(ends, blocks, n, dtype=LD):
    """the 6 n square matrix that holds Sigma_{p,e} for every pose p and every endpoint e, zero elsewhere: all of Sigma that A^T
    multiplies"""
    S = np.zeros((6 * n, 6 * n), dtype=dtype)
    for e in sorted(set(int(x) for x in np.asarray(ends).reshape(-1))):
        for p in range(n):
            S[6 * p:6 * p + 6, 6 * e:6 * e + 6] = np.asarray(blocks.sigma(p, e), dtype=dtype)
    return S


def update(T, ends, Rm, tm, kappa, tau, blocks, n, pairs=(), dtype=LD, mistake=None):
    """the update from given blocks; a dict of everything formed on the way.  mistake: one of the planted mistakes of
    tests/test_updateref.py (None: the definitions)"""
    K = len(ends)
    A = a_full(T, ends, n, dtype)
    S = sigma_columns(ends, blocks, n, dtype)
    B = S @ A.T
    Rd = r_diagonal(kappa, tau, dtype)
    M = A @ B + np.diag(Rd)
    M = (M + M.T) / 2
    xi = np.asarray(J.innovations(T, ends, Rm, tm, dtype), dtype=dtype).reshape(-1)
    Gm, logdet_M = spd_inverse(M)
    z = Gm @ xi
    Um = B @ Gm
    dx = -(B @ z)
    rows = lambda p: slice(6 * p, 6 * p + 6)
    diag = np.zeros((n, 6, 6), dtype=dtype)
    for p in range(n):
        Sp = np.asarray(blocks.diag(p), dtype=dtype)
        D = Sp - Um[rows(p)] @ B[rows(p)].T
        diag[p] = (D + D.T) / 2
        if mistake == "no_mirror":  # the lower triangle left as it was
            diag[p] = np.triu(diag[p]) + np.tril(Sp, -1)
    cross = np.array([np.asarray(blocks.pair(q), dtype=dtype) - Um[rows(int(a))] @ B[rows(int(b))].T for q, (a, b) in enumerate(pairs)],
                     dtype=dtype).reshape(-1, 6, 6)
    logdet_R = sum((-3 * np.log(2 * dtype(kappa[k])) - 3 * np.log(dtype(tau[k])) for k in range(K)), dtype(0))
    # (these two are reported alone: such an M has no inverse to go on with)
    if mistake == "jacobians_swapped":
        B = S @ a_full(T, ends, n, dtype, swap=True).T
    if mistake == "sigma_meas_left_out":
        M = M - np.diag(Rd)
    return dict(A=A, S=S, B=B, M=M, G=Gm, xi=xi.reshape(K, 6), z=z, U=Um, delta=dx.reshape(n, 6), xi_post=(Rd * z).reshape(K, 6),
                cov_diag=diag, cov_pairs=cross, T=retract(T, dx, dtype, translation_in_body_frame=(mistake == "translation_in_body_frame")),
                d2_joint=xi @ z, logdet_M=logdet_M, logdet_R=logdet_R, information_gain=(logdet_M - logdet_R) / 2, Rd=Rd)


def information_form(Hr, T, ends, kappa, tau, xi, n):
    """(Sigma', dx) = ((H_red + A^T R^-1 A)^-1, -Sigma' A^T R^-1 xi) in float64; dx of the free poses 1 .. n - 1"""
    A = np.asarray(J.a_matrix(T, ends, n), dtype=F)
    Ri = 1.0 / np.asarray(r_diagonal(kappa, tau), dtype=F)
    Sp = np.linalg.inv(Hr + A.T @ (Ri[:, None] * A))
    Sp = 0.5 * (Sp + Sp.T)
    return Sp, -Sp @ (A.T @ (Ri * np.asarray(xi, dtype=F).reshape(-1)))


# ---- the error bounds the tests hold csrc/linear_update.hip to; u = 2.2e-16, elementwise unless said otherwise.
# tests/test_updateref.py shows that they reject the mistakes the conventions invite.
#
# B and M, in front of the inverse.  An element of B_p,k is one sum of 12 products Sigma[a][y] J[c][y] (gamma_12 = 12 u); the
# entries of J are themselves 3-term sums of products of entries of T (4 u); a half over for the products' own roundings:
#     |B - ref| <= 24 u |Sigma| |A|^T.
# An element of M_kl is one sum of 12 products J[a][y] B[y][c], the same count, of operands B that carry the error above; the
# symmetrisation and the addition of Sigma_meas are two more roundings, inside the half over:
#     |M - ref| <= 24 u |A| |B| + |A| b_B.
# Everything behind G.  G is the inverse through a Cholesky factorisation of K block steps, and every figure behind it is an
# accumulation of 6 K products of its entries: two accumulations in a row of at most 6 (K + 1) terms each, gamma_{12 (K + 1)},
# and a third over -- the constant of jointref.elimination_constant, c = 16 (K + 1).  The entries of G carry the relative error
# of an inverse, which cond_2(M) multiplies: e = c u cond_2(M), times the sum of the absolute values of the terms.  The errors
# of the inputs of a figure are carried through it to first order (delta G = -G delta M G):
#     z        e |G| |xi| + |G| (b_M |z| + b_xi)
#     U        e |B| |G| + b_B |G| + |B| |G| b_M |G|
#     dx       e |B| |z| + b_B |z| + |B| b_z                     (e >= the gamma_{6 K} of the sum itself)
#     xi_post  R b_z + 2 u |xi_post|
#     Sigma'   e |U_p| |B_q|^T + b_U,p |B_q|^T + |U_p| b_B,q^T + 2 u |Sigma_pq|; a diagonal block: the larger of the bound and
#              its transpose (one triangle is formed and mirrored)
#     d2_joint e |xi|^T |z| + |xi|^T b_z + b_xi^T |z|
#     logdet_M the factor is the exact factor of M + dM with |dM| <= gamma_{6 K + 1} |L| |L|^T, and d log det = tr(G dM):
#              sum(|G| o (b_M + 8 K u |L| |L|^T)) for the matrix, 8 K u sum |log L_kk^2| + 16 u 6 K for the logarithms and
#              their sum
#     logdet_R (2 K + 8) u sum_k 3 (|log 2 kappa_k| + |log tau_k|)
#     T'       the rotation R_p Exp(phi_p): Exp is Lipschitz in phi with constant 1 in the 2-norm and the rows of R_p have
#              1-norm at most sqrt(3): sqrt(3) (2 |b_phi|_inf + 16 u), the 16 u for Rodrigues (about 8 u) and the 3-term
#              product (about 3 u); the translation: b_delta + 2 u |t'|

def bounds(ref, T, ends, tm, n, pairs=()):
    """the bounds above for a reference update (a dict of update()), in float64: a dict with the keys of the outputs and of B, M"""
    K = len(ends)
    f = lambda a: np.abs(np.asarray(a, dtype=F))
    A, S, B, M, Gm, Um = f(ref["A"]), f(ref["S"]), f(ref["B"]), np.asarray(ref["M"], dtype=F), f(ref["G"]), f(ref["U"])
    xi, z, Rd = f(ref["xi"]).reshape(-1), f(ref["z"]), np.asarray(ref["Rd"], dtype=F)
    b_B = 24 * U * (S @ A.T)
    b_M = 24 * U * (A @ B) + A @ b_B
    b_xi = np.array([G.xi_bound(T, int(i), int(j), tm[k]) for k, (i, j) in enumerate(ends)]).reshape(-1)
    w = np.linalg.eigvalsh(M)
    cond = w[-1] / w[0]
    e = 16 * (K + 1) * U * cond
    b_z = e * (Gm @ xi) + Gm @ (b_M @ z + b_xi)
    b_U = e * (B @ Gm) + b_B @ Gm + B @ (Gm @ b_M @ Gm)
    b_dx = (e * (B @ z) + b_B @ z + B @ b_z).reshape(n, 6)
    rows = lambda p: slice(6 * p, 6 * p + 6)

    def sig(p, q, Spq):
        return e * (Um[rows(p)] @ B[rows(q)].T) + b_U[rows(p)] @ B[rows(q)].T + Um[rows(p)] @ b_B[rows(q)].T + 2 * U * f(Spq)

    b_diag = np.array([np.maximum(sig(p, p, ref["cov_diag"][p]), sig(p, p, ref["cov_diag"][p]).T) for p in range(n)])
    b_pairs = np.array([sig(int(a), int(b), ref["cov_pairs"][q]) for q, (a, b) in enumerate(pairs)]).reshape(-1, 6, 6)
    L = np.abs(np.linalg.cholesky(M))
    b_ldM = np.sum(Gm * (b_M + 8 * K * U * (L @ L.T))) + 8 * K * U * np.sum(np.abs(2 * np.log(np.diag(L)))) + 16 * U * 6 * K
    Tn = np.asarray(ref["T"], dtype=F).reshape(n, 4, 3)
    b_T = np.zeros((n, 4, 3))
    b_T[:, :3, :] = (np.sqrt(3.0) * (2 * b_dx[:, :3].max(axis=1) + 16 * U))[:, None, None]
    b_T[:, 3, :] = b_dx[:, 3:] + 2 * U * np.abs(Tn[:, 3, :])
    return dict(B=b_B, M=b_M, xi=b_xi.reshape(K, 6), z=b_z, delta=b_dx, xi_post=(Rd * b_z + 2 * U * f(ref["xi_post"]).reshape(-1)).reshape(K, 6),
                cov_diag=b_diag, cov_pairs=b_pairs, d2_joint=e * (xi @ z) + xi @ b_z + b_xi @ z, logdet_M=b_ldM,
                logdet_R=(2 * K + 8) * U * float(np.sum(3 * (np.abs(np.log(2 * np.asarray(ref_k(ref, "kappa")))) +
                                                               np.abs(np.log(np.asarray(ref_k(ref, "tau"))))))),
                T=b_T.reshape(-1), cond_M=cond, e=e)


def ref_k(ref, which):
    """kappa_k, tau_k back out of the diagonal of R"""
    Rd = np.asarray(ref["Rd"], dtype=F).reshape(-1, 6)
    return 1.0 / (2.0 * Rd[:, 0]) if which == "kappa" else 1.0 / Rd[:, 3]


def ratio(err, bound):
    """the largest |err| / bound over the elements; an error where the bound is zero must be zero itself"""
    err, bound = np.abs(np.asarray(err, dtype=F)), np.asarray(bound, dtype=F)
    assert (err[bound == 0] == 0).all(), "an error where nothing may differ"
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))

"""numpy statement of the leave-one-out audit of measurements that are in the graph, in longdouble by default,
written from the definitions and not from csrc/audit_block.h.  It builds on tests/gateref.py: T, Sigma, the perturbation,
R_ij, t_ij, J_i, J_j, Sigma_rel, xi and the logarithm are the gate's.

A record is a measurement (i -> j, R~, t~, kappa, tau) that IS in the weighted graph at weight w >= 0.
    s = (sqrt(2 kappa) x 3, sqrt(tau) x 3),  diag(s)^2 = Sigma_meas^-1 = W0
    z = s o xi,   C = diag(s) Sigma_rel diag(s)
    A = I - w C,  B = I + (1 - w) C
    rho = 1 - w tr(C) / 6
    A = L L^T, p_min the smallest pivot before the square root (the factorisation stops at a non-positive one);
    testable: p_min > min_redundancy
    u = A^-1 z,  v = B^-1 z,  d2 = u^T v
    xi_loo = u / s
    Sigma_loo = diag(1 / s) sym(A^-1 C) diag(1 / s)  ( = (Sigma_rel^-1 - w W0)^-1 )
    untestable, or a non-positive pivot of B: d2 = +inf, xi_loo = 0; untestable: Sigma_loo = 0 too.

Bounds (u = gateref.U = 2.2e-16; |.| elementwise, b_x the bound on x; every one is a function of the reference's own values).
The inputs of the 6 x 6 algebra carry the errors of the gate's quantities:
    b_C = b_Sigma o (s s^T) + 8 u |C|      b_Sigma = gateref.sigma_rel_bound; the scaling is a square root (u), the product
                                           s_a s_b (2 u more) and one product with Sigma_rel: 4 u, doubled
    b_z = s o b_xi + 4 u |z|               b_xi = gateref.xi_bound; one square root and one product
    b_A = w b_C + 2 u |A|                  one fused multiply-add per entry
    b_B = |1 - w| b_C + 2 u (|B| + |C|)    1 - w is rounded before the fused multiply-add
A solve x = M^-1 r with perturbed M and r moves by M^-1 (dr - dM x) to first order, and its own factorisation and the two
triangular solves (6 x 6: 6 + 15 + 15 + 15 fused operations a column, an error of about 36 u cond_2) add 100 u cond_2(M) |x|_2
to every entry, as in gateref.d2_bound:
    b_u = |A^-1| (b_z + b_A |u|) + 100 u cond_2(A) |u|_2,       b_v likewise with B
    b_d2 = |u|^T b_v + b_u^T |v| + b_u^T b_v + 8 u |u|^T |v|     (the product rule, its second-order term, a 6-term sum)
    b_xi_loo = b_u / s + 4 u |xi_loo|
    X = A^-1 C column by column: b_X[:, b] = |A^-1| (b_C[:, b] + b_A |X[:, b]|) + 100 u cond_2(A) |X[:, b]|_2
    b_Sigma_loo = ((b_X + b_X^T) / 2 + 2 u |sym X|) o (1 / s)(1 / s)^T + 6 u |Sigma_loo|
    b_rho = w tr(b_C) / 6 + 8 u (1 + w tr |C| / 6)
The pivot c of a Cholesky factorisation is p_c = 1 / (A_c^-1)_cc with A_c the leading block of order c + 1, so a perturbation
dA moves it by h^T dA_c h, h = p_c A_c^-1 e_c = (-A_{c-1}^-1 a, 1); the computed factor is the exact factor of A + dA' with
|dA'| <= 8 u |L| |L|^T (Higham, Theorem 10.3, gamma_7):
    b_p(c) = 2 |h|^T (b_A + 8 u |L| |L|^T) |h|      (the factor 2 for the terms beyond first order)
    b_pmin = max_c b_p(c)                            (|min a - min b| <= max |a - b|)
All of them grow like 1 / p_min or faster through |A^-1|: they are stated for testable records, and the tests choose records
with p_min > 1e-3 wherever a bound is to hold."""
import numpy as np

from tests import gateref as G

LD = G.LD
U = G.U


def scaling(kappa, tau, dtype=LD):
    return np.r_[np.full(3, np.sqrt(2 * dtype(kappa))), np.full(3, np.sqrt(dtype(tau)))].astype(dtype)


def cholesky(S, floor, dtype=LD):
    """(L or None, p_min, ok): the lower factor written out (numpy's LAPACK wrappers take no longdouble); it stops at a
    non-positive pivot; ok: every pivot > floor"""
    L = np.zeros((6, 6), dtype=dtype)
    pmin, ok = dtype(np.inf), True
    for c in range(6):
        p = S[c, c] - L[c, :c] @ L[c, :c]
        pmin = min(pmin, p)
        ok = ok and bool(p > floor)
        if not p > 0:
            return None, pmin, False
        L[c, c] = np.sqrt(p)
        for r in range(c + 1, 6):
            L[r, c] = (S[r, c] - L[r, :c] @ L[c, :c]) / L[c, c]
    return L, pmin, ok


def chol_solve(L, r, dtype=LD):
    """(L L^T)^-1 r for a vector or the columns of a matrix"""
    x = np.array(r, dtype=dtype)
    for c in range(6):
        x[c] = (x[c] - L[c, :c] @ x[:c]) / L[c, c]
    for c in range(5, -1, -1):
        x[c] = (x[c] - L[c + 1:, c] @ x[c + 1:]) / L[c, c]
    return x


def audit_from(Sr, xi, kappa, tau, w, min_redundancy=1e-6, dtype=LD):
    """the 6 x 6 algebra behind Sigma_rel and xi: a dict with every output and the intermediate quantities the bounds need"""
    Sr, xi, w = np.asarray(Sr, dtype=dtype), np.asarray(xi, dtype=dtype), dtype(w)
    s = scaling(kappa, tau, dtype)
    z = s * xi
    Cm = Sr * np.outer(s, s)
    I = np.eye(6, dtype=dtype)
    A, B = I - w * Cm, I + (1 - w) * Cm
    out = dict(xi=xi, s=s, z=z, C=Cm, A=A, B=B, w=w, rho=1 - w * np.trace(Cm) / 6)
    LA, pmin, testable = cholesky(A, min_redundancy, dtype)
    LB, _, okb = cholesky(B, 0, dtype)
    out.update(pmin=pmin, testable=testable, d2=dtype(np.inf), xi_loo=np.zeros(6, dtype=dtype), sigma_loo=np.zeros((6, 6), dtype=dtype),
               u=None, v=None, X=None)
    if not testable:
        return out
    X = chol_solve(LA, Cm, dtype)
    out["X"] = X
    out["sigma_loo"] = (X + X.T) / 2 / np.outer(s, s)
    if okb:
        u, v = chol_solve(LA, z, dtype), chol_solve(LB, z, dtype)
        out.update(u=u, v=v, d2=u @ v, xi_loo=u / s)
    return out


def audit(T, i, j, Rm, tm, kappa, tau, w, Sii, Sjj, Sij, min_redundancy=1e-6, dtype=LD):
    """one record from the covariance blocks of its pair; the dict of audit_from with sigma_rel beside it"""
    Sr = G.sigma_rel(T, i, j, Sii, Sjj, Sij, dtype)
    out = audit_from(Sr, G.innovation(T, i, j, Rm, tm, dtype), kappa, tau, w, min_redundancy, dtype)
    out["sigma_rel"] = Sr
    return out


def rho_bound(r, b_sigma):
    """b_rho alone: it needs no factor of A, so it holds on untestable records too"""
    s, Cm, w = np.asarray(r["s"], dtype=np.float64), np.asarray(r["C"], dtype=np.float64), float(r["w"])
    b_C = np.asarray(b_sigma) * np.outer(s, s) + 8 * U * np.abs(Cm)
    return w * np.trace(b_C) / 6 + 8 * U * (1 + w * np.trace(np.abs(Cm)) / 6)


def bounds(r, b_sigma, b_xi):
    """the bounds of the module's docstring for the testable record r (a dict of audit / audit_from), from the elementwise
    bounds on Sigma_rel and xi: a dict d2, xi_loo[6], sigma_loo[6, 6], rho, pmin, and C, z"""
    F = np.float64
    s, z, Cm, A, B, w = (np.asarray(r[k], dtype=F) for k in ("s", "z", "C", "A", "B", "w"))
    w = float(w)
    b_C = np.asarray(b_sigma) * np.outer(s, s) + 8 * U * np.abs(Cm)
    b_z = s * np.asarray(b_xi) + 4 * U * np.abs(z)
    b_A = w * b_C + 2 * U * np.abs(A)
    b_B = abs(1 - w) * b_C + 2 * U * (np.abs(B) + np.abs(Cm))
    out = dict(C=b_C, z=b_z, rho=rho_bound(r, b_sigma))
    # the pivots
    L = np.linalg.cholesky(A)
    dA = b_A + 8 * U * (np.abs(L) @ np.abs(L).T)
    bp = 0.0
    for c in range(6):
        h = np.r_[-np.linalg.solve(A[:c, :c], A[:c, c]), 1.0] if c else np.ones(1)
        bp = max(bp, 2 * (np.abs(h) @ dA[:c + 1, :c + 1] @ np.abs(h)))
    out["pmin"] = bp
    Ai, Bi = np.abs(np.linalg.inv(A)), np.abs(np.linalg.inv(B))
    cA, cB = np.linalg.cond(A), np.linalg.cond(B)
    X = np.asarray(r["X"], dtype=F)
    b_X = Ai @ (b_C + b_A @ np.abs(X)) + 100 * U * cA * np.linalg.norm(X, axis=0)[None, :]
    sl = np.asarray(r["sigma_loo"], dtype=F)
    out["sigma_loo"] = ((b_X + b_X.T) / 2 + 2 * U * np.abs(X + X.T) / 2) / np.outer(s, s) + 6 * U * np.abs(sl)
    if r["u"] is not None:
        u, v = np.asarray(r["u"], dtype=F), np.asarray(r["v"], dtype=F)
        b_u = Ai @ (b_z + b_A @ np.abs(u)) + 100 * U * cA * np.linalg.norm(u)
        b_v = Bi @ (b_z + b_B @ np.abs(v)) + 100 * U * cB * np.linalg.norm(v)
        out["d2"] = np.abs(u) @ b_v + b_u @ np.abs(v) + b_u @ b_v + 8 * U * (np.abs(u) @ np.abs(v))
        out["xi_loo"] = b_u / s + 4 * U * np.abs(np.asarray(r["xi_loo"], dtype=F))
    return out


def record_bounds(T, i, j, tm, Sii, Sjj, Sij, r):
    """bounds(r) with the gate's bounds on Sigma_rel and xi for the pair (i, j) of T"""
    return bounds(r, G.sigma_rel_bound(T, i, j, Sii, Sjj, Sij), G.xi_bound(T, i, j, tm))

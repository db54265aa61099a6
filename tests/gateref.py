"""numpy statement of the Mahalanobis gate of candidate measurements, in longdouble by default, written from
the definitions and not from csrc/gate.hip.

T = (R_i, t_i), flat, 12 doubles per pose (R column-major, then t: the layout of tests/covref.py), perturbed as in 5e:
R_i <- R_i Exp(phi_i), t_i <- t_i + delta_i, rotation first.  For poses i != j
    R_ij = R_i^T R_j,   t_ij = R_i^T (t_j - t_i),   perturbed the same way (delta_ij in frame i),
    J_i = [[-R_ij^T, 0], [[t_ij]x, -R_i^T]],   J_j = [[I, 0], [0, R_i^T]],
    Sigma_rel = J_i S_ii J_i^T + J_i S_ij J_j^T + J_j S_ij^T J_i^T + J_j S_jj J_j^T,
    xi = (Log(R~^T R_ij), t_ij - t~),   Sigma_meas = diag(I / (2 kappa), I / tau),
    d2 = xi^T (Sigma_rel + Sigma_meas)^-1 xi."""
import numpy as np

LD = np.longdouble


def skew(v, dtype=LD):
    v = np.asarray(v, dtype=dtype)
    z = dtype(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=dtype)


def pose(T, g, dtype=LD):
    """(R, t) of pose g"""
    P = np.asarray(T, dtype=dtype).reshape(-1, 4, 3)[g]
    return P[:3, :].T.copy(), P[3, :].copy()


def relative_pose(T, i, j, dtype=LD):
    Ri, ti = pose(T, i, dtype)
    Rj, tj = pose(T, j, dtype)
    return Ri.T @ Rj, Ri.T @ (tj - ti)


def jacobians(T, i, j, dtype=LD):
    """(J_i, J_j): d (phi_ij, delta_ij) / d (phi_i, delta_i) and / d (phi_j, delta_j)"""
    Ri, _ = pose(T, i, dtype)
    Rij, tij = relative_pose(T, i, j, dtype)
    Ji, Jj = np.zeros((6, 6), dtype=dtype), np.zeros((6, 6), dtype=dtype)
    Ji[:3, :3] = -Rij.T
    Ji[3:, :3] = skew(tij, dtype)
    Ji[3:, 3:] = -Ri.T
    Jj[:3, :3] = np.eye(3, dtype=dtype)
    Jj[3:, 3:] = Ri.T
    return Ji, Jj


def log_so3(E, dtype=LD):
    """the rotation vector of E in SO(3); near pi the axis comes from the symmetric part"""
    E = np.asarray(E, dtype=dtype)
    a = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]], dtype=dtype) / 2
    c = (np.trace(E) - 1) / 2
    s = np.sqrt(a @ a)
    th = np.arctan2(s, c)
    if c < 0 and s < 1e-3:
        Sm = (E + E.T) / 2
        k = int(np.argmax(np.diag(Sm)))
        n = Sm[:, k].copy()
        n[k] -= c
        n = n / np.sqrt(n @ n)
        if n @ a < 0:
            n = -n
        return th * n
    if s == 0:
        return a
    return (th / s) * a


def sigma_rel(T, i, j, Sii, Sjj, Sij, dtype=LD):
    Ji, Jj = jacobians(T, i, j, dtype)
    Sii, Sjj, Sij = (np.asarray(B, dtype=dtype) for B in (Sii, Sjj, Sij))
    A = Ji @ Sii @ Ji.T + Ji @ Sij @ Jj.T + Jj @ Sij.T @ Ji.T + Jj @ Sjj @ Jj.T
    return (A + A.T) / 2


def innovation(T, i, j, Rm, tm, dtype=LD):
    """Rm: the measured rotation, 3 x 3 (a row-major record reshaped)"""
    Rij, tij = relative_pose(T, i, j, dtype)
    Rm = np.asarray(Rm, dtype=dtype).reshape(3, 3)
    return np.r_[log_so3(Rm.T @ Rij, dtype), tij - np.asarray(tm, dtype=dtype)]


def sigma_meas(kappa, tau, dtype=LD):
    return np.diag(np.r_[np.full(3, 1 / (2 * dtype(kappa))), np.full(3, 1 / dtype(tau))]).astype(dtype)


def gate(T, i, j, Rm, tm, kappa, tau, Sii, Sjj, Sij, dtype=LD):
    """(xi, d2, Sigma_rel, S) of one candidate from the given blocks"""
    Sr = sigma_rel(T, i, j, Sii, Sjj, Sij, dtype)
    xi = innovation(T, i, j, Rm, tm, dtype)
    S = Sr + sigma_meas(kappa, tau, dtype)
    # (numpy's LAPACK wrappers take no longdouble: Cholesky and the forward solve written out)
    L = np.zeros((6, 6), dtype=dtype)
    y = np.zeros(6, dtype=dtype)
    for c in range(6):
        p = S[c, c] - L[c, :c] @ L[c, :c]
        if not p > 0:
            return xi, dtype(np.inf), Sr, S
        L[c, c] = np.sqrt(p)
        for r in range(c + 1, 6):
            L[r, c] = (S[r, c] - L[r, :c] @ L[c, :c]) / L[c, c]
        y[c] = (xi[c] - L[c, :c] @ y[:c]) / L[c, c]
    return xi, y @ y, Sr, S


def blocks_of(Sigma, i, j):
    """(S_ii, S_jj, S_ij) of the full 6 (n - 1) square Sigma of the reduced problem; a block that names pose 0 is zero"""
    def blk(a, b):
        if a == 0 or b == 0:
            return np.zeros((6, 6))
        return Sigma[6 * (a - 1):6 * a, 6 * (b - 1):6 * b]
    return blk(i, i), blk(j, j), blk(i, j)


# ---- the bounds the GPU tests hold csrc/gate.hip to (tests/test_gpu_gate.py), derived there; u = 2.2e-16.  Shared with
# tests/test_gateref.py, which shows that each of them rejects the mistakes the conventions invite.
U = 2.2e-16
XI_R_BOUND = 64 * U / np.sin(3.0)  # residual angles up to 3.0 rad: the direction of a is divided by |a| = sin theta


def sigma_rel_bound(T, i, j, Sii, Sjj, Sij):
    """elementwise: 32 u (|J| |Sigma_12| |J|^T), J = [J_i J_j], Sigma_12 the joint 12 x 12 block: two 12-term products,
    gamma_24 and a third over"""
    Ji, Jj = jacobians(T, i, j, np.float64)
    J = np.abs(np.c_[Ji, Jj])
    S12 = np.abs(np.block([[np.asarray(Sii), np.asarray(Sij)], [np.asarray(Sij).T, np.asarray(Sjj)]]))
    return 32 * U * (J @ S12 @ J.T)


def xi_bound(T, i, j, tm):
    """elementwise over the 6 entries of xi, residual angle <= 3.0 rad: the rotation part XI_R_BOUND, the translation part
    16 u (|t_i| + |t_j| + |t~|)"""
    _, ti = pose(T, i, np.float64)
    _, tj = pose(T, j, np.float64)
    bt = 16 * U * (np.linalg.norm(ti) + np.linalg.norm(tj) + np.linalg.norm(np.asarray(tm, dtype=np.float64)))
    return np.r_[np.full(3, XI_R_BOUND), np.full(3, bt)]


def d2_bound(xi, S, d2, b_xi, b_sigma):
    """the two bounds above propagated through d2 = xi^T S^-1 xi, plus 100 u cond_2(S) d2 for the 6 x 6 solve (its own error
    is about 36 u cond_2).  d2(xi + e) - d2(xi) = 2 e^T S^-1 xi + e^T S^-1 e exactly: the first-order term 2 |S^-1 xi|^T b_xi,
    the term |S^-1 xi|^T b_sigma |S^-1 xi| of the matrix, and the second-order term b_xi^T |S^-1| b_xi, which is all there is
    at a zero residual (xi = 0, where the first-order bound alone would be 0)"""
    S = np.asarray(S, dtype=np.float64)
    w = np.abs(np.linalg.solve(S, np.asarray(xi, dtype=np.float64)))
    return 2 * (w @ b_xi) + w @ b_sigma @ w + b_xi @ np.abs(np.linalg.inv(S)) @ b_xi + 100 * U * np.linalg.cond(S) * float(d2)

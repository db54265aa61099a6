"""numpy statement of X = Sigma V, the estimate's covariance applied to vectors (csrc/covariance_apply.h), written
from the definitions on top of the dense reduced Hessian of tests/covref.py and the sets of tests/covnested_ref.py.

V and X are 6 n x m; rows 6 p .. 6 p + 5 belong to pose p; Sigma is the full 6 n square covariance whose rows and columns of
pose 0 are zero, so pose 0's rows of V are not read and those of X are zero.  X_red = H_red^-1 V_red.
    dense_solve   the reference: float64 solves refined with longdouble residuals (numpy.linalg takes no longdouble)
    eliminate     the elimination in the device's order, in float64: with v_b the rows of block b, v_S the separator's,
                      u_b = C_b v_b,  r_S = v_S - sum_b scatter_{N_b}(W_b^T v_b)  (blocks in order),
                      x_S = Sigma_SS r_S,  x_b = u_b - W_b x_S[N_b]
    bound         per column 6 (n - 1) u cond_2(H_red) |Sigma_red|_2 |v_red|_2: the shape of 5j's end-to-end bound.  A backward
                  stable solve errs by about (dimension) u cond_2 |x|_2 <= (dimension) u cond_2 |Sigma|_2 |v|_2 per column; the
                  elimination forms explicit inverses, whose error has the same shape."""
import numpy as np

from tests.covschur_ref import rows

LD = np.longdouble
F = np.float64
U = 2.2e-16


def dense_solve(Hr, Vr, sweeps=6):
    """H_red^-1 V_red in longdouble: X <- X + solve(H, V - H X), the residual in longdouble, until it stops shrinking"""
    H64, HL, VL = np.asarray(Hr, dtype=F), np.asarray(Hr, dtype=LD), np.asarray(Vr, dtype=LD)
    X = np.linalg.solve(H64, VL.astype(F)).astype(LD)
    for _ in range(sweeps):
        X = X + np.linalg.solve(H64, (VL - HL @ X).astype(F)).astype(LD)
    return X


def full(Xr):
    """the 6 n-row matrix with zero rows for pose 0"""
    return np.vstack([np.zeros((6, Xr.shape[1]), dtype=Xr.dtype), Xr])


def reference(Hr, V):
    """X = Sigma V for a 6 n-row V (pose 0's rows not read), longdouble"""
    return full(dense_solve(Hr, np.asarray(V)[6:]))


def apply_sigma(Sigma, V):
    """X = Sigma V by the definition, from the explicit 6 (n - 1) square Sigma of the reduced problem"""
    return full(np.asarray(Sigma) @ np.asarray(V)[6:])


def bound(Hr, V):
    """the per-column bound, m figures"""
    w = np.linalg.eigvalsh(np.asarray(Hr, dtype=F))
    return Hr.shape[0] * U * (w[-1] / w[0]) * (1.0 / w[0]) * np.linalg.norm(np.asarray(V, dtype=F)[6:], axis=0)


def worst(X, Xref, b):
    """the largest column error (2-norm) over its bound"""
    err = np.linalg.norm(np.asarray(np.asarray(X, dtype=LD) - np.asarray(Xref, dtype=LD), dtype=F), axis=0)
    return float((err / b).max())


def plan_from_separator(n, rowptr, col, sep):
    """block_of for a hand-made separator: the blocks are the connected components of the other free poses, numbered by their
    first pose"""
    block_of = np.full(n, -1, dtype=np.int64)
    block_of[0] = -2
    free = [g for g in range(1, n) if g not in set(sep)]
    seen, nb = set(), 0
    for g in free:
        if g in seen:
            continue
        stack = [g]
        seen.add(g)
        while stack:
            v = stack.pop()
            block_of[v] = nb
            for u in col[rowptr[v]:rowptr[v + 1]]:
                u = int(u)
                if u != 0 and u not in seen and u in free:
                    seen.add(u)
                    stack.append(u)
        nb += 1
    return block_of


def eliminate(Hr, info, V, mistake=None):
    """X (6 n x m, float64) by the elimination in the device's order; info: covnested_ref.sets(...).  mistake: one of the
    planted mistakes of tests/test_applyref.py (None: the definitions) -- "sign": + W_b x_S; ("skip", b): block b's
    contribution to r_S left out; ("untransposed", b): W_b where W_b^T belongs (a block with |I_b| = |N_b|); "pose0": pose 0's
    rows of V added into the first rows that are read"""
    sep, blocks, coupled = info["separator"], info["blocks"], info["coupled"]
    Hr, V = np.asarray(Hr, dtype=F), np.asarray(V, dtype=F)
    Vr = V[6:].copy()
    if mistake == "pose0":
        Vr[:6] += V[:6]
    m = V.shape[1]
    rS = rows(sep) if sep else np.zeros(0, dtype=np.int64)
    Sc = Hr[np.ix_(rS, rS)].copy()
    r_S = Vr[rS].copy()
    Xr = np.zeros((Hr.shape[0], m))
    W, loc, rI = [], [], []
    for b, (I, N) in enumerate(zip(blocks, coupled)):
        r = rows(I)
        la = (6 * np.asarray(N, dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)
        B = Hr[np.ix_(r, rS[la])]
        Cb = np.linalg.inv(Hr[np.ix_(r, r)])
        Wb = Cb @ B
        Sc[np.ix_(la, la)] -= B.T @ Wb
        Xr[r] = Cb @ Vr[r]  # u_b
        t = (Wb if mistake == ("untransposed", b) else Wb.T) @ Vr[r]
        if mistake != ("skip", b):
            r_S[la] -= t
        W.append(Wb); loc.append(la); rI.append(r)
    if sep:
        Sc = 0.5 * (Sc + Sc.T)
        x_S = np.linalg.inv(Sc) @ r_S
        Xr[rS] = x_S
        for Wb, la, r in zip(W, loc, rI):
            Xr[r] = Xr[r] + Wb @ x_S[la] if mistake == "sign" else Xr[r] - Wb @ x_S[la]
    return full(Xr)

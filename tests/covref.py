"""numpy / scipy reference of the marginal pose covariances, written from the definition:

T = (R_i, t_i), pose i perturbed by xi_i = (phi_i, delta_i), rotation first: R_i <- R_i Exp(phi_i), t_i <- t_i + delta_i.
g(xi) = f(T [+] xi), f = 1/2 <T, T Q>.  H = Hessian of g at 0 = J^T (S (x) I_3) J with S = Q - Lambda(T) (the certificate
matrix at rank 3) and J the linear map xi -> Tdot (rotation columns of pose i: R_i [phi_i]x, translation column: delta_i).
H_red = H without the first 6 rows and columns (pose 0 held fixed), Sigma = H_red^-1.

T is flat, 12 doubles per pose (R column-major, then t): a K = 3 block of the iterate layout, element (b, column 4 g + c) at
[(4 g + c) 3 + b]."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.test_certificate import as_matrix, certificate_matrix, q_full  # noqa: F401  (q_full: re-exported)

EPS = 2.2e-16


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(phi):
    th = np.linalg.norm(phi)
    K = skew(phi)
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


def rotations(T, n):
    """[n, 3, 3] with R[g][b][c]"""
    return np.asarray(T).reshape(n, 4, 3)[:, :3, :].transpose(0, 2, 1)


def cost(Q, T, n):
    Tm = as_matrix(T, 3, n)
    return 0.5 * float(np.sum(Tm * (Q @ Tm.T).T))


def perturb(T, xi, n):
    """T [+] xi"""
    P = np.array(T, dtype=np.float64).reshape(n, 4, 3)
    X = np.asarray(xi).reshape(n, 6)
    for g in range(n):
        R = P[g, :3, :].T @ exp_so3(X[g, :3])
        P[g, :3, :] = R.T
        P[g, 3, :] += X[g, 3:]
    return P.reshape(-1)


def jacobian(T, n):
    """sparse 12 n x 6 n: xi -> Tdot in the flat layout of T"""
    R = rotations(T, n)
    blocks = []
    for g in range(n):
        J = np.zeros((12, 6))
        for c in range(3):
            e = np.zeros(3)
            e[c] = 1.0
            J[3 * c:3 * c + 3, :3] = -R[g] @ skew(e)  # column c of R [phi]x = R (phi x e_c) = -R [e_c]x phi
        J[9:, 3:] = np.eye(3)
        blocks.append(J)
    return sp.block_diag(blocks, format="csr")


def hessian(Q, T, n):
    """sparse 6 n x 6 n H = J^T (S (x) I_3) J"""
    S = certificate_matrix(Q, T, 3, n)
    J = jacobian(T, n)
    H = (J.T @ sp.kron(S, sp.identity(3), format="csr") @ J).tocsr()
    return 0.5 * (H + H.T)


def reduced(H):
    return H[6:, 6:].tocsc()


def dense_reference(Q, T, n):
    """(H_red dense, Sigma = inv(H_red), eigenvalues of H_red ascending)"""
    Hr = reduced(hessian(Q, T, n)).toarray()
    Hr = 0.5 * (Hr + Hr.T)
    return Hr, np.linalg.inv(Hr), np.linalg.eigvalsh(Hr)


def extreme_eigenvalues(Hr):
    """(smallest by shift-invert at 0, largest) of the sparse symmetric H_red"""
    hi = float(spla.eigsh(Hr, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0])
    lo = float(spla.eigsh(Hr, k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-6)[0])
    return lo, hi


def full_sigma(diag, cross, pairs, n):
    """the 6 (n - 1) square matrix put together from the diagonal blocks and the cross blocks of ALL pairs (a != b)"""
    S = np.zeros((6 * n, 6 * n))
    for g in range(n):
        S[6 * g:6 * g + 6, 6 * g:6 * g + 6] = diag[g]
    for (a, b), B in zip(pairs, cross):
        if a != b:
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = B
    return S[6:, 6:]


def team_measurements_global(team):
    """the team's measurements with their current weights in team-order numbering, each shared edge once (the copy of the
    lower robot)"""
    offs, o = {}, 0
    for i in team.ids:
        offs[i] = o
        o += team.agents[i].n
    out = []
    for i in team.ids:
        for e in team.agents[i].measurements():
            r1, r2 = int(e["r1"]), int(e["r2"])
            if r1 != r2 and min(r1, r2) != i:
                continue
            q = e.copy()
            q["p1"], q["p2"] = offs[r1] + int(e["p1"]), offs[r2] + int(e["p2"])
            q["r1"] = q["r2"] = 0
            out.append(q)
    return np.array(out, dtype=out[0].dtype), o

"""numpy statement of the marginal covariances by nested dissection inside each robot (DESIGN.md 5e "nested",
csrc/covariance_nested.hip), written from the formulas, on top of the dense reduced Hessian of tests/covref.py.

Pose 0 is fixed and belongs to no set.  block_of[g] is the block of pose g, -1 for a separator pose (public, or promoted by
the dissection), -2 for pose 0.  S = the separator poses in team order, I_b = the poses of block b in order, N_b = the
separator poses coupled to block b, ascending.  With C_b = H_bb^-1, B_b = H[I_b, N_b] (the coupled columns alone),
W_b = C_b B_b:
    S_c = H_SS - sum_b scatter_{N_b}(B_b^T W_b)  (blocks in order),   Sigma_SS = S_c^-1,
    Sigma[I_b, I_b] = C_b + W_b Sigma_SS[N_b, N_b] W_b^T,   Sigma[I_b, I_c] = W_b Sigma_SS[N_b, N_c] W_c^T  (b != c),
    Sigma[I_b, S]   = -W_b Sigma_SS[N_b, :],
    log det H_red   = sum_b log det H_bb + log det S_c   (blocks in order, the separator last)."""
import numpy as np

from dpgo_ros_amd import capi
from tests.covschur_ref import rows


def pattern(m, n):
    """(rowptr, col) of the symmetric block pattern of n poses with the diagonal, from measurements in single-robot numbering"""
    a, b = np.asarray(m["p1"], dtype=np.int64), np.asarray(m["p2"], dtype=np.int64)
    i = np.r_[a, b, np.arange(n)]
    j = np.r_[b, a, np.arange(n)]
    key = np.unique(i * n + j)
    i, j = key // n, key % n
    rowptr = np.zeros(n + 1, dtype=np.int32)
    np.add.at(rowptr, i + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), j.astype(np.int32)


def restrict(rowptr, col, keep):
    """the pattern restricted to the listed poses (ascending), renumbered"""
    n = len(rowptr) - 1
    loc = np.full(n, -1, dtype=np.int64)
    loc[keep] = np.arange(len(keep))
    rp, cl = [0], []
    for g in keep:
        c = loc[col[rowptr[g]:rowptr[g + 1]]]
        cl.extend(c[c >= 0].tolist())
        rp.append(len(cl))
    return np.array(rp, dtype=np.int32), np.array(cl, dtype=np.int32)


def robots_of(n, num_robots):
    """the contiguous rule of capi.partition"""
    return np.minimum(np.arange(n) // (n // num_robots), num_robots - 1).astype(np.int32)


def sets(block_of, rowptr, col):
    """blocks (team poses each, in order), the separator (team poses) and, per block, N_b as ascending separator indices"""
    block_of = np.asarray(block_of)
    n = len(block_of)
    nb = int(block_of.max()) + 1 if (block_of >= 0).any() else 0
    sep = [g for g in range(1, n) if block_of[g] == -1]
    spos = {g: k for k, g in enumerate(sep)}
    blocks = [[] for _ in range(nb)]
    for g in range(1, n):
        if block_of[g] >= 0:
            blocks[block_of[g]].append(g)
    coupled = []
    for I in blocks:
        s = set()
        for g in I:
            for u in col[rowptr[g]:rowptr[g + 1]]:
                if block_of[u] == -1:
                    s.add(spos[int(u)])
        coupled.append(sorted(s))
    return dict(blocks=blocks, separator=sep, coupled=coupled)


def nested_bytes(info):
    """the bytes of the large device buffers of the path (include/dpgo_hip.h): 8 (3 s^2 + sum_b n_b K_b + max_b (3 n_b^2 +
    n_b K_b + K_b^2)), s = 6 |S|, n_b = 6 |I_b|, K_b = 6 |N_b|; the call adds the small ones (outputs, lists, scratch)"""
    s = 6 * len(info["separator"])
    nk = [(6 * len(I), 6 * len(N)) for I, N in zip(info["blocks"], info["coupled"])]
    return 8 * (3 * s * s + sum(n * k for n, k in nk) + max(3 * n * n + n * k + k * k for n, k in nk))


def nested_reference(Hr, info):
    """(Sigma, logdet) through the elimination; Hr dense, of order 6 (n - 1); info: sets(...)"""
    sep, blocks, coupled = info["separator"], info["blocks"], info["coupled"]
    rS = rows(sep) if sep else np.zeros(0, dtype=np.int64)
    Sc = Hr[np.ix_(rS, rS)].copy()
    Sigma = np.zeros_like(Hr)
    logdet = 0.0
    C, W, loc, rI = [], [], [], []
    for I, N in zip(blocks, coupled):
        r = rows(I)
        la = (6 * np.asarray(N, dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)  # inside the separator
        # a block touches no other block and no separator pose outside its N_b
        other = np.ones(Hr.shape[0], dtype=bool)
        other[r] = False
        other[rS[la]] = False
        assert not Hr[np.ix_(r, np.flatnonzero(other))].any()
        B = Hr[np.ix_(r, rS[la])]
        Cb = np.linalg.inv(Hr[np.ix_(r, r)])
        Wb = Cb @ B
        Sc[np.ix_(la, la)] -= B.T @ Wb
        sign, ld = np.linalg.slogdet(Hr[np.ix_(r, r)])
        assert sign > 0
        logdet += ld
        C.append(Cb); W.append(Wb); loc.append(la); rI.append(r)
    SS = np.zeros((0, 0))
    if sep:
        Sc = 0.5 * (Sc + Sc.T)
        SS = np.linalg.inv(Sc)
        sign, ld = np.linalg.slogdet(Sc)
        assert sign > 0
        logdet += ld
        Sigma[np.ix_(rS, rS)] = SS
    Z = [Wb @ SS[la, :] for Wb, la in zip(W, loc)]  # W_b Sigma_SS[N_b, :]
    for b in range(len(blocks)):
        Sigma[np.ix_(rI[b], rI[b])] = C[b] + Z[b][:, loc[b]] @ W[b].T
        if sep:
            Sigma[np.ix_(rI[b], rS)] = -Z[b]
            Sigma[np.ix_(rS, rI[b])] = -Z[b].T
        for c in range(len(blocks)):
            if c != b:
                Sigma[np.ix_(rI[b], rI[c])] = Z[b][:, loc[c]] @ W[c].T
    return Sigma, logdet


def first_failing_factor(Hr, info):
    """the factor at which the elimination meets its first non-positive pivot, the factors taken in the order of the call
    (the blocks in order, the separator last) and each one's pivots in row order, as a Cholesky factorisation without
    pivoting meets them.  Hr: H_red, sparse or dense.  Returns None when every pivot is positive, else a dict: kind
    ("block" or "separator"), block (-1 for the separator), row (of that factor), pose (team pose of that row), pivot, and
    margin -- the smallest |pivot| / (largest diagonal entry of its factor) over every pivot up to and including the failing
    one: a caller that predicts what a floating-point factorisation reports asks for a margin far above its round-off"""
    sep, blocks, coupled = info["separator"], info["blocks"], info["coupled"]

    def sub(r, c):
        M = Hr[r][:, c]
        return M.toarray() if hasattr(M, "toarray") else np.array(M)

    def pivots(A):
        """(pivots met, in row order, up to and including the first non-positive one; whether the last one failed)"""
        A = 0.5 * (A + A.T)
        d = []
        for k in range(A.shape[0]):
            d.append(A[k, k])
            if not d[-1] > 0.0:
                return np.array(d), True
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k]) / d[-1]
        return np.array(d), False

    margin = np.inf
    rS = rows(sep) if sep else np.zeros(0, dtype=np.int64)
    Sc = sub(rS, rS)
    for b, (I, N) in enumerate(zip(blocks, coupled)):
        r = rows(I)
        Hbb = sub(r, r)
        d, failed = pivots(Hbb.copy())
        margin = min(margin, np.abs(d).min() / Hbb.diagonal().max())
        if failed:
            k = len(d) - 1
            return dict(kind="block", block=b, row=k, pose=I[k // 6], pivot=d[-1], margin=margin)
        la = (6 * np.asarray(N, dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)
        B = sub(r, rS[la])
        Sc[np.ix_(la, la)] -= B.T @ np.linalg.solve(Hbb, B)
    if sep:
        d, failed = pivots(Sc.copy())
        margin = min(margin, np.abs(d).min() / Sc.diagonal().max())
        if failed:
            k = len(d) - 1
            return dict(kind="separator", block=-1, row=k, pose=sep[k // 6], pivot=d[-1], margin=margin)
    return None


def spoil_rotations(T, n, poses, seed):
    """T with the rotations of the listed poses replaced by random ones of SO(3): still a trajectory on SE(3), no longer a
    minimum.  Lambda and the diagonal of H change at these poses and their neighbours only, so a factor that holds neither
    stays what it was"""
    rng = np.random.default_rng(seed)
    P = np.array(T, dtype=np.float64).reshape(n, 4, 3).copy()
    for g in poses:
        Qm, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(Qm) < 0:
            Qm[:, 2] *= -1.0
        P[g, :3, :] = Qm
    return P.reshape(-1)


def banded_chain(n, seed, window=40, longs=0):
    """a noise-free pose graph of n poses with a random ground truth (rotations uniform by angle-axis of a normal vector,
    positions in a box of side 10, pose 0 the identity), as test_gpu_covariance_schur.loop_chain: the odometry i -> i + 1,
    n // 4 closures (a, min(a + k, n - 1)) with a uniform and k uniform in [2, window], and `longs` closures with both ends
    uniform; edges with a = b are dropped.  The closures reach at most `window` poses ahead, so a level set of a breadth-
    first search is a narrow band and the dissection finds small separators.  Returns (measurements in single-robot
    numbering, the ground truth in the layout of chordal_init)"""
    rng = np.random.default_rng(seed)

    def rot(w):
        th = np.linalg.norm(w, axis=-1, keepdims=True)
        k = w / np.maximum(th, 1e-12)
        K = np.zeros(w.shape[:-1] + (3, 3))
        K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
        K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
        s, c = np.sin(th)[..., None], (1 - np.cos(th))[..., None]
        return np.eye(3) + s * K + c * (K @ K)

    Rg = rot(rng.standard_normal((n, 3)))
    tg = rng.uniform(-5.0, 5.0, (n, 3))
    Rg[0], tg[0] = np.eye(3), 0.0
    a = rng.integers(0, n, n // 4)
    b = np.minimum(a + rng.integers(2, window + 1, n // 4), n - 1)
    la, lb = rng.integers(0, n, longs), rng.integers(0, n, longs)
    src = np.r_[np.arange(n - 1), np.minimum(a, b), np.minimum(la, lb)]
    dst = np.r_[np.arange(1, n), np.maximum(a, b), np.maximum(la, lb)]
    keep = src != dst
    src, dst = src[keep], dst[keep]
    m = np.zeros(len(src), dtype=capi.MEAS_DTYPE)
    m["p1"], m["p2"] = src, dst
    m["R"] = np.einsum("eji,ejk->eik", Rg[src], Rg[dst]).reshape(len(src), 9)
    m["t"] = np.einsum("eji,ej->ei", Rg[src], tg[dst] - tg[src])
    m["kappa"], m["tau"], m["weight"] = 100.0, 50.0, 1.0
    T = np.zeros((n, 4, 3))
    T[:, :3, :] = Rg.transpose(0, 2, 1)
    T[:, 3, :] = tg
    return m, T.reshape(-1)

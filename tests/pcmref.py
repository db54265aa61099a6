"""numpy statement of pairwise consistency maximisation between two teams, in longdouble by default, written
from the definitions and not from csrc/consistency_block.h.

A pose X = (R, t) is perturbed as R <- R Exp(phi), t <- t + delta (the convention of 5e / 5f), a product of poses the same
way.  Candidate k is Z_k ~ (T^A_{i_k})^-1 G T^B_{j_k}.  For k < l
    A_kl = (T^A_{i_l})^-1 T^A_{i_k},   B_kl = (T^B_{j_k})^-1 T^B_{j_l},   E_kl = Z_l^-1 A_kl Z_k B_kl,
    xi = (Log(R_E), t_E),   S = J_A Sigma_A J_A^T + J_B Sigma_B J_B^T + J_k N_k J_k^T + J_l N_l J_l^T,  N = diag(I / (2 kappa), I / tau),
    d2 = xi^T S^-1 xi.
The Jacobians are those of a product X_1 X_2 X_3 X_4 in this convention (product_jacobians), Z_l entering through its inverse
(inverse_jacobian); tests/test_pcmref.py checks them against central differences of the perturbed loop.

The bounds the GPU and host tests hold csrc/consistency_block.h to (u = 2.2e-16):
  rotations.  An entry of a computed product of two rotations is off by at most 3 u (a 3-term product of unit rows and
    columns); multiplied on by another rotation an entrywise error e becomes at most sqrt(3) e + 3 u.  R_E is the fifth level
    (a segment is itself a product): 3, 8.2, 17.2, 32.8, 59.8 u, held as E_R = 64 u per entry.
  S.  A Jacobian is [[P, 0], [Q, W]] with P, W rotations (or their negatives) and Q = -R [s]x (+ [u]x for Z_l), so entrywise
    |J| <= Jbar = [[1, 0], [sbar 1, 1]] (1 the all-ones 3 x 3 block), sbar the sum of the norms of the six translations that
    enter (t~_k, t~_l and the four trajectory poses).  The computed J is off by at most 48 u Jbar (E_R, the 8 u of a chained
    translation, the 2-term product of the skew), which enters each term twice; the two 6-term products, the four-term sum and
    the symmetrisation add 16 u: |S - ref| <= 128 u sum_X Jbar |Sigma_X| Jbar^T elementwise (s_bound).
  xi.  theta = atan2(|a|, c), xi_R = (theta / sin theta) a with |da| <= sqrt(3) E_R, |dc| <= 1.5 E_R:
    |d xi_R| <= 2 (theta / sin theta) sqrt(3) E_R + |d theta| <= (2 (3 / sin 3) 64 sqrt(3) + 160) u for residual angles up to 3.0 rad
    (XI_R_BOUND).  t_E chains four rotation-vector products on entries that are E_R off: |d xi_t| <= 160 u sbar (xi_bound).
  d2.  Both propagated through xi^T S^-1 xi, plus 100 u cond_2(S) d2 for the 6 x 6 solve: gateref.d2_bound, as 5f."""
import itertools

import numpy as np

from tests import gateref as G

LD = np.longdouble
U = G.U
E_R = 64 * U
XI_R_BOUND = (2 * (3.0 / np.sin(3.0)) * 64 * np.sqrt(3.0) + 160) * U


def exp_so3(phi, dtype=LD):
    phi = np.asarray(phi, dtype=dtype)
    th = np.sqrt(phi @ phi)
    K = G.skew(phi, dtype)
    if th < 1e-12:
        return np.eye(3, dtype=dtype) + K + K @ K / 2
    return np.eye(3, dtype=dtype) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)


def mul(X, Y):
    return X[0] @ Y[0], X[0] @ Y[1] + X[1]


def inv(X):
    return X[0].T, -(X[0].T @ X[1])


def perturb(X, xi, dtype=LD):
    xi = np.asarray(xi, dtype=dtype)
    return X[0] @ exp_so3(xi[:3], dtype), X[1] + xi[3:]


def pose_of(T, g, dtype=LD):
    return G.pose(T, g, dtype)


def segment(T, a, b, dtype=LD):
    """(T_a)^-1 T_b; the identity when a == b"""
    return G.relative_pose(T, a, b, dtype)


def candidate_pose(c, dtype=LD):
    return np.asarray(c["R"], dtype=dtype).reshape(3, 3), np.asarray(c["t"], dtype=dtype)


def noise(c, dtype=LD):
    return G.sigma_meas(c["kappa"], c["tau"], dtype)


def loop(Zk, Zl, A, B):
    """E_kl = Z_l^-1 A_kl Z_k B_kl"""
    return mul(mul(mul(inv(Zl), A), Zk), B)


def coordinates(E, dtype=LD):
    return np.r_[G.log_so3(E[0], dtype), E[1]]


def product_jacobians(X, dtype=LD):
    """d (phi_E, delta_E) / d (phi_m, delta_m) of E = X_1 .. X_n, every factor and E perturbed as R Exp(phi), t + delta"""
    n = len(X)
    I = (np.eye(3, dtype=dtype), np.zeros(3, dtype=dtype))
    out = []
    for m in range(n):
        pre, upto, suf = I, I, I
        for Y in X[:m]:
            pre = mul(pre, Y)
        upto = mul(pre, X[m])
        for Y in X[m + 1:]:
            suf = mul(suf, Y)
        J = np.zeros((6, 6), dtype=dtype)
        J[:3, :3] = suf[0].T
        J[3:, :3] = -upto[0] @ G.skew(suf[1], dtype)
        J[3:, 3:] = pre[0]
        out.append(J)
    return out


def inverse_jacobian(Z, dtype=LD):
    """the perturbation of Z^-1 as a function of that of Z"""
    J = np.zeros((6, 6), dtype=dtype)
    J[:3, :3] = -Z[0]
    J[3:, :3] = -G.skew(Z[0].T @ Z[1], dtype)
    J[3:, 3:] = -Z[0].T
    return J


def jacobians(Zk, Zl, A, B, dtype=LD):
    """(J_l, J_A, J_k, J_B) of E_kl with respect to the perturbations of Z_l, A, Z_k, B"""
    J1, JA, Jk, JB = product_jacobians([inv(Zl), A, Zk, B], dtype)
    return J1 @ inverse_jacobian(Zl, dtype), JA, Jk, JB


def mahalanobis(xi, S, dtype=LD):
    L = np.zeros((6, 6), dtype=dtype)
    y = np.zeros(6, dtype=dtype)
    for c in range(6):
        p = S[c, c] - L[c, :c] @ L[c, :c]
        if not p > 0:
            return dtype(np.inf)
        L[c, c] = np.sqrt(p)
        for r in range(c + 1, 6):
            L[r, c] = (S[r, c] - L[r, :c] @ L[c, :c]) / L[c, c]
        y[c] = (xi[c] - L[c, :c] @ y[:c]) / L[c, c]
    return y @ y


def pair(Zk, Zl, A, B, SA, SB, Nk, Nl, dtype=LD):
    """(xi, d2, S) of the ordered pair k < l"""
    Jl, JA, Jk, JB = jacobians(Zk, Zl, A, B, dtype)
    SA, SB = np.asarray(SA, dtype=dtype), np.asarray(SB, dtype=dtype)
    S = JA @ SA @ JA.T + JB @ SB @ JB.T + Jk @ Nk @ Jk.T + Jl @ Nl @ Jl.T
    S = (S + S.T) / 2
    xi = coordinates(loop(Zk, Zl, A, B), dtype)
    return xi, mahalanobis(xi, S, dtype), S


def endpoints(cand, offs_a, offs_b):
    """team poses (i_k, j_k); offs: {robot id: first team pose}"""
    i = np.array([offs_a[int(c["r1"])] + int(c["p1"]) for c in cand])
    j = np.array([offs_b[int(c["r2"])] + int(c["p2"]) for c in cand])
    return i, j


def segment_pairs(i, j):
    """the ordered pose pairs the segments of K candidates need, per team, each once in order of first use (k < l, k outer),
    as the library lists them: team A (i_l, i_k), team B (j_k, j_l); coinciding poses need none"""
    pa, pb = {}, {}
    for k, l in itertools.combinations(range(len(i)), 2):
        if i[l] != i[k]:
            pa.setdefault((int(i[l]), int(i[k])), len(pa))
        if j[k] != j[l]:
            pb.setdefault((int(j[k]), int(j[l])), len(pb))
    return pa, pb


def pair_inputs(cand, TA, TB, i, j, k, l, sig_a, sig_b, dtype=LD):
    """the arguments of pair() for k < l; sig_a(a, b) -> Sigma^A_rel(a, b) for a != b"""
    Zk, Zl = candidate_pose(cand[k], dtype), candidate_pose(cand[l], dtype)
    A, B = segment(TA, i[l], i[k], dtype), segment(TB, j[k], j[l], dtype)
    SA = sig_a(int(i[l]), int(i[k])) if i[l] != i[k] else np.zeros((6, 6))
    SB = sig_b(int(j[k]), int(j[l])) if j[k] != j[l] else np.zeros((6, 6))
    return Zk, Zl, A, B, SA, SB, noise(cand[k], dtype), noise(cand[l], dtype)


def sbar(cand, TA, TB, i, j, k, l):
    f = np.float64
    return float(sum(np.linalg.norm(v) for v in (cand[k]["t"], cand[l]["t"], pose_of(TA, i[k], f)[1], pose_of(TA, i[l], f)[1],
                                                 pose_of(TB, j[k], f)[1], pose_of(TB, j[l], f)[1])))


def s_bound(sb, SA, SB, Nk, Nl):
    one = np.ones((3, 3))
    Jb = np.block([[one, np.zeros((3, 3))], [sb * one, one]])
    tot = sum(np.abs(np.asarray(M, dtype=np.float64)) for M in (SA, SB, Nk, Nl))
    return 128 * U * (Jb @ tot @ Jb.T)


def xi_bound(sb):
    return np.r_[np.full(3, XI_R_BOUND), np.full(3, 160 * U * sb)]


def bounds(cand, TA, TB, i, j, k, l, args, xi, S, d2):
    """(b_S elementwise, b_xi, b_d2) of the pair k < l; args: pair_inputs(...)"""
    sb = sbar(cand, TA, TB, i, j, k, l)
    b_s, b_x = s_bound(sb, *args[4:]), xi_bound(sb)
    return b_s, b_x, G.d2_bound(xi, S, d2, b_x, b_s)


def d2_matrix(cand, TA, TB, i, j, sig_a, sig_b, dtype=LD):
    """d2[K, K]: symmetric, zero diagonal"""
    K = len(cand)
    D = np.zeros((K, K), dtype=dtype)
    for k, l in itertools.combinations(range(K), 2):
        D[k, l] = D[l, k] = pair(*pair_inputs(cand, TA, TB, i, j, k, l, sig_a, sig_b, dtype), dtype=dtype)[1]
    return D


def sigma_from_dense(T, Sigma, dtype=LD):
    """sig(a, b) from the full inverse reduced Hessian, through gateref.sigma_rel"""
    return lambda a, b: G.sigma_rel(T, a, b, *G.blocks_of(Sigma, a, b), dtype)


def max_clique_brute(adj):
    """a maximum clique of a bool matrix by Bron-Kerbosch with pivoting (exact); ascending members"""
    adj = np.asarray(adj, dtype=bool)
    K = len(adj)
    nb = [set(np.flatnonzero(adj[v]).tolist()) - {v} for v in range(K)]
    best = []

    def bk(R, P, X):
        nonlocal best
        if not P and not X:
            if len(R) > len(best):
                best = sorted(R)
            return
        if len(R) + len(P) <= len(best):
            return
        piv = max(P | X, key=lambda v: len(P & nb[v]))
        for v in sorted(P - nb[piv]):
            bk(R | {v}, P & nb[v], X & nb[v])
            P = P - {v}
            X = X | {v}

    bk(set(), set(range(K)), set())
    return best


# ---- the planted case of tests/test_pcmref.py and tests/test_gpu_consistency.py
PLANTED = dict(n=24, seed_a=3, seed_b=5, seed_g=17, seed_c=1, inliers=16, outliers=8, kappa=2000.0, tau=1000.0, quantile=0.99)


def random_pose(rng, box=5.0):
    w = rng.standard_normal(3)
    w *= rng.uniform(0, np.pi) / np.linalg.norm(w)
    return np.asarray(exp_so3(w, np.float64)), rng.uniform(-box, box, 3)


def move_gauge(T, Gm):
    """the trajectory G^-1 T (every pose from the left); pose 0 is then no longer the identity"""
    n = len(T) // 12
    Gi = inv(Gm)
    out = np.zeros((n, 4, 3))
    for g in range(n):
        R, t = mul(Gi, pose_of(T, g, np.float64))
        out[g, :3, :], out[g, 3, :] = R.T, t
    return out.reshape(-1)


def planted_case(p=PLANTED):
    """(m_a, T_a, m_b, T_b, cand, is_true): two banded chains, B in a gauge moved by a seeded G, 16 true candidates at random
    endpoints with noise from their own N and 8 outliers that are random poses"""
    from dpgo_ros_amd import capi
    from tests import covnested_ref as NR
    n = p["n"]
    ma, Ta = NR.banded_chain(n, p["seed_a"], window=8)
    mb, Tb0 = NR.banded_chain(n, p["seed_b"], window=8)
    Gm = random_pose(np.random.default_rng(p["seed_g"]))
    Tb = move_gauge(Tb0, Gm)  # T^B in its own gauge: T^B_j = G^-1 (pose j in A's frame)
    rng = np.random.default_rng(p["seed_c"])
    K = p["inliers"] + p["outliers"]
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    is_true = np.zeros(K, dtype=bool)
    is_true[rng.permutation(K)[:p["inliers"]]] = True
    f = np.float64
    for k in range(K):
        i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
        cand[k]["r1"], cand[k]["p1"], cand[k]["r2"], cand[k]["p2"] = 0, i, 0, j
        cand[k]["kappa"], cand[k]["tau"], cand[k]["weight"] = p["kappa"], p["tau"], 1.0
        if is_true[k]:
            Z = mul(mul(inv(pose_of(Ta, i, f)), Gm), pose_of(Tb, j, f))
            e = np.r_[rng.standard_normal(3) / np.sqrt(2 * p["kappa"]), rng.standard_normal(3) / np.sqrt(p["tau"])]
            Z = perturb(Z, e, f)
        else:
            Z = random_pose(rng, 10.0)
        cand[k]["R"], cand[k]["t"] = np.asarray(Z[0], dtype=f).reshape(-1), np.asarray(Z[1], dtype=f)
    return ma, Ta, mb, Tb, cand, is_true


MIX_AXIS = np.array([1.0, -2.0, 2.0]) / 3.0


def mixed_candidates(Ta, Tb, K, seed, split_a=None, kappa=100.0, tau=50.0):
    """K candidates with G = I for the edge tests: Z = (T^A_i)^-1 T^B_j Exp(th a), so that the loop through an exact candidate
    and this one has the residual angle th.  By index: 0 -- 0.3 rad; 1 -- shares i with 0, exact; 2 -- shares i and j with 0,
    exact (both segments coincide); 3 -- i is pose 0 of team A; 4 -- j is pose 0 of team B; 5 -- exact; 6 -- 1e-9 rad; 7 -- 0.3;
    8 -- 3.0; 9 -- candidate 7 again; the others at random endpoints with th cycling through 0, 1e-9, 0.3, 0.3.  A candidate
    with th > 0 also has its translation moved by 0.05 N(0, I).  split_a: the first team pose of each robot of team A (None:
    one robot)"""
    from dpgo_ros_amd import capi
    rng = np.random.default_rng(seed)
    na, nb = len(Ta) // 12, len(Tb) // 12
    f = np.float64
    ends = [(5, 7), (5, 11), (5, 7), (0, 9), (13, 0), (17, 3), (2, 20), (21, 14), (8, 16), (21, 14)]
    ths = [0.3, 0.0, 0.0, 0.3, 0.3, 0.0, 1e-9, 0.3, 3.0, 0.3]
    while len(ends) < K:
        ends.append((int(rng.integers(0, na)), int(rng.integers(0, nb))))
        ths.append((0.0, 1e-9, 0.3, 0.3)[len(ths) % 4])
    offs = np.array([0] if split_a is None else split_a)
    cand = np.zeros(K, dtype=capi.MEAS_DTYPE)
    for k in range(K):
        (i, j), th = ends[k], ths[k]
        Z = mul(inv(pose_of(Ta, i, f)), pose_of(Tb, j, f))
        R = Z[0] @ np.asarray(exp_so3(th * MIX_AXIS, f)) if th else Z[0]
        t = Z[1] + (0.05 * rng.standard_normal(3) if th else 0.0)
        r = int(np.searchsorted(offs, i, side="right") - 1)
        cand[k]["r1"], cand[k]["p1"], cand[k]["r2"], cand[k]["p2"] = r, i - offs[r], 0, j
        cand[k]["R"], cand[k]["t"] = R.reshape(-1), t
        cand[k]["kappa"], cand[k]["tau"] = kappa * rng.uniform(0.5, 2.0), tau * rng.uniform(0.5, 2.0)
        cand[k]["weight"] = rng.uniform()  # ignored
    if K > 9:
        cand[9] = cand[7]
    return cand

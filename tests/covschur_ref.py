"""numpy statement of the marginal covariances by robot-wise Schur complement (csrc/covariance_schur.hip),
written from the formulas, on top of the dense reduced Hessian of tests/covref.py.

Pose 0 is fixed and belongs to no set.  A pose is PUBLIC when an edge between two robots names it (whatever its weight),
INTERIOR otherwise.  S = the public poses in team order, I_a = robot a's interior poses in order.  With C_a = H_II,a^-1,
B_a = H[I_a, s_a] (s_a: robot a's own public poses; an interior pose touches no other column of S), W_a = C_a B_a:
    S_c = H_SS - blockdiag_a(B_a^T W_a),   Sigma_SS = S_c^-1,
    Sigma[I_a, I_a] = C_a + W_a Sigma_SS[s_a, s_a] W_a^T,   Sigma[I_a, I_b] = W_a Sigma_SS[s_a, s_b] W_b^T  (a != b),
    Sigma[I_a, S]   = -W_a Sigma_SS[s_a, :],
    log det H_red   = sum_a log det H_II,a + log det S_c   (robots in order, the separator last)."""
import numpy as np


def partition(mp, n, num_robots, all_public=False):
    """(robot_of[n], public[n] bool) in team order for measurements already split by capi.partition (num_robots > 1) or in
    single-robot numbering.  The contiguous rule: robot of pose i = min(i // (n // N), N - 1).  all_public: every pose but
    pose 0 is put into the separator (the path then is one dense inverse)"""
    per = n // num_robots
    robot_of = np.minimum(np.arange(n) // per, num_robots - 1)
    first = np.array([np.flatnonzero(robot_of == a)[0] for a in range(num_robots)])
    public = np.zeros(n, dtype=bool)
    if num_robots > 1:
        cross = mp["r1"] != mp["r2"]
        public[first[mp["r1"][cross]] + mp["p1"][cross]] = True
        public[first[mp["r2"][cross]] + mp["p2"][cross]] = True
    if all_public:
        public[:] = True
    public[0] = False
    return robot_of, public


def rows(poses):
    """rows of H_red of the listed team poses (all >= 1)"""
    p = np.asarray(poses, dtype=np.int64)
    return (6 * (p[:, None] - 1) + np.arange(6)[None, :]).reshape(-1)


def sets(robot_of, public):
    """the separator, the interiors and their sizes: what the device partition must reproduce"""
    n = len(robot_of)
    A = int(robot_of.max()) + 1
    sep = [g for g in range(1, n) if public[g]]
    interior = [[g for g in range(1, n) if not public[g] and robot_of[g] == a] for a in range(A)]
    sep_of = [[k for k, g in enumerate(sep) if robot_of[g] == a] for a in range(A)]
    return dict(separator=sep, interior=interior, sep_of=sep_of, s=[len(x) for x in sep_of],
                largest_interior=max(len(i) for i in interior))


def schur_bytes(info):
    """the bytes of the large device buffers of the path: 8 (3 M^2 + (6 |S|)^2 + sum_a 36 |I_a| s_a +
    max_a 36 |I_a| s_a), M = max(6 max_a |I_a|, 6 |S|); the call adds the small ones (outputs, lists, scratch)"""
    ms, mi = 6 * len(info["separator"]), 6 * info["largest_interior"]
    M = max(ms, mi)
    w = [36 * len(i) * k for i, k in zip(info["interior"], info["s"])]
    return 8 * (3 * M * M + ms * ms + sum(w) + max(w))


def schur_reference(Hr, robot_of, public):
    """(Sigma, logdet, info) through the elimination; Hr dense, of order 6 (n - 1); info: sets(robot_of, public)"""
    info = sets(robot_of, public)
    sep, interior, sep_of = info["separator"], info["interior"], info["sep_of"]
    A = len(interior)
    rS = rows(sep) if sep else np.zeros(0, dtype=np.int64)
    Sc = Hr[np.ix_(rS, rS)].copy()
    Sigma = np.zeros_like(Hr)
    logdet = 0.0
    C, W, loc = {}, {}, {}
    for a in range(A):
        if not interior[a]:
            continue
        rI = rows(interior[a])
        la = (6 * np.asarray(sep_of[a], dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)  # inside the separator
        HII = Hr[np.ix_(rI, rI)]
        B = Hr[np.ix_(rI, rS[la])]
        # an interior pose touches no public pose of another robot
        other = np.setdiff1d(np.arange(len(rS)), la)
        assert not Hr[np.ix_(rI, rS[other])].any()
        C[a] = np.linalg.inv(HII)
        W[a] = C[a] @ B
        loc[a] = la
        Sc[np.ix_(la, la)] -= B.T @ W[a]
        sign, ld = np.linalg.slogdet(HII)
        assert sign > 0
        logdet += ld
    SS = np.zeros((0, 0))
    if sep:
        Sc = 0.5 * (Sc + Sc.T)
        SS = np.linalg.inv(Sc)
        sign, ld = np.linalg.slogdet(Sc)
        assert sign > 0
        logdet += ld
        Sigma[np.ix_(rS, rS)] = SS
    for a in C:
        rI = rows(interior[a])
        Sigma[np.ix_(rI, rI)] = C[a] + W[a] @ SS[np.ix_(loc[a], loc[a])] @ W[a].T
        if sep:
            X = -W[a] @ SS[loc[a], :]
            Sigma[np.ix_(rI, rS)] = X
            Sigma[np.ix_(rS, rI)] = X.T
        for b in C:
            if b != a:
                Sigma[np.ix_(rI, rows(interior[b]))] = W[a] @ SS[np.ix_(loc[a], loc[b])] @ W[b].T
    return Sigma, logdet, info

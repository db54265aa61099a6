"""numpy statement of the first-order update over a team split across participants (DESIGN.md 5j "Across teams",
dpgo_team_linear_update_across in csrc/linear_update.hip), written from the definitions.

Three parts.
    restate     steps 2-7 of the call in float64, on covschur_ref.partition's robot-wise sets and applyacross_ref's
                elimination: who holds which rows of V and of B, the compact tables T_C and B_C sorted by global pose, M from
                the gathered rows, the local outputs from B_loc and the pair blocks from the compact tables.  The blocks of
                Sigma it subtracts from are those of the float64 inverse of H_red (the path's own blocks are checked
                elsewhere).
    closures    a seeded generator on a graph of applyacross_ref.GRAPHS whose sets hold, from K = 5 on, every kind of closure
                a split invites (covers() says which, for a split).
    the measuring stick is tests/updateref.py's: updateref.update in longdouble on the blocks of the longdouble inverse of
                covref's H_red of the whole problem.  The bound is updateref.bounds' propagation with B's term widened:
                b_B + beta, column c of beta = applyref.bound(H_red, A^T)[c] = 6 (n - 1) u cond_2(H_red) |Sigma|_2 |A^T[:, c]|_2,
                the forward bound of the solve that forms B.  updateref.bounds takes no b_B, so the propagation
                is restated here with b_B as an argument; with b_B = None it is updateref.bounds' own."""
import numpy as np

from tests import applyacross_ref as XR
from tests import applyref as AR
from tests import covref
from tests import gateref as G
from tests import jointref as J
from tests import updateref as R

F = np.float64
LD = np.longdouble
U = R.U
SIZES = (1, 2, 5, 11, 22, 43)
MISTAKES = ("remote_dropped", "remote_swapped", "local_rows_only", "local_index", "pose0_read", "pair_transposed")
KEYS = ("T", "delta", "cov_diag", "cov_pairs", "xi", "xi_post", "d2_joint", "logdet_M", "logdet_R")


# ---- who holds what

def holders(g, parts):
    """(participant of every pose, the poses of every participant in team order: robots by id, then poses)"""
    part_of_robot = np.zeros(g["N"], dtype=np.int64)
    for q, ids in enumerate(parts):
        part_of_robot[list(ids)] = q
    holder = part_of_robot[g["robot_of"]]
    return holder, [np.flatnonzero(holder == q) for q in range(len(parts))]


def rows(poses):
    p = np.asarray(poses, dtype=np.int64)
    return (6 * p[:, None] + np.arange(6)[None, :]).reshape(-1)


# ---- the closures and the pairs

def fixed_closures(g):
    """the closures every set from K = 5 on begins with: pose 0 to a pose of another robot; two interior poses of one robot;
    two public poses of two robots; a closure between two further robots, twice (the same ordered pair)"""
    robot_of, public, n, N = g["robot_of"], g["public"], g["n"], g["N"]
    of = lambda a, pub: [p for p in range(1, n) if robot_of[p] == a and bool(public[p]) == pub]
    inner = next(of(a, False) for a in range(N) if len(of(a, False)) >= 2)
    if N == 1:
        return [(0, n - 2), (inner[0], inner[-1]), (n - 1, 3), (5, n // 2), (5, n // 2)]
    last = [p for p in range(n) if robot_of[p] == 1][-1]
    return [(0, last), (inner[0], inner[-1]), (of(0, True)[0], of(2, True)[-1]), (of(2, True)[0], of(1, True)[0]),
            (of(2, True)[0], of(1, True)[0])]


def kinds(g, parts, ends):
    """which kinds of closure `ends` holds under the split"""
    robot_of, public = g["robot_of"], g["public"]
    holder, _ = holders(g, parts)
    k = dict.fromkeys(("one_robot", "robots_of_one_participant", "between_participants", "pose0", "both_interior", "both_public",
                       "same_ordered_pair"), False)
    seen = set()
    for i, j in ends:
        i, j = int(i), int(j)
        k["one_robot"] |= robot_of[i] == robot_of[j]
        k["robots_of_one_participant"] |= robot_of[i] != robot_of[j] and holder[i] == holder[j]
        k["between_participants"] |= holder[i] != holder[j]
        k["pose0"] |= i == 0 or j == 0
        k["both_interior"] |= not public[i] and not public[j] and i != 0 and j != 0
        k["both_public"] |= bool(public[i] and public[j])
        k["same_ordered_pair"] |= (i, j) in seen
        seen.add((i, j))
    return k


def covers(g, parts, ends):
    """asserts that `ends` holds every kind of closure the split can have"""
    k = kinds(g, parts, ends)
    want = ["one_robot", "pose0", "both_interior", "same_ordered_pair"]
    if g["N"] > 1:
        want.append("both_public")
    if any(len(ids) > 1 for ids in parts):
        want.append("robots_of_one_participant")
    if len(parts) > 1:
        want.append("between_participants")
    missing = [w for w in want if not k[w]]
    assert not missing, (parts, missing)


def closures(g, K, seed=17, scale=0.05):
    """(ends[K, 2] global poses, Rm, tm, kappa, tau): jointref.seeded_batch on the fixed closures, the relative poses of T moved
    so that the innovation of closure k is `scale` times the unit vector of the batch's own noise draw"""
    T, n = g["T"], g["n"]
    fixed = fixed_closures(g)
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, K, seed, outliers=0.0, fixed=fixed)
    for k, (i, j) in enumerate(ends):
        Rij, tij = G.relative_pose(T, int(i), int(j), F)
        x = np.asarray(G.innovation(T, int(i), int(j), Rm[k], tm[k]), dtype=F)
        x = scale * x / np.linalg.norm(x)
        Rm[k], tm[k] = Rij @ covref.exp_so3(-x[:3]), tij - x[3:]
    if K >= 5:  # (the duplicate carries the same measurement)
        Rm[4], tm[4], kap[4], ta[4] = Rm[3], tm[3], kap[3], ta[3]
        assert [tuple(e) for e in ends[:5].tolist()] == fixed
    return ends, Rm, tm, kap, ta


def pairs_of(g):
    """pose 0; (p, p); a pair between the first and the last robot (between participants under every split of more than one)
    and its reverse; a pair inside one robot"""
    n = g["n"]
    return np.array([(0, n // 2 + 1), (n // 3, n // 3), (1, n - 1), (n - 1, 1), (n - 2, n - 3), (n - 1, 0)], dtype=np.int32)


def records(g, ends, Rm, tm, kap, ta):
    """the closures as MEAS_DTYPE records (robot, pose of the robot) of the graph's N robots"""
    from dpgo_ros_amd import capi
    robot_of = g["robot_of"]
    first = np.array([np.flatnonzero(robot_of == a)[0] for a in range(g["N"])])
    c = np.zeros(len(ends), dtype=capi.MEAS_DTYPE)
    for k, (i, j) in enumerate(ends):
        c[k]["r1"], c[k]["p1"], c[k]["r2"], c[k]["p2"] = robot_of[i], i - first[robot_of[i]], robot_of[j], j - first[robot_of[j]]
        c[k]["R"], c[k]["t"], c[k]["kappa"], c[k]["tau"] = Rm[k].reshape(-1), tm[k], kap[k], ta[k]
        c[k]["weight"] = 0.25  # ignored
    return c


# ---- steps 2-7 in float64

def restate(g, parts, ends, Rm, tm, kap, ta, pairs, mistake=None, Sigma=None):
    """the outputs in global pose order (a dict with KEYS and B, M).  mistake: one of MISTAKES --
    "remote_dropped": a participant writes J^T only for closures whose other endpoint it holds too;
    "remote_swapped": where the lower endpoint lives elsewhere, J_i^T is written in the place of J_j^T;
    "local_rows_only": M from participant 0's own rows of B, the others' left zero;
    "local_index": the compact table filled by the holder's team pose, not by the global pose;
    "pose0_read": pose 0's rows of V are written and read;
    "pair_transposed": Sigma'_pq with U_q B_p^T"""
    assert mistake is None or mistake in MISTAKES
    n, T, Hr = g["n"], np.asarray(g["T"], dtype=F), g["Hr"]
    K = len(ends)
    holder, local = holders(g, parts)
    lidx = np.zeros(n, dtype=np.int64)  # team pose of a global pose on its holder
    for poses in local:
        lidx[poses] = np.arange(len(poses))
    pr = [(int(a), int(b)) for a, b in pairs]
    # step 2: the compact set, sorted by global pose, and its table of T -- the same bytes on every participant
    comp = sorted(set(int(x) for x in np.asarray(ends).reshape(-1)) | set(x for ab in pr for x in ab))
    rank = {p: c for c, p in enumerate(comp)}
    T_C = np.concatenate([T[12 * p:12 * p + 12] for p in comp])
    cends = np.array([(rank[int(i)], rank[int(j)]) for i, j in ends], dtype=np.int64)
    jac = list(J.row_blocks(T_C, cends, F))  # (ci, Ji, cj, Jj) from the compact table alone
    # step 3: every participant's rows of V = A^T
    V = np.zeros((6 * n, 6 * K))
    for q, poses in enumerate(local):
        Vq = np.zeros((6 * len(poses), 6 * K))
        for k, (ci, Ji, cj, Jj) in enumerate(jac):
            i, j = comp[ci], comp[cj]
            both = holder[i] == q and holder[j] == q
            for p, Jp, other in ((i, Ji, Jj), (j, Jj, Ji)):
                if holder[p] != q or (p == 0 and mistake != "pose0_read"):
                    continue
                if mistake == "remote_dropped" and not both:
                    continue
                if mistake == "remote_swapped" and p == j and holder[i] != q:
                    Jp = other
                Vq[6 * lidx[p]:6 * lidx[p] + 6, 6 * k:6 * k + 6] = np.asarray(Jp, dtype=F).T
        V[rows(poses)] = Vq
    # the hook's X = Sigma V, each participant its own rows
    X = XR.eliminate(Hr, g["robot_of"], g["public"], V, mistake="pose0" if mistake == "pose0_read" else None)
    B_loc = [X[rows(poses)] for poses in local]
    # step 5: the compact B_C from the holders' rows
    B_C = np.zeros((6 * len(comp), 6 * K))
    for c, p in enumerate(comp):
        q = holder[p]
        if mistake == "local_rows_only" and q != 0:
            continue
        src = B_loc[q][6 * lidx[p]:6 * lidx[p] + 6]
        dst = lidx[p] if mistake == "local_index" and lidx[p] < len(comp) else c
        B_C[6 * dst:6 * dst + 6] = src if p != 0 or mistake == "pose0_read" else 0.0
    # step 6: everything of order 6 K on the compact tables
    A_C = np.zeros((6 * K, 6 * len(comp)))
    for k, (ci, Ji, cj, Jj) in enumerate(jac):
        A_C[6 * k:6 * k + 6, 6 * ci:6 * ci + 6], A_C[6 * k:6 * k + 6, 6 * cj:6 * cj + 6] = Ji, Jj
    Rd = np.asarray(R.r_diagonal(kap, ta, F), dtype=F)
    M = A_C @ B_C + np.diag(Rd)
    M = 0.5 * (M + M.T)
    xi = np.asarray(J.innovations(T_C, cends, Rm, tm, F), dtype=F).reshape(-1)
    if mistake is not None and np.linalg.eigvalsh(M)[0] <= 0:  # (the call would refuse with a pivot: M and B are what is left)
        return dict(B=X, M=M, refused=True)
    L = np.linalg.cholesky(M)
    Gm = np.linalg.inv(M)
    Gm = 0.5 * (Gm + Gm.T)
    z = Gm @ xi
    U_C = B_C @ Gm
    # step 7: the local outputs, placed in global order; the pair blocks from the compact tables
    if Sigma is None:
        Sigma = np.linalg.inv(Hr)
    blk = J.blocks_from_sigma(0.5 * (Sigma + Sigma.T))
    delta, diag = np.zeros((n, 6)), np.zeros((n, 6, 6))
    for q, poses in enumerate(local):
        U_loc = B_loc[q] @ Gm
        dq = -(B_loc[q] @ z)
        for l, p in enumerate(poses):
            s = slice(6 * l, 6 * l + 6)
            D = np.asarray(blk(int(p), int(p)), dtype=F) - U_loc[s] @ B_loc[q][s].T
            delta[p], diag[p] = dq[s], np.triu(D) + np.triu(D, 1).T
    cross = np.zeros((len(pr), 6, 6))
    for e, (a, b) in enumerate(pr):
        ua, bb = (rank[b], rank[a]) if mistake == "pair_transposed" else (rank[a], rank[b])
        cross[e] = np.asarray(blk(a, b), dtype=F) - U_C[6 * ua:6 * ua + 6] @ B_C[6 * bb:6 * bb + 6].T
    logdet_R = float(sum(-3 * np.log(2 * kap[k]) - 3 * np.log(ta[k]) for k in range(K)))
    return dict(B=X, M=M, xi=xi.reshape(K, 6), delta=delta, cov_diag=diag, cov_pairs=cross, xi_post=(Rd * z).reshape(K, 6),
                T=np.asarray(R.retract(T, delta.reshape(-1), F), dtype=F), d2_joint=float(xi @ z),
                logdet_M=float(2 * np.sum(np.log(np.diag(L)))), logdet_R=logdet_R)


# ---- the measuring stick

_sigma = {}


def sigma_ld(g):
    """the longdouble inverse of H_red, once per (poses, seed)"""
    key = (g["n"], g["Hr"].tobytes()[:64])
    if key not in _sigma:
        S, _ = R.spd_inverse(np.asarray(g["Hr"], dtype=LD))
        _sigma[key] = (S + S.T) / 2
    return _sigma[key]


def reference(g, ends, Rm, tm, kap, ta, pairs):
    """(updateref.update in longdouble on the blocks of the longdouble inverse of H_red, the widened bounds, updateref.bounds'
    own)"""
    n, T = g["n"], g["T"]
    ref = R.update(T, ends, Rm, tm, kap, ta, R.blocks_from_sigma(sigma_ld(g), pairs), n, pairs=pairs)
    beta = AR.bound(g["Hr"], np.asarray(ref["A"], dtype=F).T)  # 6 K figures: the solve's forward bound per column of A^T
    extra = np.broadcast_to(beta[None, :], (6 * n, len(beta))).copy()
    extra[:6] = 0.0  # (B_0 = 0 exactly)
    return ref, bounds(ref, T, ends, tm, n, pairs, extra), bounds(ref, T, ends, tm, n, pairs, None)


def bounds(ref, T, ends, tm, n, pairs=(), b_B_extra=None):
    """updateref.bounds' propagation with b_B <- b_B + b_B_extra (None: nothing added, updateref.bounds' own figures)"""
    K = len(ends)
    f = lambda a: np.abs(np.asarray(a, dtype=F))
    A, S, B, M, Gm, Um = f(ref["A"]), f(ref["S"]), f(ref["B"]), np.asarray(ref["M"], dtype=F), f(ref["G"]), f(ref["U"])
    xi, z, Rd = f(ref["xi"]).reshape(-1), f(ref["z"]), np.asarray(ref["Rd"], dtype=F)
    b_B = 24 * U * (S @ A.T)
    if b_B_extra is not None:
        b_B = b_B + b_B_extra
    b_M = 24 * U * (A @ B) + A @ b_B
    b_xi = np.array([G.xi_bound(T, int(i), int(j), tm[k]) for k, (i, j) in enumerate(ends)]).reshape(-1)
    w = np.linalg.eigvalsh(M)
    cond = w[-1] / w[0]
    e = 16 * (K + 1) * U * cond
    b_z = e * (Gm @ xi) + Gm @ (b_M @ z + b_xi)
    b_U = e * (B @ Gm) + b_B @ Gm + B @ (Gm @ b_M @ Gm)
    b_dx = (e * (B @ z) + b_B @ z + B @ b_z).reshape(n, 6)
    rw = lambda p: slice(6 * p, 6 * p + 6)

    def sig(p, q, Spq):
        return e * (Um[rw(p)] @ B[rw(q)].T) + b_U[rw(p)] @ B[rw(q)].T + Um[rw(p)] @ b_B[rw(q)].T + 2 * U * f(Spq)

    b_diag = np.array([np.maximum(sig(p, p, ref["cov_diag"][p]), sig(p, p, ref["cov_diag"][p]).T) for p in range(n)])
    b_pairs = np.array([sig(int(a), int(b), ref["cov_pairs"][q]) for q, (a, b) in enumerate(pairs)]).reshape(-1, 6, 6)
    L = np.abs(np.linalg.cholesky(M))
    b_ldM = np.sum(Gm * (b_M + 8 * K * U * (L @ L.T))) + 8 * K * U * np.sum(np.abs(2 * np.log(np.diag(L)))) + 16 * U * 6 * K
    Tn = np.asarray(ref["T"], dtype=F).reshape(n, 4, 3)
    b_T = np.zeros((n, 4, 3))
    b_T[:, :3, :] = (np.sqrt(3.0) * (2 * b_dx[:, :3].max(axis=1) + 16 * U))[:, None, None]
    b_T[:, 3, :] = b_dx[:, 3:] + 2 * U * np.abs(Tn[:, 3, :])
    return dict(B=b_B, M=b_M, xi=b_xi.reshape(K, 6), z=b_z, delta=b_dx,
                xi_post=(Rd * b_z + 2 * U * f(ref["xi_post"]).reshape(-1)).reshape(K, 6), cov_diag=b_diag, cov_pairs=b_pairs,
                d2_joint=e * (xi @ z) + xi @ b_z + b_xi @ z, logdet_M=b_ldM,
                logdet_R=(2 * K + 8) * U * float(np.sum(3 * (np.abs(np.log(2 * np.asarray(R.ref_k(ref, "kappa")))) +
                                                               np.abs(np.log(np.asarray(R.ref_k(ref, "tau"))))))),
                T=b_T.reshape(-1), cond_M=cond, e=e)


def ratios(out, ref, b, keys=KEYS):
    """error / bound per key (of a refused restatement: of M alone)"""
    if out.get("refused"):
        keys = ("M",)
    return {k: R.ratio(np.asarray(np.asarray(out[k], dtype=LD) - np.asarray(ref[k], dtype=LD), dtype=F), b[k]) for k in keys}

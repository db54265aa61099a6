"""numpy reference of the Newton refinement of a trajectory on SE(3) (csrc/refine.hip), on top of tests/covref.py
(cost, perturb, jacobian, hessian).

g(xi) = f(T [+] xi), f = 1/2 <T, T Q>, the perturbation, the layout and pose 0 held fixed are covref's.
    gradient      J^T vec(T Q) in longdouble, 6 numbers per pose (rotation rows first), pose 0's rows zero
    edge_cost     f as the sum over the measurements of w / 2 (kappa |R_j - R_i R~|^2 + tau |t_j - t_i - R_i t~|^2): the terms
                  are not negative, which <T, T Q> does not offer, so the rounding of the sum is a multiple of u f
    newton        the iteration of the device in float64 with a dense solve: X = Sigma g, the trial points T [+] (-2^-l X),
                  l = 0 .. ladder - 1, the first l with f_l <= f - armijo 2^-l g^T X + eps_f(f) taken
    eps_f         (EPS_CHAIN + ceil(edges / 256)) u f: the additions an edge's term passes through (EPS_CHAIN = 24: 16 inside
                  the term, 8 levels of the workgroup's tree) and the workgroups' partial sums added one after another
    noisy         every measurement's R~ multiplied by Exp(sigma_R z) and t~ shifted by sigma_t z, seeded
    optimum       a minimum near a start outside the positive definite basin, by Newton steps on H + mu I (the reference's own
                  tool: the library has no shift)"""
import numpy as np

from tests import covref

LD = np.longdouble
F = np.float64
U = 2.0 ** -53
EPS_CHAIN = 24
STATUS = ("converged", "max_iters", "indefinite", "no_descent")


def noisy(m, sigma_R, sigma_t, seed):
    rng = np.random.default_rng(seed)
    out = m.copy()
    for k in range(len(out)):
        R = np.asarray(out[k]["R"], dtype=F).reshape(3, 3) @ covref.exp_so3(sigma_R * rng.standard_normal(3))
        out[k]["R"] = R.reshape(-1)
        out[k]["t"] = np.asarray(out[k]["t"]) + sigma_t * rng.standard_normal(3)
    return out


def start(T, n, s, seed):
    """T perturbed by s N(0, I), pose 0 fixed"""
    xi = s * np.random.default_rng(seed).standard_normal(6 * n)
    xi[:6] = 0.0
    return covref.perturb(T, xi, n)


def edge_terms(m, T, n, dtype=F):
    """the terms of f, one per measurement"""
    P = np.asarray(T, dtype=dtype).reshape(n, 4, 3)
    out = np.zeros(len(m), dtype=dtype)
    for k, e in enumerate(m):
        i, j = int(e["p1"]), int(e["p2"])
        Ri, Rj = P[i, :3, :].T, P[j, :3, :].T
        Rm, tm = np.asarray(e["R"], dtype=dtype).reshape(3, 3), np.asarray(e["t"], dtype=dtype)
        rr = Rj - Ri @ Rm
        rt = P[j, 3, :] - P[i, 3, :] - Ri @ tm
        w = dtype(e["weight"])
        out[k] = dtype(0.5) * (w * dtype(e["kappa"]) * np.sum(rr * rr) + w * dtype(e["tau"]) * np.sum(rt * rt))
    return out


def edge_cost(m, T, n, dtype=F):
    return edge_terms(m, T, n, dtype).sum()


def eps_f(f, num_edges):
    return (EPS_CHAIN + (num_edges + 255) // 256) * U * abs(f)


def edge_bounds(m, T, n):
    """per measurement, what a float64 evaluation of its term may differ by from the exact one: the residuals are differences
    of numbers of size |R_j|, |R_i| |R~| (and |t_j|, |t_i|, |R_i| |t~|) formed to 4 u of these, squared and weighted (the first
    part, which does not shrink with the residual), and the 16 roundings of the term's own chain"""
    Ps = np.asarray(T, dtype=F).reshape(n, 4, 3)
    P = np.abs(Ps)
    b = np.zeros(len(m))
    for k, e in enumerate(m):
        i, j = int(e["p1"]), int(e["p2"])
        Ri, Rj = Ps[i, :3, :].T, Ps[j, :3, :].T
        Rm, tm = np.asarray(e["R"], dtype=F).reshape(3, 3), np.asarray(e["t"], dtype=F)
        rr, rt = np.abs(Rj - Ri @ Rm), np.abs(Ps[j, 3, :] - Ps[i, 3, :] - Ri @ tm)
        mr = np.abs(Rj) + np.abs(Ri) @ np.abs(Rm)
        mt = P[j, 3, :] + P[i, 3, :] + np.abs(Ri) @ np.abs(tm)
        b[k] = 8.0 * U * e["weight"] * (e["kappa"] * np.sum(rr * mr) + e["tau"] * np.sum(rt * mt))
    return b + 16.0 * U * np.asarray(edge_terms(m, T, n), dtype=F)


def cost_bound(m, T, n):
    """the same for the sum: the terms' bounds and the sum's own eps_f"""
    return float(edge_bounds(m, T, n).sum()) + eps_f(float(edge_cost(m, T, n)), len(m))


def gradient_from_E(T, E, n):
    """(J^T vec(E) in longdouble with pose 0's rows zero, |J|^T |vec(E)|) for a given E in the layout of T: what the per-pose rows
    of csrc/refine_block.h are checked against"""
    J = np.asarray(covref.jacobian(T, n).toarray(), dtype=LD)
    g = J.T @ np.asarray(E, dtype=LD)
    mag = np.asarray(np.abs(J).T @ np.abs(np.asarray(E, dtype=LD)), dtype=F)
    g[:6] = 0
    return g, mag


def exp_so3_ld(phi):
    phi = np.asarray(phi, dtype=LD)
    th = np.sqrt(np.sum(phi * phi))
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]], dtype=LD)
    if th < LD(1e-6):
        a, b = 1 - th * th / 6, LD(0.5) - th * th / 24
    else:
        a, b = np.sin(th) / th, 2 * (np.sin(th / 2) / th) ** 2
    return np.eye(3, dtype=LD) + a * K + b * (K @ K)


def trial_ld(T, X, alpha, n):
    """T [+] (-alpha X) in longdouble, pose 0 kept"""
    P = np.array(T, dtype=LD).reshape(n, 4, 3)
    xi = -LD(alpha) * np.asarray(X, dtype=LD).reshape(n, 6)
    for g in range(1, n):
        P[g, :3, :] = (P[g, :3, :].T @ exp_so3_ld(xi[g, :3])).T
        P[g, 3, :] += xi[g, 3:]
    return P.reshape(-1)


def final_bound(Q, Tstar, n, grad_tol):
    """|T - T*|_inf for a T with |g|_inf <= grad_tol as the device sees it: to first order xi = Sigma (g(T) - g(T*)), an entry of
    T moves by no more than its xi, so |Sigma_red|_2 (sqrt(6 (n - 1)) (grad_tol + |g(T*)|_inf) + 2 |gradient_bound|_2).
    sqrt(6 (n - 1)) takes the inf-norm of the 6 (n - 1) free entries to their 2-norm.  The gradient's rounding bound enters twice:
    grad_tol is met by the gradient as the device rounds it at T, and |g(T*)|_inf is measured with T* taken as exact while the
    device's Q and E at T* differ from the reference's by the same bound"""
    w = np.linalg.eigvalsh(hessian_red(Q, Tstar, n))
    gs = float(np.abs(np.asarray(gradient(Q, Tstar, n), dtype=F)).max())
    return (np.sqrt(6.0 * (n - 1)) * (grad_tol + gs) + 2.0 * float(np.linalg.norm(gradient_bound(Q, Tstar, n)))) / w[0]


def gradient(Q, T, n, mistake=None):
    """J^T vec(T Q), longdouble, 6 n numbers; pose 0's rows zero.  mistake: one of the planted mistakes of
    tests/test_refineref.py -- "half": the rotation rows from the antisymmetric part with its factor 1/2 kept; "pose0": pose 0's
    rows left in"""
    Tm = covref.as_matrix(T, 3, n).astype(LD)
    E = Tm @ np.asarray(Q.toarray(), dtype=LD)  # (Q is symmetric)
    J = np.asarray(covref.jacobian(T, n).toarray(), dtype=LD)
    g = J.T @ E.T.reshape(-1)
    g = g.reshape(n, 6)
    if mistake == "half":
        g[:, :3] *= LD(0.5)
    if mistake != "pose0":
        g[0] = 0
    return g.reshape(-1)


def gradient_bound(Q, T, n):
    """per entry, what the device's float64 gradient may differ by from `gradient`: (T Q)_i is a sum of 4 terms per stored block
    of row i, formed by fused multiply-adds on a Q whose entries are themselves rounded sums of up to (degree) products of three
    numbers, and a row of J^T adds 6 of its entries: (4 d + 16) u |J|^T vec(|T| |Q|), d the largest number of blocks in a row"""
    Qa = abs(Q).tocsr()
    d = int(np.diff(Qa[::4].indptr).max() // 4) + 1
    Ea = np.abs(covref.as_matrix(T, 3, n)) @ Qa.toarray()
    Ja = np.abs(covref.jacobian(T, n).toarray())
    b = (4 * d + 16) * U * (Ja.T @ Ea.T.reshape(-1))
    b[:6] = 0.0
    return b


def hessian_red(Q, T, n):
    Hr = covref.reduced(covref.hessian(Q, T, n)).toarray()
    return 0.5 * (Hr + Hr.T)


def trial(T, X, alpha, n, mistake=None):
    """T [+] (-alpha X).  mistake: "sign": + alpha X; "body": the translation moved in the body frame, t + R delta"""
    xi = (alpha if mistake == "sign" else -alpha) * np.asarray(X, dtype=F)
    if mistake == "body":
        P = np.array(T, dtype=F).reshape(n, 4, 3)
        x6 = xi.reshape(n, 6).copy()
        for g in range(n):
            x6[g, 3:] = P[g, :3, :].T @ x6[g, 3:]
        xi = x6.reshape(-1)
    return covref.perturb(T, xi, n)


def newton(m, n, T0, max_iters=10, grad_tol=1e-8, armijo=1e-4, ladder=8, backoff=None, mistake=None):
    """the iteration of dpgo_team_refine in float64.  backoff: the smallest step length of a fixed 2^-k back-off in the place of
    the ladder.  Returns a dict in the shape of Team.refine's, with `eig_min` (the smallest eigenvalue of H_red at every iterate
    a step was taken from) and `X` (the steps)"""
    Q = covref.q_full(m, n)
    T = np.array(T0, dtype=F)
    hist = dict(f=[], grad_inf=[], alpha=[], decrement=[], eig_min=[], X=[])
    status = None
    k = 0
    while True:
        g = np.asarray(gradient(Q, T, n, mistake=mistake if mistake in ("half", "pose0") else None), dtype=F)
        f = float(edge_cost(m, T, n))
        hist["f"].append(f)
        hist["grad_inf"].append(float(np.abs(g).max()))
        if hist["grad_inf"][-1] <= grad_tol:
            status = "converged"
            break
        if k == max_iters:
            status = "max_iters"
            break
        Hr = hessian_red(Q, T, n)
        w = np.linalg.eigvalsh(Hr)
        if not w[0] > 0:
            status = "indefinite"
            hist["eig_min"].append(float(w[0]))
            break
        hist["eig_min"].append(float(w[0]))
        gr = g[6:] if mistake != "pose0" else g[6:] + np.r_[g[:6], np.zeros(len(g) - 12)]
        X = np.r_[np.zeros(6), np.linalg.solve(Hr, gr)]
        dec = float(g[6:] @ X[6:])
        hist["decrement"].append(dec)
        hist["X"].append(X)
        steps = [2.0 ** -l for l in range(ladder)]
        if backoff is not None:
            steps = [2.0 ** -l for l in range(64) if 2.0 ** -l >= backoff]
        took = None
        for a in steps:
            Tl = trial(T, X, a, n, mistake=mistake if mistake in ("sign", "body") else None)
            fl = float(edge_cost(m, Tl, n))
            if fl <= f - armijo * a * dec + eps_f(f, len(m)):
                took = (a, Tl)
                break
        if took is None:
            status = "no_descent"
            break
        hist["alpha"].append(took[0])
        T = took[1]
        k += 1
    return dict(T=T, status=status, iterations=k, f0=hist["f"][0], f=hist["f"][-1], grad_inf0=hist["grad_inf"][0],
                grad_inf=hist["grad_inf"][-1], history=hist)


def optimum(m, n, T0, iters=60, tol=1e-11):
    """a minimum near T0: Newton on H_red + mu I with mu just above what makes it positive definite, step lengths backed off to
    a decrease of the cost, then the plain iteration"""
    Q = covref.q_full(m, n)
    T = np.array(T0, dtype=F)
    for _ in range(iters):
        g = np.asarray(gradient(Q, T, n), dtype=F)
        if np.abs(g).max() <= tol:
            break
        Hr = hessian_red(Q, T, n)
        lo = np.linalg.eigvalsh(Hr)[0]
        mu = 0.0 if lo > 1e-3 else 1e-2 - lo
        X = np.r_[np.zeros(6), np.linalg.solve(Hr + mu * np.eye(len(Hr)), g[6:])]
        f = float(edge_cost(m, T, n))
        a = 1.0
        while a > 1e-9:
            Tl = trial(T, X, a, n)
            if float(edge_cost(m, Tl, n)) <= f:
                break
            a *= 0.5
        T = Tl
    return T


_cases = {}


def case(name):
    """the inputs of the tests, computed once: "chain12" = covnested_ref.banded_chain(12, 1, window=8) with noise (0.02, 0.05),
    "chain40" = banded_chain(40, 3, window=8) with noise (0.05, 0.1), both at seed 7; T*: the optimum next to the ground truth.
    Returns dict(m, n, truth, Tstar, Q, clean)"""
    from tests import covnested_ref as NR
    if name not in _cases:
        n, seed, noise = dict(chain12=(12, 1, (0.02, 0.05)), chain40=(40, 3, (0.05, 0.1)))[name]
        clean, truth = NR.banded_chain(n, seed, window=8)
        m = noisy(clean, noise[0], noise[1], 7)
        Tstar = optimum(m, n, truth)
        _cases[name] = dict(m=m, n=n, truth=truth, Tstar=Tstar, Q=covref.q_full(m, n), clean=clean)
    return _cases[name]

"""numpy statement of the selection of candidate closures under a budget, in longdouble by default, written from
the definitions and not from csrc/select.hip.

Conventions of tests/gateref.py and tests/jointref.py.  P candidates, candidate k joining the team poses i_k != j_k with the
expected noise Sigma_meas,k = diag(I / (2 kappa_k), I / tau_k); M = A Sigma A^T + R is jointref.joint_M.
    given a selected set A:  S_k|A = M_kk - M_kA M_AA^-1 M_Ak,
    gain_k|A = (log det S_k|A - log det Sigma_meas,k) / 2,  log det Sigma_meas,k = -3 log(2 kappa_k) - 3 log tau_k,
    -inf where S_k|A has a non-positive pivot;  gain_k = gain_k|{};
    greedy: the open candidate of largest gain_k|A, the lower index on ties, taken while gain > min_gain and |A| < budget,
    else stop;  given: k = 0 .. budget - 1 in turn under the same test;
    gain_total = the sum of the gains at selection = (log det M_AA - log det R_A) / 2,  logdet_joint = log det M_AA.
gain_k|A is the mutual information between measurement k and the trajectory once A has been measured, and the set function
is monotone submodular (Gaussian mutual information with independent noise): greedy reaches (1 - 1 / e) of the best set."""
import numpy as np

from tests import gateref as G
from tests import jointref as J

LD = np.longdouble
U = G.U


def logdet_meas(kappa, tau, dtype=LD):
    """log det Sigma_meas,k of every candidate"""
    return -3 * np.log(2 * np.asarray(kappa, dtype=dtype)) - 3 * np.log(np.asarray(tau, dtype=dtype))


def gains(E, logdet_R):
    """gain_k|A of every candidate from the conditional blocks of the elimination E (meaningful where open)"""
    L, ok = J._chol6(E.D)
    with np.errstate(divide="ignore", invalid="ignore"):
        ld = 2 * np.sum(np.log(np.where(ok[:, None], np.einsum("kcc->kc", L), 1)), axis=1)
    return np.where(ok, 0.5 * (ld - logdet_R), E.dtype(-np.inf))


def argmax_lower_index(g, open_mask):
    """the open candidate of largest gain, the lower index on ties; -1 when none is open or none has a gain above -inf"""
    idx = np.flatnonzero(open_mask & (g > -np.inf))
    if not len(idx):
        return -1
    return int(idx[np.argmax(g[idx])])  # (argmax returns the first of equal values)


def run(M, logdet_R, budget, order="greedy", min_gain=-np.inf, pivots=None, dtype=LD):
    """Both selection rules, or (pivots given) the replay of a recorded selection order: at every step the recorded pivot is
    taken in the place of the rule's own choice, which is kept beside it with its nearest rivals, and the replay stops behind
    the last recorded pivot.  Returns a dict: gain[P] (marginal), gain_cond[P] (at the moment k was selected; for the rest:
    given the final set), rank[P], selected, num_selected, gain_total, logdet_joint, and steps: one record per selection, and
    a last one with stop=True for what is left, with
        k (the candidate taken, -1 at the stop), n_acc (|A| before), gain (of all P given A), open (mask before), choice (the
        rule's own candidate), near (the up to four open candidates of largest gain), stop, rows (for k, choice and near, at
        the stop for every open candidate: mag_D, S, gain in float64)."""
    E = J.Elimination(M, np.zeros(len(M)), dtype)
    P = E.K
    ldR = np.asarray(logdet_R, dtype=dtype)
    rank = np.full(P, -1)
    gain_cond = np.zeros(P, dtype=dtype)
    at, steps = [], []

    def record(k, g, choice, stop=False):
        idx = np.flatnonzero(E.open)
        near = idx[np.argsort(-g[idx], kind="stable")[:4]]
        want = set(int(r) for r in (idx if stop else near)) | set(int(r) for r in (k, choice) if r >= 0)
        rows = {r: dict(mag_D=np.asarray(E.mag_D[r], dtype=np.float64), S=np.asarray(E.D[r], dtype=np.float64), gain=float(g[r]))
                for r in want}
        steps.append(dict(k=int(k), n_acc=len(E.accepted), gain=g.copy(), open=E.open.copy(), choice=int(choice),
                          near=[int(r) for r in near], rows=rows, stop=stop))

    g = gains(E, ldR)
    marginal = g.copy()
    for s in range(int(budget)):
        if order == "greedy":
            choice = argmax_lower_index(g, E.open)
        elif order == "given":
            choice = s
        else:
            raise ValueError(order)
        if pivots is not None:
            if s >= len(pivots):
                break
            k = int(pivots[s])
        else:
            k = choice
            if k < 0 or not g[k] > min_gain:
                break
        record(k, g, choice)
        gain_cond[k], rank[k] = g[k], s
        at.append(g[k])
        E.pivot(k)
        g = gains(E, ldR)
    rest = E.open.copy()
    if rest.any():
        record(-1, g, argmax_lower_index(g, E.open) if order == "greedy" else -1, stop=True)
        gain_cond[rest] = g[rest]
    total = dtype(0)
    for v in at:
        total = total + v
    return dict(gain=marginal, gain_cond=gain_cond, rank=rank, selected=np.array(E.accepted, dtype=int), num_selected=len(E.accepted),
                gain_total=total, logdet_joint=E.logdet, steps=steps)


def set_value(M, logdet_R, subset, dtype=LD):
    """(log det M_AA - log det R_A) / 2 of a set, straight from the definition"""
    if not len(subset):
        return dtype(0)
    rows = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in subset])
    MA = np.asarray(M, dtype=dtype)[np.ix_(rows, rows)]
    n = len(rows)  # (numpy's LAPACK takes no longdouble: Cholesky written out)
    Lf = np.zeros((n, n), dtype=dtype)
    for c in range(n):
        p = MA[c, c] - Lf[c, :c] @ Lf[c, :c]
        assert p > 0
        Lf[c, c] = np.sqrt(p)
        Lf[c + 1:, c] = (MA[c + 1:, c] - Lf[c + 1:, :c] @ Lf[c, :c]) / Lf[c, c]
    return 0.5 * (2 * np.sum(np.log(np.diag(Lf))) - np.sum(np.asarray(logdet_R, dtype=dtype)[list(subset)]))


# ---- the error bounds the tests hold csrc/select.hip and csrc/select_block.h to; u = 2.2e-16, every constant one of
# tests/gateref.py or tests/jointref.py.  tests/test_selectref.py shows that each of them rejects the mistakes the conventions
# invite.

def d_bound(T, i, j, blk):
    """elementwise on D_k = M_kk: jointref.m_block_bound of the block (k, k)"""
    return J.m_block_bound(T, i, j, i, j, blk)


def s_bound(row, n_acc, cond_A, b_D):
    """elementwise on S_k|A: the rounding of M_kk itself, b_D, and the elimination of |A| = n_acc pivots,
    elimination_constant(|A|) u cond_2(M_AA) mag_D with mag_D the sum of the absolute terms the block was formed from.  The
    blocks M_kp of the pivots' columns are formed on the fly, each within m_block_bound <= 32 u x its absolute terms; they enter
    S_k|A through the products W W^T that mag_D sums, and 32 <= elimination_constant(|A|) for |A| >= 1, so the second term
    carries them.  With A empty it vanishes against b_D by at least the factor 2 of 32 / 16 and is kept for uniformity."""
    return b_D + J.elimination_constant(n_acc) * U * cond_A * row["mag_D"]


def gain_bound(row, b_S, ld_meas):
    """on gain = (log det S - log det Sigma_meas) / 2: half of
        sum_ab |S^-1|_ab b_S,ab       the first-order perturbation of log det (d log det S = tr(S^-1 dS)),
        100 u cond_2(S)               the 6 x 6 factorisation's own term in the idiom of gateref.d2_bound: the factor is that of
                                      S + dS with |dS| <= 8 u |L| |L|^T, so tr(S^-1 dS) <= 6 x 8 u cond_2(S), doubled,
        16 u (|log det S| + |log det Sigma_meas|)   six logarithms and their sum on either side, gamma_8 and a half over;
    inf where the gain is -inf"""
    if not np.isfinite(row["gain"]):
        return np.inf
    S = row["S"]
    ld_S = 2 * row["gain"] + float(ld_meas)
    return 0.5 * (np.sum(np.abs(np.linalg.inv(S)) * b_S) + 100 * U * np.linalg.cond(S) + 16 * U * (abs(ld_S) + abs(float(ld_meas))))


def step_bound(step, r, cond_A, b_D, ld_meas):
    """the gain bound of candidate r of a step's rows given cond_A = cond_2(M_AA) of the set selected before it"""
    row = step["rows"][int(r)]
    return gain_bound(row, s_bound(row, step["n_acc"], cond_A, b_D), ld_meas)


# ---- seeded pools of candidates

def seeded_pool(T, n, P, seed, fixed=(), duplicates=()):
    """P candidates on seeded pairs of the n poses of T with kappa and tau spread as jointref.seeded_batch spreads them:
    ends[P, 2], kappa[P], tau[P].  The first len(fixed) pairs are `fixed`; duplicates: (record, its exact copy further on)."""
    ends, _, _, kap, ta, _ = J.seeded_batch(T, n, P, seed, outliers=0.0, fixed=fixed)
    for src, dst in duplicates:
        if dst < P:
            ends[dst], kap[dst], ta[dst] = ends[src], kap[src], ta[src]
    return ends, kap, ta


# ---- what the host build and the device are held to, in one place (tests/test_select_host.py, tests/test_gpu_select.py)

def check_marginal(out, M, ld_R, b_D, worst):
    """gain against the reference on the same blocks: D_k = M_kk within b_D, nothing eliminated"""
    M = np.asarray(M, dtype=LD)
    E = J.Elimination(M, np.zeros(len(M)))
    g = gains(E, np.asarray(ld_R, dtype=LD))
    for k in range(E.K):
        row = dict(S=np.asarray(E.D[k], dtype=np.float64), mag_D=np.asarray(E.mag_D[k], dtype=np.float64), gain=float(g[k]))
        b = gain_bound(row, s_bound(row, 0, 1.0, b_D[k]), ld_R[k])
        e = abs(out["gain"][k] - float(g[k]))
        worst["gain"] = max(worst.get("gain", 0.0), e / b)
        assert e <= b, (k, e, b)


def check_replay(out, M, ld_R, b_D, order, budget, worst, every=1):
    """the selection order of `out` replayed in the reference on M: at every step the gain reported for the pick within its
    bound and (greedy) the pick's gain within the sum of the two bounds of the rule's own choice; the gains at selection do not
    increase beyond the bounds (greedy); what is left at the end within its bounds; the ranks; gain_total the sum in selection
    order bit for bit and within the summed bounds, logdet_joint within jointref's elimination bound.  Returns the reference."""
    sel = [int(k) for k in out["selected"]]
    P = len(ld_R)
    assert len(sel) == out["num_selected"] <= budget and len(set(sel)) == len(sel)
    assert (np.sort(out["rank"][sel]) == np.arange(len(sel))).all() and ((out["rank"] >= 0).sum() == len(sel)) and (out["rank"] >= -1).all()
    assert [int(out["rank"][k]) for k in sel] == list(range(len(sel)))
    ref = run(M, ld_R, budget, order, pivots=sel)
    conds = J.prefix_conditions(M, sel, every)
    assert (ref["rank"] == out["rank"]).all()
    total, b_total, prev = 0.0, 0.0, None
    for s in ref["steps"]:
        cA = conds[s["n_acc"]]
        if s["stop"]:
            for r in sorted(s["rows"]):
                b = step_bound(s, r, cA, b_D[r], ld_R[r])
                e = abs(out["gain_cond"][r] - float(ref["gain_cond"][r]))
                if np.isfinite(b):
                    worst["gain_left"] = max(worst.get("gain_left", 0.0), e / b)
                    assert e <= b, (r, s["n_acc"], e, b)
                else:
                    assert out["gain_cond"][r] == -np.inf
            continue
        k = s["k"]
        b = step_bound(s, k, cA, b_D[k], ld_R[k])
        e = abs(out["gain_cond"][k] - float(ref["gain_cond"][k]))
        worst["gain_cond"] = max(worst.get("gain_cond", 0.0), e / b)
        assert e <= b, (k, s["n_acc"], e, b)
        if order == "greedy":
            c = s["choice"]
            short = float(s["gain"][c] - s["gain"][k])
            two = b + step_bound(s, c, cA, b_D[c], ld_R[c])
            worst["rule"] = max(worst.get("rule", 0.0), short / two)
            assert short <= two, (k, c, s["n_acc"], short, two)
            if prev is not None:
                assert out["gain_cond"][k] <= prev[0] + prev[1] + b, (k, s["n_acc"])
            prev = (out["gain_cond"][k], b)
        else:
            assert k == s["n_acc"]
        total += out["gain_cond"][k]
        b_total += b
    if order == "greedy" and len(sel) < min(budget, P):  # stopped early: nothing open had a gain above the threshold
        assert ref["steps"][-1]["stop"]
    assert out["gain_total"] == total, "gain_total is not the sum of gain_cond[selected] in selection order"
    assert abs(out["gain_total"] - float(ref["gain_total"])) <= b_total + 16 * U * len(sel) * abs(float(ref["gain_total"]))
    tol = J.elimination_constant(len(sel)) * U * conds[len(sel)] * 6 * max(len(sel), 1)
    worst["logdet_joint"] = max(worst.get("logdet_joint", 0.0), abs(out["logdet_joint"] - float(ref["logdet_joint"])) / tol)
    assert abs(out["logdet_joint"] - float(ref["logdet_joint"])) <= tol
    return ref

"""GPU checks of pairwise consistency maximisation (csrc/consistency.hip, capi.pairwise_consistency).

The graphs are covnested_ref.banded_chain(24, seed, window=8): noise-free, the ground truth is an exact minimum, no solve.
Team A has seed 3, team B seed 5 in a gauge moved by a seeded G (tests/pcmref.py, planted_case).

Bounds (u = 2.2e-16; derived in the docstring of tests/pcmref.py, and tests/test_pcmref.py shows that they reject a swapped
candidate, a reversed segment, a Z_l that is not inverted, a flipped [.]x and a wrong noise model by more than 1000 x):
  the kernel alone, against pcmref in longdouble on the Sigma_rel that Team.relative_covariances returns for the same pairs --
    d2 within gateref.d2_bound of the elementwise bounds on S (128 u sum_X Jbar |Sigma_X| Jbar^T) and on xi (XI_R_BOUND for
    residual angles up to 3.0 rad, 160 u sbar for the translation), plus 100 u cond_2(S) d2 for the 6 x 6 solve; beyond 3.0 rad
    d2 is only required to be finite;
  end to end, against the numpy inverse of each dense reduced Hessian --
    B_X = 6 (n - 1) u cond_2(H_red) |Sigma|_F is what the covariance tests hold team X's blocks to, so a segment's Sigma_rel is
    within |[J_i J_j]|_2^2 B_X in the Frobenius norm (5f), S within |J_A|_2^2 times that of team A plus |J_B|_2^2 times that of
    team B, and d2 within |S^-1 xi|^2 times that plus the kernel's own bound above.
Every test prints its largest error / bound."""
import ctypes as C
import itertools

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import covnested_ref as NR
from tests import covref
from tests import gateref as G
from tests import pcmref as P
from tests.test_gpu_covariance_nested import team_of

pytestmark = pytest.mark.gpu

F = np.float64
N_POSES = P.PLANTED["n"]
NESTED_BLOCK = 6
COUNTS = (1, 2, 63, 64, 65, 129)
METHOD_CODE = dict(dense=capi.GATE_DENSE, schur=capi.GATE_SCHUR, nested=capi.GATE_NESTED)


@pytest.fixture(scope="module")
def graphs():
    ma, Ta, mb, Tb, cand, is_true = P.planted_case()
    return dict(ma=ma, Ta=Ta, mb=mb, Tb=Tb, planted=cand, is_true=is_true, mixed=P.mixed_candidates(Ta, Tb, max(COUNTS), seed=2))


def block(method):
    return NESTED_BLOCK if method == "nested" else None


def call(ta, tb, cand, g, method, **kw):
    return capi.pairwise_consistency(ta, tb, cand, g["Ta"], g["Tb"], method=method, max_block=block(method), **kw)


def sigma_lookup(t, T, pairs, method):
    """{(a, b): Sigma_rel} from Team.relative_covariances for the listed ordered pairs"""
    if not pairs:
        return {}
    rel = t.relative_covariances(list(pairs), T, method=method, max_block=block(method))
    return {p: rel[k] for k, p in enumerate(pairs)}


def reference(cand, g, i, j, pairs, sa, sb):
    """per pair (k, l): (d2, bound on d2, residual angle) of pcmref in longdouble on the given Sigma_rel"""
    out = {}
    for k, l in pairs:
        args = P.pair_inputs(cand, g["Ta"], g["Tb"], i, j, k, l, lambda a, b: sa[(a, b)], lambda a, b: sb[(a, b)])
        xi, d2, S = P.pair(*args)
        _, _, b_d = P.bounds(cand, g["Ta"], g["Tb"], i, j, k, l, args, xi, S, d2)
        out[(k, l)] = (float(d2), b_d, float(np.linalg.norm(np.asarray(xi[:3], dtype=F))))
    return out


@pytest.mark.parametrize("method,robots_a", [("dense", 1), ("schur", 1), ("nested", 1), ("schur", 2)])
def test_kernel_against_the_reference_at_wave_and_word_edges(graphs, method, robots_a):
    g = graphs
    split = None if robots_a == 1 else [0, N_POSES // 2]
    cand = g["mixed"] if split is None else P.mixed_candidates(g["Ta"], g["Tb"], max(COUNTS), seed=2, split_a=split)
    ta, tb = team_of(g["ma"], N_POSES, robots_a, g["Ta"]), team_of(g["mb"], N_POSES, 1, g["Tb"])
    if method == "nested":
        assert ta.covariance_plan(NESTED_BLOCK)[1]["promoted_poses"] > 0
    offs_a = {r: o for r, o in enumerate(split or [0])}
    i, j = P.endpoints(cand, offs_a, {0: 0})
    assert i[1] == i[0] and (i[2], j[2]) == (i[0], j[0]) and i[3] == 0 and j[4] == 0 and cand[9].tobytes() == cand[7].tobytes()
    # the reference, once: every pair below 65 and a seeded sample of the pairs that reach beyond the first word
    rng = np.random.default_rng(6)
    K = max(COUNTS)
    pairs = list(itertools.combinations(range(65), 2))
    pairs += sorted({(int(k), int(l)) for k, l in zip(rng.integers(0, K, 300), rng.integers(65, K, 300)) if k < l} | {(0, 128), (64, 128), (127, 128)})
    pa, pb = P.segment_pairs(i, j)
    sa, sb = sigma_lookup(ta, g["Ta"], list(pa), method), sigma_lookup(tb, g["Tb"], list(pb), method)
    ref = reference(cand, g, i, j, pairs, sa, sb)
    thr2 = capi.error_threshold_at_quantile(0.99, 6) ** 2
    worst, checked, first = 0.0, 0, None
    for K in COUNTS:
        out = call(ta, tb, cand[:K], g, method)
        d2 = out["d2"]
        assert d2.shape == (K, K) and out["consistent"].shape == (K, K)
        assert d2.tobytes() == np.ascontiguousarray(d2.T).tobytes() and not d2.diagonal().any()
        assert (out["consistent"] == ((d2 <= thr2) & ~np.eye(K, dtype=bool))).all()
        assert out["proven"] and out["consistent"][np.ix_(out["inliers"], out["inliers"])].sum() == len(out["inliers"]) * (len(out["inliers"]) - 1)
        if K == 1:
            assert out["inliers"].tolist() == [0] and out["res_a"].n == 0 and out["res_b"].n == 0
            continue
        if K > 2:  # (candidates 0 and 1 share their pose of team A: with K = 2 that team has no segment and is not asked)
            assert out["res_a"].n == 6 * (N_POSES - 1) == out["res_b"].n and out["res_a"].min_pivot > 0
        else:
            assert out["res_a"].n == 0 and out["res_b"].n == 6 * (N_POSES - 1)
        for (k, l), (rd, bd, angle) in ref.items():
            if l >= K:
                continue
            if angle > 3.0 + 1e-9:
                assert np.isfinite(d2[k, l])
                continue
            checked += 1
            worst = max(worst, abs(d2[k, l] - rd) / bd)
            assert abs(d2[k, l] - rd) <= bd, (K, k, l, d2[k, l], rd, bd)
        if K > 9:  # the duplicate: the bits of the original, and a zero distance between the two
            rest = np.setdiff1d(np.arange(K), [7, 8, 9])  # (against 8 the two stand on different sides of the ordered pair)
            assert d2[7, rest].tobytes() == d2[9, rest].tobytes() and d2[7, 9] <= 1e-20
        # the exact candidates agree with each other exactly
        exact = [q for q in (1, 2, 5) if q < K]
        assert all(d2[a, b] <= 1e-18 for a, b in itertools.combinations(exact, 2))
        if K == 65:
            first = d2.copy()
        if K == 129:  # the same pairs in a larger call: the same bits
            assert d2[:65, :65].tobytes() == first.tobytes()
    print("%s, team A as %d robot(s): %d comparisons, largest |d2 - ref| / bound %.3g" % (method, robots_a, checked, worst))
    assert checked > 4000
    ta.close()
    tb.close()


def raw_call(ta, Ta, tb, Tb, method, max_block, cand, quantile, max_nodes, out, num=None, skip=()):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    arg = lambda name: None if name in skip else (C.byref(out[name]) if not isinstance(out[name], np.ndarray) else p(out[name]))
    return capi.lib().dpgo_team_pairwise_consistency(
        None if ta is None else ta.h, p(Ta), None if tb is None else tb.h, p(Tb), method, max_block, len(cand) if num is None else num,
        p(cand), C.c_double(quantile), C.c_longlong(max_nodes), arg("d2"), arg("adj"), arg("members"), arg("size"), arg("proven"),
        arg("res_a"), arg("res_b"))


def fresh_outputs(K, fill=7.25):
    W = (K + 63) // 64
    return dict(d2=np.full((K, K), fill), adj=np.full((K, W), 0x5555555555555555, dtype=np.uint64), members=np.full(K, -7, dtype=np.int32),
                size=C.c_int(-7), proven=C.c_int(-7), res_a=capi.Covariance(), res_b=capi.Covariance())


def test_bits(graphs):
    g = graphs
    ta, tb, tb2 = (team_of(g["ma"], N_POSES, 1, g["Ta"]), team_of(g["mb"], N_POSES, 1, g["Tb"]), team_of(g["ma"], N_POSES, 1, g["Ta"]))
    K = 70
    cand = g["mixed"][:K]
    thr2 = capi.error_threshold_at_quantile(0.9, 6) ** 2
    for method in ("dense", "schur", "nested"):
        outs = []
        for _ in range(2):
            o = fresh_outputs(K)
            assert raw_call(ta, g["Ta"], tb, g["Tb"], METHOD_CODE[method], NESTED_BLOCK, cand, 0.9, 0, o) == capi.OK, capi.lib().dpgo_last_error()
            outs.append(o)
        a, b = outs
        assert a["d2"].tobytes() == b["d2"].tobytes() and a["adj"].tobytes() == b["adj"].tobytes()
        assert a["members"].tobytes() == b["members"].tobytes() and a["size"].value == b["size"].value
        for r in ("res_a", "res_b"):  # (the record also holds the times of the call)
            assert (a[r].n, a[r].logdet, a[r].min_pivot, a[r].max_pivot) == (b[r].n, b[r].logdet, b[r].min_pivot, b[r].max_pivot)
        d2 = a["d2"]
        assert d2.tobytes() == np.ascontiguousarray(d2.T).tobytes() and not d2.diagonal().any()
        # every bit of every word, the 58 columns at and beyond K included
        bits = np.unpackbits(np.ascontiguousarray(a["adj"]).view(np.uint8).reshape(K, -1), axis=1, bitorder="little").astype(bool)
        assert bits.shape == (K, 128)
        assert not bits[:, K:].any() and not bits[:, :K].diagonal().any()
        assert (bits[:, :K] == ((d2 <= thr2) & ~np.eye(K, dtype=bool))).all()
        # the segment records: Sigma_rel is Team.relative_covariances bit for bit, R and t the relative pose
        i, j = P.endpoints(cand, {0: 0}, {0: 0})
        for t, T, pairs in ((ta, g["Ta"], list(P.segment_pairs(i, j)[0])), (tb, g["Tb"], list(P.segment_pairs(i, j)[1]))):
            pr = np.array(pairs, dtype=np.int32)
            rec, res = np.zeros((len(pr), 48)), capi.Covariance()
            assert capi.lib().dpgo_internal_segment_records(t.h, T.ctypes.data_as(C.c_void_p), METHOD_CODE[method], NESTED_BLOCK, len(pr),
                                                            pr.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), C.byref(res)) == capi.OK
            rel = t.relative_covariances(pr, T, method=method, max_block=block(method))
            assert rec[:, 12:].tobytes() == rel.tobytes()
            for k, (x, y) in enumerate(pairs[:20]):
                R, tt = G.relative_pose(T, x, y, F)
                assert np.abs(rec[k, :9] - R.reshape(-1)).max() <= 8 * G.U and np.abs(rec[k, 9:12] - tt).max() <= 16 * G.U * 20
    # the same handle as A and B: the bits of two equal teams
    same = P.mixed_candidates(g["Ta"], g["Ta"], 40, seed=4)
    one = capi.pairwise_consistency(ta, ta, same, g["Ta"], g["Ta"], method="schur")
    two = capi.pairwise_consistency(ta, tb2, same, g["Ta"], g["Ta"], method="schur")
    assert one["d2"].tobytes() == two["d2"].tobytes() and (one["consistent"] == two["consistent"]).all()
    assert one["inliers"].tobytes() == two["inliers"].tobytes()
    for t in (ta, tb, tb2):
        t.close()


def test_planted_case_end_to_end(graphs):
    g = graphs
    cand, is_true = g["planted"], g["is_true"]
    ta, tb = team_of(g["ma"], N_POSES, 1, g["Ta"]), team_of(g["mb"], N_POSES, 1, g["Tb"])
    n = N_POSES
    dense = [covref.dense_reference(covref.q_full(m, n), T, n) for m, T in ((g["ma"], g["Ta"]), (g["mb"], g["Tb"]))]
    Bx = [6 * (n - 1) * G.U * (w[-1] / w[0]) * np.linalg.norm(S) for _, S, w in dense]
    sig = [P.sigma_from_dense(T, S) for T, (_, S, _) in zip((g["Ta"], g["Tb"]), dense)]
    i, j = P.endpoints(cand, {0: 0}, {0: 0})
    K = len(cand)
    ref = {}
    for k, l in itertools.combinations(range(K), 2):
        args = P.pair_inputs(cand, g["Ta"], g["Tb"], i, j, k, l, sig[0], sig[1])
        xi, d2, S = P.pair(*args)
        _, _, b_kernel = P.bounds(cand, g["Ta"], g["Tb"], i, j, k, l, args, xi, S, d2)
        Jl, JA, Jk, JB = P.jacobians(*args[:4], dtype=F)
        es = 0.0
        for T, (x, y), J, B in ((g["Ta"], (i[l], i[k]), JA, Bx[0]), (g["Tb"], (j[k], j[l]), JB, Bx[1])):
            if x != y:
                es += np.linalg.norm(J, 2) ** 2 * np.linalg.norm(np.c_[G.jacobians(T, x, y, F)], 2) ** 2 * B
        w = np.linalg.solve(np.asarray(S, dtype=F), np.asarray(xi, dtype=F))
        ref[(k, l)] = (float(d2), (w @ w) * es + b_kernel, float(np.linalg.norm(np.asarray(xi[:3], dtype=F))))
    for method in ("dense", "schur", "nested"):
        out = call(ta, tb, cand, g, method, quantile=P.PLANTED["quantile"])
        assert out["proven"] and out["inliers"].tolist() == np.flatnonzero(is_true).tolist() and len(out["inliers"]) == P.PLANTED["inliers"]
        worst = 0.0
        for (k, l), (rd, bd, angle) in ref.items():
            if angle > 3.0 + 1e-9:
                assert np.isfinite(out["d2"][k, l])
                continue
            worst = max(worst, abs(out["d2"][k, l] - rd) / bd)
            assert abs(out["d2"][k, l] - rd) <= bd, (method, k, l, out["d2"][k, l], rd, bd)
        for o in np.flatnonzero(~is_true):
            assert out["consistent"][o, is_true].sum() <= 1
        print("%s: the planted %d of %d recovered, largest |d2 - ref| / end-to-end bound %.3g" % (method, len(out["inliers"]), K, worst))
    ta.close()
    tb.close()


def test_refusals_leave_the_outputs_untouched(graphs):
    g = graphs
    ta, tb = team_of(g["ma"], N_POSES, 2, g["Ta"]), team_of(g["mb"], N_POSES, 1, g["Tb"])
    good = P.mixed_candidates(g["Ta"], g["Tb"], 5, seed=2, split_a=[0, N_POSES // 2])  # (both teams have segments)
    K = len(good)
    o = fresh_outputs(K)
    blank = {k: (v.copy() if isinstance(v, np.ndarray) else None) for k, v in o.items()}

    def refused(what, cand=good, method=capi.GATE_DENSE, max_block=0, quantile=0.99, max_nodes=0, A=ta, B=tb, Ta=g["Ta"], Tb=g["Tb"], **kw):
        o["res_a"].n = o["res_b"].n = 5
        rc = raw_call(A, Ta, B, Tb, method, max_block, cand, quantile, max_nodes, o, **kw)
        msg = capi.lib().dpgo_last_error().decode()
        assert rc == capi.ERR and what in msg, (rc, msg)
        for k in ("d2", "adj", "members"):
            assert o[k].tobytes() == blank[k].tobytes(), k
        assert o["size"].value == -7 and o["proven"].value == -7 and o["res_a"].n == 5 and o["res_b"].n == 5
        return msg

    refused("num must be positive", num=0)
    refused("num must be positive", num=-1)
    for name in ("members", "size", "proven", "res_a", "res_b"):
        refused("null argument", skip=(name,))
    refused("null argument", A=None)
    refused("null argument", Tb=None)
    refused("method must be", method=3)
    refused("method must be", method=-1)
    for q in (0.0, 1.0, -0.5, 1.5, float("nan")):
        refused("quantile must lie inside (0, 1)", quantile=q)
    refused("max_nodes must not be negative", max_nodes=-1)

    def changed(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k][1] = v
        return c

    refused("candidate 1 names robot 2, which is not in team A", changed(r1=2))
    refused("candidate 1 names robot 1, which is not in team B", changed(r2=1))
    refused("candidate 1 names pose 12 of robot 0 of team A", changed(r1=0, p1=12))
    refused("candidate 1 names pose -1 of robot 0 of team B", changed(p2=-1))
    refused("candidate 1 names pose 24 of robot 0 of team B", changed(p2=24))
    refused("candidate 1 has kappa", changed(kappa=0.0))
    refused("candidate 1 has kappa", changed(tau=-1.0))
    refused("candidate 1 has kappa", changed(kappa=float("inf")))
    bad = good.copy()
    bad["R"][1][0] *= 1.001
    refused("the measurement of candidate 1 is not in SE(3)", bad)
    bad = good.copy()
    bad["t"][1][2] = float("nan")
    refused("the measurement of candidate 1 is not in SE(3)", bad)
    # carried over from the covariance path of either team, with its own message
    Tbad = g["Tb"].copy()
    Tbad[12 * 17] *= 1.001
    refused("pose 17 of T is not in SE", Tb=Tbad)
    Ts = NR.spoil_rotations(g["Ta"], N_POSES, [9, 10, 11], 50)
    w = np.linalg.eigvalsh(covref.reduced(covref.hessian(covref.q_full(g["ma"], N_POSES), Ts, N_POSES)).toarray())
    assert w[0] < -1e-3 * w[-1], "the spoiled trajectory is still a minimum"
    for method, mb in ((capi.GATE_DENSE, 0), (capi.GATE_SCHUR, 0), (capi.GATE_NESTED, NESTED_BLOCK)):
        msg = refused("non-positive pivot", Ta=Ts, method=method, max_block=mb)
        assert "not a minimum" in msg and msg.startswith("marginal_covariances"), msg
    # a disconnected team A: the path's own message
    cut = g["ma"][~((g["ma"]["p1"] < 12) & (g["ma"]["p2"] >= 12))]
    tc = team_of(cut, N_POSES, 1, g["Ta"])
    one = P.mixed_candidates(g["Ta"], g["Tb"], 5, seed=2)
    o["res_a"].n = o["res_b"].n = 5
    rc = raw_call(tc, g["Ta"], tb, g["Tb"], capi.GATE_DENSE, 0, one, 0.99, 0, o)
    msg = capi.lib().dpgo_last_error().decode()
    assert rc == capi.ERR and msg.startswith("marginal_covariances") and o["d2"].tobytes() == blank["d2"].tobytes() and o["size"].value == -7, msg
    print("a disconnected team A:", msg)
    with pytest.raises(ValueError, match="method must be"):
        capi.pairwise_consistency(ta, tb, good, g["Ta"], g["Tb"], method="sparse")
    with pytest.raises(capi.DpgoError, match="quantile"):
        capi.pairwise_consistency(ta, tb, good, g["Ta"], g["Tb"], quantile=1.0)
    for t in (ta, tb, tc):
        t.close()

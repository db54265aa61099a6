"""GPU checks of the first-order update over a team split across participants (dpgo_team_linear_update_across,
csrc/linear_update.hip behind csrc/covariance_schur.hip; Team.linear_update with transport=; DESIGN.md 5j "Across teams"):
LocalGroup threads on one device, on the four graphs of tests/applyacross_ref.py with T the ground truth, the teams set to the
lifted T and nothing solved.  The splits are test_gpu_covariance_apply_across.SPLITS; 6 N_loc is never a multiple of 64
(asserted).  K = 1, 2, 5, 11, 22, 43 closures and the pairs of tests/updateacross_ref.py.
  1. every output of every participant, assembled in global order, within updateacross_ref's widened bound of the longdouble
     update; error / bound is printed per key, and beside it the ratio against the unwidened updateref.bounds
  2. every split gives the bits of the one-participant call (T, delta, cov_diag row for row; cov_pairs, xi, xi_post and the three
     scalars on every participant); two calls give the same bytes; cov_diag is bitwise symmetric; on its holder pose 0 has delta
     and cov_diag zero bits and T unchanged bits; the Covariance scalars are those of covariances(transport=) with the same
     pairs, and the transport calls are that call's plus ADDED_ALLGATHERS
  3. against the joined single team's linear_update(columns="solve") by "nested" at max_block = 6 and by "dense": within the sum
     of both bounds; xi bit for bit (the same kernel on the same bytes of T)
  4. information_gain == (logdet_M - logdet_R) / 2 > 0, and no trace of cov_diag grows
  5. global_X(), the weights and cost() are untouched on every team
  6. every refusal reaches every participant with its words, sentinel-filled outputs untouched and *res zero, and a good call
     behind each gives check 2's bits
No test provokes a device fault: a spoiled T is refused by a pivot, which the host reads from the factorisation's status.
Each test prints its largest error / bound (DESIGN.md 5j records them)."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyacross_ref as XR
from tests import covnested_ref as NR
from tests import updateacross_ref as UX
from tests.test_gpu_certify_across import JOIN, Split, _expect_refusal, bits
from tests.test_gpu_covariance_across import scalars
from tests.test_gpu_covariance_apply_across import G12, G40, SPLITS, state
from tests.test_gpu_covariance_nested import team_of

pytestmark = pytest.mark.gpu

F = np.float64
ADDED_ALLGATHERS = 2  # T of the compact poses, and their rows of B: whatever K, the pairs and the split
LOCAL = ("T", "delta", "cov_diag")
COMMON = ("cov_pairs", "xi", "xi_post")
FIGURES = ("d2_joint", "logdet_M", "logdet_R")
_case = {}


def update_split(sp, g, cand, pairs, group=None):
    """Team.linear_update on every participant with its poses of T: the dicts in rank order"""
    return sp.run(lambda tm, tr: tm.linear_update(cand, g["T"][sp.cols(tr.rank, 12)], pairs=pairs, transport=tr, owner_of_robot=sp.owner),
                  group)


def assemble(sp, outs, n):
    out = dict(T=np.full(12 * n, np.nan), delta=np.full((n, 6), np.nan), cov_diag=np.full((n, 6, 6), np.nan))
    for q, o in enumerate(outs):
        poses = sp.cols(q, 1)
        out["T"][sp.cols(q, 12)], out["delta"][poses], out["cov_diag"][poses] = o["T"], o["delta"], o["cov_diag"]
    for k in COMMON + FIGURES + ("information_gain",):
        out[k] = outs[0][k]
    return out


def case(key):
    """the graph, the lifted iterate, and per K the closures, their records, the longdouble reference with both bounds and the
    one-participant call's dict: computed once per graph and left unchanged"""
    if key not in _case:
        n, seed, N = key
        g = dict(XR.graph(n, seed, N))
        t = team_of(g["m"], n, N, g["T"])
        g["X0"] = t.global_X()
        t.close()
        g["pairs"] = UX.pairs_of(g)
        sp = Split(g["mp"], N, [list(range(N))], g["X0"])
        g["K"] = {}
        for K in UX.SIZES:
            cl = UX.closures(g, K)
            cand = UX.records(g, *cl)
            ref, b, b0 = UX.reference(g, *cl, g["pairs"])
            g["K"][K] = dict(cl=cl, cand=cand, ref=ref, b=b, b0=b0, one=update_split(sp, g, cand, g["pairs"])[0])
        sp.close()
        _case[key] = g
    return _case[key]


def same_bits(sp, outs, one):
    for q, o in enumerate(outs):
        per = dict(T=12, delta=1, cov_diag=1)
        for k in LOCAL:
            want = one[k][sp.cols(q, per[k])]
            assert o[k].shape == want.shape and bits(o[k]) == bits(want), (k, q)
        for k in COMMON:
            assert bits(o[k]) == bits(one[k]), (k, q)
        assert all(o[k] == one[k] for k in FIGURES), q
        assert scalars(o["covariance"]) == scalars(one["covariance"]), q


@pytest.mark.parametrize("key,parts", SPLITS)
def test_every_split_is_within_the_bound_and_bitwise_the_one_participant_call(key, parts):
    n, seed, N = key
    g = case(key)
    pairs = g["pairs"]
    sp = Split(g["mp"], N, parts, g["X0"])
    for q in range(len(parts)):
        assert (6 * len(sp.cols(q, 1))) % 64 != 0
    before = [state(t) for t in sp.teams]
    zero = sp.owner[0]  # the holder of robot 0, whose first pose is the problem's pose 0: its team pose 0 (ids are sorted)
    worst = {}
    for K in UX.SIZES:
        c = g["K"][K]
        if K >= 5:
            UX.covers(g, parts, c["cl"][0])
        grp = capi.LocalGroup(len(parts))
        outs = update_split(sp, g, c["cand"], pairs, grp)
        out = assemble(sp, outs, n)
        # 1. the bound
        r, r0 = UX.ratios(out, c["ref"], c["b"]), UX.ratios(out, c["ref"], c["b0"])
        print("%d poses, %d robots, %s, K = %d: error / bound " % (n, N, parts, K) + ", ".join("%s %.3g (unwidened %.3g)" % (k, r[k], r0[k])
                                                                                           for k in r))
        for k in r:
            worst[k] = max(worst.get(k, 0.0), r[k])
            worst[k + " unwidened"] = max(worst.get(k + " unwidened", 0.0), r0[k])
        assert all(v <= 1.0 for v in r.values()), (K, r)
        # 2. the one-participant call's bits
        same_bits(sp, outs, c["one"])
        for q, o in enumerate(outs):
            assert bits(o["cov_diag"]) == bits(o["cov_diag"].transpose(0, 2, 1)), "not bitwise symmetric"
            assert o["covariance"].n == 6 * (n - 1) and o["covariance"].min_pivot > 0
            # 4. the information gain
            assert o["information_gain"] == 0.5 * (o["logdet_M"] - o["logdet_R"]) and o["information_gain"] > 0
        oz = outs[zero]
        assert bits(oz["delta"][0]) == bits(np.zeros(6)) and bits(oz["cov_diag"][0]) == bits(np.zeros((6, 6)))
        assert bits(oz["T"][:12]) == bits(g["T"][sp.cols(zero, 12)][:12])
        if K in (11, 43):
            again = update_split(sp, g, c["cand"], pairs)
            for a, o in zip(again, outs):
                assert all(bits(a[k]) == bits(o[k]) for k in LOCAL + COMMON) and all(a[k] == o[k] for k in FIGURES)
        if K == 11:
            # the scalars and the transport calls of covariances(transport=) with the same pairs; no trace grows
            g2 = capi.LocalGroup(len(parts))
            cov = sp.run(lambda tm, tr: tm.covariances(g["T"][sp.cols(tr.rank, 12)], pairs, transport=tr, owner_of_robot=sp.owner), g2)
            for q in range(len(parts)):
                assert scalars(cov[q][0]) == scalars(outs[q]["covariance"]), q
                want = dict(g2[q].calls)
                want["allgather"] += ADDED_ALLGATHERS
                assert dict(grp[q].calls) == want, (q, grp[q].calls, g2[q].calls)
                tr0, tr1 = np.trace(cov[q][1], axis1=1, axis2=2), np.trace(outs[q]["cov_diag"], axis1=1, axis2=2)
                assert (tr1 <= tr0 * (1 + 1e-12)).all(), q
    assert [state(t) for t in sp.teams] == before  # 5.
    print("%d poses, %d robots, %s: largest error / bound: " % (n, N, parts) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    sp.close()


@pytest.mark.parametrize("key,parts", [(G12, [[0, 1], [2]]), (G40, [[0, 2], [1]])])
def test_against_the_joined_team(key, parts):
    n, seed, N = key
    g = case(key)
    pairs = g["pairs"]
    sp = Split(g["mp"], N, parts, g["X0"])
    t = team_of(g["m"], n, N, g["T"])
    worst = {}
    for K in UX.SIZES:
        c = g["K"][K]
        out = assemble(sp, update_split(sp, g, c["cand"], pairs), n)
        for method, mb in (("nested", 6), ("dense", None)):
            joined = t.linear_update(c["cand"], g["T"], method=method, max_block=mb, pairs=pairs, columns="solve")
            two = {k: 2.0 * np.asarray(c["b"][k]) for k in UX.KEYS}
            r = UX.ratios(out, joined, two)
            worst[method] = max(worst.get(method, 0.0), max(r.values()))
            assert all(v <= 1.0 for v in r.values()), (K, method, r)
            assert bits(out["xi"]) == bits(joined["xi"]), (K, method)
    print("%d poses, %d robots, %s against the joined team: largest difference / the sum of both bounds: " % (n, N, parts) +
          ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()
    sp.close()


def raw_update_across(tm, tr, own, T, num, cand, num_pairs, pairs, outs, res):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dpgo_team_linear_update_across(tm.h, C.byref(tr.struct), p(own), p(T), num, p(cand), num_pairs, p(pairs),
                                                   *[p(a) for a in outs], None if res is None else C.byref(res))
    return rc, capi.lib().dpgo_last_error().decode()


def test_refusals_reach_every_participant():
    key, parts, K = G40, [[0, 2], [1]], 5
    n, seed, N = key
    g = case(key)
    c = g["K"][K]
    pairs = g["pairs"]
    P = len(pairs)
    sp = Split(g["mp"], N, parts, g["X0"])
    own = capi._owner_array(sp.owner)
    Tq = [np.ascontiguousarray(g["T"][sp.cols(q, 12)]) for q in range(2)]
    Nq = [len(sp.cols(q, 1)) for q in range(2)]
    OUTS = ("T_new", "delta", "cov_diag", "cov_pairs", "xi", "xi_post", "scalars")

    def good():  # the transport is not left half-way: a good call goes through and gives check 2's bits
        same_bits(sp, update_split(sp, g, c["cand"], pairs), c["one"])

    def refused(args, match, prefix="linear_update_across:"):
        """args(q): the keywords that differ from a good call on participant q (null: the name of an output passed as NULL)"""
        grp = capi.LocalGroup(2, timeout=60.0)

        def call(q):
            kw = dict(own=own, T=Tq[q], num=K, cand=c["cand"], num_pairs=P, pairs=pairs, res=capi.Covariance(), null=None)
            kw.update(args(q))
            outs = [np.full(12 * Nq[q], 7.25), np.full((Nq[q], 6), 7.25), np.full((Nq[q], 6, 6), 7.25), np.full((P, 6, 6), 7.25),
                    np.full((K, 6), 7.25), np.full((K, 6), 7.25), np.full(3, 7.25)]
            null = kw.pop("null")
            if kw["res"] is not None:
                kw["res"].n = 5
            rc, msg = raw_update_across(sp.teams[q], grp[q], outs=[None if name == null else a for name, a in zip(OUTS, outs)], **kw)
            return rc, msg, all(bool((a == 7.25).all()) for a in outs), kw["res"] is None or bytes(kw["res"]) == bytes(capi.Covariance())

        msgs = []
        for q, (r, e) in enumerate(grp.run([lambda q=q: call(q) for q in range(2)], timeout=JOIN)):
            assert e is None, (q, e)
            rc, msg, untouched, zero = r
            assert rc == capi.ERR and match in msg and msg.startswith(prefix), (q, rc, msg)
            assert untouched and zero, (q, msg)
            msgs.append(msg)
        good()
        return msgs

    def one_sided(change, words):
        msgs = refused(lambda q: change if q else {}, "")
        assert "rank 1: invalid arguments" in msgs[0] and words in msgs[1], (change.keys(), msgs)

    def spoiled(field, value, k=2):
        bad = c["cand"].copy()
        bad[field][k] = value
        return bad

    # an argument error of one participant: its own words there, "rank 1: invalid arguments" on the other
    for null in [dict(null=name) for name in OUTS] + [dict(T=None), dict(own=None), dict(res=None), dict(cand=None), dict(pairs=None)]:
        one_sided(null, "null argument")
    one_sided(dict(num=0), "num must be positive, not 0")
    one_sided(dict(num=-2), "num must be positive, not -2")
    one_sided(dict(num_pairs=-1), "num_pairs must not be negative, not -1")
    one_sided(dict(cand=spoiled("kappa", 0.0)), "closure 2 has kappa = 0")
    one_sided(dict(cand=spoiled("tau", -1.0)), "both must be positive")
    selfloop = c["cand"].copy()
    selfloop["r2"][1], selfloop["p2"][1] = selfloop["r1"][1], selfloop["p1"][1]
    one_sided(dict(cand=selfloop), "closure 1 joins a pose to itself")
    off = c["cand"].copy()
    off["R"][3][0] *= 1.001
    one_sided(dict(cand=off), "the measurement of closure 3 is not in SE(3)")
    # 2^24 closures: decided before a record is read and before any allocation, with the bytes named
    msgs = refused(lambda q: dict(num=2 ** 24) if q else {}, "")
    assert "rank 1: invalid arguments" in msgs[0] and "bytes" in msgs[1] and "are available on the device" in msgs[1], msgs
    # lists that differ: refused on both in the gate's words
    msgs = refused(lambda q: dict(num=K - q), "the number of records")
    assert "disagree" in msgs[0] and msgs[0] == msgs[1], msgs
    msgs = refused(lambda q: dict(cand=spoiled("kappa", 123.0)) if q else {}, "the record list")
    assert msgs[0] == msgs[1], msgs
    other = pairs.copy()
    other[1] = (2, 3)
    msgs = refused(lambda q: dict(pairs=other) if q else {}, "the record list")
    assert msgs[0] == msgs[1], msgs
    msgs = refused(lambda q: dict(num_pairs=P - q), "the record list")  # (the hash covers the pair list)
    assert "disagree" in msgs[0] and msgs[0] == msgs[1], msgs
    # behind the agreement, the same words everywhere: an endpoint or a pair pose outside the problem
    msgs = refused(lambda q: dict(cand=spoiled("p2", 999, k=4)), "closure 4 names pose 999 of robot")
    assert msgs[0] == msgs[1], msgs
    msgs = refused(lambda q: dict(cand=spoiled("r1", N, k=0)), "closure 0 names robot %d" % N)
    assert msgs[0] == msgs[1], msgs
    far = pairs.copy()
    far[2, 1] = n
    msgs = refused(lambda q: dict(pairs=far), "pair 2 names pose %d, outside [0, %d)" % (n, n))
    assert msgs[0] == msgs[1], msgs
    # carried over from the covariances across in their own words: T off SE(3) on one participant only
    Tb = Tq[1].copy()
    Tb[12 * 4] *= 1.001
    msgs = refused(lambda q: dict(T=Tb) if q else {}, "rank 1")
    assert "SE(3)" in msgs[1] and "pose 4 of T" in msgs[1], msgs
    # a T that is no minimum: the path's pivot message, the same on both
    Ts = NR.spoil_rotations(g["T"], n, [9, 10, 11, 28, 29], 50)
    msgs = refused(lambda q: dict(T=np.ascontiguousarray(Ts[sp.cols(q, 12)])), "non-positive pivot")
    assert msgs[0] == msgs[1] and "not a minimum" in msgs[0], msgs
    # through the Python interface: a DpgoError on every participant
    _expect_refusal(sp, lambda q, tm, tr: tm.linear_update(c["cand"][:K - q], Tq[q], pairs=pairs, transport=tr, owner_of_robot=sp.owner),
                    "the number of records")
    good()
    # method="nested" (or "dense", a max_block, columns="blocks") with a transport: a ValueError before any transport call
    grp = capi.LocalGroup(2)
    for kw in (dict(method="nested"), dict(method="dense"), dict(max_block=16), dict(columns="blocks")):
        with pytest.raises(ValueError, match="transport"):
            sp.teams[0].linear_update(c["cand"], Tq[0], transport=grp[0], owner_of_robot=sp.owner, **kw)
    assert grp[0].calls == dict(allgather=0, exchange=0)
    sp.close()

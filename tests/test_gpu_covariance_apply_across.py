"""GPU checks of X = Sigma V over a team split across participants (dpgo_team_covariance_apply_across,
csrc/covariance_apply.hip behind csrc/covariance_schur.hip; Team.covariance_apply with transport=; DESIGN.md 5m "across
teams"): LocalGroup threads on one device, on the four graphs of tests/applyacross_ref.py with T the ground truth, the teams
set to the lifted T and nothing solved.

m = 1, 6, 31, 32, 33, 64, 65, 258 columns: the 32-slab and the 64-tile edges of the product; 6 N_loc is never a multiple of
64 (asserted).  The splits: one participant that holds every robot, two participants, one participant per robot.
  1. seeded normal V with nonzero rows at pose 0, X assembled in global order: every column within applyref's bound
     6 (n - 1) u cond_2(H_red) |Sigma_red|_2 |v_red|_2 of the longdouble dense solve on covref's H_red of the whole problem, on
     every participant; pose 0's rows zero bits on its holder; 1e30 and then NaN in pose 0's rows of V change no bit
  2. every split gives the bits of the one-participant call, row for row; two calls give the same bytes; the Covariance
     scalars are identical on every participant and those of covariances(transport=) with no pairs; the transport calls are
     those of that call
  3. the unit columns of four (three) poses against the blocks covariances(T, pairs, transport=) returns, pairs between
     participants included, within the sum of both bounds
  4. global_X(), the weights and cost() are untouched on every team
  5. every refusal reaches every participant with its words, sentinel-filled X untouched and *res zero, and a good call
     behind each gives check 2's bits
  6. method="dense" / "nested" or a max_block with a transport: ValueError before any transport call
No test provokes a device fault: a spoiled T is refused by a pivot, which the host reads from the factorisation's status.
Each test prints its largest error / bound (DESIGN.md 5m records them)."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyacross_ref as XR
from tests import applyref as AR
from tests import covnested_ref as NR
from tests.test_gpu_certify_across import JOIN, Split, _expect_refusal, bits
from tests.test_gpu_covariance_across import scalars
from tests.test_gpu_covariance_nested import team_of

pytestmark = pytest.mark.gpu

COLS = (1, 6, 31, 32, 33, 64, 65, 258)
G12, G40, G40_8, G40_1 = [c[:3] for c in XR.GRAPHS]
UNIT_POSES = {12: (1, 5, 11), 40: (1, 13, 27, 39)}
SPLITS = [(G12, [[0, 1, 2]]), (G12, [[0, 1], [2]]), (G12, [[0], [1], [2]]),
          (G40, [[0, 1, 2]]), (G40, [[0, 2], [1]]), (G40, [[0], [1], [2]]),
          (G40_8, [list(range(8))]), (G40_8, [[0, 2, 4, 6], [1, 3, 5, 7]]), (G40_8, [[i] for i in range(8)]),
          (G40_1, [[0]])]
_case = {}


def case(key):
    """the graph, the lifted iterate, the 258 seeded columns (V of m columns is their first m), their longdouble solve and
    bound, and the one-participant call's (scalars, X) for every m: computed once per graph and left unchanged"""
    if key not in _case:
        n, seed, N = key
        g = dict(XR.graph(n, seed, N))
        t = team_of(g["m"], n, N, g["T"])
        g["X0"] = t.global_X()
        t.close()
        V = np.random.default_rng(24).standard_normal((6 * n, max(COLS)))
        assert np.abs(V[:6]).min() > 0
        E = np.zeros((6 * n, 6 * len(UNIT_POSES[n])))
        for k, p in enumerate(UNIT_POSES[n]):
            E[6 * p:6 * p + 6, 6 * k:6 * k + 6] = np.eye(6)
        Xref, b = XR.reference(g["Hr"], V)
        g.update(V=V, Xref=Xref, b=b, E=E, bE=AR.bound(g["Hr"], E))
        sp = Split(g["mp"], N, [list(range(N))], g["X0"])
        own = np.zeros(N, dtype=np.int32)
        tr = capi.LocalGroup(1)[0]
        g["one"] = {}
        for m in COLS:
            res, X = sp.teams[0].covariance_apply(V[:, :m], g["T"], transport=tr, owner_of_robot=own)
            g["one"][m] = (scalars(res), X)
        sp.close()
        _case[key] = g
    return _case[key]


def state(t):
    return t.global_X().tobytes(), b"".join(t.agents[i].measurements().tobytes() for i in t.ids), t.cost()


def apply_split(sp, g, V, group=None):
    """Team.covariance_apply on every participant with its rows of V and its poses of T: [(Covariance, X_local)]"""
    return sp.run(lambda tm, tr: tm.covariance_apply(V[sp.cols(tr.rank, 6)], g["T"][sp.cols(tr.rank, 12)], transport=tr,
                                                     owner_of_robot=sp.owner), group)


def assemble(sp, outs, n):
    X = np.full((6 * n, outs[0][1].shape[1]), np.nan)
    for q, (_, Xq) in enumerate(outs):
        X[sp.cols(q, 6)] = Xq
    return X


@pytest.mark.parametrize("key,parts", SPLITS)
def test_every_split_is_within_the_bound_and_bitwise_the_one_participant_call(key, parts):
    n, seed, N = key
    g = case(key)
    sp = Split(g["mp"], N, parts, g["X0"])
    for q in range(len(parts)):
        assert (6 * len(sp.cols(q, 1))) % 64 != 0
    before = [state(t) for t in sp.teams]
    zero = sp.owner[0]  # the holder of robot 0, whose first pose is the problem's pose 0: its team pose 0 (ids are sorted)
    worst = 0.0
    for m in COLS:
        V = g["V"][:, :m]
        grp = capi.LocalGroup(len(parts))
        outs = apply_split(sp, g, V, grp)
        X = assemble(sp, outs, n)
        assert bits(outs[zero][1][:6]) == bits(np.zeros((6, m))), "pose 0's rows of X are not zero bits"
        # 1. the bound, on the rows of every participant (a participant's rows alone err by no more than all rows)
        w = AR.worst(X, g["Xref"][:, :m], g["b"][:m])
        print("%d poses, %d robots, %s, m = %d: largest column error / bound %.3g" % (n, N, parts, m, w))
        worst = max(worst, w)
        assert w <= 1.0, (m, w)
        # 2. the one-participant call's bits, row for row, and its scalars on every participant
        sc, X1 = g["one"][m]
        for q, (res, Xq) in enumerate(outs):
            assert Xq.shape == (len(sp.cols(q, 6)), m)
            assert bits(Xq) == bits(X1[sp.cols(q, 6)]), (m, q)
            assert scalars(res) == sc and res.n == 6 * (n - 1) and res.min_pivot > 0, (m, q)
        if m in (33, 258):
            again = apply_split(sp, g, V)
            assert all(bits(a[1]) == bits(o[1]) and scalars(a[0]) == scalars(o[0]) for a, o in zip(again, outs))
        if m == 33:
            # the scalars and the transport calls of covariances(transport=) with no pairs
            g2 = capi.LocalGroup(len(parts))
            cov = sp.run(lambda tm, tr: tm.covariances(g["T"][sp.cols(tr.rank, 12)], transport=tr, owner_of_robot=sp.owner), g2)
            for q in range(len(parts)):
                assert scalars(cov[q][0]) == sc, q
                assert dict(grp[q].calls) == dict(g2[q].calls), (q, grp[q].calls, g2[q].calls)
            # pose 0's rows of V are not read
            Vb = V.copy()
            for bad in (1e30, np.nan):
                Vb[:6] = bad
                assert all(bits(a[1]) == bits(o[1]) for a, o in zip(apply_split(sp, g, Vb), outs)), bad
    # one column as a vector
    v1 = sp.run(lambda tm, tr: tm.covariance_apply(g["V"][sp.cols(tr.rank, 6), 0], g["T"][sp.cols(tr.rank, 12)], transport=tr,
                                                   owner_of_robot=sp.owner))
    assert all(bits(v1[q][1]) == bits(g["one"][1][1][sp.cols(q, 6)]) for q in range(len(parts)))
    assert [state(t) for t in sp.teams] == before  # 4.
    print("%d poses, %d robots, %s: largest error / bound over all m %.3g" % (n, N, parts, worst))
    sp.close()


@pytest.mark.parametrize("key,parts", [s for s in SPLITS if len(s[1]) > 1])
def test_unit_columns_against_the_blocks_of_the_covariances_across(key, parts):
    n, seed, N = key
    g = case(key)
    unit = UNIT_POSES[n]
    sp = Split(g["mp"], N, parts, g["X0"])
    X = assemble(sp, apply_split(sp, g, g["E"]), n)
    pairs = np.array([(q, p) for p in unit for q in range(n)], dtype=np.int32)  # (q = p: the diagonal block; q = 0: zeros)
    holder = {int(g0): q for q in range(len(parts)) for g0 in sp.cols(q, 1)}
    assert sum(holder[int(a)] != holder[int(b)] for a, b in pairs) >= n // 4, "no pairs between participants"
    cov = sp.run(lambda tm, tr: tm.covariances(g["T"][sp.cols(tr.rank, 12)], pairs, transport=tr, owner_of_robot=sp.owner))
    for q, (_, _, cross) in enumerate(cov):
        S = np.zeros_like(X)
        for k, p in enumerate(unit):
            S[:, 6 * k:6 * k + 6] = cross[k * n:(k + 1) * n].reshape(6 * n, 6)
        w = AR.worst(X, S, 2.0 * g["bE"])
        assert w <= 1.0, (q, w)
    w_ref = AR.worst(X, AR.reference(g["Hr"], g["E"]), g["bE"])
    print("%d poses, %d robots, %s, unit columns of poses %s: against the blocks %.3g of both bounds, against the dense solve "
          "%.3g of the bound" % (n, N, parts, unit, w, w_ref))
    assert w_ref <= 1.0
    sp.close()


def raw_apply_across(tm, tr, own, T, num_cols, V, X, res):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dpgo_team_covariance_apply_across(tm.h, C.byref(tr.struct), p(own), p(T), num_cols, p(V), p(X),
                                                      None if res is None else C.byref(res))
    return rc, capi.lib().dpgo_last_error().decode()


def test_refusals_reach_every_participant():
    key, parts, m = G40, [[0, 2], [1]], 6
    n, seed, N = key
    g = case(key)
    sp = Split(g["mp"], N, parts, g["X0"])
    own = capi._owner_array(sp.owner)
    Tq = [np.ascontiguousarray(g["T"][sp.cols(q, 12)]) for q in range(2)]
    Vq = [np.asfortranarray(g["V"][sp.cols(q, 6), :m]) for q in range(2)]
    rows = [len(sp.cols(q, 6)) for q in range(2)]

    def good():  # the transport is not left half-way: a good call goes through and gives check 2's bits
        outs = apply_split(sp, g, g["V"][:, :m])
        assert all(bits(outs[q][1]) == bits(g["one"][m][1][sp.cols(q, 6)]) for q in range(2))

    def refused(args, match, prefix="covariance_apply_across:"):
        """args(q): the keywords that differ from a good call on participant q"""
        grp = capi.LocalGroup(2, timeout=60.0)

        def call(q):
            kw = dict(own=own, T=Tq[q], num_cols=m, V=Vq[q], res=capi.Covariance())
            kw.update(args(q))
            X = np.full((rows[q], m), 7.25, order="F")
            if kw["res"] is not None:
                kw["res"].n = 5
            rc, msg = raw_apply_across(sp.teams[q], grp[q], X=None if kw.pop("no_X", False) else X, **kw)
            return rc, msg, bool((X == 7.25).all()), kw["res"] is None or bytes(kw["res"]) == bytes(capi.Covariance())

        msgs = []
        for q, (r, e) in enumerate(grp.run([lambda q=q: call(q) for q in range(2)], timeout=JOIN)):
            assert e is None, (q, e)
            rc, msg, untouched, zero = r
            assert rc == capi.ERR and match in msg and msg.startswith(prefix), (q, rc, msg)
            assert untouched and zero, (q, msg)
            msgs.append(msg)
        good()
        return msgs

    # num_cols that differs: refused on both, naming it
    msgs = refused(lambda q: dict(num_cols=m - q), "num_cols")
    assert "disagree" in msgs[0] and msgs[0] == msgs[1], msgs
    # an argument error of one participant: its own words there, "rank 1: invalid arguments" on the other
    for bad in (np.nan, np.inf):
        Vb = Vq[1].copy(order="F")
        Vb[6 * 7 + 2, 3] = bad
        msgs = refused(lambda q: dict(V=Vb) if q else {}, "")
        assert "rank 1: invalid arguments" in msgs[0] and "V is not finite at row 44 (team pose 7) of column 3" in msgs[1], msgs
    for null in (dict(V=None), dict(T=None), dict(own=None), dict(res=None), dict(no_X=True)):
        msgs = refused(lambda q: null if q else {}, "")
        assert "rank 1: invalid arguments" in msgs[0] and "null argument" in msgs[1], (null, msgs)
    msgs = refused(lambda q: dict(num_cols=0), "num_cols must be positive, not 0")
    msgs = refused(lambda q: dict(num_cols=-2) if q else {}, "")
    assert "rank 1: invalid arguments" in msgs[0] and "num_cols must be positive, not -2" in msgs[1], msgs
    # a non-finite entry in pose 0's rows on its holder is no error (check 1), one row further it is
    Vb = Vq[0].copy(order="F")
    Vb[6, 0] = np.nan
    msgs = refused(lambda q: {} if q else dict(V=Vb), "")
    assert "V is not finite at row 6 (team pose 1) of column 0" in msgs[0] and "rank 0: invalid arguments" in msgs[1], msgs
    # carried over from the covariances across in their own words: T off SE(3) on one participant only
    Tb = Tq[1].copy()
    Tb[12 * 4] *= 1.001
    msgs = refused(lambda q: dict(T=Tb) if q else {}, "rank 1")
    assert "SE(3)" in msgs[1] and "pose 4 of T" in msgs[1], msgs
    # a T that is no minimum: the path's pivot message, the same on both
    Ts = NR.spoil_rotations(g["T"], n, [9, 10, 11, 28, 29], 50)
    msgs = refused(lambda q: dict(T=np.ascontiguousarray(Ts[sp.cols(q, 12)])), "non-positive pivot")
    assert msgs[0] == msgs[1] and "not a minimum" in msgs[0], msgs
    # 2^28 columns: V and X alone are beyond any device; decided before V is read and before any allocation, told to the
    # other participant in the words of the path's own memory refusal
    msgs = refused(lambda q: dict(num_cols=2 ** 28), "rank 0: the Schur path does not fit its device")
    assert "%d" % (2 * 8 * rows[0] * 2 ** 28) in msgs[0] and "are available" in msgs[0], msgs
    # through the Python interface: a DpgoError on every participant
    _expect_refusal(sp, lambda q, tm, tr: tm.covariance_apply(g["V"][sp.cols(q, 6), :m - q], Tq[q], transport=tr, owner_of_robot=sp.owner),
                    "num_cols")
    good()
    # 6. method="nested" (or "dense", or a max_block) with a transport: a ValueError before any transport call
    grp = capi.LocalGroup(2)
    for kw in (dict(method="nested"), dict(method="dense"), dict(max_block=16)):
        with pytest.raises(ValueError, match="transport"):
            sp.teams[0].covariance_apply(Vq[0], Tq[0], transport=grp[0], owner_of_robot=sp.owner, **kw)
    assert grp[0].calls == dict(allgather=0, exchange=0)
    with pytest.raises(ValueError, match="V has shape"):
        sp.teams[0].covariance_apply(Vq[0][:-6], Tq[0], transport=grp[0], owner_of_robot=sp.owner)
    # without a transport nothing changes: the single team's call still refuses the Schur path
    t = team_of(g["m"], n, N, g["T"])
    with pytest.raises(capi.DpgoError, match="Schur path's sets"):
        t.covariance_apply(g["V"][:, :m], g["T"], method="schur")
    t.close()
    sp.close()

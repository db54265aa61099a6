"""GPU checks of the Newton refinement over a team split across participants (dpgo_team_refine_across, csrc/refine.hip behind
csrc/covariance_schur.hip; Team.refine with transport=; DESIGN.md 5n "Across teams"): LocalGroup threads on one device, on the
inputs of tests/refineacross_ref.py (tests/test_refineacross_ref.py asserts their sets, owned measurements and the reference's
iteration counts), the teams set to the lifted ground truth and nothing solved.  grad_tol = 1e-9 throughout.

The splits: chain12 / 3 and chain40 / 3 as one, two and three participants, chain40 / 8 as one, two and eight, chain40 / 1 and
band40 / 1 through LocalGroup(1), band40 / 2 (robot 0 owns 320 measurements: two workgroups) as one and two.
  1. after one iteration (max_iters = 1): grad_inf0 and f0 within refineref.gradient_bound / cost_bound of the longdouble values,
     the step -- Log(T_0^-1 T_1) / -alpha, assembled in global order -- within 5m's column bound, the decrement within
     tests/test_gpu_refine.py's bound, alpha the reference's
  2. the full call converges in the reference's iterations in every split; the longdouble |g|_inf at the returned T is below
     grad_tol + the gradient's bound, |T - T*|_inf within refineref.final_bound, every R_i in SO(3) to 100 u; the problem's pose
     0 is bit for bit on its holder, the first pose of a participant without robot 0 has moved
  3. every split gives the bits of the one-participant call: T row for row, the history, the scalars; two calls give the same
     bytes; history and scalars are identical on every participant
  4. T within 2 final_bound of Team.refine(method="nested") on the joined team, with its status and iterations
  5. armijo = 0.7, max_iters = 4: alpha = 1/2 four times, status max_iters, the bits of check 3
  6. the transport calls are the formula's, the path's own taken from covariances(transport=) with no pairs on a fresh group
  7. the noise-free ground truth comes back bit for bit with 0 iterations: the agreement, one evaluation, the closing word
  8. global_X(), the weights and cost() are untouched on every team
  9. refusals on one participant only reach every participant, T_out and history untouched, *out and *res zero, and a good call
     behind each gives check 3's bits
 10. method="nested" or a max_block with a transport: ValueError before any transport call
No test provokes a device fault: a start outside the basin is refused by a pivot, which the host reads from the
factorisation's status.  Each test prints its largest error / bound (DESIGN.md 5n records them)."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyref as AR
from tests import refineacross_ref as XF
from tests import refineref as RR
from tests.test_gpu_certify_across import JOIN, Split, _expect_refusal, bits
from tests.test_gpu_covariance_across import scalars
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_refine import recovered_step

pytestmark = pytest.mark.gpu

F = np.float64
LD = np.longdouble
GRAD_TOL = 1e-9
# (case, robots, splits, (start, iterations of the reference))
CASES = [("chain12", 3, ([[0, 1, 2]], [[0, 1], [2]], [[0], [1], [2]]), ((1e-4, 2), (1e-3, 3), (1e-2, 5))),
         ("chain40", 3, ([[0, 1, 2]], [[0, 2], [1]], [[0], [1], [2]]), ((1e-4, 3), (1e-3, 3))),
         ("chain40", 8, ([list(range(8))], [[0, 2, 4, 6], [1, 3, 5, 7]], [[i] for i in range(8)]), ((1e-4, 3), (1e-3, 3))),
         ("chain40", 1, ([[0]],), ((1e-4, 3), (1e-3, 3))),
         ("band40", 2, ([[0, 1]], [[0], [1]]), ((1e-3, 3), (1e-2, 4))),
         ("band40", 1, ([[0]],), ((1e-3, 3), (1e-2, 4)))]
LADDER = dict(chain12=1e-3, chain40=1e-3, band40=1e-2)
_case, _ref, _one = {}, {}, {}


def case(name, N):
    """the inputs, the split measurements and the lifted iterate the teams are set to: computed once, left unchanged"""
    if (name, N) not in _case:
        c = dict(XF.case(name))
        c.update(XF.split(name, N))
        t = team_of(c["m"], c["n"], N, c["truth"])
        c["X0"] = t.global_X()
        t.close()
        _case[(name, N)] = c
    return _case[(name, N)]


def reference(name, s):
    """the start and the longdouble figures of its first step (the formulas of tests/test_gpu_refine.py), computed once"""
    if (name, s) not in _ref:
        c = XF.case(name)
        m, n, Q = c["m"], c["n"], c["Q"]
        T0 = RR.start(c["Tstar"], n, s, 11)
        g = RR.gradient(Q, T0, n)
        Hr = RR.hessian_red(Q, T0, n)
        g64 = np.asarray(g, dtype=F)
        X = AR.reference(Hr, g64.reshape(-1, 1))[:, 0]
        w = np.linalg.eigvalsh(Hr)
        gb = RR.gradient_bound(Q, T0, n)
        sb = float(AR.bound(Hr, g64.reshape(-1, 1))[0])
        X64 = np.asarray(X, dtype=F)
        _ref[(name, s)] = dict(T0=T0, g=g, X=X, gb=gb, step_bound=sb, f0=RR.edge_cost(m, T0, n, LD), f0_bound=RR.cost_bound(m, T0, n),
                               dec=float(g @ X),
                               dec_bound=float(np.linalg.norm(g64)) * (sb + float(np.linalg.norm(gb)) / w[0])
                               + float(np.linalg.norm(gb) * np.linalg.norm(X64)) + 6 * n * RR.U * float(np.abs(g64) @ np.abs(X64)))
    return _ref[(name, s)]


def state(t):
    return t.global_X().tobytes(), b"".join(t.agents[i].measurements().tobytes() for i in t.ids), t.cost()


def refine_split(sp, T0, group=None, **kw):
    """Team.refine on every participant with its poses of T0: the dicts in rank order"""
    kw.setdefault("grad_tol", GRAD_TOL)
    return sp.run(lambda tm, tr: tm.refine(T0[sp.cols(tr.rank, 12)], transport=tr, owner_of_robot=sp.owner, **kw), group)


def assemble(sp, outs, n):
    T = np.full(12 * n, np.nan)
    for q, o in enumerate(outs):
        T[sp.cols(q, 12)] = o["T"]
    return T


def record(o):
    """everything of a result that must be the same on every participant and in every split"""
    h = o["history"]
    return (o["status"], o["iterations"], bits(np.array([o["f0"], o["f"], o["grad_inf0"], o["grad_inf"]])),
            tuple(bits(h[k]) for k in ("f", "grad_inf", "alpha", "decrement", "pivot_min")), scalars(o["covariance"]))


def one_participant(name, N, s, **kw):
    """(record, T in global order) of the call of one participant that holds every robot: computed once per input"""
    key = (name, N, s, tuple(sorted(kw.items())))
    if key not in _one:
        c = case(name, N)
        sp = Split(c["mp"], N, [list(range(N))], c["X0"])
        outs = refine_split(sp, reference(name, s)["T0"], **kw)
        _one[key] = (record(outs[0]), outs[0]["T"].copy(), outs[0])
        sp.close()
    return _one[key]


def path_calls(sp, T0):
    """the transport calls of one covariances(transport=) with no pairs, per participant, on a fresh group"""
    g = capi.LocalGroup(len(sp.teams))
    sp.run(lambda tm, tr: tm.covariances(T0[sp.cols(tr.rank, 12)], transport=tr, owner_of_robot=sp.owner), g)
    return [dict(g[q].calls) for q in range(len(sp.teams))]


def expected_calls(path, k):
    """k steps: the driver's two agreement allgathers and its closing one, k + 1 evaluations of one exchange and one allgather,
    per step the path's calls and the ladder's allgather"""
    return dict(allgather=3 + (k + 1) + k * (path["allgather"] + 1), exchange=(k + 1) + k * path["exchange"])


@pytest.mark.parametrize("name,N,splits,starts", CASES)
def test_first_iteration_against_the_reference(name, N, splits, starts):
    c = case(name, N)
    n = c["n"]
    worst = 0.0
    for parts in splits:
        sp = Split(c["mp"], N, parts, c["X0"])
        for s, _ in starts:
            r = reference(name, s)
            outs = refine_split(sp, r["T0"], max_iters=1)
            o = outs[0]
            h = o["history"]
            assert all(record(x) == record(o) for x in outs)
            assert o["status"] == "max_iters" and o["iterations"] == 1 and len(h["alpha"]) == 1
            eg = abs(o["grad_inf0"] - float(np.abs(r["g"]).max())) / r["gb"].max()
            ef = abs(float(LD(o["f0"]) - r["f0"])) / r["f0_bound"]
            ed = abs(h["decrement"][0] - r["dec"]) / r["dec_bound"]
            X = recovered_step(r["T0"], assemble(sp, outs, n), h["alpha"][0], n)
            ex = float(np.linalg.norm(np.asarray(X - r["X"], dtype=F))) / r["step_bound"]
            print("%s, %d robots, %s, s = %g: grad_inf0 %.3g, f0 %.3g, step %.3g, decrement %.3g of their bounds; alpha %g, pivot_min "
                  "%.3g" % (name, N, parts, s, eg, ef, ex, ed, h["alpha"][0], h["pivot_min"][0]))
            worst = max(worst, eg, ef, ex, ed)
            assert eg <= 1.0 and ef <= 1.0 and ex <= 1.0 and ed <= 1.0
            assert h["alpha"][0] == 1.0  # (the reference's: tests/test_refineacross_ref.py)
            assert h["pivot_min"][0] > 0 and o["covariance"].n == 6 * (n - 1) and o["covariance"].min_pivot == h["pivot_min"][0]
            assert record(o) == one_participant(name, N, s, max_iters=1)[0]
        sp.close()
    print("%s, %d robots: largest error / bound of the first iteration %.3g" % (name, N, worst))


@pytest.mark.parametrize("name,N,splits,starts", CASES)
def test_convergence_split_invariance_and_transport_calls(name, N, splits, starts):
    c = case(name, N)
    n, Q = c["n"], c["Q"]
    fb = RR.final_bound(Q, c["Tstar"], n, GRAD_TOL)
    joined = team_of(c["m"], n, N, c["truth"])
    worst = 0.0
    for parts in splits:
        sp = Split(c["mp"], N, parts, c["X0"])
        before = [state(t) for t in sp.teams]
        zero = int(sp.owner[0])
        path = None
        for s, its in starts:
            r = reference(name, s)
            grp = capi.LocalGroup(len(parts))
            outs = refine_split(sp, r["T0"], grp)
            o = outs[0]
            T = assemble(sp, outs, n)
            # 2. convergence
            g = float(np.abs(np.asarray(RR.gradient(Q, T, n), dtype=F)).max())
            P = T.reshape(n, 4, 3)[:, :3, :]
            orth = float(np.abs(np.einsum("gcb,gdb->gcd", P, P) - np.eye(3)).max())
            det = float(np.abs(np.linalg.det(P) - 1.0).max())
            err = float(np.abs(T - c["Tstar"]).max())
            print("%s, %d robots, %s, s = %g: %s in %d iterations (reference %d), alpha %s, |g|_inf %s, longdouble |g|_inf %.3g, "
                  "|R^T R - I| %.3g u, |T - T*|_inf %.3g of the bound" %
                  (name, N, parts, s, o["status"], o["iterations"], its, o["history"]["alpha"],
                   ["%.3g" % v for v in o["history"]["grad_inf"]], g, orth / RR.U, err / fb))
            worst = max(worst, err / fb)
            assert o["status"] == "converged" and o["iterations"] == its
            assert o["grad_inf"] <= GRAD_TOL and g <= GRAD_TOL + float(RR.gradient_bound(Q, T, n).max())
            assert orth <= 100 * RR.U and det <= 100 * RR.U and err <= fb
            assert outs[zero]["T"][:12].tobytes() == r["T0"][:12].tobytes(), "the problem's pose 0 moved"
            for q in range(len(parts)):
                if q != zero:
                    assert outs[q]["T"][:12].tobytes() != r["T0"][sp.cols(q, 12)][:12].tobytes(), "a first pose without robot 0 is held"
            # 3. the one-participant call's bits, and the same record everywhere; twice the same bytes
            rec1, T1, _ = one_participant(name, N, s)
            for q, x in enumerate(outs):
                assert record(x) == rec1, (parts, s, q)
                assert bits(x["T"]) == bits(T1[sp.cols(q, 12)]), (parts, s, q)
            if s == starts[0][0]:
                again = refine_split(sp, r["T0"])
                assert all(bits(a["T"]) == bits(x["T"]) and record(a) == record(x) for a, x in zip(again, outs))
            # 4. the single team's nested call on the joined team
            single = joined.refine(r["T0"], method="nested", grad_tol=GRAD_TOL)
            d = float(np.abs(T - single["T"]).max())
            assert single["status"] == o["status"] and single["iterations"] == o["iterations"] and d <= 2 * fb, (d, fb)
            # 6. the transport calls
            if path is None:
                path = path_calls(sp, r["T0"])
            for q in range(len(parts)):
                assert dict(grp[q].calls) == expected_calls(path[q], its), (q, grp[q].calls, path[q], its)
        assert [state(t) for t in sp.teams] == before  # 8.
        sp.close()
    joined.close()
    print("%s, %d robots: largest |T - T*|_inf / bound %.3g" % (name, N, worst))


@pytest.mark.parametrize("name,N,splits,starts", [x for x in CASES if not (x[0] == "chain40" and x[1] == 1)])
def test_a_strict_armijo_takes_half_steps(name, N, splits, starts):
    c = case(name, N)
    s = LADDER[name]
    kw = dict(armijo=0.7, max_iters=4)
    rec1, T1, o1 = one_participant(name, N, s, **kw)
    for parts in splits:
        sp = Split(c["mp"], N, parts, c["X0"])
        outs = refine_split(sp, reference(name, s)["T0"], **kw)
        o = outs[0]
        g = o["history"]["grad_inf"]
        print("%s, %d robots, %s, s = %g, armijo 0.7: %s, alpha %s, |g|_inf %s" %
              (name, N, parts, s, o["status"], o["history"]["alpha"], ["%.3g" % v for v in g]))
        assert o["status"] == "max_iters" and list(o["history"]["alpha"]) == [0.5] * 4
        assert all(0.4 < g[k + 1] / g[k] < 0.6 for k in range(4))
        for q, x in enumerate(outs):
            assert record(x) == rec1 and bits(x["T"]) == bits(T1[sp.cols(q, 12)]), (parts, q)
        sp.close()


@pytest.mark.parametrize("parts", [[[0, 1, 2]], [[0, 2], [1]], [[0], [1], [2]]])
def test_noise_free_ground_truth_comes_back_bit_for_bit(parts):
    c = XF.case("chain40")
    n, N = c["n"], 3
    t = team_of(c["clean"], n, N, c["truth"])
    X0 = t.global_X()
    t.close()
    sp = Split(capi.partition(c["clean"], n, N), N, parts, X0)
    grp = capi.LocalGroup(len(parts))
    outs = refine_split(sp, c["truth"], grp, grad_tol=1e-8)
    for q, o in enumerate(outs):
        assert o["status"] == "converged" and o["iterations"] == 0 and bits(o["T"]) == bits(c["truth"][sp.cols(q, 12)])
        assert o["covariance"].n == 0 and len(o["history"]["alpha"]) == 0 and o["f0"] == o["f"]
        assert dict(grp[q].calls) == dict(allgather=4, exchange=1), grp[q].calls
    print("noise-free ground truth, %s: f %.3g, |g|_inf %.3g" % (parts, outs[0]["f"], outs[0]["grad_inf"]))
    sp.close()


def raw_refine_across(tm, tr, own, T, max_iters, grad_tol, armijo, ladder, T_out, hist, out, res):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dpgo_team_refine_across(tm.h, C.byref(tr.struct), p(own), p(T), max_iters, C.c_double(grad_tol), C.c_double(armijo),
                                            ladder, p(T_out), p(hist), None if out is None else C.byref(out),
                                            None if res is None else C.byref(res))
    return rc, capi.lib().dpgo_last_error().decode()


def test_refusals_reach_every_participant():
    name, N, parts, s = "chain40", 3, [[0, 2], [1]], 1e-4
    c = case(name, N)
    n = c["n"]
    sp = Split(c["mp"], N, parts, c["X0"])
    own = capi._owner_array(sp.owner)
    T0 = reference(name, s)["T0"]
    Tq = [np.ascontiguousarray(T0[sp.cols(q, 12)]) for q in range(2)]
    rec1, T1, _ = one_participant(name, N, s)

    def good():  # the transport is not left half-way: a good call goes through and gives check 3's bits
        outs = refine_split(sp, T0)
        assert all(record(outs[q]) == rec1 and bits(outs[q]["T"]) == bits(T1[sp.cols(q, 12)]) for q in range(2))

    def refused(args, match, prefix="refine_across:"):
        """args(q): the keywords that differ from a good call on participant q"""
        grp = capi.LocalGroup(2, timeout=60.0)

        def call(q):
            kw = dict(own=own, T=Tq[q], max_iters=10, grad_tol=GRAD_TOL, armijo=1e-4, ladder=8, hist=np.full((11, 5), 7.25),
                      out=capi.Refine(), res=capi.Covariance())
            kw.update(args(q))
            T_out = np.full(len(Tq[q]), 7.25)
            hist = np.full((11, 5), 7.25) if kw["hist"] is not None else None
            kw["hist"] = hist
            if kw["out"] is not None:
                kw["out"].iterations = 5
            if kw["res"] is not None:
                kw["res"].n = 5
            rc, msg = raw_refine_across(sp.teams[q], grp[q], T_out=None if kw.pop("no_T_out", False) else T_out, **kw)
            zero = (kw["out"] is None or bytes(kw["out"]) == bytes(capi.Refine())) and \
                   (kw["res"] is None or bytes(kw["res"]) == bytes(capi.Covariance()))
            return rc, msg, bool((T_out == 7.25).all()) and (hist is None or bool((hist == 7.25).all())), zero

        msgs = []
        for q, (r, e) in enumerate(grp.run([lambda q=q: call(q) for q in range(2)], timeout=JOIN)):
            assert e is None, (q, e)
            rc, msg, untouched, zero = r
            assert rc == capi.ERR and match in msg and msg.startswith(prefix), (q, rc, msg)
            assert untouched and zero, (q, msg)
            msgs.append(msg)
        good()
        return msgs

    # parameters that differ: refused on both, naming them
    for key, other in (("max_iters", 9), ("ladder", 7), ("grad_tol", 2e-9), ("armijo", 1e-3)):
        msgs = refused(lambda q: {key: other} if q else {}, "the participants disagree on " + key)
        assert msgs[0] == msgs[1], msgs
    # an argument error of one participant: its own words there, "rank 1: invalid arguments" on the other
    for null in (dict(T=None), dict(own=None), dict(res=None), dict(out=None), dict(hist=None), dict(no_T_out=True)):
        msgs = refused(lambda q: null if q else {}, "")
        assert "rank 1: invalid arguments" in msgs[0] and "null argument" in msgs[1], (null, msgs)
    for kw, words in ((dict(max_iters=-1), "max_iters must not be negative, not -1"), (dict(ladder=0), "ladder must lie in [1, 32], not 0"),
                      (dict(ladder=33), "ladder must lie in [1, 32], not 33"), (dict(grad_tol=0.0), "grad_tol must be positive"),
                      (dict(grad_tol=np.nan), "grad_tol must be positive"), (dict(armijo=1.0), "armijo must lie in (0, 1)"),
                      (dict(armijo=np.nan), "armijo must lie in (0, 1)")):
        msgs = refused(lambda q: kw if q else {}, "")
        assert "rank 1: invalid arguments" in msgs[0] and words in msgs[1], (kw, msgs)
    Tb = Tq[1].copy()
    Tb[12 * 4] *= 1.001
    msgs = refused(lambda q: dict(T=Tb) if q else {}, "")
    assert "rank 1: invalid arguments" in msgs[0] and "pose 4 of T (team order) is not in SE(3)" in msgs[1], msgs
    # a start outside the basin: the path's pivot message behind "refine: ", the same words on both
    Ts = RR.start(c["Tstar"], n, 1e-2, 11)
    msgs = refused(lambda q: dict(T=np.ascontiguousarray(Ts[sp.cols(q, 12)])), "non-positive pivot", prefix="refine: ")
    assert msgs[0] == msgs[1] and "not a minimum" in msgs[0], msgs
    # through the Python interface: a DpgoError on every participant
    _expect_refusal(sp, lambda q, tm, tr: tm.refine(Tq[q], max_iters=10 - q, transport=tr, owner_of_robot=sp.owner), "max_iters")
    _expect_refusal(sp, lambda q, tm, tr: tm.refine(np.ascontiguousarray(Ts[sp.cols(q, 12)]), transport=tr, owner_of_robot=sp.owner),
                    "not a minimum")
    good()
    # 10. method="nested" (or "dense", or a max_block) with a transport: a ValueError before any transport call
    grp = capi.LocalGroup(2)
    for kw in (dict(method="nested"), dict(method="dense"), dict(max_block=16)):
        with pytest.raises(ValueError, match="transport"):
            sp.teams[0].refine(Tq[0], transport=grp[0], owner_of_robot=sp.owner, **kw)
    with pytest.raises(ValueError, match="T holds"):
        sp.teams[0].refine(Tq[0][:-12], transport=grp[0], owner_of_robot=sp.owner)
    assert grp[0].calls == dict(allgather=0, exchange=0)
    sp.close()


def test_the_other_refusal_case_is_refused_by_a_pivot_in_every_split():
    name, N = "chain12", 3
    c = case(name, N)
    Ts = RR.start(c["Tstar"], c["n"], 3e-2, 11)
    for parts in CASES[0][2]:
        sp = Split(c["mp"], N, parts, c["X0"])
        _expect_refusal(sp, lambda q, tm, tr: tm.refine(np.ascontiguousarray(Ts[sp.cols(q, 12)]), transport=tr, owner_of_robot=sp.owner),
                        "not a minimum")
        sp.close()

"""CPU checks of tests/updateacross_ref.py, the numpy statement of the first-order update over a split team (DESIGN.md 5j
"Across teams"), and of the call's presence in the header, the library and capi.

The graphs are applyacross_ref.GRAPHS: 12 poses / 3 robots, and 40 poses as 3, as 8 and as 1 robot; the splits are one
participant, two, and one per robot.  K = 1, 2, 5, 11, 22, 43 closures from updateacross_ref.closures (6 K = 6 ... 258 crosses the
32-slab and 64-tile edges); from K = 5 on a set holds a closure inside one robot, one between two robots of one participant, one
between participants, one with pose 0 as an endpoint, one on two interior and one on two public poses, and two closures on the
same ordered pair (asserted per split).  The pairs hold one between participants, two that name pose 0, and (p, p).
  1. the restatement stays within the widened bound of the longdouble update for every graph, split and K
  2. the bound rejects the six planted mistakes the call invites, at K = 5 and 11 (the factor is printed).  The input is
     sharpened to those K: on the 40-pose graph the widened bound lets Sigma'_pq taken with U_q B_p^T through at K = 22 and 43
     (0.07 to 1.03 of the bound; more closures shrink what the transposition changes while the bound grows with K); the other
     five are rejected at every K, by factors of 5 to 1e8
  3. dpgo_team_linear_update_across is declared in the header, exported by the built library and bound in capi
  4. the ValueErrors of the Python layer are raised with a counting transport still at zero calls, without a device
Each test prints its figures (DESIGN.md 5j records them)."""
import inspect
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyacross_ref as XR
from tests import updateacross_ref as UX
from tests.util import ROOT

G12, G40, G40_8, G40_1 = [c[:3] for c in XR.GRAPHS]
SPLITS = [(G12, [[0, 1, 2]]), (G12, [[0, 1], [2]]), (G12, [[0], [1], [2]]),
          (G40, [[0, 1, 2]]), (G40, [[0, 2], [1]]), (G40, [[0], [1], [2]]),
          (G40_8, [list(range(8))]), (G40_8, [[0, 2, 4, 6], [1, 3, 5, 7]]), (G40_8, [[i] for i in range(8)]),
          (G40_1, [[0]])]
MISTAKE_SIZES = (5, 11)
_ref = {}


def case(key, K):
    """the graph, the closures, the pairs and the longdouble reference with both bounds: once per (graph, K)"""
    if (key, K) not in _ref:
        g = XR.graph(*key)
        cl = UX.closures(g, K)
        pairs = UX.pairs_of(g)
        _ref[(key, K)] = (g, cl, pairs) + UX.reference(g, *cl, pairs)
    return _ref[(key, K)]


def test_the_pairs_hold_what_the_call_must_serve():
    for key, parts in SPLITS:
        g = XR.graph(*key)
        holder, _ = UX.holders(g, parts)
        pairs = UX.pairs_of(g)
        assert any(a == b for a, b in pairs) and any(a == 0 for a, b in pairs) and any(b == 0 for a, b in pairs)
        if len(parts) > 1:
            assert any(holder[a] != holder[b] for a, b in pairs), (key, parts)


@pytest.mark.parametrize("key,parts", SPLITS)
def test_the_restatement_is_within_the_bound_of_the_longdouble_update(key, parts):
    worst = {}
    for K in UX.SIZES:
        g, cl, pairs, ref, b, b0 = case(key, K)
        if K >= 5:
            UX.covers(g, parts, cl[0])
        out = UX.restate(g, parts, *cl, pairs)
        r, r0 = UX.ratios(out, ref, b), UX.ratios(out, ref, b0)
        print("%d poses, %d robots, %s, K = %d: error / bound " % (key[0], key[2], parts, K) + ", ".join("%s %.3g" % kv for kv in r.items()))
        for k in r:
            worst[k] = max(worst.get(k, 0.0), r[k])
            worst[k + " (unwidened)"] = max(worst.get(k + " (unwidened)", 0.0), r0[k])
        assert all(v <= 1.0 for v in r.values()), (K, r)
        assert (out["delta"][0] == 0).all() and (out["cov_diag"][0] == 0).all()
    print("%d poses, %d robots, %s: largest error / bound: " % (key[0], key[2], parts) + ", ".join("%s %.3g" % kv for kv in worst.items()))


@pytest.mark.parametrize("key,parts", [s for s in SPLITS if len(s[1]) > 1])
@pytest.mark.parametrize("mistake", UX.MISTAKES)
def test_the_bound_rejects_the_planted_mistakes(mistake, key, parts):
    for K in MISTAKE_SIZES:
        g, cl, pairs, ref, b, b0 = case(key, K)
        out = UX.restate(g, parts, *cl, pairs, mistake=mistake)
        r = UX.ratios(out, ref, b)
        k = max(r, key=r.get)
        print("%d poses, %d robots, %s, K = %d, mistake %s: %.3g times the bound (%s)" % (key[0], key[2], parts, K, mistake, r[k], k))
        assert r[k] > 1.0, (mistake, K, r)


def test_the_call_is_declared_exported_and_bound():
    sym = "dpgo_team_linear_update_across"
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    assert sym in capi.EXPORTS, sym
    assert hasattr(capi.lib(), sym), sym
    sig = inspect.signature(capi.Team.linear_update)
    assert list(sig.parameters)[1:] == ["closures", "T", "method", "max_block", "pairs", "columns", "transport", "owner_of_robot"]
    assert sig.parameters["columns"].default is None
    from dpgo_ros_amd import distributed
    assert list(inspect.signature(distributed.linear_update).parameters) == ["backend_or_team", "dist", "owner_of_robot", "closures", "T",
                                                                            "pairs", "gather"]


class Counting(capi.Transport):
    def allgather(self, x):
        raise AssertionError("the transport was called")

    def exchange(self, parts, recv_counts):
        raise AssertionError("the transport was called")


def test_the_python_layer_refuses_before_any_transport_call():
    t = object.__new__(capi.Team)  # (no device: every refusal below is raised before the team is touched)
    tr = Counting(0, 2)
    cand = np.zeros(2, dtype=capi.MEAS_DTYPE)
    T = np.zeros(24)
    with pytest.raises(ValueError, match="columns must be"):
        t.linear_update(cand, T, columns="rows", transport=tr, owner_of_robot=[0, 1])
    with pytest.raises(ValueError, match="columns must be"):
        t.linear_update(cand, T, columns="rows")
    with pytest.raises(ValueError, match="columns=\"blocks\" with a transport"):
        t.linear_update(cand, T, columns="blocks", transport=tr, owner_of_robot=[0, 1])
    for kw in (dict(method="nested"), dict(method="dense"), dict(max_block=16), dict(method="nested", columns="solve")):
        with pytest.raises(ValueError, match="transport"):
            t.linear_update(cand, T, transport=tr, owner_of_robot=[0, 1], **kw)
    assert tr.calls == dict(allgather=0, exchange=0)

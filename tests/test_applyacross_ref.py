"""CPU checks of tests/applyacross_ref.py, the numpy statement of X = Sigma V over a split team (DESIGN.md 5m "across teams"),
and of the call's presence in the header, the library and capi.

The graphs are covnested_ref.banded_chain(12, 1, window=8) as 3 robots and banded_chain(40, 3, window=8) as 3, 8 and 1: their
(public, interior) counts per robot are asserted, so that the cases they stand for -- a robot with no interior pose, one among
seven that have some, an empty separator -- are there.  V is seeded normal with nonzero rows at pose 0; m = 1, 33, 258.
  1. the robot-wise elimination is within applyref's bound of the longdouble dense solve on the whole problem's H_red
  2. the bound rejects four planted mistakes: the wrong sign of W_a x_S, r_a without its W_a^T v_a term, two robots' r_a
     swapped in r_S, pose 0's rows read
  3. dpgo_team_covariance_apply_across is declared in the header, exported by the built library and bound in capi
Each test prints its figures (DESIGN.md 5m records them)."""
import inspect
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyacross_ref as XR
from tests import applyref as AR
from tests.util import ROOT

COLS = (1, 33, 258)


def columns(n):
    V = np.random.default_rng(24).standard_normal((6 * n, max(COLS)))
    assert np.abs(V[:6]).min() > 0
    return V


@pytest.mark.parametrize("n,seed,N,want", XR.GRAPHS)
def test_the_elimination_is_within_the_bound_of_the_dense_solve(n, seed, N, want):
    g = XR.graph(n, seed, N)
    assert XR.counts(g["robot_of"], g["public"]) == want
    V = columns(n)
    Xref, b = XR.reference(g["Hr"], V)
    for m in COLS:
        X = XR.eliminate(g["Hr"], g["robot_of"], g["public"], V[:, :m])
        assert (X[:6] == 0).all()
        w = AR.worst(X, Xref[:, :m], b[:m])
        print("%d poses, %d robots, m = %d: largest column error / bound %.3g" % (n, N, m, w))
        assert w <= 1.0, (m, w)


@pytest.mark.parametrize("n,seed,N,want", [c for c in XR.GRAPHS if c[2] > 1])
@pytest.mark.parametrize("mistake", XR.MISTAKES)
def test_the_bound_rejects_the_planted_mistakes(mistake, n, seed, N, want):
    g = XR.graph(n, seed, N)
    V = columns(n)
    Xref, b = XR.reference(g["Hr"], V)
    for m in COLS:
        X = XR.eliminate(g["Hr"], g["robot_of"], g["public"], V[:, :m], mistake=mistake)
        w = AR.worst(X, Xref[:, :m], b[:m])
        print("%d poses, %d robots, m = %d, mistake %s: %.3g times the bound" % (n, N, m, mistake, w))
        assert w > 1.0, (mistake, m, w)


def test_the_call_is_declared_exported_and_bound():
    sym = "dpgo_team_covariance_apply_across"
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    assert sym in capi.EXPORTS, sym
    assert hasattr(capi.lib(), sym), sym
    sig = inspect.signature(capi.Team.covariance_apply)
    assert list(sig.parameters)[1:] == ["V", "T", "method", "max_block", "transport", "owner_of_robot"]
    from dpgo_ros_amd import distributed
    assert list(inspect.signature(distributed.covariance_apply).parameters) == ["backend_or_team", "dist", "owner_of_robot", "V", "T",
                                                                                 "gather"]

"""CPU checks of tests/applyref.py, the numpy statement of X = Sigma V: the elimination in the device's order
against the dense longdouble solve within the per-column bound, V = A^T against updateref's B, the bound's power to reject
planted mistakes, and the declaration of the two new calls.  No device."""
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import applyref as AR
from tests import covnested_ref as NR
from tests import covref
from tests import jointref as J
from tests import updateref as R
from tests.util import ROOT

F = np.float64
N_POSES = 12
COLS = (1, 33, 258)
_cache = {}


def graph(seed):
    """(H_red, T, rowptr, col) of banded_chain(12, seed, window=8), computed once"""
    if seed not in _cache:
        m, T = NR.banded_chain(N_POSES, seed, window=8)
        Hr = covref.dense_reference(covref.q_full(m, N_POSES), T, N_POSES)[0]
        _cache[seed] = (Hr, T) + NR.pattern(m, N_POSES)
    return _cache[seed]


def info_for(rowptr, col, sep):
    return NR.sets(AR.plan_from_separator(N_POSES, rowptr, col, sep), rowptr, col)


def vectors(m, seed):
    """seeded normal V with nonzero rows at pose 0"""
    return np.random.default_rng(100 + seed).standard_normal((6 * N_POSES, m))


def square_block_plan(rowptr, col):
    """a plan with a block of two consecutive poses coupled to exactly two separator poses: every other free pose is in the
    separator"""
    for g in range(1, N_POSES - 1):
        info = info_for(rowptr, col, [p for p in range(1, N_POSES) if p not in (g, g + 1)])
        if len(info["blocks"]) == 1 and len(info["coupled"][0]) == 2:
            return info
    raise AssertionError("no pair of consecutive poses has exactly two neighbours")


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_elimination_against_the_dense_solve(seed):
    Hr, T, rowptr, col = graph(seed)
    plans = dict(split=info_for(rowptr, col, [6]), two_separators=info_for(rowptr, col, [4, 8]),
                 one_block=info_for(rowptr, col, []), square=square_block_plan(rowptr, col))
    assert len(plans["one_block"]["blocks"]) == 1 and not plans["one_block"]["separator"] and plans["one_block"]["coupled"] == [[]]
    worst = {}
    for name, info in plans.items():
        for m in COLS:
            V = vectors(m, seed)
            X = AR.eliminate(Hr, info, V)
            assert (X[:6] == 0).all()
            worst[name, m] = AR.worst(X, AR.reference(Hr, V), AR.bound(Hr, V))
    print("seed %d: largest error / bound of the elimination: " % seed + ", ".join("%s m=%d %.3g" % (k + (v,)) for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_a_block_with_no_coupling_beside_a_split_part():
    """poses 1 .. 5 cut off from the rest (a principal block-diagonal of an SPD matrix is SPD): their block has an empty N_b
    while the other poses are split by a separator"""
    Hr, T, rowptr, col = graph(2)
    Hc = Hr.copy()
    Hc[:30, 30:] = 0.0
    Hc[30:, :30] = 0.0
    info = dict(blocks=[[1, 2, 3, 4, 5], [6, 7], [9, 10, 11]], separator=[8], coupled=[[], [0], [0]])
    assert not Hc[np.ix_(np.r_[30:42], np.r_[48:66])].any(), "poses 6, 7 touch 9 .. 11: choose another separator"
    for m in COLS:
        V = vectors(m, 7)
        w = AR.worst(AR.eliminate(Hc, info, V), AR.reference(Hc, V), AR.bound(Hc, V))
        print("empty N_b beside a split part, m = %d: largest error / bound %.3g" % (m, w))
        assert w <= 1.0


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_transposed_A_gives_the_columns_of_the_update(seed):
    Hr, T, rowptr, col = graph(seed)
    n, K = N_POSES, 12
    ends, Rm, tm, kap, ta, _ = J.seeded_batch(T, n, K, 5, outliers=0.0, fixed=((0, 5), (5, 0), (3, 9), (9, 3)))
    Sigma = AR.dense_solve(Hr, np.eye(6 * (n - 1)))
    blocks = R.blocks_from_sigma(Sigma)
    A = R.a_full(T, ends, n)
    B = R.sigma_columns(ends, blocks, n) @ A.T
    ref = R.update(T, ends, Rm, tm, kap, ta, blocks, n)
    b_B = R.bounds(ref, T, ends, tm, n)["B"]
    # (by the definition, on the same Sigma: an element that is zero in exact arithmetic has a bound of zero, which no solve meets)
    X = AR.apply_sigma(Sigma, A.T)
    print("seed %d: V = A^T against updateref's B: largest error / bound %.3g" % (seed, R.ratio(X - B, b_B)))
    assert R.ratio(X - B, b_B) <= 1.0
    # and the float64 elimination of the same right-hand side, within the bound of the solve
    V = np.asarray(A.T, dtype=F)
    w = AR.worst(AR.eliminate(Hr, info_for(rowptr, col, [6]), V), B, AR.bound(Hr, V))
    assert w <= 1.0, w


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_bound_rejects_planted_mistakes(seed):
    Hr, T, rowptr, col = graph(seed)
    split, square = info_for(rowptr, col, [4, 8]), square_block_plan(rowptr, col)
    V = vectors(33, seed)
    Xref, b = AR.reference(Hr, V), AR.bound(Hr, V)
    cases = [("sign", split, "sign"), ("a block left out of r_S", split, ("skip", 1)), ("W_b for W_b^T", square, ("untransposed", 0)),
             ("pose 0's rows read", split, "pose0")]
    for name, info, mistake in cases:
        assert AR.worst(AR.eliminate(Hr, info, V), Xref, b) <= 1.0
        w = AR.worst(AR.eliminate(Hr, info, V, mistake=mistake), Xref, b)
        print("seed %d, %s: %.3g x the bound" % (seed, name, w))
        assert w > 1000.0, (name, w)


def test_the_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    for sym in ("dpgo_team_covariance_apply", "dpgo_team_linear_update_solved"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in capi.EXPORTS, sym
        assert hasattr(capi.lib(), sym), sym
    assert callable(getattr(capi.Team, "covariance_apply", None))

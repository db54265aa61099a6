"""GPU checks of linear_update(columns="solve") (csrc/linear_update.hip, dpgo_team_linear_update_solved): B = Sigma A^T
formed by the covariance path's own solve instead of from N m extracted blocks.  The graph, the closures, the pairs and the
reference are those of tests/test_gpu_linear_update.py: every output stays within updateref.bounds against updateref.update
on the blocks covariances() returns for the rectangular set.  N = 1, 2, 3 robots, the dense path and the nested path at
max_block = 6, K = 1, 2, 5, 11, 22, 43 closures.  The largest error / bound ratios are printed (DESIGN.md 5m records them)."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import updateref as R
from tests.test_gpu_gate import blocks_call
from tests.test_gpu_gate_joint import NESTED_BLOCK, records, setup
from tests.test_gpu_linear_update import N_POSES, PAIRS, SIZES, check_rotations, closures, update_call

pytestmark = pytest.mark.gpu

F = np.float64
KEYS = ("T", "delta", "cov_diag", "cov_pairs", "xi", "xi_post")


@pytest.mark.parametrize("method", ["dense", "nested"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_the_update_on_the_solve_at_tile_and_block_edges(N, method):
    n = N_POSES
    m, T, t = setup(n, N, method)
    X0 = t.global_X().copy()
    worst = {}
    for K in SIZES:
        ends, Rm, tm, kap, ta = closures(T, n, K, seed=17)
        cand = records(n, N, ends, Rm, tm, kap, ta)
        out = update_call(t, cand, T, method, pairs=PAIRS, columns="solve")
        assert out["T"].shape == (12 * n,) and out["delta"].shape == (n, 6) and out["cov_diag"].shape == (n, 6, 6)
        assert out["cov_pairs"].shape == (len(PAIRS), 6, 6) and out["xi"].shape == out["xi_post"].shape == (K, 6)
        assert out["covariance"].n == 6 * (n - 1) and out["covariance"].min_pivot > 0
        # against updateref on the blocks the covariance call returns for the rectangular set and the pairs
        poses = sorted(set(ends.reshape(-1).tolist()))
        _, diag, cross = blocks_call(t, T, np.r_[R.rect_pairs(poses, n), PAIRS], method)
        ref = R.update(T, ends, Rm, tm, kap, ta, R.blocks_from_rect(poses, n, diag, cross), n, pairs=PAIRS)
        b = R.bounds(ref, T, ends, tm, n, PAIRS)
        for key in ("xi", "delta", "T", "cov_diag", "cov_pairs", "xi_post", "d2_joint", "logdet_M", "logdet_R"):
            r = R.ratio(np.asarray(out[key] - np.asarray(ref[key], dtype=F)), b[key])
            print("%d robots, %s, K = %d, %s: error / bound %.3g" % (N, method, K, key, r))
            worst[key] = max(worst.get(key, 0.0), r)
        assert all(v <= 1.0 for v in worst.values()), (K, worst)
        assert out["information_gain"] == 0.5 * (out["logdet_M"] - out["logdet_R"]) and out["information_gain"] > 0
        assert out["cov_diag"].tobytes() == np.ascontiguousarray(out["cov_diag"].transpose(0, 2, 1)).tobytes(), "not bitwise symmetric"
        assert (out["delta"][0] == 0).all() and (out["cov_diag"][0] == 0).all() and (out["cov_pairs"][0] == 0).all()
        assert out["T"][:12].tobytes() == T[:12].tobytes()
        worst["rotations"] = max(worst.get("rotations", 0.0), check_rotations(out["T"], n))
        if K in (11, 43):  # two calls: the same bytes
            again = update_call(t, cand, T, method, pairs=PAIRS, columns="solve")
            for key in KEYS:
                assert out[key].tobytes() == again[key].tobytes(), key
            assert (out["d2_joint"], out["logdet_M"], out["logdet_R"]) == (again["d2_joint"], again["logdet_M"], again["logdet_R"])
    assert t.global_X().tobytes() == X0.tobytes()
    print("%d robots, %s, columns=\"solve\": largest error / bound: " % (N, method) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    t.close()


def test_the_default_is_the_blocks_route_and_schur_has_no_solve():
    n, N, K = N_POSES, 2, 11
    m, T, t = setup(n, N, "dense")
    ends, Rm, tm, kap, ta = closures(T, n, K, seed=17)
    cand = records(n, N, ends, Rm, tm, kap, ta)
    for method in ("dense", "nested"):
        a, b = update_call(t, cand, T, method, pairs=PAIRS), update_call(t, cand, T, method, pairs=PAIRS, columns="blocks")
        for key in KEYS:
            assert a[key].tobytes() == b[key].tobytes(), key
        assert (a["d2_joint"], a["logdet_M"], a["logdet_R"]) == (b["d2_joint"], b["logdet_M"], b["logdet_R"])
    with pytest.raises(ValueError, match="columns must be"):
        t.linear_update(cand, T, columns="rows")
    with pytest.raises(capi.DpgoError, match="Schur path's sets"):
        t.linear_update(cand, T, method="schur", columns="solve")
    # the raw call: refused with the outputs untouched
    bufs = [np.full(12 * n, 7.25), np.full((n, 6), 7.25), np.full((n, 6, 6), 7.25), np.full((len(PAIRS), 6, 6), 7.25),
            np.full((K, 6), 7.25), np.full((K, 6), 7.25), np.full(3, 7.25)]
    res = capi.Covariance()
    res.n = 5
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dpgo_team_linear_update_solved(t.h, p(T), capi.GATE_SCHUR, 0, K, p(cand), len(PAIRS), p(PAIRS), *[p(a) for a in bufs],
                                                   C.byref(res))
    msg = capi.lib().dpgo_last_error().decode()
    assert rc == capi.ERR and msg.startswith("linear_update:") and "Schur path's sets" in msg, msg
    assert all((a == 7.25).all() for a in bufs)
    t.close()

"""CPU checks of the covariances by nested dissection inside each robot (DESIGN.md 5e "nested"): the host-only plan on
the bundled graphs and on a banded chain, the numpy statement of the elimination (tests/covnested_ref.py) against the dense
reference inverse, and the Python layer's refusals, which need no device."""
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests import covnested_ref as NR
from tests import covref
from tests.util import DATA, ROOT

EPS = covref.EPS


def test_entries_are_declared_and_mirrored():
    txt = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    m = re.search(r"^#define\s+DPGO_COV_NESTED_DEFAULT_BLOCK\s+(\d+)\s*$", txt, flags=re.M)
    assert m and int(m.group(1)) == capi.COV_NESTED_DEFAULT_BLOCK
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {"dpgo_covariance_nested_plan": ["num_poses", "robot_of", "rowptr", "col", "max_block", "block_of", "info"],
            "dpgo_team_covariance_nested_plan": ["t", "max_block", "block_of", "info"],
            "dpgo_team_marginal_covariances_nested": ["t", "T", "max_block", "num_pairs", "pairs", "cov_diag", "cov_pairs", "res"]}
    for name, args in want.items():
        d = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert d, "%s is not declared" % name
        assert [a.strip().split()[-1].lstrip("*") for a in d.group(1).split(",")] == args
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    import inspect
    assert list(inspect.signature(capi.Team.covariances_nested).parameters)[1:] == ["T", "pairs", "max_block"]
    assert list(inspect.signature(capi.Team.covariance_plan).parameters)[1:] == ["max_block"]
    assert "covariance_max_block" in inspect.signature(capi.solve_certified).parameters


def check_plan(tag, rowptr, col, robot_of, max_block):
    """what every plan must satisfy; returns (block_of, info, sets)"""
    n = len(robot_of)
    block_of, info = capi.covariance_nested_plan(robot_of, rowptr, col, max_block)
    again, info2 = capi.covariance_nested_plan(robot_of, rowptr, col, max_block)
    assert block_of.tobytes() == again.tobytes() and info == info2  # deterministic
    s = NR.sets(block_of, rowptr, col)
    # every pose is placed exactly once
    assert block_of[0] == -2 and (block_of[1:] >= -1).all()
    assert sum(len(I) for I in s["blocks"]) + len(s["separator"]) == n - 1
    assert all(len(I) > 0 for I in s["blocks"])
    assert info["blocks"] == len(s["blocks"]) and info["separator_poses"] == len(s["separator"])
    assert info["largest_block"] == max(len(I) for I in s["blocks"])
    assert info["largest_coupling"] == max(len(N) for N in s["coupled"]) and info["coupling_total"] == sum(len(N) for N in s["coupled"])
    # blocks are ordered by robot, then by first pose; a block lies in one robot; it holds at most max_block + max_block // 5
    first = [(robot_of[I[0]], I[0]) for I in s["blocks"]]
    assert first == sorted(first)
    for I, N in zip(s["blocks"], s["coupled"]):
        assert len(set(robot_of[I])) == 1 and len(I) <= max_block + max_block // 5
        # every N_b lies in its own robot's range
        assert all(robot_of[s["separator"][k]] == robot_of[I[0]] for k in N)
    # no edge joins two blocks (a block and a separator pose outside its N_b: N_b is read off the same pattern, and
    # the numpy elimination asserts that H has nothing outside it)
    for g in range(1, n):
        if block_of[g] >= 0:
            nb = block_of[col[rowptr[g]:rowptr[g + 1]]]
            assert ((nb == block_of[g]) | (nb < 0)).all(), "pose %d of block %d touches another block" % (g, block_of[g])
    # public poses are separator poses
    for g in range(n):
        if (robot_of[col[rowptr[g]:rowptr[g + 1]]] != robot_of[g]).any() and g > 0:
            assert block_of[g] == -1
    print("%s at max_block %d: %r" % (tag, max_block, info))
    return block_of, info, s


@pytest.mark.parametrize("ds,max_block", [("sphere2500", 256), ("torus3D", 256), ("cubicle", 512), ("parking-garage", 256)])
def test_plan_of_a_bundled_graph_as_one_robot(ds, max_block):
    m, n = O.read_g2o(os.path.join(DATA, ds + ".g2o"))
    rowptr, col = NR.pattern(m, n)
    robot_of = np.zeros(n, dtype=np.int32)
    block_of, info, s = check_plan(ds + " / 1", rowptr, col, robot_of, max_block)
    assert info["blocks"] > 1 and info["promoted_poses"] == info["separator_poses"] > 0
    # one robot: the blocks are those of the two-level preconditioner's plan on the pattern without pose 0
    rp, cl = NR.restrict(rowptr, col, np.arange(1, n))
    sub_of, tl = capi.two_level_plan(rp, cl, max_block)
    assert (block_of[1:] == sub_of).all() and tl["subdomains"] == info["blocks"] and tl["separator_poses"] == info["separator_poses"]


def test_plan_of_sphere2500_among_five_robots():
    ds, N = "sphere2500", 5
    m, n = O.read_g2o(os.path.join(DATA, ds + ".g2o"))
    rowptr, col = NR.pattern(m, n)
    robot_of = NR.robots_of(n, N)
    block_of, info, s = check_plan("%s / %d" % (ds, N), rowptr, col, robot_of, 128)
    public = np.array([(robot_of[col[rowptr[g]:rowptr[g + 1]]] != robot_of[g]).any() for g in range(n)])
    public[0] = False
    assert info["separator_poses"] - info["promoted_poses"] == public.sum() and info["promoted_poses"] > 0
    # a robot whose interior fits is left whole: a block size between the smallest and the largest interior
    sizes = sorted(int((~public[1:] & (robot_of[1:] == a)).sum()) for a in range(N))
    assert sizes[0] < sizes[-1]
    mid = sizes[0]
    block_of, info, s = check_plan("%s / %d" % (ds, N), rowptr, col, robot_of, mid)
    whole = 0
    for a in range(N):
        I = [g for g in range(1, n) if robot_of[g] == a and not public[g]]
        if len(I) <= mid:
            assert len(set(block_of[I])) == 1 and block_of[I[0]] >= 0 and (block_of == block_of[I[0]]).sum() == len(I)
            whole += 1
        else:
            assert len(set(block_of[I])) > 2
    assert 0 < whole < N
    # a block size at or above every interior: no robot is split, the sets are those of the robot-wise Schur path
    block_of, info, s = check_plan("%s / %d" % (ds, N), rowptr, col, robot_of, sizes[-1])
    assert info["promoted_poses"] == 0 and info["blocks"] == N and (block_of[public] == -1).all()


def test_plan_of_a_banded_chain():
    n = 2400
    m, _ = NR.banded_chain(n, 5)
    rowptr, col = NR.pattern(m, n)
    block_of, info, s = check_plan("banded chain %d" % n, rowptr, col, np.zeros(n, dtype=np.int32), 128)
    assert info["separator_poses"] <= n // 4
    # two robots: the cut makes poses public, the rest of either robot is dissected on its own
    check_plan("banded chain %d / 2" % n, rowptr, col, NR.robots_of(n, 2), 128)


def test_plan_refuses_what_is_not_team_order():
    rowptr, col = NR.pattern(NR.banded_chain(40, 1)[0], 40)
    for bad in (np.r_[np.ones(20), np.zeros(20)], np.r_[np.zeros(20), 2 * np.ones(20)]):
        with pytest.raises(capi.DpgoError, match="team order"):
            capi.covariance_nested_plan(bad, rowptr, col, 4)
    with pytest.raises(ValueError, match="robot_of holds"):
        capi.covariance_nested_plan(np.zeros(39), rowptr, col, 4)


def elimination_case(tag, m, n, T, robot_of, max_block):
    Hr, Sref, w = covref.dense_reference(covref.q_full(m.view(O.MEAS_DTYPE), n), T, n)
    assert w[0] > 0
    rowptr, col = NR.pattern(m, n)
    block_of, info, s = check_plan(tag, rowptr, col, robot_of, max_block)
    assert info["promoted_poses"] > 0, "the case does not split a robot"
    S, logdet = NR.nested_reference(Hr, s)
    nn, cond = 6 * (n - 1), w[-1] / w[0]
    bound = nn * EPS * cond
    err = np.linalg.norm(S - Sref) / np.linalg.norm(Sref)
    sign, ld = np.linalg.slogdet(Hr)
    lerr = abs(logdet - ld) / abs(ld)
    print("%s: cond_2 %.3e, |Sigma - ref|_F / |ref|_F = %.3e (bound %.3e, ratio %.3e), logdet rel %.3e, large buffers %d bytes"
          % (tag, cond, err, bound, err / bound, lerr, NR.nested_bytes(s)))
    assert err <= bound and sign > 0 and lerr <= bound


def test_numpy_elimination_on_smallGrid3D_between_two_robots():
    ds, N = "smallGrid3D", 2
    m, n = O.read_g2o(os.path.join(DATA, ds + ".g2o"))
    elimination_case("%s / %d" % (ds, N), m.view(capi.MEAS_DTYPE), n, O.chordal_init(m, n), NR.robots_of(n, N), 16)


@pytest.mark.parametrize("n,max_block,longs", [(40, 1, 0), (120, 4, 0), (360, 11, 3)])
def test_numpy_elimination_on_a_banded_chain(n, max_block, longs):
    m, T = NR.banded_chain(n, 5, longs=longs)
    elimination_case("banded chain (%d, %d, %d)" % (n, max_block, longs), m, n, T, np.zeros(n, dtype=np.int32), max_block)


def test_python_refusals_need_no_device():
    t = object.__new__(capi.Team)  # (no team is created: no device is touched)
    with pytest.raises(ValueError, match="no call across teams"):
        capi.Team.covariances(t, method="nested", transport=object())
    with pytest.raises(ValueError, match='method must be "dense", "schur" or "nested"'):
        capi.Team.covariances(t, method="sparse")


def test_first_failing_factor_names_the_spoiled_block_or_the_separator():
    """the CPU prediction of the pivot refusal (covnested_ref.first_failing_factor), which the GPU tests hold the message to:
    none at the ground truth; one block's rotations replaced -> that block, and the leading minor that numpy's Cholesky
    rejects first; a separator pose's rotation replaced -> the separator, every block still positive definite"""
    n, max_block = 120, 4
    m, Tg = NR.banded_chain(n, 5)
    rowptr, col = NR.pattern(m, n)
    block_of, info = capi.covariance_nested_plan(np.zeros(n, dtype=np.int32), rowptr, col, max_block)
    s = NR.sets(block_of, rowptr, col)
    Q = covref.q_full(m, n)
    assert NR.first_failing_factor(covref.reduced(covref.hessian(Q, Tg, n)).tocsr(), s) is None
    b = [k for k in range(len(s["blocks"]) // 2, len(s["blocks"])) if len(s["blocks"][k]) >= 2][0]
    Hr = covref.reduced(covref.hessian(Q, NR.spoil_rotations(Tg, n, s["blocks"][b], 1), n)).toarray()
    f = NR.first_failing_factor(Hr, s)
    print(f)
    assert f["kind"] == "block" and f["block"] == b and f["pose"] == s["blocks"][b][f["row"] // 6] and f["pivot"] <= 0
    r = NR.rows(s["blocks"][b])
    Hbb = Hr[np.ix_(r, r)]
    np.linalg.cholesky(Hbb[:f["row"], :f["row"]])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(Hbb[:f["row"] + 1, :f["row"] + 1])
    for k in range(b):
        rk = NR.rows(s["blocks"][k])
        np.linalg.cholesky(Hr[np.ix_(rk, rk)])
    for seed in range(20):
        Hs = covref.reduced(covref.hessian(Q, NR.spoil_rotations(Tg, n, s["separator"][seed:seed + 1], seed), n)).toarray()
        g = NR.first_failing_factor(Hs, s)
        if g is not None and g["kind"] == "separator":
            break
    else:
        raise AssertionError("no spoiled separator pose left every block positive definite")
    print(g)
    assert g["block"] == -1 and g["pose"] == s["separator"][g["row"] // 6] and block_of[g["pose"]] == -1
    for I in s["blocks"]:
        rk = NR.rows(I)
        np.linalg.cholesky(Hs[np.ix_(rk, rk)])
    assert np.linalg.eigvalsh(Hs)[0] < 0

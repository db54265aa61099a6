"""CPU checks of the covariances by robot-wise Schur complement: the interface is declared and mirrored,
the numpy statement of the path (tests/covschur_ref.py) agrees with the dense reference inverse, and the Python layer's
refusals need no device."""
import os
import re

import numpy as np
import pytest

from dpgo_ros_amd import capi
from oracle import oracle as O
from tests import covref, covschur_ref
from tests.util import DATA, ROOT

EPS = covref.EPS


def test_flag_and_across_entry_are_declared_and_mirrored():
    txt = open(os.path.join(ROOT, "include", "dpgo_hip.h")).read()
    m = re.search(r"^#define\s+DPGO_COV_SCHUR\s+(\d+)\s*$", txt, flags=re.M)
    assert m and int(m.group(1)) == 1 == capi.COV_SCHUR
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    d = re.search(r"\bint\s+dpgo_team_marginal_covariances_across\s*\(([^;]*)\)\s*;", code)
    assert d, "the across entry is not declared"
    args = [a.strip().split()[-1].lstrip("*") for a in d.group(1).split(",")]
    assert args == ["t", "tr", "owner_rank_of_robot", "T", "flags", "num_pairs", "pairs", "cov_diag", "cov_pairs", "res"]
    assert "dpgo_team_marginal_covariances_across" in capi.EXPORTS
    assert hasattr(capi.lib(), "dpgo_team_marginal_covariances_across")
    import inspect
    sig = inspect.signature(capi.Team.covariances)
    assert list(sig.parameters)[1:] == ["T", "pairs", "method", "transport", "owner_of_robot"]
    assert "covariance_method" in inspect.signature(capi.solve_certified).parameters


@pytest.mark.parametrize("ds,N,all_public", [("tinyGrid3D", 1, False), ("tinyGrid3D", 2, False), ("smallGrid3D", 2, False),
                                             ("smallGrid3D", 3, False), ("smallGrid3D", 5, False), ("smallGrid3D", 3, True)])
def test_numpy_schur_path_matches_dense_reference(ds, N, all_public):
    """every block of Sigma and log det at the chordal point within n eps cond_2 of the dense inverse (measured: at most 2e-3
    of the bound)"""
    m, n = O.read_g2o(os.path.join(DATA, ds + ".g2o"))
    mc = m.view(capi.MEAS_DTYPE)
    mp = capi.partition(mc, n, N) if N > 1 else mc
    T = O.chordal_init(m, n)
    Hr, Sref, w = covref.dense_reference(covref.q_full(m, n), T, n)
    assert w[0] > 0
    robot_of, public = covschur_ref.partition(mp, n, N, all_public)
    S, logdet, info = covschur_ref.schur_reference(Hr, robot_of, public)
    nn, cond = 6 * (n - 1), w[-1] / w[0]
    bound = nn * EPS * cond
    err = np.linalg.norm(S - Sref) / np.linalg.norm(Sref)
    sign, ld = np.linalg.slogdet(Hr)
    lerr = abs(logdet - ld) / abs(ld)
    print("%s / %d%s: %d public poses, largest interior %d, |Sigma - ref|_F / |ref|_F = %.3e (bound %.3e, ratio %.3e), "
          "logdet rel %.3e" % (ds, N, ", all public" if all_public else "", len(info["separator"]), info["largest_interior"],
                               err, bound, err / bound, lerr))
    assert len(info["separator"]) + sum(len(i) for i in info["interior"]) == n - 1
    if all_public:
        assert info["largest_interior"] == 0
    if N == 1:
        assert not info["separator"]
    assert err <= bound and sign > 0 and lerr <= bound


def test_dense_method_with_a_transport_is_refused_without_a_device():
    """the Python layer decides before the library is asked for anything"""
    t = object.__new__(capi.Team)  # (no team is created: no device is touched)
    with pytest.raises(ValueError, match="no dense path"):
        capi.Team.covariances(t, method="dense", transport=object())
    with pytest.raises(ValueError, match="method must be"):
        capi.Team.covariances(t, method="sparse")
    import inspect
    assert "covariances" in inspect.signature(__import__("dpgo_ros_amd.distributed", fromlist=["x"]).certify_and_round).parameters

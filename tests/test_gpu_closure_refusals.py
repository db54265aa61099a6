"""The refusals that the six calls behind the covariance paths share (csrc/closure_frame.h): gate_candidates,
pairwise_consistency, audit_measurements, gate_candidates_jointly, linear_update and linear_removal word them from the call's
name and the noun of its records, and each is written out here in full.  tinyGrid3D over 2 robots at the chordal T; three records of which
the one at index 1 is malformed, so that the index in the message is exercised.  For every entry point and record: the error
code, the whole message, and every output still at its sentinel.  Nothing runs on the device but the team's construction and
the gate's relative-covariance query, which reads the endpoints alone and so takes the records with malformed measurement
fields."""
import os

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests.test_gpu_audit import raw_audit
from tests.test_gpu_consistency import fresh_outputs, raw_call
from tests.test_gpu_covariance_nested import team_of
from tests.test_gpu_gate import raw_gate
from tests.test_gpu_gate_joint import raw_joint
from tests.test_gpu_linear_removal import raw_removal
from tests.test_gpu_linear_update import raw_update
from tests.util import DATA

pytestmark = pytest.mark.gpu

CALLS = {  # entry point: (the call's name, the noun of its records)
    "gate": ("gate_candidates", "candidate"),
    "consistency": ("pairwise_consistency", "candidate"),
    "audit": ("audit_measurements", "record"),
    "joint": ("gate_candidates_jointly", "candidate"),
    "update": ("linear_update", "closure"),
    "removal": ("linear_removal", "record"),
}
ENDPOINT_CASES = ("robot", "pose", "self")
FIELD_CASES = ("kappa", "tau", "scaled", "reflected", "inf")
CASES = ENDPOINT_CASES + FIELD_CASES + ("weight", "unweighted")
FILL = 7.25


@pytest.fixture(scope="module")
def team():
    m, n = capi.read_g2o(os.path.join(DATA, "tinyGrid3D.g2o"))
    T = capi.chordal_init(m, n)
    t = team_of(m, n, 2, T)
    yield t, np.ascontiguousarray(T, dtype=np.float64).reshape(-1), n
    t.close()


def records(t):
    """three sound records between the two robots, identity measurements at weight 1"""
    rec = np.zeros(3, dtype=capi.MEAS_DTYPE)
    rec["r1"], rec["r2"] = t.ids[0], t.ids[1]
    rec["p1"], rec["p2"] = (1, 2, 3), (0, 1, 2)
    rec["R"] = np.eye(3).reshape(9)
    rec["kappa"] = rec["tau"] = rec["weight"] = 1.0
    return rec


def malformed(t, entry, case):
    """(records with the one at index 1 spoiled, the message behind "<name>: ")"""
    noun = CALLS[entry][1]
    rec = records(t)
    two = entry == "consistency"  # its endpoints lie in team A and team B, and its messages say which
    n1 = t.agents[t.ids[1]].n
    if case == "robot":
        rec["r1"][1] = 7
        return rec, "%s 1 names robot 7, which is not in %s" % (noun, "team A" if two else "the team")
    if case == "pose":
        rec["p2"][1] = n1
        return rec, "%s 1 names pose %d of robot %d%s, outside [0, %d)" % (noun, n1, t.ids[1], " of team B" if two else "", n1)
    if case == "self":
        rec["r2"][1], rec["p2"][1] = rec["r1"][1], rec["p1"][1]
        return rec, "%s 1 joins a pose to itself" % noun
    if case == "kappa":
        rec["kappa"][1] = 0.0
        return rec, "%s 1 has kappa = 0, tau = 1: both must be positive" % noun
    if case == "tau":
        rec["tau"][1] = np.nan
        return rec, "%s 1 has kappa = 1, tau = nan: both must be positive" % noun
    if case == "scaled":
        rec["R"][1] *= 1.0 + 1e-6
        return rec, "the measurement of %s 1 is not in SE(3) (|R R^T - I| = 2e-06, det R = 1.000003)" % noun
    if case == "reflected":
        rec["R"][1][8] = -1.0
        return rec, "the measurement of %s 1 is not in SE(3) (|R R^T - I| = 0, det R = -1)" % noun
    if case == "inf":
        rec["t"][1][2] = np.inf
        return rec, "the measurement of %s 1 is not in SE(3) (|R R^T - I| = 0, det R = 1)" % noun
    if case == "weight":
        rec["weight"][1] = -1.0
        return rec, "%s 1 has weight = -1: it must be finite and not negative" % noun
    assert case == "unweighted"
    rec["weight"][1] = 0.0
    return rec, "%s 1 has weight = 0: a record must be in the graph at a positive weight" % noun


def call(entry, t, T, n, rec):
    """the raw call on fresh sentinels: (return code, message, per output whether it still holds its sentinel)"""
    K, res = len(rec), capi.Covariance()
    res.n = 5
    if entry == "consistency":  # (one team on both sides: the refusals come before anything is asked of either)
        o = fresh_outputs(K)
        o["res_a"].n = o["res_b"].n = 5
        blank = {k: v.copy() for k, v in o.items() if isinstance(v, np.ndarray)}
        rc = raw_call(t, T, t, T, capi.GATE_DENSE, 0, rec, 0.99, 0, o)
        untouched = [o[k].tobytes() == blank[k].tobytes() for k in blank]
        untouched += [o["size"].value == -7, o["proven"].value == -7, o["res_a"].n == 5, o["res_b"].n == 5]
        return rc, capi.lib().dpgo_last_error().decode(), untouched
    ints = lambda k: np.full(k, 7, dtype=np.int32)
    if entry == "gate":
        outs = [np.full((K, 6), FILL), np.full(K, FILL), np.full((K, 6, 6), FILL)]
        rc = raw_gate(t, T, capi.GATE_DENSE, 0, rec, outs[0], outs[1], outs[2], res)
    elif entry == "audit":
        outs = [np.full(s, FILL) for s in ((K, 6), (K, 6), K, K, K, (K, 6, 6))]
        rc = raw_audit(t, T, capi.GATE_DENSE, 0, rec, 1e-6, outs, res)
    elif entry == "joint":
        outs = [np.full((K, 6), FILL), np.full(K, FILL), np.full((K, 6), FILL), np.full(K, FILL), ints(K), ints(K), ints(1),
                np.full(1, FILL), np.full(1, FILL), np.full((6 * K, 6 * K), FILL)]
        rc = raw_joint(t, T, capi.GATE_DENSE, 0, rec, capi.JOINT_GREEDY, 0.99, outs, res)
    else:
        pairs = np.array([(1, 2)], dtype=np.int32)
        outs = [np.full(12 * n, FILL), np.full((n, 6), FILL), np.full((n, 6, 6), FILL), np.full((1, 6, 6), FILL), np.full((K, 6), FILL),
                np.full((K, 6), FILL)]
        if entry == "update":
            outs += [np.full(3, FILL)]
            rc = raw_update(t, T, capi.GATE_DENSE, 0, rec, pairs, outs, res)
        else:  # (new_weight null: every record goes to weight 0)
            outs += [np.full(K, FILL), np.full(4, FILL)]
            rc = raw_removal(t, T, capi.GATE_DENSE, 0, rec, None, 1e-6, pairs, outs, res)
    untouched = [bool((a == (7 if a.dtype == np.int32 else FILL)).all()) for a in outs] + [res.n == 5]
    return rc, capi.lib().dpgo_last_error().decode(), untouched


def applies(entry, case):
    if case == "weight":
        return entry in ("audit", "removal")  # (the two that read the weight)
    if case == "unweighted":
        return entry == "removal"  # (the audit takes a record at weight 0; the removal has no weight to take out of it)
    if case == "self":
        return entry != "consistency"  # (its two endpoints lie in different teams: no pose is joined to itself)
    return True


@pytest.mark.parametrize("entry,case", [(e, c) for e in CALLS for c in CASES if applies(e, c)])
def test_a_malformed_record_is_refused_by_name_and_index(team, entry, case):
    t, T, n = team
    rec, want = malformed(t, entry, case)
    rc, msg, untouched = call(entry, t, T, n, rec)
    assert rc == capi.ERR, (rc, msg)
    assert msg == CALLS[entry][0] + ": " + want
    assert all(untouched), untouched


@pytest.mark.parametrize("case", FIELD_CASES)
def test_the_relative_covariance_query_reads_the_endpoints_alone(team, case):
    """gate_candidates with xi = d2 = null forms sigma_rel only and does not read the measurement fields"""
    t, T, n = team
    rec, _ = malformed(t, "gate", case)
    sg, res = np.full((3, 6, 6), FILL), capi.Covariance()
    assert raw_gate(t, T, capi.GATE_DENSE, 0, rec, None, None, sg, res) == capi.OK, capi.lib().dpgo_last_error().decode()
    assert np.isfinite(sg).all() and not (sg == FILL).any() and res.n == 6 * (n - 1)
    good = np.full((3, 6, 6), FILL)
    assert raw_gate(t, T, capi.GATE_DENSE, 0, records(t), None, None, good, capi.Covariance()) == capi.OK
    assert sg.tobytes() == good.tobytes()


@pytest.mark.parametrize("case", ENDPOINT_CASES)
def test_the_relative_covariance_query_still_checks_the_endpoints(team, case):
    t, T, n = team
    rec, want = malformed(t, "gate", case)
    sg, res = np.full((3, 6, 6), FILL), capi.Covariance()
    res.n = 5
    assert raw_gate(t, T, capi.GATE_DENSE, 0, rec, None, None, sg, res) == capi.ERR
    assert capi.lib().dpgo_last_error().decode() == "gate_candidates: " + want
    assert (sg == FILL).all() and res.n == 5

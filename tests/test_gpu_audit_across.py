"""GPU checks of the leave-one-out audit over a split team (dpgo_team_audit_measurements_across, csrc/audit.hip behind
csrc/covariance_schur.hip; Team.audit / Team.zero_weight_measurements with transport=, DESIGN.md 5h "across teams"), of the
helpers of dpgo_ros_amd.distributed over gloo, and of the absence of side effects of both calls across teams.  The contract is
bitwise, as in tests/test_gpu_gate_across.py: every output equals the single team's method="schur" call on the same T and
records and is identical on every participant."""
import ctypes as C
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests.test_gpu_certify_across import Split, bits, problem, single_team
from tests.test_gpu_covariance_across import scalars
from tests.test_gpu_gate_across import SPLITS, reference, refused_everywhere
from tests.util import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("measurements", "xi", "xi_loo", "d2", "redundancy", "pivot_min", "testable", "accept", "sigma_loo")


def same_audit(out, ref):
    return sorted(out) == sorted(ref) and scalars(out["covariance"]) == scalars(ref["covariance"]) and \
        all(bits(out[k]) == bits(ref[k]) for k in KEYS)


def shared_edges(mp, count, seed):
    """`count` seeded shared edges of the partitioned measurements, as (r1, p1, r2, p2)"""
    sh = mp[mp["r1"] != mp["r2"]]
    pick = np.random.default_rng(seed).choice(len(sh), count, replace=False)
    return [(int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"])) for e in sh[pick]]


def set_weights(t, edges):
    """the first half of the edges to weight 0, the second to 0.5, on every robot of t that stores the edge: its owner (the
    lower robot, whose weight the audit lists) and the other end (whose rows of the Hessian hold the block)"""
    for k, (r1, p1, r2, p2) in enumerate(edges):
        for a in (r1, r2):
            if a in t.agents:
                assert t.agents[a].set_measurement_weight(r1, p1, r2, p2, 0.0 if k < len(edges) // 2 else 0.5), (a, r1, p1, r2, p2)


_AUDIT = {}


def audit_reference(ds, N):
    """(edges, the single team's zero_weight_measurements(), its audit(T=T, method="schur", sigma_loo=True)) on the team with
    ten shared edges at weight 0 and ten at 0.5, computed once per dataset"""
    if (ds, N) not in _AUDIT:
        m, mp, n, X, T, cand, goff, _ = reference(ds, N)
        edges = shared_edges(mp, 20, 5)
        t = single_team(mp, N, X)
        set_weights(t, edges)
        zw = t.zero_weight_measurements()
        ref = t.audit(T=T, method="schur", sigma_loo=True)
        assert bits(ref["measurements"]) == bits(t.measurements_once())
        t.close()
        _AUDIT[(ds, N)] = (edges, zw, ref)
    return _AUDIT[(ds, N)]


def test_one_participant_equals_the_single_team_bitwise():
    ds, N = "smallGrid3D", 3
    m, mp, n, X, T, cand, goff, _ = reference(ds, N)
    edges, zw, ref = audit_reference(ds, N)
    t = single_team(mp, N, X)
    set_weights(t, edges)
    g = capi.LocalGroup(1)
    own = np.zeros(N, dtype=np.int32)
    assert same_audit(t.audit(T=T, sigma_loo=True, transport=g[0], owner_of_robot=own), ref)
    assert same_audit(t.audit(ref["measurements"], T=T, method="schur", sigma_loo=True, transport=g[0], owner_of_robot=own), ref)
    out = t.audit(T=T, transport=g[0], owner_of_robot=own)  # without sigma_loo
    assert "sigma_loo" not in out and all(bits(out[k]) == bits(ref[k]) for k in KEYS[:-1])
    assert bits(t.zero_weight_measurements(transport=g[0], owner_of_robot=own)) == bits(zw)
    # T = None rounds across first: the single team's own rounding
    assert same_audit(t.audit(sigma_loo=True, transport=g[0], owner_of_robot=own), t.audit(method="schur", sigma_loo=True))
    t.close()


@pytest.mark.parametrize("ds,N,parts", SPLITS)
def test_audit_over_every_split(ds, N, parts):
    m, mp, n, X, T, cand, goff, _ = reference(ds, N)
    edges, zw, ref = audit_reference(ds, N)
    holder = {i: q for q, ids in enumerate(parts) for i in ids}
    crossing = [holder[e[0]] != holder[e[2]] for e in edges]
    # the w = 0 branch (the gate exactly) and a fractional weight both cross a participant boundary
    assert any(crossing[:10]) and any(crossing[10:]), crossing
    assert len(zw) == 10 and (ref["measurements"]["weight"] == 0.5).sum() == 10
    sp = Split(mp, N, parts, X)
    for t in sp.teams:
        set_weights(t, edges)
    out = sp.run(lambda tm, tr: (tm.audit(T=T[sp.cols(tr.rank, 12)], sigma_loo=True, transport=tr, owner_of_robot=sp.owner),
                                 tm.zero_weight_measurements(transport=tr, owner_of_robot=sp.owner)))
    for q, (o, z) in enumerate(out):
        assert bits(o["measurements"]) == bits(ref["measurements"]), q  # (the single team's measurements_once())
        assert same_audit(o, ref), q
        assert bits(z) == bits(zw) and len(z) == 10, q
    print("%s %s: %d records, %d testable, %d accepted; w = 0 crossing %d, w = 0.5 crossing %d" % (
        ds, parts, len(ref["d2"]), ref["testable"].sum(), ref["accept"].sum(), sum(crossing[:10]), sum(crossing[10:])))
    sp.close()


def raw_audit_across(tm, tr, own, T, meas, outs, res, min_redundancy=1e-6):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dpgo_team_audit_measurements_across(tm.h, C.byref(tr.struct), p(own), p(T), len(meas), p(meas),
                                                        C.c_double(min_redundancy), *[p(a) for a in outs], C.byref(res))
    return rc, capi.lib().dpgo_last_error().decode()


def audit_outs(K):
    return [(K, 6), (K, 6), (K,), (K,), (K,), (K, 6, 6)]


def test_refusals_reach_every_participant():
    ds, N, parts = "smallGrid3D", 3, [[0, 1], [2]]
    m, mp, n, X, T, cand, goff, _ = reference(ds, N)
    sp = Split(mp, N, parts, X)
    own = capi._owner_array(sp.owner)
    Tq = [T[sp.cols(q, 12)] for q in range(2)]
    t = single_team(mp, N, X)
    meas = t.measurements_once()
    ref = t.audit(meas, T=T, method="schur", sigma_loo=True)
    t.close()

    def refused(args, match, raw=raw_audit_across):
        msgs = refused_everywhere(sp, own, args, match, raw, audit_outs)
        out = sp.run(lambda tm, tr: tm.audit(meas, T=Tq[tr.rank], sigma_loo=True, transport=tr, owner_of_robot=sp.owner))
        assert all(same_audit(o, ref) for o in out)  # (the transport is not left half-way)
        return msgs

    refused(lambda q: (Tq[q], meas[:len(meas) - q]), "the number of records")
    other = meas.copy()
    other[11]["weight"] = 0.75  # (the weight is the fifteenth double of the hash)
    refused(lambda q: (Tq[q], other if q else meas), "the record list")
    out_ = meas.copy()
    out_[3]["p1"] = int(np.diff(goff)[out_[3]["r1"]])
    msgs = refused(lambda q: (Tq[q], out_), "outside [0, ")
    assert msgs[0] == msgs[1] and "record 3 names pose" in msgs[0]
    same = meas.copy()
    same[4]["r2"], same[4]["p2"] = same[4]["r1"], same[4]["p1"]
    refused(lambda q: (Tq[q], same), "record 4 joins a pose to itself")
    neg = meas.copy()
    neg[6]["weight"] = -0.5
    refused(lambda q: (Tq[q], neg), "record 6 has weight = -0.5")
    zero = meas.copy()
    zero[9]["kappa"] = 0.0
    refused(lambda q: (Tq[q], zero), "record 9 has kappa = 0")
    refused(lambda q: (Tq[q], meas), "min_redundancy must lie in (0, 1)",
            raw=lambda *a: raw_audit_across(*a, min_redundancy=1.0))
    Tb = Tq[1].copy()
    Tb[12 * 4] *= 1.001
    msgs = refused(lambda q: (Tb if q else Tq[0], meas), "rank 1")
    assert "SE(3)" in msgs[1], msgs
    g = capi.LocalGroup(2)
    for kw in (dict(method="nested"), dict(method="dense"), dict(max_block=16)):
        with pytest.raises(ValueError, match="transport"):
            sp.teams[0].audit(meas, T=Tq[0], transport=g[0], owner_of_robot=sp.owner, **kw)
    assert g[0].calls == dict(allgather=0, exchange=0)
    sp.close()


def solver_state(t):
    """the iterate (X, Y, V), the weights and the cost of a team"""
    return [np.concatenate([t.agents[i]._get(w) for i in t.ids]) for w in (0, 1, 2)] + \
        [np.concatenate([t.agents[i].measurements()["weight"] for i in t.ids]), np.array([t.cost()])]


def test_the_calls_have_no_side_effects():
    """every participant's iterate, weights and cost are bitwise the same before and after a gate and an audit across teams,
    and a run that goes on afterwards is bitwise the run without them (the pattern of test_split_calls_have_no_side_effects)"""
    ds, N, parts = "smallGrid3D", 3, [[0, 1], [2]]
    m, mp, n, X, T, cand, goff, _ = reference(ds, N)
    edges, _, _ = audit_reference(ds, N)
    sp = Split(mp, N, parts, X)
    for t in sp.teams:
        set_weights(t, edges)
    before = [solver_state(t) for t in sp.teams]
    sp.run(lambda tm, tr: (tm.gate(cand, T[sp.cols(tr.rank, 12)], sigma_rel=True, transport=tr, owner_of_robot=sp.owner),
                           tm.audit(T=T[sp.cols(tr.rank, 12)], sigma_loo=True, transport=tr, owner_of_robot=sp.owner),
                           tm.gate(cand, transport=tr, owner_of_robot=sp.owner)))  # (T = None: rounds across first)
    for t, b in zip(sp.teams, before):
        for x, y in zip(solver_state(t), b):
            assert bits(x) == bits(y)
    sp.close()
    from tests.test_gpu_certificate import RTR_NESTEROV
    outs = []
    for with_calls in (False, True):
        t = single_team(mp, N, X, **RTR_NESTEROV)
        t.run(20)
        if with_calls:
            g = capi.LocalGroup(1)
            own = np.zeros(N, dtype=np.int32)
            t.gate(cand, T, transport=g[0], owner_of_robot=own)
            t.audit(T=T, transport=g[0], owner_of_robot=own)
        t.run(40)
        outs.append(solver_state(t))
        t.close()
    for a, b in zip(*outs):
        assert bits(a) == bits(b)


def _pack(gate_out, audit_out):
    r, xi, d2, acc, sg = gate_out
    return np.concatenate([np.array(scalars(r), dtype=float), xi.ravel(), d2, acc.astype(float), sg.ravel()] +
                          [np.asarray(audit_out[k]).astype(float).ravel() for k in KEYS[1:]] +
                          [np.frombuffer(bits(audit_out["measurements"]), np.uint8).astype(float)])


def _gloo_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd import distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    X, T = (np.load(os.path.join(outdir, f + ".npy")) for f in ("X", "T"))
    cand = np.load(os.path.join(outdir, "cand.npy")).view(capi.MEAS_DTYPE).reshape(-1)
    m, mp, n = problem("smallGrid3D", 3)
    sp = Split(mp, 3, [[0, 1], [2]], X)
    Tl = T[sp.cols(rank, 12)]
    go = distributed.gate_candidates(sp.teams[rank], dist, sp.owner, cand, T=Tl, sigma_rel=True)
    ao = distributed.audit(sp.teams[rank], dist, sp.owner, T=Tl, sigma_loo=True)
    np.save(os.path.join(outdir, "out%d.npy" % rank), _pack(go, ao))
    sp.close()
    dist.destroy_process_group()


def _gloo_worker_limited(rank, world, port, outdir):
    import faulthandler
    faulthandler.dump_traceback_later(240.0, exit=True)  # (a child that waits on a lost peer ends itself)
    _gloo_worker(rank, world, port, outdir)
    faulthandler.cancel_dump_traceback_later()


def test_two_processes_over_gloo_equal_two_threads():
    import torch.multiprocessing as mp_
    ds, N, parts = "smallGrid3D", 3, [[0, 1], [2]]
    m, mp, n, X, T, cand, goff, _ = reference(ds, N)
    sp = Split(mp, N, parts, X)
    res = sp.run(lambda tm, tr: (tm.gate(cand, T[sp.cols(tr.rank, 12)], sigma_rel=True, transport=tr, owner_of_robot=sp.owner),
                                 tm.audit(T=T[sp.cols(tr.rank, 12)], sigma_loo=True, transport=tr, owner_of_robot=sp.owner)))
    sp.close()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "X.npy"), X)
        np.save(os.path.join(d, "T.npy"), T)
        np.save(os.path.join(d, "cand.npy"), np.frombuffer(bits(cand), np.uint8))
        mp_.spawn(_gloo_worker_limited, args=(2, port, d), nprocs=2, join=True)
        for q in range(2):
            assert bits(np.load(os.path.join(d, "out%d.npy" % q))) == bits(_pack(*res[q])), q

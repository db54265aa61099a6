"""distributed.refine(..., gather=True) over two gloo ranks (one process per rank, both on one device; DESIGN.md 5n "Across
teams"), on refineref's 12-pose chain as three robots with robots 0 and 1 on rank 0 and robot 2 on rank 1, from T* perturbed by
s = 1e-3.  The processes are spawned the way tests/test_distributed_apply_gloo.py spawns its own; the teams need a GPU, so the
test is marked as the other gloo tests of the calls across teams are.  T comes back in global pose order, identical on both
ranks, the bits of the LocalGroup call on the same split, with its history and scalars.  In the same processes
distributed.certify_and_round(refine=True, covariances=True) on teams whose iterate is that start lifted: out["refine"] has
converged, out["T"] is the refined T of the whole problem within refineref.final_bound of T*, and the covariances are those of
the refined T, bit for bit."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from tests import refineacross_ref as XF
from tests import refineref as RR
from tests.util import ROOT

pytestmark = pytest.mark.gpu

NAME, N, S = "chain12", 3, 1e-3
PARTS = [[0, 1], [2]]
GRAD_TOL = 1e-9


def _problem():
    from tests.test_gpu_covariance_nested import team_of
    c = XF.case(NAME)
    sp = XF.split(NAME, N)
    t = team_of(c["m"], c["n"], N, c["truth"])
    X0 = t.global_X()
    t.close()
    return c, sp["mp"], X0, RR.start(c["Tstar"], c["n"], S, 11)


def _numbers(o):
    h = o["history"]
    return np.concatenate([[o["iterations"], o["f0"], o["f"], o["grad_inf0"], o["grad_inf"]], h["f"], h["grad_inf"], h["alpha"],
                           h["decrement"], h["pivot_min"]])


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd import distributed
    from tests.test_gpu_certify_across import Split
    dist.init_process_group("gloo", rank=rank, world_size=world)
    c, mp, X0, T0 = _problem()
    sp = Split(mp, N, PARTS, X0)
    tm = sp.teams[rank]
    Tq = T0[sp.cols(rank, 12)]
    og = distributed.refine(tm, dist, sp.owner, T=Tq, gather=True, grad_tol=GRAD_TOL)
    ol = distributed.refine(tm, dist, sp.owner, T=Tq, grad_tol=GRAD_TOL)
    assert ol["T"].tobytes() == np.ascontiguousarray(og["T"][sp.cols(rank, 12)]).tobytes() and ol["status"] == og["status"] == "converged"
    np.save(os.path.join(outdir, "T%d.npy" % rank), og["T"])
    np.save(os.path.join(outdir, "s%d.npy" % rank), _numbers(og))
    sp.close()
    # certify_and_round(refine=True): the teams at the lifted start, whose rounding is the start up to round-off
    from tests.test_gpu_covariance_nested import team_of
    t = team_of(c["m"], c["n"], N, T0)
    sp = Split(mp, N, PARTS, t.global_X())
    t.close()
    tm = sp.teams[rank]
    plain = distributed.certify_and_round(tm, dist, sp.owner, max_iters=20)
    out = distributed.certify_and_round(tm, dist, sp.owner, max_iters=20, refine=True, covariances=True)
    assert sorted(out) == sorted(list(plain) + ["refine", "covariances"]) and out["f_rounded"] == plain["f_rounded"]
    r = out["refine"]
    assert r["status"] == "converged" and r["grad_inf"] <= 1e-8 and r["iterations"] >= 1, (r["status"], r["history"]["grad_inf"])
    assert np.ascontiguousarray(out["T"][sp.cols(rank, 12)]).tobytes() == r["T"].tobytes()
    owners = sorted(set(int(o) for o in sp.owner))
    own = np.array([owners.index(int(o)) for o in sp.owner], dtype=np.int32)
    _, diag, _ = tm.covariances(r["T"], transport=distributed.TorchTransport(dist), owner_of_robot=own)
    assert out["covariances"][1][sp.cols(rank, 1)].tobytes() == diag.tobytes()  # taken at the refined T
    np.save(os.path.join(outdir, "R%d.npy" % rank), out["T"])
    sp.close()
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_the_refined_T():
    import torch.multiprocessing as mp_
    from dpgo_ros_amd import capi
    from tests.test_gpu_certify_across import Split, bits
    c, mp, X0, T0 = _problem()
    n = c["n"]
    sp = Split(mp, N, PARTS, X0)
    outs = sp.run(lambda tm, tr: tm.refine(T0[sp.cols(tr.rank, 12)], grad_tol=GRAD_TOL, transport=tr, owner_of_robot=sp.owner),
                  capi.LocalGroup(2))
    want = np.zeros(12 * n)
    for q in range(2):
        want[sp.cols(q, 12)] = outs[q]["T"]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        mp_.spawn(_worker, args=(2, port, d), nprocs=2, join=True)
        T = [np.load(os.path.join(d, "T%d.npy" % q)) for q in range(2)]
        sc = [np.load(os.path.join(d, "s%d.npy" % q)) for q in range(2)]
        R = [np.load(os.path.join(d, "R%d.npy" % q)) for q in range(2)]
    assert T[0].shape == (12 * n,)
    assert bits(T[0]) == bits(T[1]) and bits(sc[0]) == bits(sc[1])
    assert bits(T[0]) == bits(want) and bits(sc[0]) == bits(_numbers(outs[0]))
    assert outs[0]["status"] == "converged" and outs[0]["iterations"] == 3
    err = float(np.abs(T[0] - c["Tstar"]).max()) / RR.final_bound(c["Q"], c["Tstar"], n, GRAD_TOL)
    print("two gloo ranks, %s as %d robots, s = %g: %d iterations, |T - T*|_inf %.3g of the bound" % (NAME, N, S, outs[0]["iterations"], err))
    assert err <= 1.0
    fb = RR.final_bound(c["Q"], c["Tstar"], n, 1e-8)
    assert bits(R[0]) == bits(R[1]) and float(np.abs(R[0] - c["Tstar"]).max()) <= fb
    print("certify_and_round(refine=True): |T - T*|_inf %.3g of the bound" % (float(np.abs(R[0] - c["Tstar"]).max()) / fb))
    sp.close()

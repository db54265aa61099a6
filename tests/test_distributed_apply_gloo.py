"""distributed.covariance_apply(..., gather=True) over two gloo ranks (one process per rank, both on one device; DESIGN.md 5m
"across teams"), on applyacross_ref's 12-pose graph of three robots with robots 0 and 1 on rank 0 and robot 2 on rank 1.
The processes are spawned the way tests/test_distributed_gloo.py spawns its own; the teams need a GPU, so the test is marked
as the other gloo tests of the calls across teams are.  X comes back in global pose order, identical on both ranks, the bits
of the LocalGroup call on the same split, and within applyref's bound of the longdouble dense solve."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from tests import applyacross_ref as XR
from tests import applyref as AR
from tests.util import ROOT

pytestmark = pytest.mark.gpu

KEY = XR.GRAPHS[0][:3]
PARTS = [[0, 1], [2]]
M_COLS = 33


def _problem():
    from tests.test_gpu_covariance_nested import team_of
    n, seed, N = KEY
    g = XR.graph(n, seed, N)
    t = team_of(g["m"], n, N, g["T"])
    X0 = t.global_X()
    t.close()
    V = np.random.default_rng(24).standard_normal((6 * n, M_COLS))
    return g, X0, V


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd import distributed
    from tests.test_gpu_certify_across import Split
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g, X0, V = _problem()
    sp = Split(g["mp"], KEY[2], PARTS, X0)
    tm = sp.teams[rank]
    Vq, Tq = V[sp.cols(rank, 6)], g["T"][sp.cols(rank, 12)]
    res, Xg = distributed.covariance_apply(tm, dist, sp.owner, Vq, T=Tq, gather=True)
    res2, Xl = distributed.covariance_apply(tm, dist, sp.owner, Vq, T=Tq)
    assert Xl.tobytes() == np.ascontiguousarray(Xg[sp.cols(rank, 6)]).tobytes() and res2.logdet == res.logdet
    np.save(os.path.join(outdir, "X%d.npy" % rank), Xg)
    np.save(os.path.join(outdir, "s%d.npy" % rank), np.array([res.n, res.logdet, res.min_pivot, res.max_pivot]))
    sp.close()
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_the_global_X():
    import torch.multiprocessing as mp_
    from dpgo_ros_amd import capi
    from tests.test_gpu_certify_across import Split, bits
    n, seed, N = KEY
    g, X0, V = _problem()
    sp = Split(g["mp"], N, PARTS, X0)
    outs = sp.run(lambda tm, tr: tm.covariance_apply(V[sp.cols(tr.rank, 6)], g["T"][sp.cols(tr.rank, 12)], transport=tr,
                                                     owner_of_robot=sp.owner), capi.LocalGroup(2))
    want = np.zeros((6 * n, M_COLS))
    for q in range(2):
        want[sp.cols(q, 6)] = outs[q][1]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        mp_.spawn(_worker, args=(2, port, d), nprocs=2, join=True)
        X = [np.load(os.path.join(d, "X%d.npy" % q)) for q in range(2)]
        sc = [np.load(os.path.join(d, "s%d.npy" % q)) for q in range(2)]
    assert X[0].shape == (6 * n, M_COLS)
    assert bits(X[0]) == bits(X[1]) and bits(sc[0]) == bits(sc[1])
    assert bits(X[0]) == bits(want)
    assert bits(X[0][:6]) == bits(np.zeros((6, M_COLS)))
    r = outs[0][0]
    assert bits(sc[0]) == bits(np.array([r.n, r.logdet, r.min_pivot, r.max_pivot]))
    Xref, b = XR.reference(g["Hr"], V)
    w = AR.worst(X[0], Xref, b)
    print("two gloo ranks, %d poses as %d robots, m = %d: largest column error / bound %.3g" % (n, N, M_COLS, w))
    assert w <= 1.0
    sp.close()

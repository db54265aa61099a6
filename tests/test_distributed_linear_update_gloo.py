"""distributed.linear_update(..., gather=True) over two gloo ranks (one process per rank, both on one device; DESIGN.md 5j
"Across teams"), on applyacross_ref's 12-pose graph of three robots with robots 0 and 1 on rank 0 and robot 2 on rank 1, K = 11
closures and the pairs of tests/updateacross_ref.py.  The processes are spawned the way tests/test_distributed_apply_gloo.py
spawns its own; the teams need a GPU, so the test is marked as the other gloo tests of the calls across teams are.  The dict
comes back with T, delta and cov_diag in global pose order, identical on both ranks, the bits of the LocalGroup call on the same
split, and within updateacross_ref's bound of the longdouble update."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

from tests import applyacross_ref as XR
from tests import updateacross_ref as UX
from tests.util import ROOT

pytestmark = pytest.mark.gpu

KEY = XR.GRAPHS[0][:3]
PARTS = [[0, 1], [2]]
K = 11
ARRAYS = ("T", "delta", "cov_diag", "cov_pairs", "xi", "xi_post")
FIGURES = ("d2_joint", "logdet_M", "logdet_R", "information_gain")


def _problem():
    from tests.test_gpu_covariance_nested import team_of
    n, seed, N = KEY
    g = XR.graph(n, seed, N)
    t = team_of(g["m"], n, N, g["T"])
    X0 = t.global_X()
    t.close()
    cl = UX.closures(g, K)
    return g, X0, cl, UX.records(g, *cl), UX.pairs_of(g)


def _figures(out):
    r = out["covariance"]
    return np.array([out[k] for k in FIGURES] + [r.n, r.logdet, r.min_pivot, r.max_pivot])


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd import distributed
    from tests.test_gpu_certify_across import Split
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g, X0, cl, cand, pairs = _problem()
    sp = Split(g["mp"], KEY[2], PARTS, X0)
    tm = sp.teams[rank]
    Tq = g["T"][sp.cols(rank, 12)]
    og = distributed.linear_update(tm, dist, sp.owner, cand, T=Tq, pairs=pairs, gather=True)
    ol = distributed.linear_update(tm, dist, sp.owner, cand, T=Tq, pairs=pairs)
    assert ol["T"].tobytes() == np.ascontiguousarray(og["T"][sp.cols(rank, 12)]).tobytes()
    assert ol["delta"].tobytes() == np.ascontiguousarray(og["delta"][sp.cols(rank, 1)]).tobytes()
    assert ol["cov_diag"].tobytes() == np.ascontiguousarray(og["cov_diag"][sp.cols(rank, 1)]).tobytes()
    np.savez(os.path.join(outdir, "out%d.npz" % rank), figures=_figures(og), **{k: og[k] for k in ARRAYS})
    sp.close()
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_the_global_update():
    import torch.multiprocessing as mp_
    from dpgo_ros_amd import capi
    from tests.test_gpu_certify_across import Split, bits
    n, seed, N = KEY
    g, X0, cl, cand, pairs = _problem()
    sp = Split(g["mp"], N, PARTS, X0)
    outs = sp.run(lambda tm, tr: tm.linear_update(cand, g["T"][sp.cols(tr.rank, 12)], pairs=pairs, transport=tr, owner_of_robot=sp.owner),
                  capi.LocalGroup(2))
    want = dict(T=np.zeros(12 * n), delta=np.zeros((n, 6)), cov_diag=np.zeros((n, 6, 6)))
    for q in range(2):
        want["T"][sp.cols(q, 12)], want["delta"][sp.cols(q, 1)], want["cov_diag"][sp.cols(q, 1)] = (outs[q]["T"], outs[q]["delta"],
                                                                                                  outs[q]["cov_diag"])
    for k in ("cov_pairs", "xi", "xi_post"):
        want[k] = outs[0][k]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        mp_.spawn(_worker, args=(2, port, d), nprocs=2, join=True)
        got = [dict(np.load(os.path.join(d, "out%d.npz" % q))) for q in range(2)]
    assert got[0]["T"].shape == (12 * n,) and got[0]["delta"].shape == (n, 6) and got[0]["cov_diag"].shape == (n, 6, 6)
    for k in ARRAYS + ("figures",):
        assert bits(got[0][k]) == bits(got[1][k]), k
    for k in ARRAYS:
        assert bits(got[0][k]) == bits(want[k]), k
    assert bits(got[0]["figures"]) == bits(_figures(outs[0]))
    ref, b, b0 = UX.reference(g, *cl, pairs)
    out = dict(got[0], **dict(zip(FIGURES, got[0]["figures"][:4])))
    r = UX.ratios(out, ref, b)
    print("two gloo ranks, %d poses as %d robots, K = %d: error / bound " % (n, N, K) + ", ".join("%s %.3g" % kv for kv in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    sp.close()

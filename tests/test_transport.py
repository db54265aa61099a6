"""CPU checks of the transports of the calls across teams (dpgo_transport_t): capi.LocalGroup (threads of one process) and
distributed.TorchTransport over gloo, both driven through the C function pointers the library calls -- allgather order,
exchange routing with zero counts, and a failure that reaches every participant instead of a hang."""
import ctypes as C
import os
import socket
import sys
import tempfile

import numpy as np

from dpgo_ros_amd import capi
from tests.util import ROOT


def c_allgather(tr, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(tr.world * x.size)
    rc = tr.struct.allgather(None, x.ctypes.data_as(C.POINTER(C.c_double)), x.size, out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def c_exchange(tr, parts, recv_counts):
    send = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=np.float64)
    sc = np.array([len(p) for p in parts], dtype=np.int64)
    rc_ = np.array(recv_counts, dtype=np.int64)
    recv = np.zeros(int(rc_.sum()))
    rc = tr.struct.exchange(None, send.ctypes.data_as(C.POINTER(C.c_double)), sc.ctypes.data_as(C.POINTER(C.c_longlong)),
                            recv.ctypes.data_as(C.POINTER(C.c_double)), rc_.ctypes.data_as(C.POINTER(C.c_longlong)))
    return rc, recv


def payload(q, p):
    """what rank q sends to rank p: nothing when (q + p) % 3 == 0, else q * 10 + p repeated q + p + 1 times"""
    return np.zeros(0) if (q + p) % 3 == 0 else np.full(q + p + 1, 10.0 * q + p)


def check_rank(tr, q, world):
    rc, out = c_allgather(tr, np.array([q, q + 0.5, -q]))
    assert rc == 0
    assert np.array_equal(out, np.concatenate([[p, p + 0.5, -p] for p in range(world)]))
    parts = [payload(q, p) for p in range(world)]
    rc, recv = c_exchange(tr, parts, [len(payload(p, q)) for p in range(world)])
    assert rc == 0
    want = np.concatenate([payload(p, q) for p in range(world)])
    assert np.array_equal(recv, want)
    return True


def test_local_group_allgather_order_and_exchange_routing():
    for world in (1, 2, 3, 5):
        g = capi.LocalGroup(world, timeout=30)
        res = g.run([lambda q=q: check_rank(g[q], q, world) for q in range(world)], timeout=60)
        assert all(r is True and e is None for r, e in res), res
        assert all(t.calls == {"allgather": 1, "exchange": 1} for t in g)


def test_local_group_failure_reaches_every_participant():
    """rank 1 passes a different size; then rank 0 leaves the sequence: every other rank's call fails, none waits forever"""
    g = capi.LocalGroup(3, timeout=30)
    res = g.run([lambda q=q: c_allgather(g[q], np.zeros(2 if q != 1 else 3))[0] for q in range(3)], timeout=60)
    assert [r for r, _ in res] == [-1, -1, -1]
    g = capi.LocalGroup(3, timeout=5)
    res = g.run([lambda q=q: None if q == 0 else c_allgather(g[q], np.zeros(2))[0] for q in range(3)], timeout=60)
    assert [r for r, _ in res] == [None, -1, -1]


def _gloo_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dpgo_ros_amd.distributed import TorchTransport
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = TorchTransport(dist)
    ok = check_rank(tr, rank, world)
    # a failing participant's status word reaches every rank through the allgather
    rc, out = c_allgather(tr, np.array([1.0 if rank == 1 else 0.0, 7.0]))
    failed = [q for q in range(world) if out[2 * q] != 0.0]
    np.save(os.path.join(outdir, "r%d.npy" % rank), np.array([ok, rc] + failed, dtype=float))
    dist.destroy_process_group()


def test_torch_transport_over_gloo():
    import torch.multiprocessing as mp_
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        mp_.spawn(_gloo_worker, args=(2, port, d), nprocs=2, join=True)
        for q in range(2):
            assert np.array_equal(np.load(os.path.join(d, "r%d.npy" % q)), [1.0, 0.0, 1.0])

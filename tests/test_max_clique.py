"""CPU checks of dpgo_max_clique (csrc/max_clique.cpp, capi.max_clique) through the library: sizes against brute
force, the form of the answer, the word edges, the node limit and every refusal."""
import ctypes as C

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import pcmref as P


def random_graph(K, density, seed):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.random((K, K)) < density, 1)
    return A | A.T


def is_clique(A, members):
    m = np.asarray(members)
    sub = A[np.ix_(m, m)]
    return bool((sub | np.eye(len(m), dtype=bool)).all())


def greedy_seed(A):
    """the seed as DESIGN.md 5g states it: the vertex of least remaining degree (the lowest index among equals) leaves first
    and is numbered last; the greedy clique takes the vertices in that numbering"""
    K = len(A)
    deg, gone, order = A.sum(1).astype(int), np.zeros(K, dtype=bool), []
    for _ in range(K):
        live = np.flatnonzero(~gone)
        v = int(live[np.argmin(deg[live])])
        gone[v] = True
        order.append(v)
        deg[A[v] & ~gone] -= 1
    seed = []
    for v in order[::-1]:
        if all(A[v, u] for u in seed):
            seed.append(v)
    return sorted(seed)


def test_sizes_equal_brute_force_on_random_graphs():
    rng = np.random.default_rng(0)
    for g in range(200):
        K = int(rng.integers(1, 21))
        A = random_graph(K, (0.1, 0.3, 0.5, 0.7, 0.9)[g % 5], 1000 + g)
        members, proven = capi.max_clique(A)
        want = P.max_clique_brute(A)
        assert proven and len(members) == len(want), (g, K, members, want)
        assert is_clique(A, members) and (np.diff(members) > 0).all()
        again, _ = capi.max_clique(A)
        assert members.tobytes() == again.tobytes()


@pytest.mark.parametrize("K", [1, 64, 65, 129])
def test_word_edges(K):
    empty = np.zeros((K, K), dtype=bool)
    members, proven = capi.max_clique(empty)
    assert proven and len(members) == 1 and 0 <= members[0] < K
    full = ~np.eye(K, dtype=bool)
    members, proven = capi.max_clique(full)
    assert proven and members.tolist() == list(range(K))
    # a clique that straddles the last word edge, in a sparse graph
    A = random_graph(K, 0.05, K)
    top = np.arange(max(K - 5, 0), K)
    A[np.ix_(top, top)] = True
    np.fill_diagonal(A, False)
    members, proven = capi.max_clique(A)
    assert proven and is_clique(A, members) and len(members) == len(P.max_clique_brute(A)) >= len(top)


def test_a_planted_clique_is_found_and_proven():
    K = 300
    A = random_graph(K, 0.3, 7)
    planted = np.sort(np.random.default_rng(8).permutation(K)[:40])
    A[np.ix_(planted, planted)] = True
    np.fill_diagonal(A, False)
    members, proven = capi.max_clique(A)
    assert proven and members.tolist() == planted.tolist()


def test_the_node_limit_returns_a_clique_that_is_not_proven():
    K = 120
    A = random_graph(K, 0.5, 3)
    full, proven = capi.max_clique(A)
    assert proven
    members, proven = capi.max_clique(A, max_nodes=1)
    assert not proven and is_clique(A, members) and (np.diff(members) > 0).all()
    seed = greedy_seed(A)
    assert is_clique(A, seed) and len(seed) <= len(members) <= len(full)
    more, _ = capi.max_clique(A, max_nodes=50)
    assert len(members) <= len(more) <= len(full)


def raw(K, words, max_nodes=0, members=True, size=True, proven=True):
    m, s, p = np.full(max(K, 1), -7, dtype=np.int32), C.c_int(-7), C.c_int(-7)
    rc = capi.lib().dpgo_max_clique(K, None if words is None else words.ctypes.data_as(C.c_void_p), C.c_longlong(max_nodes),
                                    m.ctypes.data_as(C.c_void_p) if members else None, C.byref(s) if size else None,
                                    C.byref(p) if proven else None)
    return rc, capi.lib().dpgo_last_error().decode(), m, s.value, p.value


def test_refusals():
    A = random_graph(70, 0.4, 5)
    words = capi._adjacency_words(A)
    assert words.shape == (70, 2)

    def refused(what, K=70, w=words, **kw):
        rc, msg, m, s, p = raw(K, w, **kw)
        assert rc == capi.ERR and what in msg, (rc, msg)
        assert (m == -7).all() and s == -7 and p == -7

    refused("K must be positive", K=0)
    refused("K must be positive", K=-2)
    refused("null argument", w=None)
    refused("null argument", members=False)
    refused("null argument", size=False)
    refused("null argument", proven=False)
    refused("max_nodes must not be negative", max_nodes=-1)
    bad = words.copy()
    bad[3, 0] ^= np.uint64(1) << np.uint64(9)
    refused("not symmetric", w=bad)
    bad = words.copy()
    bad[5, 0] |= np.uint64(1) << np.uint64(5)
    refused("the diagonal bit of row 5", w=bad)
    bad = words.copy()
    bad[65, 1] |= np.uint64(1) << np.uint64(1)  # column 65: the diagonal in the second word
    refused("the diagonal bit of row 65", w=bad)
    bad = words.copy()
    bad[2, 1] |= np.uint64(1) << np.uint64(6)  # column 70 = K
    refused("at or beyond column K", w=bad)
    with pytest.raises(ValueError, match="square"):
        capi.max_clique(np.zeros((3, 4), dtype=bool))
    with pytest.raises(capi.DpgoError, match="not symmetric"):
        B = A.copy()
        B[0, 1], B[1, 0] = True, False
        capi.max_clique(B)

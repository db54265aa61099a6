"""The deep-carried one-launch iteration (csrc/step_deep.hip, k_step_fd) has its four streamer waves fetch the packed edge
coefficients and hand them to the chain: 256 lanes cover the FE_MAX_EDGES * 8 = 1280 parts of 16 bytes in five loads per lane,
a lane beyond the last part takes the last part and writes it to that part's own place (tests/test_step_coef_handoff_build.py
holds the shape of that code on the assembly).  No expression changed, so the iterates must stay bitwise those of the same run
with DPGO_FE_DEEP=0 (k_step_fe), as in tests/test_gpu_step_count_in.py, at the shared-edge counts where the cover of the parts
can go wrong.

The team is that file's: sphere2500 cut to 2494 poses, agents of 512 / 499 / 498 / 499 / 486 poses -- the smallest that still
take the form -- with 51 / 102 / 102 / 102 / 51 shared edges.  The count of the middle agent (nshared, 8 parts per edge) is moved
by synthetic measurements between poses that are ALREADY public on both sides (npub and the 24 private chunks stay), at most
one extra edge per pose, half of them towards agent 1 and half towards agent 3; rotation and translation are those of the
shared edge of the graph whose translation has the median length, kappa and tau the graph's medians.  Both teams of a pair
are built from the same measurements.

    nshared of agent 2   parts   why
    102 (the graph's)      816   the last trip of wave 0 (parts 768 ..) is partly live, waves 1-3 have none in it
    104                    832   a multiple of 8 edges: that trip is exactly full
    128                   1024   a multiple of 32: the parts end on a boundary of 256, the fifth load is all clamped
    129                   1032   eight parts into the fifth load
    160                   1280   FE_MAX_EDGES: every part live, no lane clamped

The agents beside the middle one move with it (102 -> 103 / 115 / 115 or 116 / 131), the end agents keep 51 edges (408 parts: in
the second load wave 2 is partly live and wave 3 has no live part, in the last three loads no wave has one).  Every count is reached with the
form still taken.

r = 3, 4, 5 at restart 3 and 7 on the graph as it is, r = 5 at restart 7 on the others; runs of 6, 23 and 64 iterations one
behind the other; X, Y, V of every agent, every status and the cost with np.array_equal / ==; the deep counter rises in
every run."""
import numpy as np
import pytest

from tests.test_gpu_step_count_in import RUNS, SIZES, _pair, _status
from tests.test_gpu_step_front import BASE_PUB, BASE_SHARED, _owner, _partition, _shared_counts
from oracle import oracle as O
from tests.util import load

pytestmark = pytest.mark.gpu

MID = 2
FE_MAX_EDGES = 160
# nshared of the middle agent -> the counts of all five
WANT = {
    102: (51, 102, 102, 102, 51),
    104: (51, 103, 104, 103, 51),
    128: (51, 115, 128, 115, 51),
    129: (51, 116, 129, 115, 51),
    160: (51, 131, 160, 131, 51),
}


@pytest.fixture(scope="module")
def graph():
    m, _, _ = load("sphere2500", 1)
    n = sum(SIZES)
    m = m[(m["p1"] < n) & (m["p2"] < n)].copy()
    assert _shared_counts(m) == (BASE_SHARED, BASE_PUB)
    return m, O.odometry_init(m, n)


def _extra(m, nshared):
    """the measurements that bring the middle agent to `nshared` shared edges: ceil(half) towards agent MID - 1, the rest
    towards MID + 1, each between two poses that already carry a shared edge of that pair of agents, no pose used twice"""
    add = nshared - BASE_SHARED[MID]
    assert 0 <= add and nshared <= FE_MAX_EDGES
    if add == 0:
        return m[:0].copy()
    o1, o2 = _owner(m["p1"]), _owner(m["p2"])
    x = o1 != o2
    have = set(zip(m["p1"][x].tolist(), m["p2"][x].tolist()))
    # the template: the shared edge whose translation has the median length
    sh = m[x]
    tpl = sh[np.argsort(np.linalg.norm(sh["t"], axis=1))[len(sh) // 2]]
    out = []
    for (a, b), count in (((MID - 1, MID), (add + 1) // 2), ((MID, MID + 1), add // 2)):
        e = x & (o1 == a) & (o2 == b)
        pa, pb = sorted(set(m["p1"][e].tolist())), sorted(set(m["p2"][e].tolist()))
        assert count <= min(len(pa), len(pb)), ((a, b), count, len(pa), len(pb))
        # pose k of one side with pose k + shift of the other: the first shift at which no pair repeats an edge of the graph
        for shift in range(1, len(pb)):
            pairs = [(pa[k], pb[(k + shift) % len(pb)]) for k in range(count)]
            if not any(p in have for p in pairs):
                break
        else:
            raise AssertionError("no shift without a repeated pair")
        for i, j in pairs:
            r = tpl.copy()
            r["p1"], r["p2"] = i, j
            r["kappa"], r["tau"], r["weight"] = np.median(m["kappa"]), np.median(m["tau"]), 1.0
            out.append(r)
    out = np.array(out, dtype=m.dtype)
    ends = np.concatenate([out["p1"], out["p2"]])
    assert len(set(ends.tolist())) == len(ends), "a pose carries two extra edges"
    return out


def _team_graph(m, nshared):
    mm = np.concatenate([m, _extra(m, nshared)])
    shared, pub = _shared_counts(mm)
    assert shared == WANT[nshared] and pub == BASE_PUB, (nshared, shared, pub)
    return _partition(mm, SIZES)


CASES = [(102, r, ri) for r in (3, 4, 5) for ri in (3, 7)] + [(ns, 5, 7) for ns in (104, 128, 129, 160)]


@pytest.mark.parametrize("nshared,r,restart_interval", CASES)
def test_streamers_hand_over_coefficients_bitwise(graph, nshared, r, restart_interval):
    m, T = graph
    flat, deep = _pair(_team_graph(m, nshared), T, r, restart_interval)
    assert tuple(deep.agents[k].n for k in deep.ids) == SIZES
    before = deep.counters()[9]
    for iters in RUNS:
        for t in (flat, deep):
            t.run(iters)
            t.synchronize()
        tag = (nshared, r, restart_interval, iters)
        for k in flat.ids:
            a, b = flat.agents[k], deep.agents[k]
            assert np.array_equal(a.get_X(), b.get_X()), (tag, k, "X")
            assert np.array_equal(a.get_Y(), b.get_Y()), (tag, k, "Y")
            assert np.array_equal(a.get_V(), b.get_V()), (tag, k, "V")
        sa, sb = _status(flat), _status(deep)
        assert sa == sb, (tag, sa, sb)
        ca, cb = flat.cost(), deep.cost()
        assert ca == cb, (tag, ca, cb)
        now = deep.counters()[9]
        print("nshared %d, r = %d, restart %d, run of %d: deep-carried launches %d -> %d, cost %.15g"
              % (nshared, r, restart_interval, iters, before, now, cb))
        assert now > before, (tag, "the deep-carried form did not run")
        before = now
    assert flat.counters()[9] == 0 and flat.counters()[7] > 0
    for t in (flat, deep):
        t.close()

"""The chordal initialisation (csrc/chordal.hip) and the dense SPD solve behind it (dense_spd_solve of
csrc/dense_inverse.hip: k_syrk_sb, k_solve_fwd, k_solve_bwd, k_aug_extract) against the precise reference of
tests/chordref.py, at the factored orders where the blocked kernels change shape and on relaxed blocks that are singular.

Three modes: the team path (default), DPGO_CHORDAL_DENSE=1 (the dense solve with the right-hand sides appended to the
matrix) and DPGO_CHORDAL_DENSE=1 DPGO_CHORDAL_AUG=0 (forward substitution as launches, k_solve_fwd).  Both switches are
read once per process: the default mode runs here, each of the others in ONE fresh child that loops over every case and
saves one .npz; the children run one after the other and the first that fails ends the module.

Bounds (u = 2^-53, N the factored order, kappa_2 that of the reduced matrix -- pose 0 removed --, both from the reference):
  linear solve      |x - x_ref|_F <= N u kappa_2 |x_ref|_F
  rotations         per pose 1024 u max(1, s1 / (s2 + s3)) + 2 / (s2 + s3) (stage-1 solve bound), s the reference block's
                    singular values (the projection's own conditioning plus Li's bound for the polar factor)
  translations      against the reference's stage 2 AT THE RETURNED ROTATIONS, under the linear-solve bound
None of them is taken from the kernels' output.  Largest error / bound measured on an MI355X (team / dense / dense, AUG=0):
  mesh           rotations 0.0022 / 0.0029 / 0.0029    translations 0.12 / 0.16 / 0.39
  chain          rotations 0.00084 / 0.00084 / 0.00087 translations 0.049 / 0.053 / 0.097
  stage 2 alone  0.088 / 0.070 / 0.16
  planted        rotations 4.8e-6 / 4.0e-6 / 4.0e-6    translations 1.2e-4 / 4.0e-4 / 4.9e-4
  self-loop      rotations 5.8e-5 / 7.0e-5 / 6.0e-5    translations 8.4e-4 / 4.1e-3 / 3.0e-3
(The rotation ratios are small because Li's term carries the whole stage-1 solve bound for every pose.)

Before k_project_so3 called the rounding's rd_nearest_rotation, its A V diag(w^-1/2) V^T gave, on the planted graph and
with DPGO_OK: NaN rotations on the rank-one leaf, its tail, the rank-two tail and (0.5, 1e-9, -1e-9); rotations 0.65 off
with |R^T R - I| = 0.5 on the rank-two leaf; |R^T R - I| up to 1 on the zero block; and on (0.9, 1e-6, 1e-7) rotations up
to 2.0e-3 off with |R^T R - I| up to 4e-3 -- now 8e-11 and 6e-16.  The dense path also counted a self-loop twice on the
diagonal and scattered its off-diagonal block over itself (1.4e6 times the rotation bound), and returned its errors without
a message.  The solve kernels themselves were within the bounds at every order before and after."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dpgo_ros_amd import capi
from tests import chordref as CR
from tests.util import ROOT

pytestmark = pytest.mark.gpu

MODES = {"team": {}, "dense": {"DPGO_CHORDAL_DENSE": "1"}, "dense_noaug": {"DPGO_CHORDAL_DENSE": "1", "DPGO_CHORDAL_AUG": "0"}}
BOUNDARIES = (32, 64, 256, 512, 768)  # NB = 32 rows per block, 64-wide tiles, 256 columns per super-block
# n + 3 and 3 n + 3 (n and 3 n without the appended rows) are the factored orders: 3 n + 3 is a multiple of 3, so the
# orders around 512 and 768 that are not come from stage 2 of graphs of 508 .. 512 and 764 .. 769 poses
NS = ([1, 2, 3, 10, 20, 21] + list(range(28, 34)) + list(range(60, 66)) + [84, 85, 86, 125, 169, 170, 171] +
      list(range(252, 258)) + [508, 509, 510, 511, 512, 764, 765, 766, 767, 769])
CHAIN_NS = [3, 33, 64, 86, 171, 257, 511]
N_PLANTED = 150


def orders(mode, n):
    """factored orders of stage 1 and stage 2"""
    return (3 * n, n) if mode == "dense_noaug" else (3 * n + 3, n + 3)


def test_the_orders_cover_every_block_edge():
    aug = {o for n in NS for o in orders("dense", n)}
    plain = {o for n in NS for o in orders("dense_noaug", n)}
    for b in BOUNDARIES:
        assert {b - 1, b, b + 1, b + 2, b + 3} <= aug, (b, sorted(aug))
        assert {b - 1, b, b + 1} <= plain, (b, sorted(plain))
    assert 85 in NS   # the appended rows at 255, 256, 257: across the first super-block edge
    assert 256 in NS  # a fourth super-block that holds nothing but the appended rows
    assert 257 in CHAIN_NS and len(CHAIN_NS) >= 6


# ----------------------------------------------------------------------------- the cases, rebuilt from seeds in every process
def random_poses(n, seed):
    rng = np.random.default_rng(seed)
    return CR.poses(np.array([CR.random_rotation(rng) for _ in range(n)]), rng.standard_normal((n, 3)))


def self_loop_graph():
    m, n = CR.mesh(40, seed=11)
    loop = m[5:6].copy()
    loop["p1"], loop["p2"] = 17, 17
    return np.concatenate([m[:30], loop, m[30:]]), n


def hanging_graph():
    """pose 17 hangs on edges of weight 0 only"""
    m, n = CR.mesh(40, seed=12)
    m["weight"][(m["p1"] == 17) | (m["p2"] == 17)] = 0.0
    return m, n


def graphs():
    g = {"mesh_%d" % n: CR.mesh(n) for n in NS}
    g.update({"chain_%d" % n: CR.chain(n) for n in CHAIN_NS})
    g["planted"] = CR.planted_mesh(N_PLANTED, CR.PLANTS)[:2]
    g["selfloop"] = self_loop_graph()
    return g


def run_all():
    """every case in this process's mode: {name: poses}, an error return (a numerical outcome, not a fault) as its message"""
    out = {}

    def attempt(name, fn, *args):
        try:
            out[name] = fn(*args)
        except capi.DpgoError as e:
            out[name] = np.array("refused: %s" % e)
    for name, (m, n) in graphs().items():
        attempt(name, capi.chordal_init, m, n)
        if name.startswith("mesh_"):
            attempt("stage2_%d" % n, capi.translations_given_rotations, m, n, random_poses(n, n))
    m, n = hanging_graph()
    attempt("hanging_chordal", capi.chordal_init, m, n)
    attempt("hanging_stage2", capi.translations_given_rotations, m, n, random_poses(n, 1))
    return out


@pytest.fixture(scope="module")
def results():
    assert "DPGO_CHORDAL_DENSE" not in os.environ and "DPGO_CHORDAL_AUG" not in os.environ
    res = {"team": run_all()}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("dense", "dense_noaug"):
            path = os.path.join(d, mode + ".npz")
            code = ("import sys; sys.path.insert(0, %r); import numpy as np; from tests.test_gpu_chordal_edges import run_all; "
                    "np.savez(%r, **run_all())" % (ROOT, path))
            subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, **MODES[mode]), timeout=600, cwd=ROOT)
            with np.load(path) as z:
                res[mode] = {k: z[k] for k in z.files}
    return res


_cases = {}


def case(name):
    if name not in _cases:
        m, n = graphs_cached()[name]
        precise = sorted(CR.planted_mesh(N_PLANTED, CR.PLANTS)[2]) if name == "planted" else ()
        _cases[name] = CR.Case(m, n, precise)
    return _cases[name]


def graphs_cached():
    if "graphs" not in _cases:
        _cases["graphs"] = graphs()
    return _cases["graphs"]


def check_init(name, mode, T, skip=(), cap=None):
    """finite, proper, rotations and translations within their bounds; returns the two largest error / bound ratios"""
    assert T.dtype.kind != "U", (name, mode, str(T))
    c = case(name)
    N1, N2 = orders(mode, c.n)
    assert T.shape == (12 * c.n,)
    assert np.isfinite(T).all(), (name, mode, "non-finite poses at", sorted(set(np.flatnonzero(~np.isfinite(T)) // 12)))
    if cap is not None:
        assert c.k1 <= cap and c.k2 <= cap, (name, c.k1, c.k2)
    rr = c.rotation_ratios(T, N1)
    rr[list(skip)] = 0.0
    tr = c.translation_ratio(T, N2)
    print("%-12s %-11s orders %4d %4d kappa_2 %8.3g %8.3g  rotations %.3g  translations %.3g of the bound"
          % (name, mode, N1, N2, c.k1, c.k2, rr.max(), tr))
    assert CR.proper(T) <= 1e-12, (name, mode, CR.proper(T))
    return rr, tr


def refused(results, mode, name, bad):
    """an error return where poses were due: noted in `bad`"""
    out = results[mode][name]
    if out.dtype.kind != "U":
        return False
    print("%-12s %-11s %s" % (name, mode, out))
    bad.append((name, str(out)))
    return True


def assert_all(failures):
    assert not failures, failures


@pytest.mark.parametrize("mode", list(MODES))
def test_orders_on_the_mesh(results, mode):
    """every n of NS on the well-conditioned mesh (kappa_2 <= 1e3 asserted from the reference: the bounds stay below 1e-10
    relative, where a kernel that loses digits shows).  n = 1 returns (I, 0)."""
    bad, worst = [], [0.0, 0.0]
    for n in NS:
        name = "mesh_%d" % n
        if refused(results, mode, name, bad):
            continue
        rr, tr = check_init(name, mode, results[mode][name], cap=1e3)
        worst = [max(worst[0], rr.max()), max(worst[1], tr)]
        if rr.max() > 1 or tr > 1:
            bad.append((name, float(rr.max()), int(rr.argmax()), tr))
    print("mesh, %s: largest error / bound: rotations %.3g, translations %.3g" % (mode, worst[0], worst[1]))
    assert_all(bad)


@pytest.mark.parametrize("mode", list(MODES))
def test_orders_on_the_chain(results, mode):
    """the ill-conditioned family (kappa_2 up to 7e4 at n = 511): the bounds follow it"""
    bad, worst = [], [0.0, 0.0]
    for n in CHAIN_NS:
        name = "chain_%d" % n
        if refused(results, mode, name, bad):
            continue
        rr, tr = check_init(name, mode, results[mode][name])
        worst = [max(worst[0], rr.max()), max(worst[1], tr)]
        if rr.max() > 1 or tr > 1:
            bad.append((name, float(rr.max()), int(rr.argmax()), tr))
    print("chain, %s: largest error / bound: rotations %.3g, translations %.3g" % (mode, worst[0], worst[1]))
    assert_all(bad)


@pytest.mark.parametrize("mode", list(MODES))
def test_stage_2_alone(results, mode):
    """translations_given_rotations with random rotations: the linear solve without the projection in front of it"""
    bad, worst = [], 0.0
    for n in NS:
        if refused(results, mode, "stage2_%d" % n, bad):
            continue
        m, _ = graphs_cached()["mesh_%d" % n]
        T0, T = random_poses(n, n), results[mode]["stage2_%d" % n]
        assert np.array_equal(T.reshape(n, 12)[:, :9], T0.reshape(n, 12)[:, :9])  # the rotations are the caller's
        assert np.isfinite(T).all(), (n, mode)
        if n == 1:
            assert not CR.translations_of(T).any()
            continue
        t_ref, k2 = CR.translations(m, n, CR.rotations_of(T0))
        err = float(np.linalg.norm((CR.translations_of(T) - t_ref).astype(np.float64)))
        ratio = err / CR.solve_bound(orders(mode, n)[1], k2, t_ref)
        print("stage 2 alone, n = %3d, %-11s order %4d kappa_2 %8.3g: %.3g of the bound" % (n, mode, orders(mode, n)[1], k2, ratio))
        worst = max(worst, ratio)
        if ratio > 1:
            bad.append((n, ratio))
    print("stage 2 alone, %s: largest error / bound %.3g" % (mode, worst))
    assert_all(bad)


@pytest.mark.parametrize("mode", list(MODES))
def test_planted_blocks(results, mode):
    """relaxed blocks U diag(sigma) V^T planted through four parallel edges 0 -> leaf (chordref.planted_mesh), each with a
    two-pose tail that inherits them.  Every rotation is finite and proper; blocks with one nearest rotation -- rank two,
    (0.9, 1e-6, 1e-7), the improper (-0.3, -0.2, -0.1) -- match the 40-digit reference under the rotation bound; rank one,
    rank zero and (0.5, 1e-9, -1e-9) (improper with s2 = s3: every rotation about u1 is as near) are checked for
    properness only."""
    _, _, where = CR.planted_mesh(N_PLANTED, CR.PLANTS)
    T = results[mode]["planted"]
    c = case("planted")
    for p, sigma in sorted(where.items()):
        R = CR.rotations_of(T)[p]
        print("planted pose %3d sigma %-22s reference s %s: max |R - R_ref| %.3g, |R^T R - I| %.3g"
              % (p, sigma, c.sv[p], np.abs(R - c.R[p]).max(), np.abs(R.T @ R - np.eye(3)).max()))
    skip = [p for p, sigma in where.items() if sigma in CR.NOT_UNIQUE]
    assert len(skip) == 9 and len(where) == 21
    rr, tr = check_init("planted", mode, T, skip=skip)
    print("planted, %s: largest error / bound: rotations %.3g (pose %d), translations %.3g" % (mode, rr.max(), rr.argmax(), tr))
    assert rr.max() <= 1 and tr <= 1, (mode, float(rr.max()), int(rr.argmax()), tr)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_pose_on_edges_of_weight_zero_is_refused(results, mode):
    """a singular system: an error with a message, never poses that are not finite"""
    for name in ("hanging_chordal", "hanging_stage2"):
        out = results[mode][name]
        assert out.dtype.kind == "U" and str(out).startswith("refused: "), (mode, name, out)
        assert len(str(out)) > len("refused: chordal_init failed: "), (mode, name, str(out))
        print(mode, name, str(out))
    assert "not joined to pose 0" in str(results[mode]["hanging_stage2"])


def test_a_self_loop_is_skipped(results):
    """an edge from a pose to itself constrains nothing: all three modes agree with the reference, which leaves it out"""
    m, n = graphs_cached()["selfloop"]
    assert (m["p1"] == m["p2"]).sum() == 1
    for mode in MODES:
        rr, tr = check_init("selfloop", mode, results[mode]["selfloop"], cap=1e3)
        assert rr.max() <= 1 and tr <= 1, (mode, float(rr.max()), tr)

"""CPU checks of the chordal reference tests/chordref.py: it agrees with the oracle's sparse-Cholesky chordal initialisation
under the bounds the GPU tests use (tests/test_gpu_chordal_edges.py), it reproduces closed forms (a noise-free trajectory; a
leaf joined only to pose 0 gets the weighted mean of its edge rotations), and each of those bounds rejects a planted defect
at a small and a large order: an edge dropped from the system, a 32-row block of the solution zeroed, 64 rows of it
perturbed by 1e-6 relative, and the unguarded A V diag(w^-1/2) V^T projection on the planted blocks."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import chordref as CR
from tests.util import load

LD = CR.LD


@pytest.mark.parametrize("ds", ["tinyGrid3D", "smallGrid3D"])
def test_agrees_with_the_oracle(ds):
    m, _, n = load(ds, 1)
    c = CR.Case(m, n)
    To = O.chordal_init(m, n)
    rr, tr = c.rotation_ratios(To, 3 * n).max(), c.translation_ratio(To, n)
    print("%s: kappa_2 %.3g / %.3g, rotations %.3g, translations %.3g of the bound" % (ds, c.k1, c.k2, rr, tr))
    assert rr <= 1 and tr <= 1
    assert CR.proper(c.T) <= 1e-14


def test_a_noise_free_trajectory_is_reproduced():
    """the walk's poses, composed in fp64, solve both stages up to their own rounding: within the bounds"""
    m, n, Rg, tg = CR.mesh(60, noise=0.0, truth=True)
    c = CR.Case(m, n)
    Tg = CR.poses(Rg, tg)
    assert np.abs(c.sv - 1).max() <= 1e-12  # the relaxed blocks are rotations already
    assert c.rotation_ratios(Tg, 3 * n).max() <= 1
    assert c.translation_ratio(Tg, n) <= 1
    assert np.abs(c.T - Tg).max() <= 1e-12


def test_a_leaf_on_pose_0_gets_the_weighted_mean_of_its_edges():
    m, n, where = CR.planted_mesh(150, CR.PLANTS)
    blocks, _, _ = CR.relaxed_rotations(m, n)
    for leaf, _, _, sigma in CR.PLANTS:
        e = m[(m["p1"] == 0) & (m["p2"] == leaf)]
        k = (e["weight"] * e["kappa"]).astype(LD)
        mean = (k[:, None, None] * e["R"].reshape(-1, 3, 3).astype(LD)).sum(0) / k.sum()
        assert np.abs(blocks[leaf] - mean).max() <= 16 * CR.U, (leaf, sigma)
        s = np.linalg.svd(blocks[leaf].astype(np.float64), compute_uv=False)
        assert np.abs(s - np.sort(np.abs(sigma))[::-1]).max() <= 16 * CR.U, (leaf, sigma, s)


def defects(x, rng):
    """the three defects of a solution x (rows x 3): (name, defective copy)"""
    rows = x.shape[0]
    z = x.copy()
    r0 = (rows // 2) // 32 * 32
    z[r0:r0 + 32] = 0
    p = x.copy()
    r0 = max(0, rows - 64 - 5)
    p[r0:r0 + 64] *= 1 + 1e-6 * rng.choice([-1.0, 1.0], p[r0:r0 + 64].shape)
    return [("a 32-row block zeroed", z), ("64 rows perturbed by 1e-6", p)]


@pytest.mark.parametrize("n", [33, 257])
def test_every_bound_rejects_a_planted_defect(n):
    rng = np.random.default_rng(n)
    m, _ = CR.mesh(n)
    c = CR.Case(m, n)
    N1, N2 = 3 * n + 3, n + 3
    drop = np.ones(len(m), dtype=bool)
    drop[len(m) // 2] = False
    # -- the linear-solve bound, on stage 2 alone with random rotations
    R0 = np.array([CR.random_rotation(rng) for _ in range(n)])
    L, B = CR.translation_system(m, n, R0)
    x, k2 = CR.solve(L, B)
    bound = CR.solve_bound(N2, k2, x)
    xd, _ = CR.solve(*CR.translation_system(m[drop], n, R0))
    for name, bad in [("an edge dropped", xd)] + defects(x, rng):
        err = float(np.linalg.norm((bad - x).astype(np.float64)))
        print("n = %d, stage 2, %s: %.3g of the bound" % (n, name, err / bound))
        assert err > bound, name
    # -- the rotation bound: the same defects in the stage-1 solution, projected
    blocks, Z, _ = CR.relaxed_rotations(m, n)
    Zd = CR.relaxed_rotations(m[drop], n)[1]
    for name, bad in [("an edge dropped", Zd)] + defects(Z, rng):
        bb = np.concatenate([np.eye(3, dtype=LD)[None], bad.reshape(n - 1, 3, 3).transpose(0, 2, 1)])
        Rb, _ = CR.nearest_rotations(bb)
        worst = c.rotation_ratios(CR.poses(Rb, np.zeros((n, 3))), N1).max()
        print("n = %d, rotations, %s: %.3g of the bound" % (n, name, worst))
        assert worst > 1, name
    # -- the translation bound of the whole initialisation: translations that solve a system with an edge missing, or
    # that carry the defects, at the reference's rotations
    t = CR.translations_of(c.T)
    td = CR.translations(m[drop], n, c.R)[0].astype(np.float64)
    for name, bad in [("an edge dropped", td[1:])] + defects(t[1:], rng):
        Tb = CR.poses(c.R, np.concatenate([np.zeros((1, 3)), bad]))
        assert c.translation_ratio(Tb, N2) > 1, name
    # and the reference passes all of them itself
    assert c.rotation_ratios(c.T, N1).max() <= 1 and c.translation_ratio(c.T, N2) <= 1


SMALL_PLANTS = [(20, 21, 22, (0.9, 1e-6, 1e-7)), (30, 31, 32, (0.9, 0.0, 0.0))]


@pytest.mark.parametrize("n,plants", [(40, SMALL_PLANTS), (150, CR.PLANTS)])
def test_the_unguarded_projection_is_rejected_on_the_planted_blocks(n, plants):
    """A V diag(w^-1/2) V^T in fp64.  On the rank-one block it is non-finite or improper at both orders: the finiteness and
    properness checks reject it.  On the block with singular values (0.9, 1e-6, 1e-7) the eigenvectors of A^T A resolve v2
    and v3 only to u s1^2 / (s2^2 - s3^2) = 1e-4, a hundred times the projection's own term 1024 u s1 / (s2 + s3), at
    both orders.  The whole rotation bound rejects that at the small order (measured 6.2 times the bound at order 123);
    at order 453 its second term, Li's 2 / (s2 + s3) times the stage-1 solve bound N u kappa_2 |Z|_F, is 2e-4 itself, the
    size of the defect (measured 1.1 and 0.45 of the bound on the two such leaves) -- there the figure is printed and
    the rank-one block is what rejects the formula."""
    m, _, where = CR.planted_mesh(n, plants)
    c = CR.Case(m, n, precise=sorted(where))
    Rb = np.array([CR.unguarded_projection(b) for b in c.blocks])
    Tb = CR.poses(np.nan_to_num(Rb, nan=0.0, posinf=0.0, neginf=0.0), np.zeros((n, 3)))
    ratios = c.rotation_ratios(Tb, 3 * n + 3)
    generic = [i for i in range(n) if i not in where]
    assert ratios[generic].max() <= 1  # (on well-conditioned blocks the formula is fine)
    seen = set()
    for leaf, _, _, sigma in plants:
        if sigma == (0.9, 0.0, 0.0):
            assert not np.isfinite(Rb[leaf]).all() or CR.proper(CR.poses(Rb[leaf:leaf + 1], np.zeros((1, 3)))) > 1e-12
            seen.add(sigma)
        if sigma == (0.9, 1e-6, 1e-7):
            s = c.sv[leaf]
            err = np.abs(Rb[leaf] - c.R[leaf]).max()
            print("n = %d, leaf %d: the unguarded projection is off by %.3g, %.3g of the bound" % (n, leaf, err, ratios[leaf]))
            assert err > 10 * 1024 * CR.U * s[0] / (s[1] + s[2]), (leaf, err)
            if n == 40:
                assert ratios[leaf] > 1, (leaf, ratios[leaf])
            seen.add(sigma)
    assert len(seen) == 2

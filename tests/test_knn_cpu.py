"""CPU: the numpy model of the distCUDA2 shell search (tests/knn_ref.py) on the clouds of tests/knn_cases.py.

  * the model equals the f64 brute force on every family, on the grid the product chooses and on forced grids;
  * the PARENT algorithm (one cell count for all axes over the exact bounding box, bound from the nearest face on every
    axis) examines N - 1 candidates per point on flat clouds, coincident clouds and clouds with one far outlier: pinned
    here so that the finding stays on record; the per-axis grid over the quantile box does not;
  * mutants of the model are caught, i.e. the families would notice a search that is subtly wrong:

        mutant            caught by
        no_margin         face_graze (a constructed cloud: natural clouds do not put a point one ulp beyond a face AND a
                          third neighbour one ulp further than it)
        skip_end_cell     uniform, plane, line
        wrong_face        uniform, line, lattice
        self_not_skipped  uniform, duplicates, lattice
        ties_dropped      lattice, duplicates, coincident
"""
import numpy as np
import pytest

import knn_cases as KC
import knn_ref as KR

F = np.float32
CATCHES = {
    "skip_end_cell": ("uniform", "plane", "line"),
    "wrong_face": ("uniform", "line", "lattice"),
    "self_not_skipped": ("uniform", "duplicates", "lattice"),
    "ties_dropped": ("lattice", "duplicates", "coincident"),
}
# f32: three squares, two sums, two more sums and a division, each half an ulp -> well under 1e-6 relative
MODEL_RTOL = 1e-6


def _brute(pts):
    from oracle.gsr_oracle import knn_mean_dist2

    return knn_mean_dist2(pts, "f64", nthreads=4)


def _matches(out, ref):
    if not (np.isinf(out) == np.isinf(ref)).all():
        return False
    fin = np.isfinite(ref)
    return bool(np.allclose(out[fin], ref[fin], rtol=MODEL_RTOL, atol=0.0))


@pytest.mark.parametrize("family", KC.FAMILIES)
def test_model_equals_brute_force(oracle_built, family):
    for N in (1, 3, 4, 5, 255, 256, 257):
        pts = KC.make(family, N)
        ref = _brute(pts)
        for g in (None, 1, 5):
            out, work = KR.search(pts, *KR.product_grid(pts, g))
            assert _matches(out, ref), (family, N, g)
            if g == 1 and (N == 0 or KC.multiplicity(pts).max() < 4):      # one cell and no zero exit: brute force
                assert (work == N - 1).all()
        if N < 4:
            assert np.isinf(out).all()
    pts = KC.make(family, 600)
    assert _matches(KR.search(pts, *KR.parent_grid(pts), algo="parent")[0], _brute(pts))


def test_parent_algorithm_is_quadratic_on_degenerate_clouds_and_the_per_axis_grid_is_not(oracle_built):
    """N = 1500 (parent grid 9 x 9 x 9).  Candidates examined per point, parent algorithm:
    uniform / offset ~45; plane, line, coincident N - 1 = 1499; one outlier N - 2 for every other point; near_plane and
    aniso within a sixth of N - 1.  Per-axis grid over the quantile box: all of them within (125 / 27) W(uniform)."""
    N = 1500
    W, Wp = {}, {}
    for fam in ("uniform", "offset_1e5", "plane", "line", "near_plane", "aniso", "outliers_1", "coincident"):
        pts = KC.make(fam, N)
        ref = _brute(pts)
        bbox, gdim = KR.parent_grid(pts)
        assert gdim == (9, 9, 9)
        out, work = KR.search(pts, bbox, gdim, algo="parent")
        assert _matches(out, ref), fam
        Wp[fam] = work
        out, work = KR.search(pts, *KR.product_grid(pts))
        assert _matches(out, ref), fam
        W[fam] = work
        print(f"{fam}: parent W {Wp[fam].mean():.1f}, per-axis grid W {W[fam].mean():.1f}")
    assert Wp["uniform"].mean() < 60 and Wp["offset_1e5"].mean() < 60
    for fam in ("plane", "line", "coincident"):
        assert (Wp[fam] == N - 1).all(), fam
    assert np.sort(Wp["outliers_1"])[1:].min() == N - 2 and Wp["outliers_1"].mean() > N - 3
    assert Wp["near_plane"].mean() > 5 * (N - 1) / 6 and Wp["aniso"].mean() > 5 * (N - 1) / 6
    cap = KC.WORK_SLACK * W["uniform"].mean()
    for fam in ("offset_1e5", "plane", "line", "near_plane", "aniso", "outliers_1"):
        assert W[fam].mean() <= cap, (fam, W[fam].mean(), cap)
    assert W["coincident"].max() == 3


@pytest.mark.parametrize("mutant", sorted(CATCHES))
def test_mutant_is_caught(oracle_built, mutant):
    for fam in CATCHES[mutant]:
        pts = KC.make(fam, 600)
        ref = _brute(pts)
        grid = KR.product_grid(pts)
        assert _matches(KR.search(pts, *grid)[0], ref), fam
        assert not _matches(KR.search(pts, *grid, mutant=mutant)[0], ref), (mutant, fam)


def face_graze():
    """A cloud on the x axis and a grid (box [0, 0.7], G x 1 x 1) where the margin decides: q lies one ulp ABOVE the computed
    face x * cs yet is binned below it (u * inv_cs rounds under x), p sits 64 ulp above q in cell x, and p's third nearest
    point inside its own cell is one ulp further from p than q is.  Without slack and factor the first shell's bound
    equals that distance and the search stops before it sees q."""
    E = F(0.7)
    for G in range(3, 400):
        cs, ic = E / F(G), F(G) / E
        for x in range(1, G):
            g = F(x) * cs
            uq = np.nextafter(g, F(2))
            if np.trunc(F(uq * ic)) < x:
                ulp = uq - g
                up = F(uq + F(64) * ulp)
                xs = [uq, up, up + F(16) * ulp, up + F(32) * ulp, up + F(65) * ulp, F(0), E]
                pts = np.zeros((len(xs), 3), F)
                pts[:, 0] = xs
                assert np.trunc(F(up * ic)) == x and np.trunc(F(pts[4, 0] * ic)) == x
                return pts, np.array([0, 0, 0, E, 0, 0], F), (G, 1, 1)
    raise AssertionError("no grazing face found")


def test_margin_mutant_is_caught_by_a_grazing_face(oracle_built):
    pts, bbox, gdim = face_graze()
    ref = _brute(pts)
    assert _matches(KR.search(pts, bbox, gdim)[0], ref)
    assert not _matches(KR.search(pts, bbox, gdim, mutant="no_margin")[0], ref)

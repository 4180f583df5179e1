"""Point clouds for the distCUDA2 tests (tests/test_knn_cpu.py, tests/test_gpu_knn.py): what a network predicts early in
training (collapsed, clumped, flattened, a few far outliers) and what breaks a uniform-grid shell search.  Seeded numpy
generators, float32 (N, 3).

  uniform        the baseline: a unit cube at the origin; W(uniform) is the yardstick of the work bound
  offset_1e3/1e4/1e5  the unit cube far from the origin (coordinates keep 2^-14 .. 2^-7 of resolution): a face computed as
                 lo + x * cs rounds to the spacing of lo, p - lo does not
  aniso          extents 100 : 1 : 0.01: one cell count for all axes leaves the thin axis with cells of no thickness
  plane          z = 0 exactly: zero extent, the bound along z is 0 and a search that uses it never stops early
  near_plane     z = 1e-6 * U: the same with a non-zero extent (no special case for ext == 0 helps)
  line           y, z constant: two degenerate axes
  outliers_1/3/10  the unit cube plus 1, 3, 10 points near (1e3, 1e3, 1e3): the exact bounding box puts every other point
                 into one cell
  coincident     every point identical: all distances 0, one cell whatever the grid
  duplicates     every location repeated 1 to 6 times: exact zeros where a point has 3 or more copies of itself elsewhere,
                 and j == i must be skipped by index, not by distance
  lattice        integer lattice: every distance ties (6 neighbours at 1), points sit exactly on cell faces
  clusters       two tight clusters far apart plus exact duplicates and a few far points (the case of
                 test_gpu_surfel.py::test_simple_knn_distcuda2_matches_brute_force): two scales in one grid
"""
import zlib

import numpy as np

OFFSETS = {"offset_1e3": 1e3, "offset_1e4": 1e4, "offset_1e5": 1e5}
OUTLIERS = {"outliers_1": 1, "outliers_3": 3, "outliers_10": 10}
FAMILIES = ("uniform", *OFFSETS, "aniso", "plane", "near_plane", "line", *OUTLIERS, "coincident", "duplicates", "lattice",
            "clusters")
# the families whose work is capped at (125 / 27) W(uniform)
CAPPED = (*OFFSETS, "aniso", "plane", "near_plane", "line", *OUTLIERS)
EDGE_SIZES = (0, 1, 3, 4, 5, 255, 256, 257)
WORK_SLACK = 125.0 / 27.0       # one cubic shell more than the 3 x 3 x 3 block the uniform cloud needs


def make(name, N, seed=0):
    """-> (N, 3) float32."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 7919 * N + seed)
    u = rng.random((N, 3))
    if name == "uniform":
        p = u - 0.5
    elif name in OFFSETS:
        p = u + OFFSETS[name] * np.array([1.0, -1.0, 0.5])
    elif name == "aniso":
        p = u * np.array([100.0, 1.0, 0.01])
    elif name == "plane":
        p = u * np.array([1.0, 1.0, 0.0])
    elif name == "near_plane":
        p = u * np.array([1.0, 1.0, 1e-6])
    elif name == "line":
        p = u * np.array([1.0, 0.0, 0.0]) + np.array([0.0, 0.25, -0.5])
    elif name in OUTLIERS:
        k = min(OUTLIERS[name], N)
        p = u - 0.5
        p[N - k:] = 1e3 + 5.0 * rng.standard_normal((k, 3))
    elif name == "coincident":
        p = np.tile(np.array([0.3, -1.7, 2.5]), (N, 1))
    elif name == "duplicates":
        reps = rng.integers(1, 7, size=N)
        p = np.repeat(u, reps, axis=0)[:N]
    elif name == "lattice":
        n = max(1, int(np.ceil(N ** (1.0 / 3.0) - 1e-9)))
        ijk = np.stack(np.unravel_index(np.arange(N), (n, n, n)), 1)    # the first N sites: full slabs and a partial one
        p = ijk.astype(np.float64)
    elif name == "clusters":
        k = min(5, N // 8)
        na = (N - 2 * k) // 2
        a = 0.01 * rng.standard_normal((na, 3)) + np.array([0.4, 0.4, 0.4])
        b = 0.02 * rng.standard_normal((N - 2 * k - na, 3)) - np.array([0.45, 0.3, 0.1])
        p = np.concatenate([a, b, a[:k], 3.0 * rng.standard_normal((k, 3))])
    else:
        raise KeyError(name)
    p = np.ascontiguousarray(p, dtype=np.float32)
    assert p.shape == (N, 3)
    return p[rng.permutation(N)] if N else p


def multiplicity(pts):
    """(N,) the number of points at exactly each point's location, itself included."""
    if len(pts) == 0:
        return np.zeros(0, np.int64)
    _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)]

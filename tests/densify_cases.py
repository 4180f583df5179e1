"""Case lists of the densification-mask tests (tests/test_densify_cpu.py, tests/test_gpu_densify.py): segment layouts, score
vectors and gate / split shapes.  numpy only; every generator is seeded by its arguments."""
import numpy as np

CHUNK = 1024          # rows per workgroup of the scans (csrc/densify.hip DN_CHUNK) = the sort's tile

# name -> (segment sizes, rows behind offset[-1])
LAYOUTS = {
    "one_row": ([1], 0),
    "empty_middle": ([2, 1, 0, 3], 0),
    "around_256": ([255, 256, 257], 0),
    "around_tile": ([1023, 1024, 1025, 1], 0),
    "empty_ends": ([0, 700, 0], 0),
    "three_samples": ([12000] * 3, 0),
    "tail_rows": ([300, 0, 41], 77),
    "around_chunk": ([CHUNK - 1, 1, CHUNK, CHUNK + 1, 4 * CHUNK + 3], 5),     # segments that start and end on / off a chunk border
}
SMALL_LAYOUTS = [k for k in LAYOUTS if k != "three_samples"]
RATIOS = (0.8, 0.5, 1.0 / 3.0)


def offsets(name):
    """(offset (B,) int64, N)"""
    sizes, tail = LAYOUTS[name]
    off = np.cumsum(np.asarray(sizes, dtype=np.int64))
    return off, int(off[-1]) + tail


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def values(kind, n, seed):
    """float64 scores; the caller rounds them to the dtype under test"""
    rng = np.random.default_rng(seed)
    if kind == "distinct":                       # a permutation of distinct integers (a 16-bit dtype rounds some of them together)
        return rng.permutation(n).astype(np.float64) - n // 3
    if kind == "five":                           # five distinct values only: the tie rule
        return rng.integers(0, 5, size=n).astype(np.float64) * 0.25 - 0.5
    if kind == "sigmoid":                        # what MaskModule scores look like (rounded to bf16 by the caller: heavy ties)
        return sigmoid(rng.standard_normal(n))
    if kind == "special":                        # NaN, +-0, negative numbers, subnormals, infinities
        pool = np.array([np.nan, 0.0, -0.0, -1.5, 2.0, 1e-40, -1e-40, 6e-8, -6e-8, np.inf, -np.inf, 0.333, -7.0, 1e-45])
        return pool[rng.integers(0, pool.size, size=n)]
    if kind == "dyadic":                         # multiples of 2^-16 below 2^-12: every float32 sum of <= 2^20 of them is exact
        return rng.integers(0, 16, size=n).astype(np.float64) / 65536.0
    raise KeyError(kind)


def distinct_in(dtype, n, seed, positive=False):
    """n distinct values that stay distinct in `dtype` ("f32" / "f16" / "bf16"): 8-bit significands times a power of two"""
    rng = np.random.default_rng(seed)
    grid = np.asarray([m * 2.0 ** e for e in range(-4, 5) for m in range(128, 256)])        # 1152 values, exact in bf16
    if not positive:
        grid = np.concatenate([grid, -grid])
    assert n <= grid.size
    return rng.permutation(grid)[:n]


def integers(shape, seed, lo=-8, hi=8):
    """small integers: sums of a few thousand products of them are exact in float32 in every order, and exact in bf16 singly"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


GATE_SHAPES = [(1, 8), (257, 160), (12000, 160), (257, 256), (257, 1024), (12000, 8)]     # (N, C)
MASKS = ("all", "none", "alternating")


def mask_of(kind, n):
    if kind == "all":
        return np.ones(n, dtype=bool)
    if kind == "none":
        return np.zeros(n, dtype=bool)
    if kind == "alternating":
        return np.arange(n) % 2 == 0
    return np.random.default_rng(n).random(n) < 0.7

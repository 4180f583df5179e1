"""Inputs shared by the serialization tests (tests/test_serial_cpu.py, tests/test_gpu_serial.py): the recorded reference
codes, the segment sizes of the patch-table checks, and seeded clouds whose coordinate range differs per axis."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("serial_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "serial_*.npz"))
               if not p.endswith("serial_patch.npz"))
PATCH_SIZES = (1, 4, 48)


def golden(case):
    return np.load(os.path.join(GOLDEN, f"serial_{case}.npz"))


def segment_sizes(P):
    return [0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1]


def cloud(n, depth, seed, segments=1, cells=None, full=False):
    """-> grid (n, 3) int32, batch (n) int64 (sorted).  x spans the full 2^depth, y half, z a quarter (full: all three span
    2^depth); `cells`: draw from that many distinct cells only"""
    rng = np.random.default_rng(seed)
    hi = [max(1, (1 << depth) >> (0 if full else s)) for s in (0, 1, 2)]
    m = n if cells is None else cells
    pool = np.stack([rng.integers(0, h, m) for h in hi], axis=1).astype(np.int32)
    grid = pool if cells is None else pool[rng.integers(0, m, n)]
    batch = np.sort(rng.integers(0, segments, n)).astype(np.int64)
    return grid, batch

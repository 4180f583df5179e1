"""The inputs of the Block junction tests (tests/test_block_cpu.py, tests/test_gpu_block.py): the smallest shapes at which the
mapping of csrc/block.hip can go wrong.  Everything is float64 numpy from seeded draws (never torch's generator); the tests
round it to the dtypes they run in.

  C   8 (one piece), 40 and 160 (idle lanes in the group), 256, 520 (a second piece on one lane)
  N   1, 7, 33 (one more than the backward's 32 rows per workgroup), 70 (three workgroups)
  segments (ada)   B = 3 ends (40, 40, 66) at N = 70: an empty segment, a border inside the second workgroup and rows behind
                   the last end; at smaller N the same pattern scaled
  keep   drawn at 0.7 (zeros and 1 / 0.7), and absent
  forms  the three junctions of the Block — j1: pre = norm, post = norm, no keep; j2: post = norm; j3: no norm — times plain LN,
         LN with weight and bias, and ada; one case with an ada `pre` and an affine `post`

A judged tensor is pooled over `draws(name)` draws so that the smallest one (a (C,) parameter gradient, a one-row y) has at
least 256 elements in all."""
import math

import numpy as np

ROWS_PER_WORKGROUP = 32       # include/gdr.h GDR_NORM_ROWS
EPS = 1e-5

# name -> (C, N, form, norm kind of pre / post, keep drawn)
CASES = {
    "j1_ln_c8_n70": (8, 70, "j1", ("ln", "ln"), False),
    "j1_affine_c40_n33": (40, 33, "j1", ("affine", "affine"), False),
    "j1_ada_c160_n70": (160, 70, "j1", ("ada", "ada"), False),
    "j1_ln_c520_n7": (520, 7, "j1", ("ln", "ln"), False),
    "j2_ln_c256_n7": (256, 7, "j2", (None, "ln"), True),
    "j2_ln_c160_n70_nokeep": (160, 70, "j2", (None, "ln"), False),
    "j2_affine_c520_n33": (520, 33, "j2", (None, "affine"), True),
    "j2_ada_c40_n70": (40, 70, "j2", (None, "ada"), True),
    "j2_ada_c256_n33": (256, 33, "j2", (None, "ada"), False),
    "j3_c8_n1": (8, 1, "j3", (None, None), True),
    "j3_c520_n70": (520, 70, "j3", (None, None), True),
    "j3_c40_n33_nokeep": (40, 33, "j3", (None, None), False),
    "mixed_c160_n70": (160, 70, "j1", ("ada", "affine"), True),
}
DTYPE_CASES = ["j1_affine_c40_n33", "j1_ada_c160_n70", "j2_ln_c256_n7", "j2_ada_c40_n70", "j3_c520_n70", "mixed_c160_n70"]
SEGMENTS = 3


def offsets(n):
    """B = 3 inclusive ends over n rows: the second segment is empty and the last rows lie behind the last end (n >= 7)"""
    if n < 7:
        return np.array([n, n, n], dtype=np.int64)
    a = n * 4 // 7
    return np.array([a, a, n - max(1, n // 17)], dtype=np.int64)


def draws(name):
    c, n, _, kinds, _ = CASES[name]
    smallest = n * c
    if "affine" in kinds:
        smallest = min(smallest, c)
    if "ada" in kinds:
        smallest = min(smallest, SEGMENTS * c)
    return math.ceil(256 / smallest)


def _spec(kind, c, rng):
    if kind is None:
        return None
    if kind == "ln":
        return ("ln", None, None, EPS)
    if kind == "affine":
        return ("ln", 1.0 + 0.3 * rng.standard_normal(c), 0.3 * rng.standard_normal(c), EPS)
    return ("ada", rng.standard_normal((SEGMENTS, c)), EPS)


def inputs(name, draw=0):
    """-> skip, branch, keep or None, pre, post, offset (ends, int64), grad_y, grad_n or None"""
    c, n, _, (pre_kind, post_kind), with_keep = CASES[name]
    rng = np.random.default_rng([sum(map(ord, name)), draw])
    skip = rng.standard_normal((n, c)) * 1.5 + 0.25
    branch = rng.standard_normal((n, c)) * 1.5 - 0.5
    keep = (rng.uniform(size=n) < 0.7) / 0.7 if with_keep else None
    pre, post = _spec(pre_kind, c, rng), _spec(post_kind, c, rng)
    grad_y = rng.standard_normal((n, c))
    grad_n = rng.standard_normal((n, c)) if post is not None else None
    return skip, branch, keep, pre, post, offsets(n), grad_y, grad_n


# ---- the bound forward ----------------------------------------------------------------------------------------------------

def block_point(counts, channels, global_channels=24, seed=0, extent=6):
    """a decoder point of sum(counts) sites in len(counts) segments: feat, global_feat, the segment ends, distinct voxels in an
    extent^3 grid per segment as (N, 4) int32 (batch, c0, c1, c2), and two serialization orders (permutations inside each
    segment, as a serialization gives) -> dict of numpy arrays"""
    rng = np.random.default_rng([seed, len(counts), channels])
    n = int(sum(counts))
    idx, orders = [], [[], []]
    start = 0
    for b, cnt in enumerate(counts):
        cells = rng.choice(extent ** 3, size=cnt, replace=False)
        idx.append(np.stack([np.full(cnt, b), cells // extent ** 2, cells // extent % extent, cells % extent], 1))
        for o in orders:
            o.append(start + rng.permutation(cnt))
        start += cnt
    order = np.stack([np.concatenate(o) for o in orders]).astype(np.int64)
    return {"feat": rng.standard_normal((n, channels)), "global_feat": rng.standard_normal((len(counts), global_channels)),
            "offset": np.cumsum(counts).astype(np.int64), "indices": np.concatenate(idx).astype(np.int32),
            "spatial_shape": (extent, extent, extent), "batch_size": len(counts), "serialized_order": order,
            "serialized_inverse": np.argsort(order, axis=1).astype(np.int64)}

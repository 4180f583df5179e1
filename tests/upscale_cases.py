"""The shapes and inputs the upscale tests share (tests/test_upscale_cpu.py, tests/test_gpu_upscale.py): the smallest at which
the mapping of csrc/upscale.hip can go wrong.  Everything is float64 numpy from seeded draws (never torch's generator); the
tests round it to their dtypes.  `draw` numbers the repeats a test pools its maxima over: enough that the smallest judged tensor
of a case (grad_coord, grad_scale, grad_skip) has 256 elements in all."""
import numpy as np

GRID_SIZE = 0.008

# expand: name -> (N parents, S, C, F, absolute_pe).  C = 8 is one lane's piece; 40 and 160 leave lanes of the group idle; 520
# puts a second piece on one lane; F = 1, 15, 16; S = 3 does not divide the parents of a workgroup, S = 16 fills the 48 LDS
# slots of a group; N = 1, 7, 33 are less than one workgroup at their C, 65 parents of C = 256 are nine workgroups.
EXPAND = {
    "one_parent": (1, 2, 8, 1, False),
    "c40_s3_abs": (7, 3, 40, 15, True),
    "c160_s2": (33, 2, 160, 15, False),
    "c256_s4_abs": (65, 4, 256, 15, True),
    "c520_s16": (7, 16, 520, 16, False),
    "c160_s1_abs": (33, 1, 160, 16, True),
    "c8_s4": (65, 4, 8, 15, False),
}
EXPAND_DTYPE_CASES = ("c160_s2", "c256_s4_abs", "c40_s3_abs")

# merge: name -> (N parents, S, Cout, the parents' segment ends, keep drawn at 0.7 or None).  B = 3 has an empty segment and a
# tail of parents behind the last end; 65 parents are three workgroups of the backward (32 parents each), with a segment
# border inside one.
MERGE = {
    "one_parent": (1, 2, 8, [1], False),
    "c256_s4_b3": (65, 4, 256, [20, 20, 57], True),
    "c8_s3_b3": (33, 3, 8, [10, 10, 30], True),
    "c256_s16": (7, 16, 256, [7], False),
    "c8_s1": (65, 1, 8, [65], True),
    "c256_s2": (33, 2, 256, [33], True),
    "c264_s3": (7, 3, 264, [3, 7], True),
}
MERGE_DTYPE_CASES = ("c256_s4_b3", "c8_s3_b3", "c256_s2")


def expand_draws(name):
    return -(-256 // (3 * EXPAND[name][0]))


def merge_draws(name):
    n, _, c, offset, _ = MERGE[name]
    return -(-256 // (min(n, len(offset)) * c))


def expand_inputs(name, draw=0, frequencies=None):
    """(t, coord, feat, frequencies, S, absolute_pe, grad_out_x, grad_h) in float64.  t is what delta_x returns (a few units
    wide, so tanh is neither linear nor saturated); the PE arguments reach 2^(F - 1) * 0.004."""
    n, s, c, f, absolute = EXPAND[name]
    rng = np.random.default_rng(len(name) * 29 + n + 1009 * draw)
    t = rng.standard_normal((n, 3 * s)) * 1.5
    coord = rng.uniform(-0.5, 0.5, (n, 3))
    feat = rng.standard_normal((n, c)) * 1.5 + 0.25
    freq = 2.0 ** np.arange(f, dtype=np.float64) if frequencies is None else np.asarray(frequencies, dtype=np.float64)
    grad_x = rng.standard_normal((n * s, 3))
    grad_h = rng.standard_normal((n * s, 6 * len(freq) + c))
    return t, coord, feat, freq, s, absolute, grad_x, grad_h


def merge_inputs(name, draw=0):
    """(skip, branch, keep, scale, offset, S, grad_out) in float64; keep is 0 or 1 / 0.7 per row, or None"""
    n, s, c, offset, has_keep = MERGE[name]
    rng = np.random.default_rng(len(name) * 31 + n + 1013 * draw)
    skip = rng.standard_normal((n, c)) * 1.5 + 0.25
    branch = rng.standard_normal((n * s, c))
    keep = (rng.uniform(size=n * s) < 0.7) / 0.7 if has_keep else None
    scale = rng.standard_normal((len(offset), c))
    grad = rng.standard_normal((n * s, c))
    return skip, branch, keep, scale, np.asarray(offset, dtype=np.int64), s, grad


def module_inputs(n, c, b, global_channels=24, seed=0):
    """(coord, feat, global_feat, offset) in float64 for a point of n parents in b equal segments"""
    rng = np.random.default_rng(seed * 7 + n)
    offset = np.asarray([n * (i + 1) // b for i in range(b)], dtype=np.int64)
    return rng.uniform(-0.5, 0.5, (n, 3)), rng.standard_normal((n, c)), rng.standard_normal((b, global_channels)), offset

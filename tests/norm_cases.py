"""The shapes and inputs the norm tests share (tests/test_norm_cpu.py, tests/test_gpu_norm.py): the smallest at which the
mapping of csrc/norm.hip can go wrong.  Everything is float64 numpy from seeded draws; the tests round it to their dtypes."""
import numpy as np


def many_ends(n, b, seed):
    """b non-decreasing segment ends in [0, n] that include repeats (empty segments), the last one below n"""
    rng = np.random.default_rng(seed)
    ends = np.sort(rng.integers(0, n - 20, size=b))
    ends[3] = ends[2]
    return ends.astype(np.int64)


# A: name -> (N, C, offset).  One row and one lane; one piece per lane; three segments with an empty one and a border inside a
# workgroup's 32 rows; C / 8 = 33 (64 lanes per row, 31 of them idle); C = 1024 (two full pieces per lane); a tail behind the
# last end; 1024 segments on 1500 rows; a segment over 157 workgroups next to a one-row segment; and, beside the issue's list,
# C / 8 = 97 (a second piece on lanes 0..32 only).
ADA = {
    "one_row": (1, 8, [1]),
    "c160": (65, 160, [65]),
    "empty_segment": (257, 256, [100, 100, 257]),
    "one_row_segments_c264": (130, 264, [1, 2, 130]),
    "c1024": (70, 1024, [70]),
    "tail": (300, 160, [120, 257]),
    "b1024": (1500, 8, many_ends(1500, 1024, 5).tolist()),
    "long_segment": (5000, 160, [4999, 5000]),
    "c776": (40, 776, [17, 40]),
}
ADA_DTYPE_CASES = ("c160", "empty_segment", "tail")      # the three shapes every dtype combination runs at

# B: name -> (P, S, C, F, frequency base)
PE = {
    "one_parent": (1, 2, 8, 1, 2.0),
    "c160": (33, 2, 160, 15, 2.0),
    "c256_s4": (37, 4, 256, 15, 2.0),
    "f16_base1.5": (5, 3, 16, 16, 1.5),
    "many_groups": (2100, 4, 160, 15, 2.0),
}
PE_DTYPE_CASES = ("c160", "c256_s4", "f16_base1.5")


def ada_inputs(name, constant_row=None):
    """(feat, scale, offset, grad_out) in float64; `constant_row`: that row of feat holds one value (zero variance)"""
    n, c, offset = ADA[name]
    rng = np.random.default_rng(len(name) * 131 + n)
    feat = rng.standard_normal((n, c)) * 1.5 + 0.25
    if constant_row is not None:
        feat[constant_row] = 0.75
    scale = rng.standard_normal((len(offset), c))
    grad = rng.standard_normal((n, c))
    return feat, scale, np.asarray(offset, dtype=np.int64), grad


def pe_inputs(name):
    """(x, feat, frequencies, S, grad_out) in float64.  x is what the reference forms: 0.5 * grid_size * tanh(.) with
    grid_size = 0.008, so the arguments of sin / cos reach base^(F - 1) * 0.004 (64 at the reference's 2^14)."""
    p, s, c, f, base = PE[name]
    rng = np.random.default_rng(len(name) * 17 + p)
    x = 0.004 * np.tanh(rng.standard_normal((p * s, 3)) * 2.0)
    feat = rng.standard_normal((p, c)) * 1.5 + 0.25
    freq = base ** np.arange(f, dtype=np.float64)
    grad = rng.standard_normal((p * s, 6 * f + c))
    return x, feat, freq, s, grad

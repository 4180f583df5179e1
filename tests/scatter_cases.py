"""Shapes for the segment-reduction tests: the smallest pointer arrays at which csrc/segment.hip takes each of its paths.
R is the kernel's row run (generativedensification_amd.segment.ROWS): a segment inside one run is finished there, one that
crosses a run border goes through the partials and the fold.  Every layout has N <= 4 R + 64 rows."""
import numpy as np

CHANNELS = (1, 3, 7, 8, 160, 256 + 8)     # scalar path (1, 3, 7), one 16-byte vector, the decoder's width, more than one tile
C_MAX = max(CHANNELS)
DECODER = (12_000, 160)


def _ptr(lengths, first=0):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)


def layouts(R):
    """{name: (N, indptr)}; indptr is non-decreasing and within [0, N] in every layout"""
    cyc = []
    while sum(cyc) + sum((1, 2, 7, 0, 0, R + 3)) <= 4 * R + 64:
        cyc += [1, 2, 7, 0, 0, R + 3]
    out = {
        "n0": (0, _ptr([0, 0, 0])),
        "s0": (5, np.zeros(1, dtype=np.int64)),
        "one_Rm1": (R - 1, _ptr([R - 1])),
        "one_R": (R, _ptr([R])),
        "one_Rp1": (R + 1, _ptr([R + 1])),
        "one_3Rp1": (3 * R + 1, _ptr([3 * R + 1])),
        "ones": (2 * R + 3, _ptr([1] * (2 * R + 3))),
        "cycle": (sum(cyc), _ptr(cyc)),
        "empties": (2 * R + 9, _ptr([0, 0, 5, 0, R + 1, 0, 0, 0, R - 2, 5, 0, 0])),
        "inner": (3 * R + 20, _ptr([3, R + 4, 0, R - 1, 2], first=7)),      # indptr[0] = 7 > 0, indptr[-1] = 2 R + 15 < N
    }
    for name, (n, p) in out.items():
        assert n <= 4 * R + 64 and (np.diff(p) >= 0).all() and p[0] >= 0 and p[-1] <= n, name
    return out


def integers(shape, seed):
    """small integers in [-8, 8]: sums of a few hundred of them are exact in float32 in every order"""
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float64)


def sizes_b3():
    return [700, 1, 1347]       # B = 3 with unequal sizes

"""The case table and the seeded inputs of the convolution tests (tests/test_conv3d_cpu.py, tests/test_gpu_conv3d.py).

Cases are (B, Cin, Cout, D, H, W).  The last two are derived from the voxel tile of the product kernel,
GDR_CONV3D_BRICK_D x _H x _W = 4 x 4 x 8 (include/gdr.h): one volume is exactly one brick, one exceeds it by a voxel per axis.

    unit       only the centre tap may contribute
    line       two degenerate axes
    seam       batch seam and row wrap on the smallest volume that has them
    odd        no axis a multiple of any brick; Cin != Cout
    c40        channel counts that are multiples of neither the chunk (16 / 32) nor the tile (64 / 128)
    wide_out   a full channel tile plus a remainder
    wide_in    many chunks plus a remainder
    ref_width  the reference width; the long sum
    brick      one brick of 4 x 4 x 8 voxels along each axis, exactly
    brick_plus the brick plus one voxel along each axis: 2 x 2 x 2 bricks, seven of them nearly empty
"""
import numpy as np

BRICK = (4, 4, 8)
CASES = {
    "unit": (1, 8, 8, 1, 1, 1),
    "line": (1, 8, 8, 1, 1, 5),
    "seam": (2, 8, 8, 2, 2, 2),
    "odd": (2, 16, 24, 3, 5, 7),
    "c40": (1, 40, 40, 4, 4, 4),
    "wide_out": (1, 8, 136, 3, 3, 3),
    "wide_in": (1, 264, 8, 3, 3, 3),
    "ref_width": (1, 256, 256, 4, 4, 4),
    "brick": (1, 8, 8) + BRICK,
    "brick_plus": (1, 8, 8) + tuple(n + 1 for n in BRICK),
}
SECOND_ITEM = 1000.0      # the second batch item of x and of grad_out is this many times the first
# the two items' scales: x 0.02 and 20, grad_out 0.01 and 10.  Their products, summed over a case's voxels into grad_weight,
# stay near 3e3 (4.5 sigma: 1.4e4), inside float16's range; both items stay far above its subnormals
X_ITEMS, G_ITEMS = (0.02, 0.02 * SECOND_ITEM), (0.01, 0.01 * SECOND_ITEM)


def inputs(name):
    """(x (B, Cin, D, H, W), weight (Cout, Cin, 3, 3, 3), bias (Cout,), grad_out (B, Cout, D, H, W)) in float64.  Nothing is
    symmetric, the faces carry values as large as the interior (plain normals with an offset), and in a two-item case the
    second item is SECOND_ITEM times the first, so that a bleed across the batch seam lands far above any rounding."""
    B, cin, cout, D, H, W = CASES[name]
    rng = np.random.default_rng([22, B, cin, cout, D, H, W])
    x = rng.standard_normal((B, cin, D, H, W)) * 1.5 + 0.3
    g = rng.standard_normal((B, cout, D, H, W)) - 0.2
    if B > 1:
        for b in range(2):
            x[b] *= X_ITEMS[b]
            g[b] *= G_ITEMS[b]
    weight = rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27.0 * cin) + 0.01
    bias = rng.standard_normal(cout) * 0.5
    return x, weight, bias, g

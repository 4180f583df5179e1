"""The case table and the seeded inputs of the transposed-convolution tests (tests/test_deconv3d_cpu.py,
tests/test_gpu_deconv3d.py).

Cases are (B, Cin, Cout, D, H, W) of the parent volume.  Two are derived from constants the module exports: TILE_ROWS, the
parent rows of one workgroup of the forward, and GRAD_WEIGHT_SLAB_ROWS, the parent rows per slab of the weight gradient
(include/gdr.h GDR_DECONV3D_TILE_ROWS and GDR_DECONV3D_SLAB_MIN).

    one       smallest everything
    odd       two items, odd axes; Cin a multiple of neither 16 nor 32; Cout below one MFMA tile
    ref_slim  the reference's channel counts: 5 channel tiles
    wide      Cin beyond one K chunk with a remainder (and the 16-row form of the input gradient); Cout crosses a 128 tile
    mid       Cin between 256 and 512: the 32-row form of the input gradient
    run       a full tile of parent rows plus a partial one
    slabs     one parent row past a slab boundary of the weight gradient: two slabs, and the fold
    flat      one row constant (variance 0, finite through eps) and one row 1000 times the others
"""
import numpy as np

TILE_ROWS = 64
SLAB_ROWS = 4096
CASES = {
    "one": (1, 8, 8, 1, 1, 1),
    "odd": (2, 24, 8, 3, 5, 7),
    "ref_slim": (1, 256, 80, 4, 4, 4),
    "wide": (1, 520, 136, 2, 2, 3),
    "mid": (1, 264, 8, 1, 2, 3),
    "run": (1, 8, 8, 1, 1, TILE_ROWS + 3),
    "slabs": (1, 16, 16, 1, 17, (SLAB_ROWS + 1) // 17),
    "flat": (1, 32, 16, 2, 2, 2),
}
assert 17 * ((SLAB_ROWS + 1) // 17) == SLAB_ROWS + 1
EPS = 1e-6                # the reference's
FLAT_ROW, BIG_ROW, BIG = (0, 0, 0), (1, 1, 1), 1000.0       # of `flat`: the constant voxel, the large one and its factor


def inputs(name):
    """(x (B, Cin, D, H, W), weight (Cin, Cout, 2, 2, 2), bias (Cout,), ln_weight (Cin,), ln_bias (Cin,),
    grad_out (B, Cout, 2D, 2H, 2W)) in float64.  Nothing is symmetric: plain normals with offsets."""
    B, cin, cout, D, H, W = CASES[name]
    rng = np.random.default_rng([23, B, cin, cout, D, H, W])
    x = rng.standard_normal((B, cin, D, H, W)) * 1.5 + 0.3
    g = rng.standard_normal((B, cout, 2 * D, 2 * H, 2 * W)) - 0.2
    weight = rng.standard_normal((cin, cout, 2, 2, 2)) / np.sqrt(cin) + 0.01
    bias = rng.standard_normal(cout) * 0.5
    ln_weight = 1.0 + 0.3 * rng.standard_normal(cin)
    ln_bias = 0.2 * rng.standard_normal(cin)
    if name == "flat":
        x[(0, slice(None)) + FLAT_ROW] = 0.75
        x[(0, slice(None)) + BIG_ROW] *= BIG
    return x, weight, bias, ln_weight, ln_bias, g

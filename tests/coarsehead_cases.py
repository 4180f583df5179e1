"""The case table and the seeded inputs of the coarse-head tests (tests/test_coarsehead_cpu.py, tests/test_gpu_coarsehead.py).

Cases are ((B, N), C, K, sh_dim).  Two are derived from constants the module exports: TILE_ROWS, the rows of one workgroup of
the forward, and SLAB_MIN, the rows per slab of the parameter gradients (include/gdr.h GDR_COARSEHEAD_TILE_ROWS and
GDR_COARSEHEAD_SLAB_MIN).

    one       smallest everything.  With one row an output has 1 to 4 elements, and whether torch's rounding of the last layer to
              16 bits adds to or cancels the rounding of its hidden rows is a coin flip per element, which a maximum over so
              few elements does not average out.  So x and the parameters of `one` are small multiples of 1/2 .. 1/8 and a row
              is kept only if both hidden rows are exact in bfloat16: every sum is then exact in every dtype, the kernel's
              outputs must be right to the one float32 rounding, and torch's error is its own output rounding.
    ref_slim  the reference's channel counts: C not a multiple of 32, 23 output columns not a multiple of 16
    k2        46 columns; column % P across K; two batch items with group_centers indexed by row % N
    wide      C past 128 with a remainder; 35 columns
    run       a full tile plus a partial one
    slabs     two slabs of the parameter gradients, and the fold
    sat       last-layer offsets of +-40: the sigmoid saturates, its gradient is exactly zero or denormal

The ReLU gates decide what a gradient test means, so `inputs` settles them here, on the CPU.  With the parameters fixed and
already rounded to `dtype`, the rows of x are rejection-sampled: a row is kept only if every one of its 2 C pre-activations
satisfies |z| >= 8 e, e the worst-case bound
    e1 = (|x| |W1|^T + |b1|) C 2^-23
    e2 = (2^-8 |h1| + e1) |W2|^T + (|h1| |W2|^T + |b2|) C 2^-23        (2^-8: the bf16 rounding of the hidden row; kept for f16)
so float64, torch's 16-bit composition and the kernel all gate every unit of every row alike.  A row is also kept only if its
opacities stay MASK_MARGIN[dtype] away from the mask's threshold, so the float64 mask is the mask.  `inputs` then asserts that
the gates computed with the hidden row rounded to `dtype` equal the float64 gates, that each hidden layer has units that are on
in some rows and off in others (it prints the share), that sigmoid(opacity) falls on both sides of the threshold (cases with
at least 4 elements) and that no element is left out of the mask comparison.  The parameters hold values of `dtype`, so a
test that stores them as float32 (autocast's pair) hands the kernels parameters their rounding does not change."""
import functools

import numpy as np
import torch

import coarsehead_ref as R

TILE_ROWS = 64
SLAB_MIN = 1024
CASES = {
    "one": ((1, 1), 8, 1, 3),
    "ref_slim": ((1, 67), 80, 1, 12),
    "k2": ((2, 20), 24, 2, 12),
    "wide": ((1, 19), 136, 1, 27),
    "run": ((1, TILE_ROWS + 3), 8, 1, 12),
    "slabs": ((1, SLAB_MIN + 1), 8, 1, 12),
    "sat": ((1, 16), 16, 1, 12),
}
OPACITY_SHIFT, SCALING_SHIFT = -2.1792, -4.3        # the reference's opacity shift; a scaling shift of its order
HALF_CELL, THRESHOLD = 0.0078125 * 1.7, 0.005
LOGIT_THRESHOLD = float(np.log(THRESHOLD / (1.0 - THRESHOLD)))
# how far (in opacity) a kept row stays from the threshold: beyond twice the 16-bit rounding of an opacity of magnitude 8
MASK_MARGIN = {torch.float32: 1e-4, torch.bfloat16: 0.0625, torch.float16: 0.0625}
SAT = 40.0
BATCH = 1 << 15


def rounded(a, dtype):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dtype).double().numpy()


def _bounds(x, w1, b1, w2, b2):
    C = x.shape[-1]
    u = C * 2.0 ** -23
    z1, h1, z2, _ = R.hidden(x, w1, b1, w2, b2)
    e1 = (np.abs(x) @ np.abs(w1).T + np.abs(b1)) * u
    e2 = (2.0 ** -8 * np.abs(h1) + e1) @ np.abs(w2).T + (np.abs(h1) @ np.abs(w2).T + np.abs(b2)) * u
    return z1, z2, e1, e2


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """dict of float64 arrays holding values of `dtype` (x, the six parameters) or of float32 (the upstream gradients
    g_offset, g_sh, g_scaling, g_rotation, g_opacity, g_centers and group_centers (N, 3)).  Read-only: shared by the tests."""
    (B, N), C, K, sh_dim = CASES[name]
    P, rows = sh_dim + 11, B * N
    rng = np.random.default_rng([41, B, N, C, K, sh_dim])
    wide, exact = C > 128, name == "one"
    op_cols = [k * P + 3 + sh_dim for k in range(K)]
    if exact:
        grid = lambda shape, step, top: rng.integers(-top, top + 1, shape) * step      # noqa: E731
        p = {"w1": grid((C, C), 0.5, 2), "b1": grid(C, 0.25, 4), "w2": grid((C, C), 1.0, 1), "b2": grid(C, 0.25, 4),
             "w3": grid((K * P, C), 0.125, 8), "b3": grid(K * P, 0.125, 8)}
        p["b3"][op_cols] = -3.0
        draw = lambda n: grid((n, C), 0.5, 2)      # noqa: E731
    else:
        wscale, bscale = (0.4, 1.0) if wide else (1.0, 0.3)       # a wider bias spread where the acceptance would be slow
        p = {"w1": wscale * rng.standard_normal((C, C)) / np.sqrt(C) + 0.01, "b1": bscale * rng.standard_normal(C),
             "w2": wscale * rng.standard_normal((C, C)) / np.sqrt(C) + 0.01, "b2": bscale * rng.standard_normal(C),
             "w3": rng.standard_normal((K * P, C)) / np.sqrt(C) + 0.01, "b3": 0.3 * rng.standard_normal(K * P)}
        p["w3"][op_cols] *= 3.0                                    # a wide spread of opacities around the threshold
        draw = lambda n: rounded(rng.standard_normal((n, C)) * 1.5 + 0.3, dtype)      # noqa: E731
        p = {k: rounded(v, dtype) for k, v in p.items()}
        # the opacity bias puts the median raw opacity at the threshold (about -3.1 before the shift)
        pilot = R.hidden(draw(4096), p["w1"], p["b1"], p["w2"], p["b2"])[3]
        p["b3"][op_cols] = LOGIT_THRESHOLD - OPACITY_SHIFT - np.median(pilot @ p["w3"][op_cols].T, axis=0)
    if name == "sat":
        p["b3"][0:3] = (SAT, -SAT, SAT)
        p["w3"][0:3] *= 0.01
    p = {k: rounded(v, dtype) for k, v in p.items()}
    kept, draws = [], 0
    while sum(len(k) for k in kept) < rows:
        x = draw(BATCH)
        draws += BATCH
        z1, z2, e1, e2 = _bounds(x, p["w1"], p["b1"], p["w2"], p["b2"])
        ok = (np.abs(z1) >= 8 * e1).all(1) & (np.abs(z2) >= 8 * e2).all(1)
        op = np.maximum(z2, 0.0) @ p["w3"][op_cols].T + p["b3"][op_cols] + OPACITY_SHIFT
        ok &= (np.abs(op - LOGIT_THRESHOLD) > 4 * MASK_MARGIN[dtype]).all(1)
        if exact:
            ok &= (rounded(z1, torch.bfloat16) == z1).all(1) & (rounded(z2, torch.bfloat16) == z2).all(1)
        kept.append(x[ok])
    x = np.concatenate(kept)[:rows]
    print(f"coarsehead-cases {name}/{dtype}: {rows} rows kept of about {draws} draws")
    z1, z2, e1, e2 = _bounds(x, p["w1"], p["b1"], p["w2"], p["b2"])
    # the gates of the composition whose hidden rows are rounded to `dtype` are the float64 gates, unit by unit
    z1r = rounded(z1, dtype)
    z2r = rounded(np.maximum(z1r, 0.0) @ p["w2"].T + p["b2"], dtype)
    assert ((z1r > 0) == (z1 > 0)).all() and ((z2r > 0) == (z2 > 0)).all(), name
    if rows > 1:
        for layer, z in (("1", z1), ("2", z2)):
            on = (z > 0).sum(0)
            switching = float(((on > 0) & (on < rows)).mean())
            print(f"coarsehead-cases {name}/{dtype}: layer {layer} units that switch across rows: {switching:.0%}")
            assert switching > 0, (name, layer)
    d = dict(p)
    d["x"] = x.reshape(B, N, C)
    g = np.random.default_rng([43, B, N, C, K, sh_dim])
    f32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    E = N * K
    for key, shape in (("g_offset", (B, E, 3)), ("g_sh", (B, E, sh_dim // 3, 3)), ("g_scaling", (B, E, 3)), ("g_rotation", (B, E, 4)),
                       ("g_opacity", (B, E, 1)), ("g_centers", (B, E, 3))):
        d[key] = f32(g.standard_normal(shape) - 0.2)
    d["group_centers"] = f32(g.uniform(-0.5, 0.5, (N, 3)))
    ref = R.head(d["x"], *(d[k] for k in R.PARAMS), K, sh_dim, OPACITY_SHIFT, SCALING_SHIFT, d["group_centers"], HALF_CELL, THRESHOLD)
    if B * E >= 4:
        assert ref["mask"].any() and not ref["mask"].all(), name
    left_out = np.abs(ref["opacity"][..., 0] - LOGIT_THRESHOLD) <= MASK_MARGIN[dtype]
    assert left_out.sum() <= 0.01 * left_out.size, name
    if name == "sat":
        assert (np.abs(np.abs((np.maximum(z2, 0) @ p["w3"][0:3].T + p["b3"][0:3])) - SAT) < 2.0).all()
    for a in d.values():
        a.setflags(write=False)
    return d


def shape_of(name):
    (B, N), C, K, sh_dim = CASES[name]
    return B, N, C, K, sh_dim

"""The case tables and the seeded inputs of the fine-head tests (tests/test_finehead_cpu.py, tests/test_gpu_finehead.py).

The head.  A shape is (rows, C, sh_dim).  C runs over 8, 40, 160, 256 (the smallest, one that is no multiple of 16 or 32, one past
128 with a remainder of the 16-bit sum chunk, the largest), sh_dim over 3, 12, 48 (P = 11, 20, 56: below one tile, the base
config's, the widest) and the rows over the smallest counts that cross each boundary of the kernels: 17 (one partial tile), one more
than the forward's row tile, one more than the backward's step for every compute dtype (64, 32 or 16 rows: what fits LDS at this C,
asked of the library), one more than one slab of the parameter gradients.  GELU has no gates to settle, so the inputs are plain
seeded draws; x and the parameters hold values of `dtype`, so a test that stores the parameters as float32 (autocast's pair) hands
the kernels parameters their rounding does not change.

A tensor with few elements makes the accuracy bar a coin flip: whether torch's 16-bit roundings add up or cancel on the one worst
element is luck that a maximum over 8 or 11 elements (grad_b1 at C = 8, grad_b2 at sh_dim = 3) does not average out (DESIGN §24
records the trap).  So a case is `repeats(C, sh_dim)` draws of (x, g) on the same parameters, and the bar is taken over the results of
all of them together: every tensor under it then has at least MIN_ELEMENTS elements.

The assembly.  A case is (level rows, Nc, how `mask` is drawn, how `selected` is drawn, sh_dim)."""
import functools

import numpy as np
import torch

TILE_ROWS = 64
SLAB_MIN = 512
SCAN_CHUNK = 1024
MIN_ELEMENTS = 256
HEAD_C = (8, 40, 160, 256)
HEAD_SH = (3, 12, 48)
OPACITY_SHIFT, SCALING_SHIFT = -2.1792, -4.3        # the reference's opacity shift; a scaling shift of its order


def rounded(a, dtype):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dtype).double().numpy()


def repeats(C, sh_dim):
    """draws per case: enough that grad_b1 (C elements) and grad_b2 (P) reach MIN_ELEMENTS together over all draws"""
    return -(-MIN_ELEMENTS // min(C, sh_dim + 8))


def head_rows(C, sh_dim, steps):
    """the row counts of a (C, sh_dim): `steps` are the backward's steps of the compute dtypes at this shape"""
    return sorted({17, TILE_ROWS + 1, SLAB_MIN + 1} | {s + 1 for s in steps})


def head_shapes(step_of):
    """every (rows, C, sh_dim); step_of(dtype, C, sh_dim) is generativedensification_amd.finehead.backward_step"""
    return [(rows, C, sh) for C in HEAD_C for sh in HEAD_SH
            for rows in head_rows(C, sh, [step_of(dt, C, sh) for dt in (torch.float32, torch.bfloat16, torch.float16)])]


@functools.lru_cache(maxsize=None)
def head_params(C, sh_dim, dtype):
    """float64 arrays holding values of `dtype`: w1 (C, C), b1 (C), w2 (P, C), b2 (P).  Read-only: shared by the tests."""
    P = sh_dim + 8
    rng = np.random.default_rng([47, C, sh_dim])
    p = {"w1": rng.standard_normal((C, C)) / np.sqrt(C) + 0.01, "b1": 0.3 * rng.standard_normal(C),
         "w2": rng.standard_normal((P, C)) / np.sqrt(C) + 0.01, "b2": 0.3 * rng.standard_normal(P)}
    p = {k: rounded(v, dtype) for k, v in p.items()}
    for a in p.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def head_draw(rows, C, sh_dim, dtype, rep):
    """draw `rep` of a case: x (rows, C) of values of `dtype`, and g (rows, P) of values of float32"""
    rng = np.random.default_rng([53, rows, C, sh_dim, rep])
    x = rounded(rng.standard_normal((rows, C)) * 1.5 + 0.3, dtype)
    g = (rng.standard_normal((rows, sh_dim + 8)) - 0.2).astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


# (level rows, Nc, mask, selected, sh_dim); a mask is "random", "all" or "none"
ASSEMBLY = {
    "one_level": ((5,), 37, "random", "random", 12),
    "two_levels": ((7, 13), 101, "random", "random", 3),
    "zero_row_level": ((6, 0, 9), 50, "random", "random", 12),
    "no_survivors": ((5, 3), 41, "random", "all", 12),
    "all_survive": ((3,), 43, "random", "none", 48),
    "mask_all": ((2, 5), 19, "all", "random", 12),
    "no_levels": ((), 23, "random", "random", 3),
    "chunks": ((1025, 2),2 * SCAN_CHUNK + 3, "dense", "random", 12),      # more than one scan chunk on both sides
}


@functools.lru_cache(maxsize=None)
def assembly_inputs(name, attr_dtype):
    """dict of numpy arrays: per level coord (float32) and attribute (float32 holding values of attr_dtype), the coarse tensors,
    shs_fine, the two masks, and upstream gradients (float32) of the five outputs.  Read-only: shared by the tests."""
    level_rows, Nc, how_mask, how_sel, sh_dim = ASSEMBLY[name]
    rng = np.random.default_rng([59, Nc, sh_dim, len(level_rows)])
    f32 = lambda shape: rng.standard_normal(shape).astype(np.float32)      # noqa: E731
    draw = {"random": lambda n: rng.random(n) < 0.5, "dense": lambda n: rng.random(n) < 0.8, "all": lambda n: np.ones(n, bool),
            "none": lambda n: np.zeros(n, bool)}
    mask = draw[how_mask](Nc)
    n_masked = int(mask.sum())
    selected = draw[how_sel](n_masked)
    d = {"levels": [(f32((n, 3)), rounded(f32((n, sh_dim + 8)), attr_dtype).astype(np.float32)) for n in level_rows],
         "coarse": [f32((Nc, w)) for w in (3, 1, 3, 4)], "shs_fine": f32((n_masked, sh_dim // 3, 3)), "mask": mask, "selected": selected}
    T = sum(level_rows) + int((~selected).sum())
    d["grads"] = {"centers": f32((T, 3)), "shs": f32((T, sh_dim // 3, 3)), "opacity": f32((T, 1)), "scaling": f32((T, 3)), "rotation": f32((T, 4))}
    if name not in ("no_survivors", "no_levels", "all_survive", "mask_all"):
        assert 0 < (~selected).sum() < n_masked < Nc, name
    return d

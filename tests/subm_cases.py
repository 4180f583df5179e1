"""The small shapes at which the submanifold convolution can go wrong (tests/test_subm_cpu.py, tests/test_gpu_subm.py).
Every case: indices (N, 4) int32, spatial_shape, batch_size, ksize, Cin -> Cout, asymmetric random weight, non-zero bias, a
random upstream gradient; `dense_ok` = every site inside the grid and alone in its voxel (the dense truth applies);
`slice_of` > 0 = the features are handed over as columns [off, off + Cin) of an (N, slice_of) tensor."""
import functools

import numpy as np


class Case:
    def __init__(self, name, indices, shape, batch, ksize, cin, cout, dense_ok=True, slice_of=0, slice_off=0, seed=0):
        self.name, self.shape, self.batch, self.ksize, self.cin, self.cout = name, tuple(shape), batch, tuple(ksize), cin, cout
        self.indices = np.asarray(indices, dtype=np.int32).reshape(-1, 4)
        self.dense_ok, self.slice_of, self.slice_off = dense_ok, slice_of, slice_off
        rng = np.random.default_rng(1000 + seed)
        N, K = self.indices.shape[0], ksize[0] * ksize[1] * ksize[2]
        self.N, self.K = N, K
        self.feat = rng.standard_normal((N, cin))
        self.weight = rng.standard_normal((cout,) + self.ksize + (cin,)) / np.sqrt(K * cin)
        self.bias = rng.standard_normal(cout) * 0.5 + 0.25
        self.grad_out = rng.standard_normal((N, cout))

    def __repr__(self):
        return self.name


def _distinct(rng, n, shape, batch=1):
    """n distinct (batch, c0, c1, c2) rows, in random order"""
    total = batch * shape[0] * shape[1] * shape[2]
    lin = rng.choice(total, size=n, replace=False)
    b, r = np.divmod(lin, shape[0] * shape[1] * shape[2])
    c0, r = np.divmod(r, shape[1] * shape[2])
    c1, c2 = np.divmod(r, shape[2])
    return np.stack([b, c0, c1, c2], 1)


def _faces(shape):
    """sites on every face and corner of the grid (coordinates 0 and S - 1) plus the centre"""
    pts = set()
    for a in (0, shape[0] - 1):
        for b in (0, shape[1] - 1):
            for c in (0, shape[2] - 1):
                pts.add((0, a, b, c))
    m = tuple(s // 2 for s in shape)
    for d in range(3):
        for v in (0, shape[d] - 1):
            q = list(m)
            q[d] = v
            pts.add((0,) + tuple(q))
            q2 = list(q)
            q2[(d + 1) % 3] = min(q2[(d + 1) % 3] + 1, shape[(d + 1) % 3] - 1)
            pts.add((0,) + tuple(q2))
    pts.add((0,) + m)
    return np.array(sorted(pts))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(7)
    out = []
    k3, k5, k135 = (3, 3, 3), (5, 5, 5), (1, 3, 5)
    out.append(Case("n0", np.zeros((0, 4)), (8, 8, 8), 1, k3, 16, 32, seed=0))
    out.append(Case("n1", [[0, 3, 4, 5]], (8, 8, 8), 1, k3, 16, 32, seed=1))
    out.append(Case("n63", _distinct(rng, 63, (5, 5, 5)), (5, 5, 5), 1, k3, 16, 32, seed=2))
    out.append(Case("n64_k5", _distinct(rng, 64, (6, 5, 4)), (6, 5, 4), 1, k5, 16, 32, seed=3))
    out.append(Case("n65_c40", _distinct(rng, 65, (5, 5, 5)), (5, 5, 5), 1, k3, 40, 24, seed=4))
    out.append(Case("n1500", _distinct(rng, 1500, (24, 20, 16), 2), (24, 20, 16), 2, k3, 16, 32, seed=5))
    out.append(Case("faces_k135", _faces((7, 9, 11)), (7, 9, 11), 1, k135, 40, 24, seed=6))
    out.append(Case("faces_k5", _faces((6, 6, 6)), (6, 6, 6), 1, k5, 16, 32, seed=7))
    same = _distinct(rng, 90, (5, 5, 5))
    two = np.concatenate([same, same + np.array([1, 0, 0, 0])])
    out.append(Case("two_batches", two[rng.permutation(180)], (5, 5, 5), 2, k3, 16, 32, seed=8))
    iso = np.array([[0, a, b, c] for a in range(0, 24, 3) for b in range(0, 24, 3) for c in range(0, 24, 6)])
    out.append(Case("isolated", iso[rng.permutation(len(iso))], (24, 24, 24), 1, k3, 16, 32, seed=9))
    full = np.array([[0, a + 1, b, c + 2] for a in range(6) for b in range(6) for c in range(6)])
    out.append(Case("full_block_c160", full[rng.permutation(216)], (8, 6, 9), 1, k3, 160, 160, seed=10))
    out.append(Case("full_block_k135", full[rng.permutation(216)], (8, 6, 9), 1, k135, 16, 32, seed=11))
    out.append(Case("slice", _distinct(rng, 130, (6, 6, 6)), (6, 6, 6), 1, k3, 40, 24, slice_of=64, slice_off=8, seed=12))
    out.append(Case("slice_unaligned", _distinct(rng, 70, (5, 5, 5)), (5, 5, 5), 1, k3, 16, 32, slice_of=27, slice_off=3, seed=13))
    # shared voxels: runs of 2 and 5 among single sites, and one run of the whole cloud
    base = _distinct(rng, 100, (6, 6, 6))
    shared = np.concatenate([base, base[:10], base[20:23], base[20:23], base[20:23], base[20:23]])
    out.append(Case("shared_2_5", shared[rng.permutation(len(shared))], (6, 6, 6), 1, k3, 16, 32, dense_ok=False, seed=14))
    out.append(Case("shared_2_5_c40", shared[rng.permutation(len(shared))], (6, 6, 6), 1, k3, 40, 24, dense_ok=False, seed=15))
    out.append(Case("shared_all", np.tile([[0, 2, 3, 1]], (70, 1)), (4, 4, 4), 1, k3, 16, 32, dense_ok=False, seed=16))
    # one site outside the grid (coordinate = S), one with batch = batch_size, one negative, next to real neighbours
    oor = np.concatenate([_distinct(rng, 60, (5, 5, 5)), [[0, 5, 2, 2], [1, 2, 2, 2], [0, 2, -1, 2]]])
    out.append(Case("out_of_range", oor[rng.permutation(len(oor))], (5, 5, 5), 1, k3, 16, 32, dense_ok=False, seed=17))
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)

"""Authoring only: python tests/golden/make_volcond_rsh.py REFERENCE_TREE writes tests/golden/volcond_rsh.npz, 64 seeded float64
vectors (unit, non-unit, axis-aligned, zero) and what the reference's own rsh_cart_3 (tools/rsh.py) returns for them on the
CPU.  The tests read the .npz and never the reference."""
import importlib.util
import os
import sys

import numpy as np
import torch


def vectors():
    rng = np.random.default_rng(20261)
    unit = rng.standard_normal((24, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    free = rng.standard_normal((24, 3)) * rng.uniform(0.05, 3.0, (24, 1))
    axes = np.concatenate([np.eye(3), -np.eye(3), 2.5 * np.eye(3), -0.3 * np.eye(3)])
    diag = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, -1.0], [1.0, 1.0, 1.0]]) / np.sqrt([[2.0], [2.0], [3.0]])
    return np.concatenate([unit, free, axes, diag, np.zeros((1, 3))])


def main(tree):
    spec = importlib.util.spec_from_file_location("reference_rsh", os.path.join(tree, "tools", "rsh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    v = vectors()
    assert v.shape == (64, 3)
    y = mod.rsh_cart_3(torch.from_numpy(v)).numpy()
    assert y.shape == (64, 16) and y.dtype == np.float64
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "volcond_rsh.npz"), vectors=v, rsh=y)


if __name__ == "__main__":
    main(sys.argv[1])

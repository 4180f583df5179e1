"""Child process of tests/test_gpu_knn.py::test_work_is_bounded: `python knn_work.py N` measures the candidates the
distCUDA2 search examines per point on every family of knn_cases.py at N points and prints one JSON line.  It runs in
a process of its own so that the parent can end a search that has gone quadratic instead of waiting for it."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import knn_cases as KC  # noqa: E402
from generativedensification_amd import knn  # noqa: E402


def cells_of(pts, bbox, gdim):
    """The cell id of every point in float32, as csrc/knn.hip bins them."""
    F = np.float32
    G = gdim.astype(np.int64)
    lo = bbox[:3].astype(F)
    ext = np.maximum(bbox[3:].astype(F) - lo, F(1e-20))
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.nan_to_num((pts - lo) * (G.astype(F) / ext), nan=0.0, posinf=3e9, neginf=-3e9)
    c = np.clip(np.trunc(t).astype(np.int64), 0, G - 1)
    return (c[:, 2] * G[1] + c[:, 1]) * G[0] + c[:, 0]


def measure(N, families=KC.FAMILIES, dev="cuda:0"):
    res = {}
    for fam in families:
        pts = KC.make(fam, N)
        t = torch.from_numpy(pts).to(dev)
        out, work = knn.dist2(t, return_work=True)
        bbox, gdim, _ = knn.grid(t)
        work, bbox, gdim = work.cpu().numpy().astype(np.int64), bbox.cpu().numpy(), gdim.cpu().numpy()
        cid = cells_of(pts, bbox, gdim)
        pop = np.bincount(cid)[cid]
        zero = KC.multiplicity(pts) >= 4          # three other points at distance 0
        res[fam] = dict(W=float(work.mean()), max=int(work.max()), gdim=[int(g) for g in gdim],
                        zero_points=int(zero.sum()), zero_over_cell=int((work[zero] > pop[zero]).sum()),
                        W_zero=float(work[zero].mean()) if zero.any() else 0.0,
                        pop_zero=float(pop[zero].mean()) if zero.any() else 0.0,
                        out_zero_wrong=int((out.cpu().numpy()[zero] != 0).sum()))
    return res


if __name__ == "__main__":
    print("KNN_WORK " + json.dumps(measure(int(sys.argv[1]))), flush=True)

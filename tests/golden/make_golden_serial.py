#!/usr/bin/env python
"""tests/golden/make_golden_serial.py — generates tests/golden/serial_*.npz, the codes of the reference's point
serialization (lightning/point_decoder/utils/serialization: encode under the four orders, and the Hilbert decode).

Runs only where a checkout of the reference sits next to this repository (or at $GD_REFERENCE_ROOT).  The serialization
package is pure torch and is loaded by path, on the CPU; it cannot be reached through `lightning.point_decoder`, whose
__init__ imports torch_scatter.  Every file holds grid_coord (N, 3) int32, batch (N) int64, depth, code_z, code_z_trans,
code_hilbert, code_hilbert_trans (N int64, with the batch bits) and decode_grid (N, 3) / decode_batch (N): the reference's
decode of code_hilbert.  (The reference's z decode cannot be recorded: default.py z_order_decode unpacks four values into
three and raises.)  Coordinate ranges differ per axis — x over the full 2^depth, y over half, z over a quarter — so a
swapped axis or a -trans row equal to its plain row cannot pass.  For N = 1 the reference's Hilbert encoder returns a 0-d
tensor; the files record shape (1,).

serial_patch.npz: SerializedAttention.get_padding_and_inverse (lightning/point_decoder/autoencoder.py) for segment sizes
0, 1, P-1, P, P+1, 2P, 2P+1 at P = 1, 4, 48, if autoencoder.py imports with stand-ins for the packages it does not need
for that method (spconv, torch_scatter, timm, torch_geometric, pytorch_lightning, addict, flash_attn and its sibling
modules); the script says whether that worked and writes no file if it did not.
Usage: python tests/golden/make_golden_serial.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GD_REFERENCE_ROOT",
                     os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
PD = os.path.join(REF, "lightning", "point_decoder")


def _load_package(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ser = _load_package("gd_ref_serialization", os.path.join(PD, "utils", "serialization"))


def cloud(n, depth, seed, sizes=None, same_cell=False):
    g = torch.Generator().manual_seed(seed)
    hi = [max(1, (1 << depth) >> s) for s in (0, 1, 2)]
    grid = torch.stack([torch.randint(0, h, (n,), generator=g) for h in hi], dim=1).int()
    if n:
        grid[0] = torch.tensor([hi[0] - 1, hi[1] - 1, hi[2] - 1])      # the corner: every axis reaches its top bit
    if same_cell:
        grid[:] = grid[0]
    batch = torch.zeros(n, dtype=torch.long) if sizes is None else torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return grid, batch


def record(name, grid, batch, depth):
    out = {"grid_coord": grid.numpy().astype(np.int32), "batch": batch.numpy().astype(np.int64), "depth": np.int64(depth)}
    for order in ("z", "z-trans", "hilbert", "hilbert-trans"):
        code = ser.encode(grid, batch, depth, order=order).reshape(-1)
        assert code.dtype == torch.int64 and code.shape == (grid.shape[0],)
        out["code_" + order.replace("-", "_")] = code.numpy()
    dg, db = ser.decode(torch.from_numpy(out["code_hilbert"]), depth, order="hilbert")
    out["decode_grid"] = dg.reshape(-1, 3).numpy().astype(np.int64)
    out["decode_batch"] = db.reshape(-1).numpy().astype(np.int64)
    path = os.path.join(HERE, f"serial_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: N={grid.shape[0]} depth={depth} {os.path.getsize(path)} bytes")


def patch_goldens():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            pass

    class _Dict(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    stub("spconv")
    stub("spconv.pytorch")
    stub("torch_scatter")
    stub("timm")
    stub("timm.models")
    stub("timm.models.layers", DropPath=_Any)
    stub("torch_geometric")
    stub("torch_geometric.utils", cumsum=None, scatter=None, softmax=None)
    stub("pytorch_lightning", LightningModule=torch.nn.Module)
    stub("addict", Dict=_Dict)
    stub("flash_attn")
    pkg = stub("gd_ref_pd")
    pkg.__path__ = [PD]
    stub("gd_ref_pd.point_prompt_training", PDNorm=_Any)
    stub("gd_ref_pd.utils").__path__ = [os.path.join(PD, "utils")]
    sys.modules["gd_ref_pd.utils.serialization"] = ser
    stub("gd_ref_pd.utils.structure", Point=_Dict)
    stub("gd_ref_pd.utils.modules", PointModule=torch.nn.Module, PointSequential=torch.nn.Sequential)
    stub("gd_ref_pd.layers")
    stub("gd_ref_pd.layers.normalization", AdaLayerNorm=_Any)
    spec = importlib.util.spec_from_file_location("gd_ref_pd.autoencoder", os.path.join(PD, "autoencoder.py"))
    ae = importlib.util.module_from_spec(spec)
    sys.modules["gd_ref_pd.autoencoder"] = ae
    spec.loader.exec_module(ae)
    out = {}
    for P in (1, 4, 48):
        sizes = [0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1]
        offset = torch.cumsum(torch.tensor(sizes), 0).long()
        point = _Dict(offset=offset)
        me = types.SimpleNamespace(patch_size=P)
        pad, unpad, cu = ae.SerializedAttention.get_padding_and_inverse(me, point)
        out[f"offset_{P}"] = offset.numpy()
        out[f"pad_{P}"] = pad.numpy().astype(np.int64)
        out[f"unpad_{P}"] = unpad.numpy().astype(np.int64)
        out[f"cu_seqlens_{P}"] = cu.numpy().astype(np.int32)
    path = os.path.join(HERE, "serial_patch.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


def main():
    record("n1", *cloud(1, 5, 1), 5)
    record("n2_same_cell", *cloud(2, 6, 2, same_cell=True), 6)
    for n in (63, 64, 65):
        record(f"n{n}", *cloud(n, 6, 10 + n), 6)
    for depth in (1, 2, 8, 9, 16):
        record(f"d{depth}", *cloud(257, depth, 100 + depth), depth)
    for depth in (7, 16):
        sizes = [40, 0, 90]
        record(f"b3_d{depth}", *cloud(sum(sizes), depth, 200 + depth, sizes=sizes), depth)
    try:
        patch_goldens()
    except Exception as exc:  # noqa: BLE001 — any import or call failure means: the specification is the yardstick
        print(f"serial_patch.npz NOT written: autoencoder.py did not load with stand-ins ({type(exc).__name__}: {exc})")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""tests/golden/make_golden_meshpath.py — generates tests/golden/mesh_path_*.npz, the cameras of the reference's mesh
extraction (tools/gen_video_path.py uni_mesh_path, 16 azimuths x elevations 0, -30, +30).

Runs only where a checkout of the reference sits next to this repository (or at $GD_REFERENCE_ROOT): it imports the
reference's own camera code, which is not part of this repository.  Stand-ins are
injected for what the camera path does not use: `sklearn.cluster` (imported by dataLoader/utils.py), `jaxtyping` and
`tools.camera_utils` (the 'unposed' pose interpolation), and the `dataLoader` package (its utils.py is loaded by file).
Per camera it records world_view_transform, full_proj_transform, camera_center, FoVx / FoVy and get_rays() at 16 x 16, for
both families with and without `sample` / `fov`, and once at 22 x 14 with fovx = 1.1, fovy = 0.45.  Usage: python tests/golden/make_golden_meshpath.py
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


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub("sklearn")
_stub("sklearn.cluster", KMeans=None)
_stub("jaxtyping", Float=None, Int=None, Shaped=None)
pkg = _stub("dataLoader")
pkg.__path__ = []
spec = importlib.util.spec_from_file_location("dataLoader.utils", os.path.join(REF, "dataLoader", "utils.py"))
utils = importlib.util.module_from_spec(spec)
sys.modules["dataLoader.utils"] = utils
spec.loader.exec_module(utils)
pkg.utils = utils
sys.path.insert(0, REF)
import tools  # noqa: E402  (reference package)

_stub("tools.camera_utils", get_interpolated_poses_many=None)
tools.camera_utils = sys.modules["tools.camera_utils"]
from tools.gen_video_path import uni_mesh_path  # noqa: E402  (reference code)

SIZE = (16, 16)


def transform(seed):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    T = torch.eye(4)
    T[:3, :3] = q.float()
    T[:3, 3] = 0.1 * torch.randn(3, generator=g)
    return T


def record(name, dataset_name, sample, fov, size=SIZE, prefix="mesh_path_"):
    data = types.SimpleNamespace(dataset_name=dataset_name, img_size=list(size))
    cams = uni_mesh_path(16, data, sample, fov)
    out = dict(dataset_name=dataset_name, img_size=np.array(size), n=16)
    if sample is not None:
        out["transform_mats"] = sample["transform_mats"].numpy()
    if fov is not None:
        out["fov"] = fov.numpy()
    for key, fn in (("world_view_transform", lambda c: c.world_view_transform),
                    ("full_proj_transform", lambda c: c.full_proj_transform), ("camera_center", lambda c: c.camera_center),
                    ("fov_xy", lambda c: torch.tensor([float(c.FoVx), float(c.FoVy)])),
                    ("rays", lambda c: c.get_rays()[0])):
        out[key] = np.stack([fn(c).detach().cpu().numpy() for c in cams]).astype(np.float32)
    path = os.path.join(HERE, f"{prefix}{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.basename(path)}: {len(cams)} cameras, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    fov = torch.tensor([0.61, 0.66])
    record("gobjeverse", "gobjeverse", None, None)
    record("gso_sample_fov", "GSO", {"transform_mats": transform(1)[None, None]}, fov)
    record("instant3d", "instant3d", None, None)
    record("mvgen_sample_fov", "mvgen", {"transform_mats": transform(2)[None, None]}, fov)
    record("co3d_fov", "co3d", None, fov)
    # fovx and fovy far apart on a non-square image (width 22, height 14): an x / y mix-up shows in the projection and the rays
    # (cameras only: its own prefix keeps it out of the mesh-fusion tests that take every mesh_path_*.npz)
    record("instant3d_fovxy", "instant3d", None, torch.tensor([1.1, 0.45]), size=(22, 14), prefix="pathcam_")

#!/usr/bin/env python
"""Mesh extraction at the reference's evaluation setting (evaluation.py cfg.infer.save_mesh -> MeshExtractor.extract): 48 orbit
views of 512^2 rendered from a Gaussian shell of N points, fused into the TSDF volume (voxel = radius / 256 of the AABB of
configs/infer.yaml x 1.1), marching cubes, crop, cluster filter, .obj written.  Prints one JSON line:
  phase_ms          device time of each phase of one warm extraction (render / integrate / mc / post; MeshExtractor.phase_ms)
  blocks, voxel_visits, voxel_updates   allocated blocks; voxel x view pairs the integration kernel walks; updates applied
  integrate_kernel  tsdf_integrate_kernel alone (re-run in place: it writes every voxel from zero), its byte model (voxel
                    planes written once + 8 B of depth / colour gathered per visit) and the share of the HBM peak (8 TB/s)
  numpy_ref_s       the numpy restatement (tests/tsdf_ref.py) on an analytic sphere at a size where it finishes, as context
usage: python scripts/mesh_bench.py [--n 200000] [--size 512] [--renderer 3dgs|2dgs] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
INFER_AABB = [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]


def shell(n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    bump = 0.04 * torch.sin(9.0 * d[:, :1]) * torch.cos(7.0 * d[:, 1:2])
    centers = d * (0.3 + bump)
    shs = 0.3 * torch.randn(n, 1, 3, generator=g)
    opacity = torch.full((n, 1), 4.0)
    scales = torch.full((n, 3), math.log(0.008))
    rotations = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    return [t.to(dev) for t in (centers, shs, opacity, scales, rotations)] + [None]


def numpy_reference_seconds(size=128, n_az=16):
    import tsdf_ref as R
    from generativedensification_amd.camera import mesh_path_cameras

    views = []
    for cam in mesh_path_cameras(n_az, {"dataset_name": "gobjeverse", "img_size": (size, size)}):
        f = size / (2 * math.tan(cam.FoVx / 2))
        d = R.sphere_depth(cam.view_world_transform.double().numpy(), f, f, size / 2, size / 2, size, size, 0.3)
        views.append(R.make_view(d, np.full((size, size, 3), 0.5, np.float32), f, f, size / 2, size / 2,
                                 cam.world_view_transform.T.numpy(), 10.0))
    voxel = 0.008
    t0 = time.perf_counter()
    blocks, mask, T, Wt, Cc = R.fuse(views, voxel, 2 * voxel)
    t1 = time.perf_counter()
    v, f, c = R.extract(blocks, T, Wt, Cc, voxel)
    t2 = time.perf_counter()
    return {"views": len(views), "size": size, "voxel": voxel, "blocks": int(len(blocks)), "fuse_s": round(t1 - t0, 3),
            "mc_s": round(t2 - t1, 3), "triangles": int(len(f))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--renderer", choices=("3dgs", "2dgs"), default="3dgs")
    ap.add_argument("--reps", type=int, default=20, help="re-runs of the integration kernel alone")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench.py measures on the GPU only")
    from generativedensification_amd import _lib as L
    from generativedensification_amd.mesh import MeshExtractor

    dev = torch.device("cuda:0")
    params = shell(args.n, dev)
    if args.renderer == "3dgs":
        from generativedensification_amd.renderer import Renderer
    else:
        from generativedensification_amd.renderer_2dgs import Renderer
        params[3] = params[3][:, :2].contiguous()
    ex = MeshExtractor(params, Renderer(sh_degree=0, white_background=True), aabb=INFER_AABB)
    data = {"dataset_name": "gobjeverse", "img_size": (args.size, args.size)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mesh.obj")
        ex.extract(path, data, device=dev)                    # warm-up: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = ex.extract(path, data, device=dev)
        wall = time.perf_counter() - t0
    vol = ex.volume
    nb = int(len(vol.blocks))
    words = vol.block_views.cpu().numpy().view(np.uint32)
    visits = int(sum(bin(int(w)).count("1") for w in words.reshape(-1))) * L.GDR_TSDF_R ** 3
    updates = int(vol.weight.double().sum().item())
    # the integration kernel alone, re-run in place (same output)
    lib = L.load()
    a = vol._a
    depth, rgb = torch.stack(vol._depth), torch.stack(vol._rgb)
    views = torch.from_numpy(np.stack(vol._views)).to(dev)
    cell_mask = vol._cell_mask
    before = vol._vol.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def run():
        L.check(lib.gdr_tsdf_integrate(C.byref(a), p(views), p(depth), p(rgb), p(cell_mask), p(vol._cell_block),
                                       p(vol._blocks4), p(vol._vol), st), "gdr_tsdf_integrate")
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        run()
    e1.record()
    e1.synchronize()
    k_ms = e0.elapsed_time(e1) / args.reps
    same = bool(torch.equal(before, vol._vol))
    bytes_model = nb * L.GDR_TSDF_R ** 3 * 5 * 4 + visits * 8
    line = {
        "workload": "mesh_extract", "renderer": args.renderer, "n": args.n, "views": len(vol._views), "size": args.size,
        "voxel": vol.voxel_length, "phase_ms": {k: round(v, 3) for k, v in ex.phase_ms.items()},
        "wall_s": round(wall, 3), "blocks": nb, "voxel_visits": visits, "voxel_updates": updates,
        "vertices": int(len(mesh.vertices)), "triangles": int(len(mesh.triangles)),
        "integrate_kernel": {"ms": round(k_ms, 4), "bytes_model": bytes_model,
                             "GBps": round(bytes_model / (k_ms * 1e-3) / 1e9, 1),
                             "hbm_share": round(bytes_model / (k_ms * 1e-3) / HBM_PEAK, 4),
                             "rerun_bitwise_equal": same},
    }
    if not args.no_numpy:
        line["numpy_ref"] = numpy_reference_seconds()
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

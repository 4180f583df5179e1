"""TSDF fusion and marching-cubes mesh extraction on the MI355X (csrc/tsdf.hip, include/gdr.h gdr_tsdf_*): the GPU path of
the reference's `tools/meshExtractor.py` (`cfg.infer.save_mesh` in evaluation.py), which needs Open3D's ScalableTSDFVolume.
The semantics (Open3D's published algorithm, restated; parity with Open3D unpinned) are in the header of csrc/tsdf.hip and in
tests/tsdf_ref.py.

  TSDFVolume              integrate(depth, rgb, fx, fy, cx, cy, extrinsic, depth_trunc) stages a view; extract_triangle_mesh()
                          fuses every staged view into a block-sparse volume and runs marching cubes -> TriangleMesh on the device
  crop_to_aabb, cluster_connected_triangles, keep_largest_clusters, remove_unreferenced_vertices, write_mesh (.obj / .ply)
  MeshExtractor           the reference's MeshExtractor: 48 orbit views rendered, fused, extracted, cropped, filtered, written

Deviations from the reference: an empty mesh is written as an empty file (the reference's cluster filter would raise on it);
MeshExtractor applies the Gaussian mask to all five inputs (the reference masks opacity, scale and rotation only, which fails a
shape check for any partial mask).  There is no CPU path: CUDA (ROCm) tensors only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import _marshal as M
from .camera import mesh_path_cameras

__all__ = ["TriangleMesh", "TSDFVolume", "mesh_path_cameras", "crop_to_aabb", "cluster_connected_triangles", "keep_cluster_mask",
           "keep_largest_clusters", "remove_unreferenced_vertices", "write_mesh", "read_mesh", "MeshExtractor"]


class TriangleMesh(NamedTuple):
    vertices: torch.Tensor        # (V, 3) float32
    triangles: torch.Tensor       # (F, 3) int32
    vertex_colors: torch.Tensor   # (V, 3) float32 in [0, 1]


def _empty_mesh(device) -> TriangleMesh:
    return TriangleMesh(torch.zeros(0, 3, dtype=torch.float32, device=device),
                        torch.zeros(0, 3, dtype=torch.int32, device=device),
                        torch.zeros(0, 3, dtype=torch.float32, device=device))


class TSDFVolume:
    """Block-sparse TSDF volume (Open3D ScalableTSDFVolume, RGB8 colour) fused on the GPU.

    Blocks of `block_resolution`^3 voxels (16 only) are allocated where the views' depth lands (pixels sampled every
    `depth_sampling_stride`).  `max_blocks` bounds the allocated blocks (80 KiB each) and `max_cells` the dense block-index
    grid over their bounding box: past either, extraction raises instead of failing an allocation.  After
    extract_triangle_mesh() the fused volume stays readable: `blocks` (nb, 3) block coordinates in (bz, by, bx) order,
    `block_views` (nb, words) int32 view masks, `tsdf`, `weight` (nb, R^3) and `color` (nb, R^3, 3) in 0..255."""

    def __init__(self, voxel_length, sdf_trunc, block_resolution=16, depth_sampling_stride=4, device="cuda",
                 max_blocks=1 << 16, max_cells=1 << 26):
        if block_resolution != L.GDR_TSDF_R:
            raise ValueError(f"TSDFVolume: block_resolution must be {L.GDR_TSDF_R} (the HIP kernels' block size)")
        if not (voxel_length > 0 and sdf_trunc > 0 and int(depth_sampling_stride) >= 1):
            raise ValueError("TSDFVolume: voxel_length, sdf_trunc and depth_sampling_stride must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume runs on ROCm/HIP devices only (no CPU fallback)")
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        self.stride = int(depth_sampling_stride)
        self.max_blocks, self.max_cells = int(max_blocks), int(max_cells)
        self._depth, self._rgb, self._views = [], [], []
        self.blocks = self.block_views = self.tsdf = self.weight = self.color = None

    # ---- staging ----
    def integrate(self, depth, rgb, fx, fy, cx, cy, extrinsic, depth_trunc):
        """Stage one view: depth (H, W) or (H, W, 1) float32, rgb (H, W, 3) float32 in [0, 1] or uint8, both on this
        device and read through their strides; pinhole intrinsics; extrinsic = 4x4 world-to-camera (any device)."""
        for name, t in (("depth", depth), ("rgb", rgb)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"TSDFVolume.integrate: {name} must be a ROCm/HIP tensor (no CPU fallback)")
        if depth.dtype != torch.float32 or rgb.dtype not in (torch.float32, torch.uint8):
            raise ValueError("TSDFVolume.integrate: depth must be float32 and rgb float32 or uint8")
        if depth.dim() == 3 and depth.shape[2] == 1:
            depth = depth[..., 0]
        if depth.dim() != 2 or rgb.dim() != 3 or rgb.shape[2] != 3 or tuple(rgb.shape[:2]) != tuple(depth.shape):
            raise ValueError(f"TSDFVolume.integrate: depth (H, W[, 1]) and rgb (H, W, 3) expected, got "
                             f"{tuple(depth.shape)} and {tuple(rgb.shape)}")
        H, W = depth.shape
        if self._depth and tuple(self._depth[0].shape) != (H, W):
            raise ValueError("TSDFVolume.integrate: every view must have the same size")
        E = (extrinsic.detach().cpu().double().numpy() if torch.is_tensor(extrinsic)
             else np.asarray(extrinsic, dtype=np.float64)).reshape(4, 4)
        c2w = np.linalg.inv(E).astype(np.float32)
        rec = np.zeros(28, np.float32)
        rec[:4] = np.array([fx, fy, cx, cy], np.float32)
        rec[4:16] = E.astype(np.float32)[:3].reshape(-1)
        rec[16:28] = c2w[:3].reshape(-1)
        d_out = torch.empty(H, W, dtype=torch.float32, device=depth.device)
        c_out = torch.empty(H, W, dtype=torch.int32, device=depth.device)
        lib = L.load()
        with torch.cuda.device(depth.device):
            L.check(lib.gdr_tsdf_stage(H, W, M.ptr(depth), M.strides(depth), M.ptr(rgb),
                                       M.strides(rgb), int(rgb.dtype == torch.uint8), float(depth_trunc),
                                       M.ptr(d_out), M.ptr(c_out), M.stream()), "gdr_tsdf_stage")
        self._depth.append(d_out)
        self._rgb.append(c_out)
        self._views.append(rec)

    # ---- fusion ----
    def _args(self):
        a = L.GdrTsdfArgs()
        a.V = len(self._views)
        a.H, a.W = self._depth[0].shape
        a.stride, a.words = self.stride, (a.V + 31) // 32
        a.voxel, a.trunc = self.voxel_length, self.sdf_trunc
        return a

    def fuse(self):
        """Allocate and integrate every staged view.  Returns the number of allocated blocks.  Synchronises twice with the
        host (the block bounding box and the block count size the next buffers)."""
        if not self._views:
            raise RuntimeError("TSDFVolume: no view was integrated")
        lib, dev = L.load(), self._depth[0].device
        a = self._args()
        with torch.cuda.device(dev):
            st = M.stream()
            depth, rgb = torch.stack(self._depth), torch.stack(self._rgb)
            views = torch.from_numpy(np.stack(self._views)).to(dev)
            bbox = torch.empty(6, dtype=torch.int32, device=dev)
            L.check(lib.gdr_tsdf_bounds(C.byref(a), M.ptr(views), M.ptr(depth), M.ptr(bbox), st), "gdr_tsdf_bounds")
            bb = bbox.cpu().tolist()
            if bb[0] > bb[3]:   # no depth at all
                self._set_empty(dev, a.words)
                return 0
            dims = [bb[3 + i] - bb[i] + 1 for i in range(3)]
            cells = dims[0] * dims[1] * dims[2]
            if cells > self.max_cells:
                raise RuntimeError(f"TSDFVolume: the touched blocks span a {dims[0]}x{dims[1]}x{dims[2]} block grid "
                                   f"({cells} cells) > max_cells={self.max_cells}; raise max_cells, a coarser voxel or a "
                                   "smaller depth_trunc")
            for i in range(3):
                a.lo[i], a.dims[i] = bb[i], dims[i]
            cell_mask = torch.empty(cells * a.words, dtype=torch.int32, device=dev)
            cell_block = torch.empty(cells, dtype=torch.int32, device=dev)
            cell_scan = torch.empty(cells + 1, dtype=torch.int32, device=dev)
            scratch = torch.empty(int(lib.gdr_tsdf_scan_bytes(cells)), dtype=torch.uint8, device=dev)
            L.check(lib.gdr_tsdf_allocate(C.byref(a), M.ptr(views), M.ptr(depth), M.ptr(cell_mask), M.ptr(cell_block),
                                          M.ptr(cell_scan), M.ptr(scratch), st), "gdr_tsdf_allocate")
            nb = int(cell_scan[cells].item())
            if nb > self.max_blocks:
                raise RuntimeError(f"TSDFVolume: {nb} blocks touched > max_blocks={self.max_blocks} "
                                   f"({nb * 5 * 16 ** 3 * 4 / 2 ** 30:.1f} GiB of voxels); raise max_blocks or use a "
                                   "coarser voxel")
            a.n_blocks = nb
            blocks = torch.empty(nb, 4, dtype=torch.int32, device=dev)
            vol = torch.empty(5, nb, L.GDR_TSDF_R ** 3, dtype=torch.float32, device=dev)
            L.check(lib.gdr_tsdf_integrate(C.byref(a), M.ptr(views), M.ptr(depth), M.ptr(rgb), M.ptr(cell_mask),
                                           M.ptr(cell_block), M.ptr(blocks), M.ptr(vol), st), "gdr_tsdf_integrate")
        self._a, self._cell_mask, self._cell_block, self._blocks4, self._vol = a, cell_mask, cell_block, blocks, vol
        self.blocks = blocks[:, :3]
        self.block_views = cell_mask.view(cells, a.words)[blocks[:, 3].long()]
        self.tsdf, self.weight, self.color = vol[0], vol[1], vol[2:].permute(1, 2, 0)
        return nb

    def _set_empty(self, dev, words):
        self._a = None
        self.blocks = torch.zeros(0, 3, dtype=torch.int32, device=dev)
        self.block_views = torch.zeros(0, words, dtype=torch.int32, device=dev)
        self.tsdf = self.weight = torch.zeros(0, L.GDR_TSDF_R ** 3, device=dev)
        self.color = torch.zeros(0, L.GDR_TSDF_R ** 3, 3, device=dev)

    def marching_cubes(self) -> TriangleMesh:
        """Marching cubes over the fused volume (fuse() first).  Synchronises once with the host: the vertex and triangle
        totals size the outputs."""
        a = self._a
        dev = self._depth[0].device
        if a is None:
            return _empty_mesh(dev)
        lib = L.load()
        n = a.n_blocks * L.GDR_TSDF_R ** 3
        with torch.cuda.device(dev):
            st = M.stream()
            cube_case = torch.empty(n, dtype=torch.int16, device=dev)
            vflags = torch.empty(n, dtype=torch.uint8, device=dev)
            vcount = torch.empty(n + 1, dtype=torch.int32, device=dev)
            tcount = torch.empty(n + 1, dtype=torch.int32, device=dev)
            scratch = torch.empty(int(lib.gdr_tsdf_scan_bytes(n)), dtype=torch.uint8, device=dev)
            args = (C.byref(a), M.ptr(self._cell_block), M.ptr(self._blocks4), M.ptr(self._vol))
            L.check(lib.gdr_tsdf_mc_count(*args, M.ptr(cube_case), M.ptr(vflags), M.ptr(vcount), M.ptr(tcount),
                                          M.ptr(scratch), st), "gdr_tsdf_mc_count")
            nv, nf = torch.stack([vcount[n], tcount[n]]).cpu().tolist()
            verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
            cols = torch.empty(nv, 3, dtype=torch.float32, device=dev)
            tris = torch.empty(nf, 3, dtype=torch.int32, device=dev)
            L.check(lib.gdr_tsdf_mc_emit(*args, M.ptr(cube_case), M.ptr(vflags), M.ptr(vcount), M.ptr(tcount),
                                         M.ptr(verts) if nv else None, M.ptr(cols) if nv else None, M.ptr(tris) if nf else None,
                                         st), "gdr_tsdf_mc_emit")
        return TriangleMesh(verts, tris, cols)

    def extract_triangle_mesh(self) -> TriangleMesh:
        self.fuse()
        return self.marching_cubes()


# ---- post-processing ----------------------------------------------------------------------------------------------------
def crop_to_aabb(mesh: TriangleMesh, aabb) -> TriangleMesh:
    """Drop every triangle with a vertex outside the box [aabb[0], aabb[1]] (compared in float64).  Vertices are kept; any
    device (plain tensor indexing)."""
    box = torch.as_tensor(np.asarray(aabb, dtype=np.float64).reshape(2, 3), device=mesh.vertices.device)
    v = mesh.vertices.double()
    outside = ~((v >= box[0]).all(-1) & (v <= box[1]).all(-1))
    drop = outside[mesh.triangles.long()].any(-1) if len(mesh.triangles) else torch.zeros(0, dtype=torch.bool,
                                                                                         device=v.device)
    return TriangleMesh(mesh.vertices, mesh.triangles[~drop], mesh.vertex_colors)


def cluster_connected_triangles(mesh: TriangleMesh):
    """(labels (F,) int32, counts (K,) int32): triangles sharing an edge form one cluster; clusters are numbered by their
    smallest triangle index.  Edge keys sorted with torch, union-find in HIP (gdr_tsdf_clusters); one host sync (K)."""
    tris, dev = mesh.triangles, mesh.triangles.device
    if not tris.is_cuda:
        raise RuntimeError("cluster_connected_triangles runs on ROCm/HIP tensors only (no CPU fallback)")
    F = len(tris)
    if F == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    t = tris.long()
    a = torch.cat([t[:, 0], t[:, 1], t[:, 2]])
    b = torch.cat([t[:, 1], t[:, 2], t[:, 0]])
    key = torch.minimum(a, b) * len(mesh.vertices) + torch.maximum(a, b)
    keys, idx = torch.sort(key, stable=True)
    tri_of = idx % F
    lib = L.load()
    with torch.cuda.device(dev):
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        rank = torch.empty(F + 1, dtype=torch.int32, device=dev)
        label = torch.empty(F, dtype=torch.int32, device=dev)
        counts = torch.empty(F, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(lib.gdr_tsdf_scan_bytes(F)), dtype=torch.uint8, device=dev)
        L.check(lib.gdr_tsdf_clusters(F, M.ptr(keys), M.ptr(tri_of), M.ptr(parent), M.ptr(rank), M.ptr(label), M.ptr(counts),
                                      M.ptr(scratch), M.stream()), "gdr_tsdf_clusters")
        K = int(rank[F].item())
    return label, counts[:K]


def keep_cluster_mask(counts, k: int = 10) -> np.ndarray:
    """Host-side keep rule of the reference: n = sorted(counts)[-min(#clusters, k)]; keep the clusters with count >= n
    (ties keep more than k clusters)."""
    counts = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts)
    if counts.size == 0:
        return np.zeros(0, dtype=bool)
    n = np.sort(counts)[-min(counts.size, k)]
    return counts >= n


def keep_largest_clusters(mesh: TriangleMesh, k: int = 10) -> TriangleMesh:
    label, counts = cluster_connected_triangles(mesh)
    if len(counts) == 0:
        return mesh
    keep = torch.from_numpy(keep_cluster_mask(counts, k)).to(label.device)
    return TriangleMesh(mesh.vertices, mesh.triangles[keep[label.long()]], mesh.vertex_colors)


def remove_unreferenced_vertices(mesh: TriangleMesh) -> TriangleMesh:
    """Drop the vertices no triangle uses, keeping the order of the others."""
    used = torch.zeros(len(mesh.vertices), dtype=torch.bool, device=mesh.vertices.device)
    used[mesh.triangles.reshape(-1).long()] = True
    remap = torch.cumsum(used.to(torch.int64), 0) - 1
    return TriangleMesh(mesh.vertices[used], remap[mesh.triangles.long()].to(torch.int32), mesh.vertex_colors[used])


# ---- writers ------------------------------------------------------------------------------------------------------------
def write_mesh(path, mesh: TriangleMesh) -> None:
    """.obj: `v x y z r g b` and 1-based `f a b c` lines; .ply: binary little-endian, float x y z, uchar red green blue
    (round(c * 255)), faces as uchar-count int lists.  An empty mesh gives a valid empty file."""
    v = mesh.vertices.detach().cpu().numpy().astype(np.float32)
    c = mesh.vertex_colors.detach().cpu().numpy().astype(np.float32)
    f = mesh.triangles.detach().cpu().numpy().astype(np.int32)
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".obj":
        with open(path, "w") as fh:
            if len(v):
                np.savetxt(fh, np.concatenate([v, c], 1), fmt="v %.9g %.9g %.9g %.9g %.9g %.9g")
            if len(f):
                np.savetxt(fh, f + 1, fmt="f %d %d %d")
    elif ext == ".ply":
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        vrec = np.zeros(len(v), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
        vrec["p"] = v
        vrec["c"] = np.clip(np.round(c * 255), 0, 255).astype(np.uint8)
        frec = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
        frec["n"] = 3
        frec["i"] = f
        with open(path, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(vrec.tobytes())
            fh.write(frec.tobytes())
    else:
        raise ValueError(f"write_mesh: unsupported extension {ext!r} (.obj or .ply)")


def read_mesh(path):
    """(vertices (V, 3) f32, triangles (F, 3) int32, colours (V, 3) f32) of a file written by write_mesh (numpy, host);
    .ply colours come back as uchar / 255."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".obj":
        v, f = [], []
        with open(path) as fh:
            for line in fh:
                p = line.split()
                if p and p[0] == "v":
                    v.append([float(x) for x in p[1:7]])
                elif p and p[0] == "f":
                    f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
        v = np.array(v, np.float32).reshape(-1, 6)
        return v[:, :3], np.array(f, np.int32).reshape(-1, 3), v[:, 3:]
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    vrec = np.frombuffer(data, dtype=[("p", "<f4", 3), ("c", "u1", 3)], count=nv, offset=end)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", 3)], count=nf, offset=end + vrec.nbytes)
    return vrec["p"].copy(), frec["i"].copy(), vrec["c"].astype(np.float32) / 255


# ---- the reference's MeshExtractor ------------------------------------------------------------------------------------
class MeshExtractor:
    """tools/meshExtractor.py MeshExtractor on this project's renderers (renderer.Renderer or renderer_2dgs.Renderer).
    gs_params = (centers, shs, opacity, scales, rotations, mask) as the reference's fine render package; `mask` (bool or
    index, or None) is applied to all five tensors (the reference applies it to the last three only)."""

    def __init__(self, gs_params, render, aabb, bg_color=(1.0, 1.0, 1.0)):
        self.background = torch.tensor(bg_color, dtype=torch.float32, device="cuda")
        self.aabb = None if aabb is None else np.array(aabb).reshape(2, 3) * 1.1
        self.gs_params = gs_params
        self.render = render
        self.phase_ms = {}

    @torch.no_grad()
    def extract(self, save_mesh_path, data, voxel_size=2 / 256, sdf_trunc=0.08, alpha_thres=0.08, depth_trunc=10,
                sample=None, fov=None, device="cuda") -> TriangleMesh:
        """Render the 48 orbit views, fuse them (depth zeroed where alpha < alpha_thres), extract, crop to the AABB, keep
        the 10 largest triangle clusters, drop unreferenced vertices and write `save_mesh_path`.  Returns the written mesh;
        `phase_ms` holds the device time of each phase (render / integrate / mc / post)."""
        if self.aabb is not None:
            center = self.aabb.mean(0)
            radius = np.linalg.norm(self.aabb[1] - self.aabb[0]) * 0.5
            voxel_size = radius / 256
            sdf_trunc = voxel_size * 2
        volume = TSDFVolume(voxel_size, sdf_trunc, device=device)
        cams = mesh_path_cameras(16, data, sample, fov)
        centers, shs, opacity, scales, rotations, mask = self.gs_params
        if mask is not None:
            centers, shs, opacity, scales, rotations = (t[mask] for t in (centers, shs, opacity, scales, rotations))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        render_ms = stage_ms = 0.0
        for cam in cams:
            cam.to_device(device)
            W, H = cam.image_width, cam.image_height
            fx, fy = W / (2 * math.tan(cam.FoVx / 2.0)), H / (2 * math.tan(cam.FoVy / 2.0))
            rays = cam.get_rays().squeeze(0).to(device)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            pkg = self.render.render_img(cam, rays, centers, shs, opacity, scales, rotations, device)
            e1.record()
            depth = pkg["depth"].reshape(H, W).masked_fill(pkg["acc_map"].reshape(H, W) < alpha_thres, 0)
            if self.aabb is not None:
                campos = cam.camera_center.cpu().numpy()
                depth_trunc = np.linalg.norm(campos - center, axis=-1) + radius
            volume.integrate(depth, pkg["image"], fx, fy, W / 2, H / 2, cam.world_view_transform.T, float(depth_trunc))
            e2.record()
            e2.synchronize()
            render_ms += e0.elapsed_time(e1)
            stage_ms += e1.elapsed_time(e2)
        ev[0].record()
        volume.fuse()
        ev[1].record()
        mesh = volume.marching_cubes()
        ev[2].record()
        if self.aabb is not None:
            mesh = crop_to_aabb(mesh, self.aabb)
        mesh = remove_unreferenced_vertices(keep_largest_clusters(mesh, 10))
        ev[3].record()
        ev[3].synchronize()
        self.phase_ms = {"render": render_ms, "integrate": stage_ms + ev[0].elapsed_time(ev[1]),
                         "mc": ev[1].elapsed_time(ev[2]), "post": ev[2].elapsed_time(ev[3])}
        self.volume = volume
        write_mesh(save_mesh_path, mesh)
        return mesh

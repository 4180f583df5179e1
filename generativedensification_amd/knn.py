"""`simple_knn._C.distCUDA2` for ROCm: mean squared distance to the 3 nearest neighbours of every point
(/root/reference/lightning/renderer_2dgs.py:11,92-96; point_decoder/layers/head.py:115).  HIP kernels in csrc/knn.hip
behind include/gsr.h; torch does the plumbing between the stages (quantile box, sort by cell, cell prefix).  Nothing here
waits for the device: the cells per axis are chosen by a kernel and stay on the device, and the cell prefix comes from a
searchsorted over a table whose size depends on N alone."""
from __future__ import annotations

import torch

from . import _lib as L
from . import _marshal as M

# the box spans the (N >> TRIM_SHIFT)-th smallest to the (N >> TRIM_SHIFT)-th largest coordinate of every axis: up to
# 0.4 % of the points per side fall outside it and are binned into the edge cells (csrc/knn.hip: still exact)
TRIM_SHIFT = 8


def grid(pts: torch.Tensor, cells_per_axis: int | None = None):
    """pts (N >= 1, 3) fp32 contiguous on a HIP device -> (bbox (6,) fp32: lo xyz, hi xyz; gdim (3,) int32: cells per
    axis; max_cells: the host-side bound of gdim.prod()), the grid dist2 searches."""
    lib = L.load()
    N = int(pts.shape[0])
    g = int(cells_per_axis) if cells_per_axis else 0
    if g < 0 or g > 1024:
        raise ValueError("cells_per_axis must be in 1..1024")
    stream = M.stream()
    srt = pts.t().contiguous().sort(dim=1).values
    k = N >> TRIM_SHIFT
    bbox = torch.cat([srt[:, k], srt[:, N - 1 - k]]).contiguous()
    gdim = torch.empty(3, dtype=torch.int32, device=pts.device)
    max_cells = g ** 3 if g else N + 8
    L.check(lib.gsr_knn_grid(bbox.data_ptr(), max(1, N // 2), max_cells, g, gdim.data_ptr(), stream), "gsr_knn_grid")
    return bbox, gdim, max_cells


def dist2(points: torch.Tensor, cells_per_axis: int | None = None, return_work: bool = False):
    """points (N,3) on a HIP device -> (N,) fp32, (d1 + d2 + d3) / 3 of the three nearest OTHER points (inf terms when
    fewer than 4 points exist, as the lineage's initial `best = FLT_MAX` would leave).  cells_per_axis forces that many
    cells on every axis (the result does not depend on it; the work does).  return_work: also (N,) int32, the number of
    candidate points whose distance the search evaluated for each point."""
    if not points.is_cuda:
        raise RuntimeError("simple_knn.distCUDA2 (MI355X build) runs on ROCm/HIP device tensors only; no CPU fallback")
    lib = L.load()
    dev = points.device
    pts = points.detach().to(torch.float32).reshape(-1, 3).contiguous()
    N = int(pts.shape[0])
    out = torch.empty(N, dtype=torch.float32, device=dev)
    work = torch.zeros(N, dtype=torch.int32, device=dev) if return_work else None
    if N == 0:
        return (out, work) if return_work else out
    with torch.no_grad(), torch.cuda.device(dev):
        stream = M.stream()
        bbox, gdim, max_cells = grid(pts, cells_per_axis)
        cell = torch.empty(N, dtype=torch.int32, device=dev)
        L.check(lib.gsr_knn_cells_axes(pts.data_ptr(), N, bbox.data_ptr(), gdim.data_ptr(), cell.data_ptr(), stream),
                "gsr_knn_cells_axes")
        cell_sorted, order = torch.sort(cell, stable=True)
        pts_sorted = pts.index_select(0, order).contiguous()
        cell_start = torch.searchsorted(cell_sorted, torch.arange(max_cells + 1, dtype=torch.int32, device=dev),
                                        out_int32=True).contiguous()
        out_sorted = torch.empty(N, dtype=torch.float32, device=dev)
        work_sorted = torch.empty(N, dtype=torch.int32, device=dev) if return_work else None
        L.check(lib.gsr_knn_mean_dist2_counted(pts_sorted.data_ptr(), N, bbox.data_ptr(), gdim.data_ptr(),
                                               cell_start.data_ptr(), out_sorted.data_ptr(),
                                               work_sorted.data_ptr() if return_work else None, stream),
                "gsr_knn_mean_dist2_counted")
        out[order] = out_sorted
        if return_work:
            work[order] = work_sorted
    return (out, work) if return_work else out

// knn.hip — mean squared distance to the 3 nearest neighbours of every point: the `simple_knn._C.distCUDA2` the 2DGS
// adaptor imports (/root/reference/lightning/renderer_2dgs.py:11, used at :92-96 to initialise surfel scales; the only
// other use is point_decoder/layers/head.py:115, on network-predicted positions).  SURVEY §8f-4.  The package is not in
// the reference tree; the published behaviour (graphdeco simple-knn): dist[i] = (d1 + d2 + d3) / 3 with d_k the squared
// distances of the three nearest OTHER points (by index: coincident points count with distance 0), fp32.
//
// Uniform grid instead of the lineage's Morton boxes: points are binned into Gx * Gy * Gz cells (host plumbing: torch
// sort of the cell ids, searchsorted for the cell starts), then one thread per point scans the cells of growing cubic
// shells around its own cell, keeping the three smallest distances, and stops as soon as the third best is closer than
// the nearest face of the cube searched so far.  HBM/L2-latency bound gather; ~27-125 cells of ~2 points each per query.
//
// The grid (knn_grid_kernel, one thread, so the host never waits for the extents):
//   * the box is whatever the caller passes; knn.py passes a per-axis quantile box (the N/256-th smallest and largest
//     coordinate), so a few far outliers do not stretch the cells until every other point shares one;
//   * cells per axis are chosen separately so that the cells are near cubes of edge s with Gx * Gy * Gz ~ N / 2: an axis
//     whose extent is below s (a plane, a line, a coincident cloud, extents 100 : 1 : 0.01) gets ONE cell.  A one-cell
//     axis has no interior face, so it never enters the bound below and the search is 2-D, 1-D or a single cell.
// Why the result stays exact for any box and any cells per axis:
//   * cell_coord clamps, so a point outside the box lands in an edge cell: cell k of an axis holds every point with
//     trunc(u * inv_cs) == k, cell 0 also everything below, cell G-1 everything above (u = p - lo, computed ONCE per
//     point and used for both the cell and the bound, so a cloud far from the origin loses nothing to lo + x * cs);
//   * the bound only uses faces x0 > 0 and x1 < G-1, i.e. faces with cells beyond them.  Every unseen point q beyond
//     face x0 has trunc(u_q * inv_cs) < x0 (clamping from above cannot put it there), hence u_q < x0 * cs up to
//     rounding, hence |p - q| >= |p_x - q_x| >= u_p - x0 * cs up to rounding; symmetrically for x1;
//   * the rounding: u, u * inv_cs, cs, inv_cs and x * cs are each off by 2^-24 relative, together less than
//     2^-24 * (5 ext + 2 |u_p|) absolute; KNN_SLACK * ext covers the first term, the 0.9999 factor the second (and the
//     rounding of the subtraction itself);
//   * three neighbours at distance 0 cannot be beaten: the scan leaves at once (a coincident cloud costs 3 candidates
//     per point, not N).
#include "gdr_common.h"

namespace gdr {
namespace {

constexpr float KNN_SLACK = 1e-6f;   // > 5 * 2^-24, see above

struct KnnGrid {
    const float* bbox;     // device: lo x,y,z, hi x,y,z of the grid's box (points outside it clamp into the edge cells)
    const int32_t* gdim;   // device: cells per axis x,y,z; nullptr = G on every axis
    int G;
};

struct KnnAxes {
    float lo[3], cs[3], ic[3], slack[3];
    int G[3];
};

__device__ __forceinline__ void grid_params(const KnnGrid& g, KnnAxes& a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.G[k] = g.gdim ? g.gdim[k] : g.G;
        a.lo[k] = g.bbox[k];
        const float ext = fmaxf(g.bbox[3 + k] - g.bbox[k], 1e-20f);
        a.cs[k] = ext / (float)a.G[k];
        a.ic[k] = (float)a.G[k] / ext;
        a.slack[k] = KNN_SLACK * ext;
    }
}

// u = p - lo
__device__ __forceinline__ int cell_coord(float u, float inv_cs, int G) {
    return min(G - 1, max(0, (int)(u * inv_cs)));
}

// cells per axis for `target` near-cubic cells over the box, at most `cap` cells in all (the caller's cell_start holds
// cap + 1 entries); forced > 0: that many on every axis
__global__ void knn_grid_kernel(const float* __restrict__ bbox, int target, int cap, int forced, int32_t* __restrict__ gdim) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int G[3] = {1, 1, 1};
    if (forced > 0) {
        G[0] = G[1] = G[2] = forced;
    } else {
        double e[3];
        for (int k = 0; k < 3; ++k) {
            e[k] = (double)bbox[3 + k] - (double)bbox[k];
            if (!(e[k] > 0.0) || !isfinite(e[k])) e[k] = 0.0;
        }
        const double e1 = fmax(e[0], fmax(e[1], e[2])), e3 = fmin(e[0], fmin(e[1], e[2]));
        const double e2 = e[0] + e[1] + e[2] - e1 - e3;
        const double M = (double)max(target, 1);
        if (e1 > 0.0) {
            double s = cbrt(e1 * e2 * e3 / M);                       // three axes share the cells ...
            if (!(s > 0.0 && e3 >= s)) s = sqrt(e1 * e2 / M);        // ... or two: the thinnest is below one cell ...
            if (!(s > 0.0 && e2 >= s)) s = e1 / M;                   // ... or one
            for (int k = 0; k < 3; ++k)
                if (e[k] >= s) G[k] = (int)fmin(fmax(e[k] / s + 0.5, 1.0), (double)max(cap, 1));
        }
    }
    for (int it = 0; it < 64 && (long long)G[0] * G[1] * G[2] > (long long)max(cap, 1); ++it) {   // rounding went over
        const int k = G[0] >= G[1] && G[0] >= G[2] ? 0 : (G[1] >= G[2] ? 1 : 2);
        const long long others = (long long)G[(k + 1) % 3] * G[(k + 2) % 3];
        G[k] = (int)max(1LL, min((long long)G[k] - 1, (long long)max(cap, 1) / others));
    }
    gdim[0] = G[0];
    gdim[1] = G[1];
    gdim[2] = G[2];
}

__global__ __launch_bounds__(GDR_BLOCK) void knn_cells_kernel(const float* __restrict__ pts, int N, KnnGrid g,
                                                               int32_t* __restrict__ cell) {
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i >= N) return;
    KnnAxes a;
    grid_params(g, a);
    const int cx = cell_coord(pts[3 * i] - a.lo[0], a.ic[0], a.G[0]);
    const int cy = cell_coord(pts[3 * i + 1] - a.lo[1], a.ic[1], a.G[1]);
    const int cz = cell_coord(pts[3 * i + 2] - a.lo[2], a.ic[2], a.G[2]);
    cell[i] = (cz * a.G[1] + cy) * a.G[0] + cx;
}

// pts: points in CELL-SORTED order; cell_start: (Gx Gy Gz + 1) exclusive prefix of the cell populations; out[i] for
// sorted i.  COUNT: work[i] = the number of candidates whose distance was evaluated for point i.
template <bool COUNT>
__global__ __launch_bounds__(GDR_BLOCK) void knn_mean_dist2_kernel(const float* __restrict__ pts, int N, KnnGrid g,
                                                                    const int32_t* __restrict__ cell_start,
                                                                    float* __restrict__ out, uint32_t* __restrict__ work) {
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i >= N) return;
    KnnAxes a;
    grid_params(g, a);
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const float ux = px - a.lo[0], uy = py - a.lo[1], uz = pz - a.lo[2];
    const int Gx = a.G[0], Gy = a.G[1], Gz = a.G[2];
    const int cx = cell_coord(ux, a.ic[0], Gx), cy = cell_coord(uy, a.ic[1], Gy), cz = cell_coord(uz, a.ic[2], Gz);
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    uint32_t seen = 0;
    bool done = false;   // three neighbours at distance 0
    auto visit = [&](int x, int y, int z) {
        const int c = (z * Gy + y) * Gx + x;
        const int e = cell_start[c + 1];
        for (int j = cell_start[c]; j < e; ++j) {
            if (j == i) continue;
            const float dx = pts[3 * j] - px, dy = pts[3 * j + 1] - py, dz = pts[3 * j + 2] - pz;
            float d = dx * dx + dy * dy + dz * dz;
            if (COUNT) ++seen;
            if (d < b0) { const float t = b0; b0 = d; d = t; }
            if (d < b1) { const float t = b1; b1 = d; d = t; }
            if (d < b2) {
                b2 = d;
                if (b2 == 0.f) { done = true; return; }
            }
        }
    };
    const int R = max(Gx, max(Gy, Gz));
    for (int r = 0; r < R && !done; ++r) {
        const int x0 = cx - r, x1 = cx + r, y0 = cy - r, y1 = cy + r, z0 = cz - r, z1 = cz + r;
        for (int z = max(z0, 0); z <= min(z1, Gz - 1) && !done; ++z)
            for (int y = max(y0, 0); y <= min(y1, Gy - 1) && !done; ++y) {
                const bool shell_zy = z == z0 || z == z1 || y == y0 || y == y1;
                if (shell_zy) {
                    for (int x = max(x0, 0); x <= min(x1, Gx - 1) && !done; ++x) visit(x, y, z);
                } else {  // interior rows of the shell: only the two end cells
                    if (x0 >= 0) visit(x0, y, z);
                    if (x1 < Gx && x1 != x0 && !done) visit(x1, y, z);
                }
            }
        // everything inside the cube [c - r, c + r]^3 has been seen: the distance from the point to the cube's nearest
        // face that still has cells beyond it bounds the distance of any unseen point from below (header comment)
        float bound = INFINITY;
        if (x0 > 0) bound = fminf(bound, ux - (float)x0 * a.cs[0] - a.slack[0]);
        if (x1 < Gx - 1) bound = fminf(bound, (float)(x1 + 1) * a.cs[0] - ux - a.slack[0]);
        if (y0 > 0) bound = fminf(bound, uy - (float)y0 * a.cs[1] - a.slack[1]);
        if (y1 < Gy - 1) bound = fminf(bound, (float)(y1 + 1) * a.cs[1] - uy - a.slack[1]);
        if (z0 > 0) bound = fminf(bound, uz - (float)z0 * a.cs[2] - a.slack[2]);
        if (z1 < Gz - 1) bound = fminf(bound, (float)(z1 + 1) * a.cs[2] - uz - a.slack[2]);
        if (bound == INFINITY) break;                       // the cube covers the whole grid
        bound = fmaxf(bound, 0.f) * 0.9999f;
        if (b2 <= bound * bound) break;
    }
    out[i] = (b0 + b1 + b2) / 3.0f;
    if (COUNT) work[i] = seen;
}

}  // namespace

hipError_t launch_knn_grid(const float* bbox, int target, int cap, int forced, int32_t* gdim, hipStream_t st) {
    GDR_LAUNCH(GDR_K_KNN, knn_grid_kernel, dim3(1), dim3(64), st, bbox, target, cap, forced, gdim);
    return hipGetLastError();
}

hipError_t launch_knn_cells(const float* pts, int N, const float* bbox, const int32_t* gdim, int G, int32_t* cell,
                            hipStream_t st) {
    if (N == 0) return hipSuccess;
    const KnnGrid g{bbox, gdim, G};
    GDR_LAUNCH(GDR_K_KNN, knn_cells_kernel, dim3(div_up(N, GDR_BLOCK)), dim3(GDR_BLOCK), st, pts, N, g, cell);
    return hipGetLastError();
}

hipError_t launch_knn_mean_dist2(const float* pts_sorted, int N, const float* bbox, const int32_t* gdim, int G,
                                 const int32_t* cell_start, float* out, uint32_t* work, hipStream_t st) {
    if (N == 0) return hipSuccess;
    const KnnGrid g{bbox, gdim, G};
    if (work) {
        GDR_LAUNCH(GDR_K_KNN, knn_mean_dist2_kernel<true>, dim3(div_up(N, GDR_BLOCK)), dim3(GDR_BLOCK), st, pts_sorted, N,
                   g, cell_start, out, work);
    } else {
        GDR_LAUNCH(GDR_K_KNN, knn_mean_dist2_kernel<false>, dim3(div_up(N, GDR_BLOCK)), dim3(GDR_BLOCK), st, pts_sorted, N,
                   g, cell_start, out, work);
    }
    return hipGetLastError();
}

}  // namespace gdr

// tsdf.hip — TSDF fusion of depth / colour views into a block-sparse volume, marching-cubes mesh extraction and connected
// triangle components (include/gdr.h gdr_tsdf_*), the GPU path of the reference's mesh extraction (Open3D's
// ScalableTSDFVolume integrate + extract_triangle_mesh + cluster_connected_triangles).
//
// Specification (Open3D's published algorithm restated; parity with Open3D is unpinned).  All arithmetic is fp32 in the order
// written; the file is built with -ffp-contract=off so that tests/tsdf_ref.py (the numpy restatement) is matched bit for bit.
//   depth        D(v, u) := 0 where not finite, <= 0 or > depth_trunc (the caller's alpha mask also zeroes it).  Colour is
//                uint8; float input is staged as p = rgb * 255 in fp32, truncated toward zero, then clipped to 0..255, NaN
//                giving 0 (floor(rgb * 255) on [0, 1]; +-inf, values above 1 and negatives saturate).
//   allocation   pixels with u % S == 0, v % S == 0 and d > 0: q = ((u - cx) d / fx, (v - cy) d / fy, d), p = c2w q (c2w = the
//                inverse of E in f64, cast to f32 by the host).  Every block b with floor((p - trunc) / L) <= b <=
//                floor((p + trunc) / L) per axis (L = R voxel) is touched by the view.  Blocks are kept in (bz, by, bx) order.
//   integration  view k, only into the blocks k touched, in view order: voxel g has centre x = (g + 0.5) voxel, xc = E x.
//                If z > 0: u = floor(xc.x fx / z + cx + 0.5) (v likewise) inside the image, d = D(v, u) > 0,
//                sdf = (d - z) sqrt(1 + ((u - cx) / fx)^2 + ((v - cy) / fy)^2); if sdf > -trunc: t = min(1, sdf (1 / trunc)),
//                T = (T w + t) / (w + 1), C = (C w + c) / (w + 1), w += 1.
//   extraction   a cube (lower corner voxel g) is valid when its 8 corners have w > 0; bit i of its case is T_i < 0; cases 0
//                and 255 emit nothing.  An edge (a, a + e_axis) carries a vertex when its ends differ in sign, both have
//                w > 0 and one of the <= 4 cubes around it is valid: centre(a) + (|Ta| / (|Ta| + |Tb|)) voxel along the axis,
//                colour ((|Tb| Ca + |Ta| Cb) / (|Ta| + |Tb|)) / 255.  Triangles come from the 256-case table below, wound so
//                that (v1 - v0) x (v2 - v0) points toward positive T (outward, toward the cameras).
//   order        vertices by owning voxel (block order, then the voxel's index x + R (y + R z) in its block), then axis
//                x < y < z; triangles by cube (same order), then table slot.  Both are produced by exclusive scans of
//                per-voxel counts, so the arrays do not depend on scheduling.
//   components   triangles sharing an edge (edge keys (min, max) sorted by the caller) join one cluster; a cluster is
//                labelled by the rank of its smallest triangle index.
//
// Storage: a dense int32 cell -> block index grid over the bounding box of the touched blocks (-1 = not allocated), a view
// mask of ceil(V / 32) words per cell, and per allocated block R^3 = 4096 voxels as SoA fp32 planes (tsdf, weight, r, g, b,
// each n_blocks * 4096).  Kernels:
//   tsdf_bounds_kernel / tsdf_mark_kernel   one thread per sampled pixel: the block box of the point (integer atomic
//                                           min / max into the bounding box, then atomic OR of the view bit into the cells)
//   tsdf_flag_cells_kernel + scan + tsdf_cell_index_kernel   allocated cells numbered in cell order = (bz, by, bx) order
//   tsdf_integrate_kernel                   one workgroup per block, 16 voxels per thread in registers, the block's view
//                                           mask walked in view order, each voxel written once: no atomics, reproducible
//   tsdf_mc_classify_kernel / tsdf_mc_vertex_kernel   per cube case and triangle count, per voxel vertex flags and count
//   scan, tsdf_mc_emit_*_kernel             exclusive scans give every vertex and triangle its slot; neighbour voxels
//                                           across block faces are read through the cell grid (a missing block has w = 0)
//   tsdf_cc_*_kernel                        union-find over adjacent equal edge keys: hook the larger root onto the smaller
//                                           with CAS, compress, label roots by a scan, count with integer atomics
// The host reads back the bounding box, the block count and the vertex / triangle totals to size the next buffers: mesh
// extraction is not a training-loop path, and these three synchronisations are its only ones.
//
// The triangle table is derived from face-consistent polygons (tests/tsdf_ref.py builds it from first principles and a CPU
// test checks this literal against it): on an ambiguous face the two negative corners are separated, so neighbouring cubes
// always agree and the surface has no cracks.
#include <algorithm>

#include "gdr_common.h"
#include "host_util.h"

namespace gdr {

constexpr int TS_R = GDR_TSDF_R;              // voxels per block edge
constexpr int TS_N = TS_R * TS_R * TS_R;      // voxels per block (4096)
constexpr int TS_PER = TS_N / GDR_BLOCK;      // voxels per thread (16): thread t owns x = t % 16, y = t / 16, every z
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = GDR_BLOCK * SCAN_ITEMS;

__constant__ int8_t c_tri_table[256][16] = {
{-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{1,10,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,10,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,10,0,10,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,9,2,9,10,-1,-1,-1,-1,-1,-1,-1},
{2,11,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,2,11,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,2,11,1,11,8,1,8,9,-1,-1,-1,-1,-1,-1,-1},
{1,10,11,1,11,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,1,10,0,10,11,0,11,8,-1,-1,-1,-1,-1,-1,-1},
{0,9,10,0,10,11,0,11,3,-1,-1,-1,-1,-1,-1,-1}, {8,9,10,8,10,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,3,7,1,7,4,1,4,9,-1,-1,-1,-1,-1,-1,-1},
{1,10,2,4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,4,1,10,2,-1,-1,-1,-1,-1,-1,-1},
{0,9,10,0,10,2,4,8,7,-1,-1,-1,-1,-1,-1,-1}, {2,3,7,2,7,4,2,4,9,2,9,10,-1,-1,-1,-1},
{2,11,3,4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,7,0,7,4,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,2,11,3,4,8,7,-1,-1,-1,-1,-1,-1,-1}, {1,2,11,1,11,7,1,7,4,1,4,9,-1,-1,-1,-1},
{1,10,11,1,11,3,4,8,7,-1,-1,-1,-1,-1,-1,-1}, {0,1,10,0,10,11,0,11,7,0,7,4,-1,-1,-1,-1},
{0,9,10,0,10,11,0,11,3,4,8,7,-1,-1,-1,-1}, {4,9,10,4,10,11,4,11,7,-1,-1,-1,-1,-1,-1,-1},
{4,5,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,4,5,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,4,5,0,5,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,4,1,4,5,-1,-1,-1,-1,-1,-1,-1},
{1,10,2,4,5,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,10,2,4,5,9,-1,-1,-1,-1,-1,-1,-1},
{0,4,5,0,5,10,0,10,2,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,4,2,4,5,2,5,10,-1,-1,-1,-1},
{2,11,3,4,5,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,8,4,5,9,-1,-1,-1,-1,-1,-1,-1},
{0,4,5,0,5,1,2,11,3,-1,-1,-1,-1,-1,-1,-1}, {1,2,11,1,11,8,1,8,4,1,4,5,-1,-1,-1,-1},
{1,10,11,1,11,3,4,5,9,-1,-1,-1,-1,-1,-1,-1}, {0,1,10,0,10,11,0,11,8,4,5,9,-1,-1,-1,-1},
{0,4,5,0,5,10,0,10,11,0,11,3,-1,-1,-1,-1}, {4,5,10,4,10,11,4,11,8,-1,-1,-1,-1,-1,-1,-1},
{5,9,8,5,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,5,0,5,9,-1,-1,-1,-1,-1,-1,-1},
{0,8,7,0,7,5,0,5,1,-1,-1,-1,-1,-1,-1,-1}, {1,3,7,1,7,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{1,10,2,5,9,8,5,8,7,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,5,0,5,9,1,10,2,-1,-1,-1,-1},
{0,8,7,0,7,5,0,5,10,0,10,2,-1,-1,-1,-1}, {2,3,7,2,7,5,2,5,10,-1,-1,-1,-1,-1,-1,-1},
{2,11,3,5,9,8,5,8,7,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,7,0,7,5,0,5,9,-1,-1,-1,-1},
{0,8,7,0,7,5,0,5,1,2,11,3,-1,-1,-1,-1}, {1,2,11,1,11,7,1,7,5,-1,-1,-1,-1,-1,-1,-1},
{1,10,11,1,11,3,5,9,8,5,8,7,-1,-1,-1,-1}, {0,1,10,0,10,11,0,11,7,0,7,5,0,5,9,-1},
{0,8,7,0,7,5,0,5,10,0,10,11,0,11,3,-1}, {5,10,11,5,11,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,9,5,6,10,-1,-1,-1,-1,-1,-1,-1},
{1,5,6,1,6,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,5,6,1,6,2,-1,-1,-1,-1,-1,-1,-1},
{0,9,5,0,5,6,0,6,2,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,9,2,9,5,2,5,6,-1,-1,-1,-1},
{2,11,3,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,8,5,6,10,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,2,11,3,5,6,10,-1,-1,-1,-1,-1,-1,-1}, {1,2,11,1,11,8,1,8,9,5,6,10,-1,-1,-1,-1},
{1,5,6,1,6,11,1,11,3,-1,-1,-1,-1,-1,-1,-1}, {0,1,5,0,5,6,0,6,11,0,11,8,-1,-1,-1,-1},
{0,9,5,0,5,6,0,6,11,0,11,3,-1,-1,-1,-1}, {5,6,11,5,11,8,5,8,9,-1,-1,-1,-1,-1,-1,-1},
{4,8,7,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,4,5,6,10,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,4,8,7,5,6,10,-1,-1,-1,-1,-1,-1,-1}, {1,3,7,1,7,4,1,4,9,5,6,10,-1,-1,-1,-1},
{1,5,6,1,6,2,4,8,7,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,4,1,5,6,1,6,2,-1,-1,-1,-1},
{0,9,5,0,5,6,0,6,2,4,8,7,-1,-1,-1,-1}, {2,3,7,2,7,4,2,4,9,2,9,5,2,5,6,-1},
{2,11,3,4,8,7,5,6,10,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,7,0,7,4,5,6,10,-1,-1,-1,-1},
{0,9,1,2,11,3,4,8,7,5,6,10,-1,-1,-1,-1}, {1,2,11,1,11,7,1,7,4,1,4,9,5,6,10,-1},
{1,5,6,1,6,11,1,11,3,4,8,7,-1,-1,-1,-1}, {0,1,5,0,5,6,0,6,11,0,11,7,0,7,4,-1},
{0,9,5,0,5,6,0,6,11,0,11,3,4,8,7,-1}, {4,9,5,4,5,6,4,6,11,4,11,7,-1,-1,-1,-1},
{4,6,10,4,10,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,4,6,10,4,10,9,-1,-1,-1,-1,-1,-1,-1},
{0,4,6,0,6,10,0,10,1,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,4,1,4,6,1,6,10,-1,-1,-1,-1},
{1,9,4,1,4,6,1,6,2,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,9,4,1,4,6,1,6,2,-1,-1,-1,-1},
{0,4,6,0,6,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,4,2,4,6,-1,-1,-1,-1,-1,-1,-1},
{2,11,3,4,6,10,4,10,9,-1,-1,-1,-1,-1,-1,-1}, {0,2,11,0,11,8,4,6,10,4,10,9,-1,-1,-1,-1},
{0,4,6,0,6,10,0,10,1,2,11,3,-1,-1,-1,-1}, {1,2,11,1,11,8,1,8,4,1,4,6,1,6,10,-1},
{1,9,4,1,4,6,1,6,11,1,11,3,-1,-1,-1,-1}, {0,1,9,0,9,4,0,4,6,0,6,11,0,11,8,-1},
{0,4,6,0,6,11,0,11,3,-1,-1,-1,-1,-1,-1,-1}, {4,6,11,4,11,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{6,10,9,6,9,8,6,8,7,-1,-1,-1,-1,-1,-1,-1}, {0,3,7,0,7,6,0,6,10,0,10,9,-1,-1,-1,-1},
{0,8,7,0,7,6,0,6,10,0,10,1,-1,-1,-1,-1}, {1,3,7,1,7,6,1,6,10,-1,-1,-1,-1,-1,-1,-1},
{1,9,8,1,8,7,1,7,6,1,6,2,-1,-1,-1,-1}, {0,3,7,0,7,6,0,6,2,0,2,1,0,1,9,-1},
{0,8,7,0,7,6,0,6,2,-1,-1,-1,-1,-1,-1,-1}, {2,3,7,2,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{2,11,3,6,10,9,6,9,8,6,8,7,-1,-1,-1,-1}, {0,2,11,0,11,7,0,7,6,0,6,10,0,10,9,-1},
{0,8,7,0,7,6,0,6,10,0,10,1,2,11,3,-1}, {1,2,11,1,11,7,1,7,6,1,6,10,-1,-1,-1,-1},
{1,9,8,1,8,7,1,7,6,1,6,11,1,11,3,-1}, {0,1,9,6,11,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,8,7,0,7,6,0,6,11,0,11,3,-1,-1,-1,-1}, {6,11,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{6,7,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,6,7,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,6,7,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,9,6,7,11,-1,-1,-1,-1,-1,-1,-1},
{1,10,2,6,7,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,10,2,6,7,11,-1,-1,-1,-1,-1,-1,-1},
{0,9,10,0,10,2,6,7,11,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,9,2,9,10,6,7,11,-1,-1,-1,-1},
{2,6,7,2,7,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,2,6,0,6,7,0,7,8,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,2,6,7,2,7,3,-1,-1,-1,-1,-1,-1,-1}, {1,2,6,1,6,7,1,7,8,1,8,9,-1,-1,-1,-1},
{1,10,6,1,6,7,1,7,3,-1,-1,-1,-1,-1,-1,-1}, {0,1,10,0,10,6,0,6,7,0,7,8,-1,-1,-1,-1},
{0,9,10,0,10,6,0,6,7,0,7,3,-1,-1,-1,-1}, {6,7,8,6,8,9,6,9,10,-1,-1,-1,-1,-1,-1,-1},
{4,8,11,4,11,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,11,0,11,6,0,6,4,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,4,8,11,4,11,6,-1,-1,-1,-1,-1,-1,-1}, {1,3,11,1,11,6,1,6,4,1,4,9,-1,-1,-1,-1},
{1,10,2,4,8,11,4,11,6,-1,-1,-1,-1,-1,-1,-1}, {0,3,11,0,11,6,0,6,4,1,10,2,-1,-1,-1,-1},
{0,9,10,0,10,2,4,8,11,4,11,6,-1,-1,-1,-1}, {2,3,11,2,11,6,2,6,4,2,4,9,2,9,10,-1},
{2,6,4,2,4,8,2,8,3,-1,-1,-1,-1,-1,-1,-1}, {0,2,6,0,6,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,2,6,4,2,4,8,2,8,3,-1,-1,-1,-1}, {1,2,6,1,6,4,1,4,9,-1,-1,-1,-1,-1,-1,-1},
{1,10,6,1,6,4,1,4,8,1,8,3,-1,-1,-1,-1}, {0,1,10,0,10,6,0,6,4,-1,-1,-1,-1,-1,-1,-1},
{0,9,10,0,10,6,0,6,4,0,4,8,0,8,3,-1}, {4,9,10,4,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{4,5,9,6,7,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,4,5,9,6,7,11,-1,-1,-1,-1,-1,-1,-1},
{0,4,5,0,5,1,6,7,11,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,4,1,4,5,6,7,11,-1,-1,-1,-1},
{1,10,2,4,5,9,6,7,11,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,10,2,4,5,9,6,7,11,-1,-1,-1,-1},
{0,4,5,0,5,10,0,10,2,6,7,11,-1,-1,-1,-1}, {2,3,8,2,8,4,2,4,5,2,5,10,6,7,11,-1},
{2,6,7,2,7,3,4,5,9,-1,-1,-1,-1,-1,-1,-1}, {0,2,6,0,6,7,0,7,8,4,5,9,-1,-1,-1,-1},
{0,4,5,0,5,1,2,6,7,2,7,3,-1,-1,-1,-1}, {1,2,6,1,6,7,1,7,8,1,8,4,1,4,5,-1},
{1,10,6,1,6,7,1,7,3,4,5,9,-1,-1,-1,-1}, {0,1,10,0,10,6,0,6,7,0,7,8,4,5,9,-1},
{0,4,5,0,5,10,0,10,6,0,6,7,0,7,3,-1}, {4,5,10,4,10,6,4,6,7,4,7,8,-1,-1,-1,-1},
{5,9,8,5,8,11,5,11,6,-1,-1,-1,-1,-1,-1,-1}, {0,3,11,0,11,6,0,6,5,0,5,9,-1,-1,-1,-1},
{0,8,11,0,11,6,0,6,5,0,5,1,-1,-1,-1,-1}, {1,3,11,1,11,6,1,6,5,-1,-1,-1,-1,-1,-1,-1},
{1,10,2,5,9,8,5,8,11,5,11,6,-1,-1,-1,-1}, {0,3,11,0,11,6,0,6,5,0,5,9,1,10,2,-1},
{0,8,11,0,11,6,0,6,5,0,5,10,0,10,2,-1}, {2,3,11,2,11,6,2,6,5,2,5,10,-1,-1,-1,-1},
{2,6,5,2,5,9,2,9,8,2,8,3,-1,-1,-1,-1}, {0,2,6,0,6,5,0,5,9,-1,-1,-1,-1,-1,-1,-1},
{0,8,3,0,3,2,0,2,6,0,6,5,0,5,1,-1}, {1,2,6,1,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{1,10,6,1,6,5,1,5,9,1,9,8,1,8,3,-1}, {0,1,10,0,10,6,0,6,5,0,5,9,-1,-1,-1,-1},
{0,8,3,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{5,7,11,5,11,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,5,7,11,5,11,10,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,5,7,11,5,11,10,-1,-1,-1,-1,-1,-1,-1}, {1,3,8,1,8,9,5,7,11,5,11,10,-1,-1,-1,-1},
{1,5,7,1,7,11,1,11,2,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,1,5,7,1,7,11,1,11,2,-1,-1,-1,-1},
{0,9,5,0,5,7,0,7,11,0,11,2,-1,-1,-1,-1}, {2,3,8,2,8,9,2,9,5,2,5,7,2,7,11,-1},
{2,10,5,2,5,7,2,7,3,-1,-1,-1,-1,-1,-1,-1}, {0,2,10,0,10,5,0,5,7,0,7,8,-1,-1,-1,-1},
{0,9,1,2,10,5,2,5,7,2,7,3,-1,-1,-1,-1}, {1,2,10,1,10,5,1,5,7,1,7,8,1,8,9,-1},
{1,5,7,1,7,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,1,5,0,5,7,0,7,8,-1,-1,-1,-1,-1,-1,-1},
{0,9,5,0,5,7,0,7,3,-1,-1,-1,-1,-1,-1,-1}, {5,7,8,5,8,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{4,8,11,4,11,10,4,10,5,-1,-1,-1,-1,-1,-1,-1}, {0,3,11,0,11,10,0,10,5,0,5,4,-1,-1,-1,-1},
{0,9,1,4,8,11,4,11,10,4,10,5,-1,-1,-1,-1}, {1,3,11,1,11,10,1,10,5,1,5,4,1,4,9,-1},
{1,5,4,1,4,8,1,8,11,1,11,2,-1,-1,-1,-1}, {0,3,11,0,11,2,0,2,1,0,1,5,0,5,4,-1},
{0,9,5,0,5,4,0,4,8,0,8,11,0,11,2,-1}, {2,3,11,4,9,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{2,10,5,2,5,4,2,4,8,2,8,3,-1,-1,-1,-1}, {0,2,10,0,10,5,0,5,4,-1,-1,-1,-1,-1,-1,-1},
{0,9,1,2,10,5,2,5,4,2,4,8,2,8,3,-1}, {1,2,10,1,10,5,1,5,4,1,4,9,-1,-1,-1,-1},
{1,5,4,1,4,8,1,8,3,-1,-1,-1,-1,-1,-1,-1}, {0,1,5,0,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,9,5,0,5,4,0,4,8,0,8,3,-1,-1,-1,-1}, {4,9,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{4,7,11,4,11,10,4,10,9,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,4,7,11,4,11,10,4,10,9,-1,-1,-1,-1},
{0,4,7,0,7,11,0,11,10,0,10,1,-1,-1,-1,-1}, {1,3,8,1,8,4,1,4,7,1,7,11,1,11,10,-1},
{1,9,4,1,4,7,1,7,11,1,11,2,-1,-1,-1,-1}, {0,3,8,1,9,4,1,4,7,1,7,11,1,11,2,-1},
{0,4,7,0,7,11,0,11,2,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,4,2,4,7,2,7,11,-1,-1,-1,-1},
{2,10,9,2,9,4,2,4,7,2,7,3,-1,-1,-1,-1}, {0,2,10,0,10,9,0,9,4,0,4,7,0,7,8,-1},
{0,4,7,0,7,3,0,3,2,0,2,10,0,10,1,-1}, {1,2,10,4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{1,9,4,1,4,7,1,7,3,-1,-1,-1,-1,-1,-1,-1}, {0,1,9,0,9,4,0,4,7,0,7,8,-1,-1,-1,-1},
{0,4,7,0,7,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{8,11,10,8,10,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,11,0,11,10,0,10,9,-1,-1,-1,-1,-1,-1,-1},
{0,8,11,0,11,10,0,10,1,-1,-1,-1,-1,-1,-1,-1}, {1,3,11,1,11,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{1,9,8,1,8,11,1,11,2,-1,-1,-1,-1,-1,-1,-1}, {0,3,11,0,11,2,0,2,1,0,1,9,-1,-1,-1,-1},
{0,8,11,0,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{2,10,9,2,9,8,2,8,3,-1,-1,-1,-1,-1,-1,-1}, {0,2,10,0,10,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,8,3,0,3,2,0,2,10,0,10,1,-1,-1,-1,-1}, {1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{1,9,8,1,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,1,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
{0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}
};
// edge e of a cube: offset of its lower corner (bit 0 x, bit 1 y, bit 2 z) and its axis
__constant__ uint8_t c_edge_off[12] = {0, 1, 2, 0, 4, 5, 6, 4, 0, 1, 3, 2};
__constant__ uint8_t c_edge_axis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};
// corner i of a cube: offset (bit 0 x, bit 1 y, bit 2 z)
__constant__ uint8_t c_corner_off[8] = {0, 1, 3, 2, 4, 5, 7, 6};

struct TsGrid {
    int lo[3], dims[3];
    __device__ __forceinline__ int cell(int bx, int by, int bz) const {   // -1 outside the grid
        const int x = bx - lo[0], y = by - lo[1], z = bz - lo[2];
        if (x < 0 || y < 0 || z < 0 || x >= dims[0] || y >= dims[1] || z >= dims[2]) return -1;
        return (z * dims[1] + y) * dims[0] + x;
    }
};

TsGrid make_grid(const gdr_tsdf_args* a) {
    TsGrid g;
    for (int i = 0; i < 3; ++i) {
        g.lo[i] = a->lo[i];
        g.dims[i] = a->dims[i];
    }
    return g;
}

// ---- exclusive scan of uint32 counts (in place; total written at [n]) -----------------------------------------------------
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds /* GDR_BLOCK / 64 + 1 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    const uint32_t total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    if (threadIdx.x == 0) lds[4] = total;
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(GDR_BLOCK) void scan_reduce_kernel(const uint32_t* __restrict__ in, int64_t n,
                                                                uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[GDR_BLOCK / GDR_WAVE + 1];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) s += in[base + i];
    block_exclusive_scan(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = lds[4];
}

// one workgroup: exclusive scan of the tile sums in place, the grand total into out_total
__global__ __launch_bounds__(GDR_BLOCK) void scan_partials_kernel(uint32_t* __restrict__ partial, int tiles,
                                                                  uint32_t* __restrict__ out_total) {
    __shared__ uint32_t lds[GDR_BLOCK / GDR_WAVE + 1];
    uint32_t carry = 0;
    for (int b = 0; b < tiles; b += GDR_BLOCK) {
        const int i = b + threadIdx.x;
        const uint32_t v = i < tiles ? partial[i] : 0u;
        const uint32_t ex = block_exclusive_scan(v, lds);
        if (i < tiles) partial[i] = carry + ex;
        carry += lds[4];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out_total = carry;
}

__global__ __launch_bounds__(GDR_BLOCK) void scan_apply_kernel(uint32_t* __restrict__ data, int64_t n,
                                                               const uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[GDR_BLOCK / GDR_WAVE + 1];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = base + i < n ? data[base + i] : 0u;
        s += v[i];
    }
    uint32_t run = partial[blockIdx.x] + block_exclusive_scan(s, lds);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) data[base + i] = run;
        run += v[i];
    }
}

// ---- staging ---------------------------------------------------------------------------------------------------------
struct TsStage {
    const float* depth; int64_t ds[2];
    const void* rgb; int64_t cs[3]; int u8;
    float depth_trunc;
};

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_stage_kernel(TsStage s, int H, int W, float* __restrict__ depth_out,
                                                               uint32_t* __restrict__ rgb_out) {
    const int64_t i = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int v = (int)(i / W), u = (int)(i - (int64_t)v * W);
    const float d = s.depth[v * s.ds[0] + u * s.ds[1]];
    depth_out[i] = (isfinite(d) && d > 0.f && d <= s.depth_trunc) ? d : 0.f;
    uint32_t packed = 0;
    for (int c = 0; c < 3; ++c) {
        const int64_t o = v * s.cs[0] + u * s.cs[1] + c * s.cs[2];
        uint32_t q;
        if (s.u8) {
            q = ((const uint8_t*)s.rgb)[o];
        } else {
            const float p = ((const float*)s.rgb)[o] * 255.f;
            q = p >= 255.f ? 255u : (p > 0.f ? (uint32_t)p : 0u);
        }
        packed |= q << (8 * c);
    }
    rgb_out[i] = packed;
}

// ---- allocation --------------------------------------------------------------------------------------------------------
struct TsAlloc {
    int V, H, W, S, sh, sw;   // sampled grid sh x sw per view
    float L, trunc;
};

// the block box [lo, hi] of sampled pixel i (false: no depth there)
__device__ __forceinline__ bool sample_box(const TsAlloc& A, const gdr_tsdf_view* __restrict__ views,
                                           const float* __restrict__ depth, int64_t i, int* k_out, int lo[3], int hi[3]) {
    const int64_t per = (int64_t)A.sh * A.sw;
    const int k = (int)(i / per);
    const int r = (int)(i - (int64_t)k * per);
    const int v = (r / A.sw) * A.S, u = (r % A.sw) * A.S;
    const float d = depth[(int64_t)k * A.H * A.W + (int64_t)v * A.W + u];
    if (!(d > 0.f)) return false;
    const gdr_tsdf_view& vw = views[k];
    const float qx = ((float)u - vw.cx) * d / vw.fx, qy = ((float)v - vw.cy) * d / vw.fy, qz = d;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float* M = vw.c2w + 4 * a;
        const float p = M[0] * qx + M[1] * qy + M[2] * qz + M[3];
        const float l = fminf(fmaxf(floorf((p - A.trunc) / A.L), -1e9f), 1e9f);
        const float h = fminf(fmaxf(floorf((p + A.trunc) / A.L), -1e9f), 1e9f);
        lo[a] = (int)l;
        hi[a] = (int)h;
    }
    *k_out = k;
    return true;
}

__global__ void tsdf_bounds_init_kernel(int* bbox) {
    if (threadIdx.x < 3) bbox[threadIdx.x] = 0x7fffffff;
    else if (threadIdx.x < 6) bbox[threadIdx.x] = (int)0x80000000;
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_bounds_kernel(TsAlloc A, const gdr_tsdf_view* __restrict__ views,
                                                                const float* __restrict__ depth, int* __restrict__ bbox) {
    const int64_t i = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000}, k;
    if (i < (int64_t)A.V * A.sh * A.sw) {
        int l[3], h[3];
        if (sample_box(A, views, depth, i, &k, l, h))
            for (int a = 0; a < 3; ++a) { lo[a] = l[a]; hi[a] = h[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // wave reduction first: one atomic per wave and bound
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = max(hi[a], __shfl_xor(hi[a], off, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {   // every wave targets the same 6 words: skip the atomic where the box already covers it
        for (int a = 0; a < 3; ++a) {
            if (lo[a] < __hip_atomic_load(bbox + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(bbox + a, lo[a]);
            if (hi[a] > __hip_atomic_load(bbox + 3 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(bbox + 3 + a, hi[a]);
        }
    }
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_mark_kernel(TsAlloc A, TsGrid G, int words,
                                                              const gdr_tsdf_view* __restrict__ views,
                                                              const float* __restrict__ depth, uint32_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i >= (int64_t)A.V * A.sh * A.sw) return;
    int lo[3], hi[3], k;
    if (!sample_box(A, views, depth, i, &k, lo, hi)) return;
    const uint32_t bit = 1u << (k & 31);
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const int c = G.cell(x, y, z);
                if (c < 0) continue;   // cannot happen: the grid is the bounding box of these boxes
                uint32_t* w = mask + (int64_t)c * words + (k >> 5);
                if (!(*w & bit)) atomicOr(w, bit);
            }
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_flag_cells_kernel(int64_t cells, int words, const uint32_t* __restrict__ mask,
                                                                    uint32_t* __restrict__ flag) {
    const int64_t c = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (c >= cells) return;
    uint32_t any = 0;
    for (int w = 0; w < words; ++w) any |= mask[c * words + w];
    flag[c] = any != 0;
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_cell_index_kernel(int64_t cells, int words, const uint32_t* __restrict__ mask,
                                                                    const uint32_t* __restrict__ offs, int* __restrict__ cell_block) {
    const int64_t c = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (c >= cells) return;
    uint32_t any = 0;
    for (int w = 0; w < words; ++w) any |= mask[c * words + w];
    cell_block[c] = any ? (int)offs[c] : -1;
}

// ---- integration -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GDR_BLOCK) void tsdf_block_list_kernel(TsGrid G, int64_t cells, const int* __restrict__ cell_block,
                                                                    int4* __restrict__ blocks) {
    const int64_t c = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const int b = cell_block[c];
    if (b < 0) return;
    const int x = (int)(c % G.dims[0]), y = (int)((c / G.dims[0]) % G.dims[1]), z = (int)(c / ((int64_t)G.dims[0] * G.dims[1]));
    blocks[b] = make_int4(G.lo[0] + x, G.lo[1] + y, G.lo[2] + z, (int)c);
}

struct TsVol {
    float* t; float* w; float* r; float* g; float* b;   // planes of n_blocks * 4096
};

TsVol make_vol(float* vol, int n_blocks) {
    const int64_t P = (int64_t)n_blocks * TS_N;
    return TsVol{vol, vol + P, vol + 2 * P, vol + 3 * P, vol + 4 * P};
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_integrate_kernel(int H, int W, int words, float voxel, float trunc,
                                                                   float inv_trunc, const gdr_tsdf_view* __restrict__ views,
                                                                   const float* __restrict__ depth,
                                                                   const uint32_t* __restrict__ rgb,
                                                                   const int4* __restrict__ blocks,
                                                                   const uint32_t* __restrict__ mask, TsVol vol) {
    const int4 bc = blocks[blockIdx.x];
    const int lx = threadIdx.x & (TS_R - 1), ly = threadIdx.x / TS_R;
    const float x = ((float)(bc.x * TS_R + lx) + 0.5f) * voxel;
    const float y = ((float)(bc.y * TS_R + ly) + 0.5f) * voxel;
    float T[TS_PER], Wt[TS_PER], Cr[TS_PER], Cg[TS_PER], Cb[TS_PER];
#pragma unroll
    for (int j = 0; j < TS_PER; ++j) T[j] = Wt[j] = Cr[j] = Cg[j] = Cb[j] = 0.f;
    const int64_t HW = (int64_t)H * W;
    for (int wd = 0; wd < words; ++wd) {
        uint32_t m = mask[(int64_t)bc.w * words + wd];
        while (m) {
            const int k = wd * 32 + (__ffs(m) - 1);
            m &= m - 1;
            const gdr_tsdf_view& vw = views[k];
            const float* E = vw.E;
            const float* dk = depth + k * HW;
            const uint32_t* ck = rgb + k * HW;
            // the x, y terms of xc = E x are the same for the 16 voxels of the column
            const float ax = E[0] * x + E[1] * y, ay = E[4] * x + E[5] * y, az = E[8] * x + E[9] * y;
#pragma unroll
            for (int j = 0; j < TS_PER; ++j) {
                const float zw = ((float)(bc.z * TS_R + j) + 0.5f) * voxel;
                const float xx = ax + E[2] * zw + E[3], xy = ay + E[6] * zw + E[7], z = az + E[10] * zw + E[11];
                if (!(z > 0.f)) continue;
                const float uf = floorf(xx * vw.fx / z + vw.cx + 0.5f), vf = floorf(xy * vw.fy / z + vw.cy + 0.5f);
                if (!(uf >= 0.f && uf < (float)W && vf >= 0.f && vf < (float)H)) continue;
                const int u = (int)uf, v = (int)vf;
                const float d = dk[(int64_t)v * W + u];
                if (!(d > 0.f)) continue;
                const float a = ((float)u - vw.cx) / vw.fx, b = ((float)v - vw.cy) / vw.fy;
                const float sdf = (d - z) * sqrtf(1.f + a * a + b * b);
                if (!(sdf > -trunc)) continue;
                const float t = fminf(1.f, sdf * inv_trunc);
                const uint32_t c = ck[(int64_t)v * W + u];
                const float w0 = Wt[j], wn = w0 + 1.f;
                T[j] = (T[j] * w0 + t) / wn;
                Cr[j] = (Cr[j] * w0 + (float)(c & 255u)) / wn;
                Cg[j] = (Cg[j] * w0 + (float)((c >> 8) & 255u)) / wn;
                Cb[j] = (Cb[j] * w0 + (float)((c >> 16) & 255u)) / wn;
                Wt[j] = wn;
            }
        }
    }
    const int64_t base = (int64_t)blockIdx.x * TS_N + threadIdx.x;
#pragma unroll
    for (int j = 0; j < TS_PER; ++j) {
        const int64_t o = base + j * (TS_R * TS_R);
        vol.t[o] = T[j];
        vol.w[o] = Wt[j];
        vol.r[o] = Cr[j];
        vol.g[o] = Cg[j];
        vol.b[o] = Cb[j];
    }
}

// ---- marching cubes ----------------------------------------------------------------------------------------------------
// the 27 neighbour blocks (dz, dy, dx in -1..1) of workgroup blockIdx.x's block, -1 = not allocated
__device__ __forceinline__ void load_neighbours(TsGrid G, const int* __restrict__ cell_block, int4 bc, int* nbr) {
    if (threadIdx.x < 27) {
        const int dx = threadIdx.x % 3 - 1, dy = (threadIdx.x / 3) % 3 - 1, dz = threadIdx.x / 9 - 1;
        const int c = G.cell(bc.x + dx, bc.y + dy, bc.z + dz);
        nbr[threadIdx.x] = c < 0 ? -1 : cell_block[c];
    }
    __syncthreads();
}

// voxel (lx, ly, lz) relative to the workgroup's block, each in -16..31: (block index or -1, index inside that block)
__device__ __forceinline__ int locate(const int* nbr, int lx, int ly, int lz, int* li) {
    const int dx = (lx >= TS_R) - (lx < 0), dy = (ly >= TS_R) - (ly < 0), dz = (lz >= TS_R) - (lz < 0);
    *li = (lx - dx * TS_R) + TS_R * ((ly - dy * TS_R) + TS_R * (lz - dz * TS_R));
    return nbr[(dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)];
}

// cube_case[cube] = case (0..255) or -1 (a corner has w = 0); tcount[cube] = its triangles
__global__ __launch_bounds__(GDR_BLOCK) void tsdf_mc_classify_kernel(TsGrid G, const int* __restrict__ cell_block,
                                                                     const int4* __restrict__ blocks, TsVol vol,
                                                                     int16_t* __restrict__ cube_case,
                                                                     uint32_t* __restrict__ tcount) {
    __shared__ int nbr[27];
    load_neighbours(G, cell_block, blocks[blockIdx.x], nbr);
    const int lx = threadIdx.x & (TS_R - 1), ly = threadIdx.x / TS_R;
    for (int lz = 0; lz < TS_R; ++lz) {
        int cs = 0;
        bool valid = true;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = c_corner_off[i];
            int li;
            const int b = locate(nbr, lx + (o & 1), ly + ((o >> 1) & 1), lz + (o >> 2), &li);
            if (b < 0) { valid = false; continue; }
            const int64_t idx = (int64_t)b * TS_N + li;
            if (!(vol.w[idx] > 0.f)) valid = false;
            if (vol.t[idx] < 0.f) cs |= 1 << i;
        }
        const int64_t cube = (int64_t)blockIdx.x * TS_N + lx + TS_R * (ly + TS_R * lz);
        cube_case[cube] = valid ? (int16_t)cs : (int16_t)-1;
        int n = 0;
        if (valid)
            while (n < 5 && c_tri_table[cs][3 * n] >= 0) ++n;
        tcount[cube] = (uint32_t)n;
    }
}

__device__ __forceinline__ bool cube_valid_at(const int* nbr, const int16_t* __restrict__ cube_case, int lx, int ly, int lz) {
    int li;
    const int b = locate(nbr, lx, ly, lz, &li);
    return b >= 0 && cube_case[(int64_t)b * TS_N + li] >= 0;
}

// vflags[voxel] bit ax = the edge (voxel, voxel + e_ax) carries a vertex; vcount[voxel] = its popcount
__global__ __launch_bounds__(GDR_BLOCK) void tsdf_mc_vertex_kernel(TsGrid G, const int* __restrict__ cell_block,
                                                                   const int4* __restrict__ blocks, TsVol vol,
                                                                   const int16_t* __restrict__ cube_case,
                                                                   uint8_t* __restrict__ vflags, uint32_t* __restrict__ vcount) {
    __shared__ int nbr[27];
    load_neighbours(G, cell_block, blocks[blockIdx.x], nbr);
    const int lx = threadIdx.x & (TS_R - 1), ly = threadIdx.x / TS_R;
    for (int lz = 0; lz < TS_R; ++lz) {
        const int64_t own = (int64_t)blockIdx.x * TS_N + lx + TS_R * (ly + TS_R * lz);
        const float ta = vol.t[own], wa = vol.w[own];
        uint32_t f = 0;
        if (wa > 0.f) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                int li;
                const int b = locate(nbr, lx + (ax == 0), ly + (ax == 1), lz + (ax == 2), &li);
                if (b < 0) continue;
                const int64_t idx = (int64_t)b * TS_N + li;
                if (!(vol.w[idx] > 0.f) || ((ta < 0.f) == (vol.t[idx] < 0.f))) continue;
                // the cubes around the edge have lower corners own - sj e_j - sk e_k (j < k: the two other axes)
                const int j = ax == 0 ? 1 : 0, k = ax == 2 ? 1 : 2;
                bool any = false;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int o[3] = {lx, ly, lz};
                    o[j] -= q & 1;
                    o[k] -= q >> 1;
                    any |= cube_valid_at(nbr, cube_case, o[0], o[1], o[2]);
                }
                if (any) f |= 1u << ax;
            }
        }
        vflags[own] = (uint8_t)f;
        vcount[own] = __popc(f);
    }
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_mc_emit_vertices_kernel(TsGrid G, const int* __restrict__ cell_block,
                                                                          const int4* __restrict__ blocks, TsVol vol,
                                                                          float voxel, const uint8_t* __restrict__ vflags,
                                                                          const uint32_t* __restrict__ voff,
                                                                          float* __restrict__ verts, float* __restrict__ cols) {
    __shared__ int nbr[27];
    const int4 bc = blocks[blockIdx.x];
    load_neighbours(G, cell_block, bc, nbr);
    const int lx = threadIdx.x & (TS_R - 1), ly = threadIdx.x / TS_R;
    for (int lz = 0; lz < TS_R; ++lz) {
        const int64_t own = (int64_t)blockIdx.x * TS_N + lx + TS_R * (ly + TS_R * lz);
        const uint32_t f = vflags[own];
        if (!f) continue;
        const float ta = fabsf(vol.t[own]);
        const float ca[3] = {vol.r[own], vol.g[own], vol.b[own]};
        const float px = ((float)(bc.x * TS_R + lx) + 0.5f) * voxel, py = ((float)(bc.y * TS_R + ly) + 0.5f) * voxel,
                    pz = ((float)(bc.z * TS_R + lz) + 0.5f) * voxel;
        uint32_t slot = voff[own];
        for (int ax = 0; ax < 3; ++ax) {
            if (!(f & (1u << ax))) continue;
            int li;
            const int b = locate(nbr, lx + (ax == 0), ly + (ax == 1), lz + (ax == 2), &li);
            const int64_t idx = (int64_t)b * TS_N + li;   // b >= 0: the flag was set only with both ends allocated
            const float tb = fabsf(vol.t[idx]);
            const float cb[3] = {vol.r[idx], vol.g[idx], vol.b[idx]};
            const float s = ta + tb, r = ta / s;
            float p[3] = {px, py, pz};
            p[ax] = p[ax] + r * voxel;
            for (int c = 0; c < 3; ++c) {
                verts[(int64_t)slot * 3 + c] = p[c];
                cols[(int64_t)slot * 3 + c] = ((tb * ca[c] + ta * cb[c]) / s) / 255.f;
            }
            ++slot;
        }
    }
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_mc_emit_triangles_kernel(TsGrid G, const int* __restrict__ cell_block,
                                                                           const int4* __restrict__ blocks,
                                                                           const int16_t* __restrict__ cube_case,
                                                                           const uint8_t* __restrict__ vflags,
                                                                           const uint32_t* __restrict__ voff,
                                                                           const uint32_t* __restrict__ toff,
                                                                           int* __restrict__ tris) {
    __shared__ int nbr[27];
    load_neighbours(G, cell_block, blocks[blockIdx.x], nbr);
    const int lx = threadIdx.x & (TS_R - 1), ly = threadIdx.x / TS_R;
    for (int lz = 0; lz < TS_R; ++lz) {
        const int64_t cube = (int64_t)blockIdx.x * TS_N + lx + TS_R * (ly + TS_R * lz);
        const int cs = cube_case[cube];
        if (cs <= 0 || cs == 255) continue;
        const uint32_t t0 = toff[cube];
        for (int n = 0; n < 5 && c_tri_table[cs][3 * n] >= 0; ++n) {
            int id[3];
            for (int c = 0; c < 3; ++c) {
                const int e = c_tri_table[cs][3 * n + c], o = c_edge_off[e], ax = c_edge_axis[e];
                int li;
                const int b = locate(nbr, lx + (o & 1), ly + ((o >> 1) & 1), lz + (o >> 2), &li);
                const int64_t idx = (int64_t)b * TS_N + li;   // every corner of a valid cube is allocated
                id[c] = (int)(voff[idx] + __popc(vflags[idx] & ((1u << ax) - 1u)));
            }
            int* t = tris + (int64_t)(t0 + n) * 3;
            t[0] = id[0];
            t[1] = id[1];
            t[2] = id[2];
        }
    }
}

// ---- connected components ----------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_find(int* parent, int x) {
    int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {   // parent[x] <= x: the chain strictly decreases
        x = p;
        p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_cc_init_kernel(int F, int* __restrict__ parent, int* __restrict__ counts) {
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i < F) {
        parent[i] = i;
        counts[i] = 0;
    }
}

// adjacent equal edge keys join their triangles: hook the larger root onto the smaller with CAS (a failed CAS means another
// thread hooked that root first; retry from the new roots)
__global__ __launch_bounds__(GDR_BLOCK) void tsdf_cc_hook_kernel(int64_t n, const int64_t* __restrict__ keys,
                                                                 const int64_t* __restrict__ tri_of, int* parent) {
    const int64_t i = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x + 1;
    if (i >= n || keys[i] != keys[i - 1]) return;
    int a = (int)tri_of[i], b = (int)tri_of[i - 1];
    while (true) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_cc_compress_kernel(int F, int* parent, uint32_t* __restrict__ is_root) {
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i >= F) return;
    const int r = cc_find(parent, i);
    parent[i] = r;
    is_root[i] = r == i;
}

__global__ __launch_bounds__(GDR_BLOCK) void tsdf_cc_label_kernel(int F, const int* __restrict__ parent,
                                                                  const uint32_t* __restrict__ root_rank,
                                                                  int* __restrict__ label, int* __restrict__ counts) {
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    const int l = i < F ? (int)root_rank[parent[i]] : -1;
    if (i < F) label[i] = l;
    // most triangles belong to one cluster: the lanes that share lane 0's label add once per wave (one address for all
    // waves otherwise serialises the atomics), the others add alone
    const int l0 = __shfl(l, 0, 64);
    const uint64_t same = __ballot(l == l0);
    if ((threadIdx.x & 63) == 0 && l0 >= 0) atomicAdd(counts + l0, (int)__popcll(same));
    if (l >= 0 && l != l0) atomicAdd(counts + l, 1);
}

}  // namespace gdr

// ---- host side -------------------------------------------------------------------------------------------------------
using namespace gdr;

namespace {

int64_t ts_cells(const gdr_tsdf_args* a) { return (int64_t)a->dims[0] * a->dims[1] * a->dims[2]; }

const char* ts_check(const gdr_tsdf_args* a, bool grid, bool blocks) {
    if (!a) return "NULL args";
    if (a->V <= 0 || a->H <= 0 || a->W <= 0 || a->stride <= 0) return "V, H, W and stride must be positive";
    if (a->words != (a->V + 31) / 32) return "words must be ceil(V / 32)";
    if ((int64_t)a->V * a->H * a->W > ((int64_t)1 << 40)) return "views too large";
    if (!(a->voxel > 0.f) || !(a->trunc > 0.f)) return "voxel and trunc must be positive";
    if (grid && (a->dims[0] <= 0 || a->dims[1] <= 0 || a->dims[2] <= 0 || ts_cells(a) > ((int64_t)1 << 31) - 1))
        return "block grid dims must be positive with fewer than 2^31 cells";
    if (blocks && (a->n_blocks <= 0 || (int64_t)a->n_blocks * TS_N > ((int64_t)1 << 31) - 1))
        return "n_blocks must be positive, with fewer than 2^31 voxels in all";
    return nullptr;
}

TsAlloc make_alloc(const gdr_tsdf_args* a) {
    TsAlloc A;
    A.V = a->V;
    A.H = a->H;
    A.W = a->W;
    A.S = a->stride;
    A.sh = (a->H + a->stride - 1) / a->stride;
    A.sw = (a->W + a->stride - 1) / a->stride;
    A.L = (float)TS_R * a->voxel;
    A.trunc = a->trunc;
    return A;
}

size_t scan_bytes(int64_t n) { return (size_t)(div_up(n, SCAN_TILE) + 1) * sizeof(uint32_t); }

// exclusive scan of data[0, n) in place, total into data[n]; scratch: scan_bytes(n)
int scan(uint32_t* data, int64_t n, uint32_t* scratch, hipStream_t st) {
    const int tiles = div_up(n, SCAN_TILE);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(tiles), dim3(GDR_BLOCK), 0, st, (const uint32_t*)data, n, scratch);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(GDR_BLOCK), 0, st, scratch, tiles, data + n);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(tiles), dim3(GDR_BLOCK), 0, st, data, n, (const uint32_t*)scratch);
    return launch_status("scan");
}

}  // namespace

extern "C" {

size_t gdr_tsdf_scan_bytes(int64_t n) { return n > 0 ? scan_bytes(n) : 0; }

int gdr_tsdf_stage(int32_t H, int32_t W, const float* depth, const int64_t* depth_strides, const void* rgb,
                   const int64_t* rgb_strides, int32_t rgb_u8, float depth_trunc, float* depth_out, uint32_t* rgb_out,
                   void* stream) {
    if (H <= 0 || W <= 0) return invalid_arg("tsdf_stage: H, W must be positive");
    if (!depth || !depth_strides || !rgb || !rgb_strides || !depth_out || !rgb_out)
        return invalid_arg("tsdf_stage: NULL argument");
    TsStage s;
    s.depth = depth;
    s.ds[0] = depth_strides[0];
    s.ds[1] = depth_strides[1];
    s.rgb = rgb;
    for (int i = 0; i < 3; ++i) s.cs[i] = rgb_strides[i];
    s.u8 = rgb_u8 != 0;
    s.depth_trunc = depth_trunc;
    hipLaunchKernelGGL(tsdf_stage_kernel, dim3(div_up((int64_t)H * W, GDR_BLOCK)), dim3(GDR_BLOCK), 0, (hipStream_t)stream, s,
                       H, W, depth_out, rgb_out);
    return launch_status("tsdf_stage_kernel");
}

int gdr_tsdf_bounds(const gdr_tsdf_args* a, const gdr_tsdf_view* views, const float* depth, int32_t* bbox, void* stream) {
    if (const char* why = ts_check(a, false, false)) return invalid_arg(why);
    if (!views || !depth || !bbox) return invalid_arg("tsdf_bounds: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const TsAlloc A = make_alloc(a);
    hipLaunchKernelGGL(tsdf_bounds_init_kernel, dim3(1), dim3(64), 0, st, bbox);
    hipLaunchKernelGGL(tsdf_bounds_kernel, dim3(div_up((int64_t)A.V * A.sh * A.sw, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, A,
                       views, depth, bbox);
    return launch_status("tsdf_bounds_kernel");
}

int gdr_tsdf_allocate(const gdr_tsdf_args* a, const gdr_tsdf_view* views, const float* depth, uint32_t* cell_mask,
                      int32_t* cell_block, uint32_t* cell_scan, void* scratch, void* stream) {
    if (const char* why = ts_check(a, true, false)) return invalid_arg(why);
    if (!views || !depth || !cell_mask || !cell_block || !cell_scan || !scratch)
        return invalid_arg("tsdf_allocate: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const TsAlloc A = make_alloc(a);
    const TsGrid G = make_grid(a);
    const int64_t cells = ts_cells(a);
    if (hipMemsetAsync(cell_mask, 0, (size_t)cells * a->words * sizeof(uint32_t), st) != hipSuccess)
        return launch_status("tsdf_allocate: clear");
    hipLaunchKernelGGL(tsdf_mark_kernel, dim3(div_up((int64_t)A.V * A.sh * A.sw, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, A, G,
                       a->words, views, depth, cell_mask);
    hipLaunchKernelGGL(tsdf_flag_cells_kernel, dim3(div_up(cells, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, cells, a->words,
                       (const uint32_t*)cell_mask, cell_scan);
    if (int rc = launch_status("tsdf_mark_kernel")) return rc;
    if (int rc = scan(cell_scan, cells, (uint32_t*)scratch, st)) return rc;
    hipLaunchKernelGGL(tsdf_cell_index_kernel, dim3(div_up(cells, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, cells, a->words,
                       (const uint32_t*)cell_mask, (const uint32_t*)cell_scan, cell_block);
    return launch_status("tsdf_cell_index_kernel");
}

int gdr_tsdf_integrate(const gdr_tsdf_args* a, const gdr_tsdf_view* views, const float* depth, const uint32_t* rgb,
                       const uint32_t* cell_mask, const int32_t* cell_block, int32_t* blocks, float* vol, void* stream) {
    if (const char* why = ts_check(a, true, true)) return invalid_arg(why);
    if (!views || !depth || !rgb || !cell_mask || !cell_block || !blocks || !vol)
        return invalid_arg("tsdf_integrate: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const TsGrid G = make_grid(a);
    const int64_t cells = ts_cells(a);
    hipLaunchKernelGGL(tsdf_block_list_kernel, dim3(div_up(cells, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, G, cells, cell_block,
                       (int4*)blocks);
    if (int rc = launch_status("tsdf_block_list_kernel")) return rc;
    const float inv_trunc = 1.f / a->trunc;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(a->n_blocks), dim3(GDR_BLOCK), 0, st, a->H, a->W, a->words, a->voxel,
                       a->trunc, inv_trunc, views, depth, rgb, (const int4*)blocks, cell_mask, make_vol(vol, a->n_blocks));
    return launch_status("tsdf_integrate_kernel");
}

int gdr_tsdf_mc_count(const gdr_tsdf_args* a, const int32_t* cell_block, const int32_t* blocks, const float* vol,
                      int16_t* cube_case, uint8_t* vflags, uint32_t* vcount, uint32_t* tcount, void* scratch, void* stream) {
    if (const char* why = ts_check(a, true, true)) return invalid_arg(why);
    if (!cell_block || !blocks || !vol || !cube_case || !vflags || !vcount || !tcount || !scratch)
        return invalid_arg("tsdf_mc_count: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const TsGrid G = make_grid(a);
    const TsVol V = make_vol((float*)vol, a->n_blocks);
    const int64_t n = (int64_t)a->n_blocks * TS_N;
    hipLaunchKernelGGL(tsdf_mc_classify_kernel, dim3(a->n_blocks), dim3(GDR_BLOCK), 0, st, G, cell_block, (const int4*)blocks,
                       V, cube_case, tcount);
    hipLaunchKernelGGL(tsdf_mc_vertex_kernel, dim3(a->n_blocks), dim3(GDR_BLOCK), 0, st, G, cell_block, (const int4*)blocks, V,
                       (const int16_t*)cube_case, vflags, vcount);
    if (int rc = launch_status("tsdf_mc_classify_kernel / tsdf_mc_vertex_kernel")) return rc;
    if (int rc = scan(vcount, n, (uint32_t*)scratch, st)) return rc;
    return scan(tcount, n, (uint32_t*)scratch, st);
}

int gdr_tsdf_mc_emit(const gdr_tsdf_args* a, const int32_t* cell_block, const int32_t* blocks, const float* vol,
                     const int16_t* cube_case, const uint8_t* vflags, const uint32_t* voff, const uint32_t* toff,
                     float* vertices, float* colors, int32_t* triangles, void* stream) {
    if (const char* why = ts_check(a, true, true)) return invalid_arg(why);
    if (!cell_block || !blocks || !vol || !cube_case || !vflags || !voff || !toff)
        return invalid_arg("tsdf_mc_emit: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const TsGrid G = make_grid(a);
    const TsVol V = make_vol((float*)vol, a->n_blocks);
    if (vertices && colors) {
        hipLaunchKernelGGL(tsdf_mc_emit_vertices_kernel, dim3(a->n_blocks), dim3(GDR_BLOCK), 0, st, G, cell_block,
                           (const int4*)blocks, V, a->voxel, vflags, voff, vertices, colors);
        if (int rc = launch_status("tsdf_mc_emit_vertices_kernel")) return rc;
    }
    if (triangles) {
        hipLaunchKernelGGL(tsdf_mc_emit_triangles_kernel, dim3(a->n_blocks), dim3(GDR_BLOCK), 0, st, G, cell_block,
                           (const int4*)blocks, cube_case, vflags, voff, toff, triangles);
        if (int rc = launch_status("tsdf_mc_emit_triangles_kernel")) return rc;
    }
    return GDR_OK;
}

int gdr_tsdf_clusters(int32_t F, const int64_t* keys, const int64_t* tri_of, int32_t* parent, uint32_t* root_rank,
                      int32_t* label, int32_t* counts, void* scratch, void* stream) {
    if (F <= 0 || (int64_t)F * 3 > ((int64_t)1 << 31) - 1) return invalid_arg("tsdf_clusters: F must be in 1 .. 2^31 / 3");
    if (!keys || !tri_of || !parent || !root_rank || !label || !counts || !scratch)
        return invalid_arg("tsdf_clusters: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)F * 3;
    hipLaunchKernelGGL(tsdf_cc_init_kernel, dim3(div_up(F, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, F, parent, counts);
    hipLaunchKernelGGL(tsdf_cc_hook_kernel, dim3(div_up(n - 1, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, n, keys, tri_of, parent);
    hipLaunchKernelGGL(tsdf_cc_compress_kernel, dim3(div_up(F, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, F, parent, root_rank);
    if (int rc = launch_status("tsdf_cc_hook_kernel")) return rc;
    if (int rc = scan(root_rank, F, (uint32_t*)scratch, st)) return rc;
    hipLaunchKernelGGL(tsdf_cc_label_kernel, dim3(div_up(F, GDR_BLOCK)), dim3(GDR_BLOCK), 0, st, F, (const int*)parent,
                       (const uint32_t*)root_rank, label, counts);
    return launch_status("tsdf_cc_label_kernel");
}

}  // extern "C"

// conv3d.hip — dense 3x3x3 convolution of channels-last volumes (gfx950), forward and the three gradients: the
// nn.Conv3d(C, C, 3, padding=1) at the tail of the reference's GroupAttBlock (lightning/network.py), whose input and result
// the fused norms of csrc/groupattn.hip keep as (B, D, H, W, C) rows.  Public ABI: include/gdr.h gdr_conv3d_*.
//
// Semantics, restated (tests/conv3d_ref.py holds the f64 statement):
//   x (B, D, H, W, Cin) rows, weight (Cout, Cin, 27) as nn.Conv3d stores it, tap k = (kd 3 + kh) 3 + kw, offset_k = (kd, kh, kw) - 1.
//   out[b, z, y, x][co] = bias[co] + addend[b, z, y, x][co] + sum_k sum_ci x[b, (z, y, x) + offset_k][ci] weight[co][ci][k],
//   a voxel outside [0, D) x [0, H) x [0, W) contributing zero (stride 1, padding 1, cross-correlation, as F.conv3d).
//   grad_x   = the same product on grad_out with the weight transposed and tap-mirrored (packed [26 - k][ci][co]); with an
//              added input the grad_out rows are that product's addend.
//   grad_weight[co][ci][k] = sum over voxels of grad_out[voxel][co] x[voxel + offset_k][ci];  grad_bias = column sums of grad_out.
//
// Structure.
//   pack: one launch rounds the parameter to the compute dtype and lays it out [tap][CB][CA], contiguous along the sum index.
//   product kernel (forward and grad_x): output-stationary implicit GEMM.  A 256-thread workgroup owns a brick of
//     4 x 4 x 8 = 128 voxels of ONE batch item times 128 output channels; every wave a 64 x 64 quarter in 4 x 4 MFMA tiles
//     (16x16x32 f16 / bf16 into f32; f32 operands through the 16x16x4 f64 form, see mma_row).  Per chunk of KC input channels (32 of 16 bits, 16 of f32: 64 bytes either
//     way) the brick is staged in LDS once with its one-voxel halo, 6 x 6 x 10 = 360 rows; the 27 taps read their fragments
//     from that image at shifted row addresses, so an input row is fetched once per workgroup and chunk.  A halo row outside
//     the volume is a zero row, decided per axis on coordinates.  The packed weight is streamed three taps (one kw line) per
//     stage.  Epilogue: bias and addend are added to the accumulator, one rounding, one packed store of 4 channels per lane
//     and tile.
//   grad_weight: a workgroup owns (tap, 64 input channels, 64 output channels, slab of voxels); it walks the slab 64 voxels
//     at a time, transposing the shifted x rows and the grad_out rows into LDS so that the voxel is the MFMA's sum index,
//     and writes a partial tile (f32; f64 for f32 operands); one fold launch adds the slabs in order, rounds once and writes
//     nn.Conv3d's layout.  No atomics.
//   grad_bias: per-block column sums in f64, then one launch adds the partials in order and rounds once.
// Tile sizes are an unmeasured choice.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "mfma_rows.h"

namespace gdr {
namespace {

constexpr int CV_BLOCK = GDR_BLOCK;
constexpr int CV_BD = GDR_CONV3D_BRICK_D, CV_BH = GDR_CONV3D_BRICK_H, CV_BW = GDR_CONV3D_BRICK_W;
constexpr int CV_TM = CV_BD * CV_BH * CV_BW;      // voxels per workgroup
constexpr int CV_TN = 128;                        // output channels per workgroup
constexpr int CV_HH = CV_BH + 2, CV_HW = CV_BW + 2;
constexpr int CV_HROWS = (CV_BD + 2) * CV_HH * CV_HW;
constexpr int CV_ROWV = 5;                        // 16-byte vectors per LDS row: 4 of data, 1 of padding
constexpr int CV_STAGE_TAPS = 3;                  // taps of weight per stage (one kw line)
constexpr int CV_TAPS = 27;
constexpr int CV_GT = 64;                         // grad_weight: channels per tile side, voxels per step
constexpr int CV_MAX_SLABS = 8;
constexpr int CV_SLAB_MIN = 4096;                 // voxels per slab below which no further slab is cut
constexpr int CV_BIAS_BLOCKS = 256;
static_assert(CV_TM == 128 && CV_BLOCK == 256, "the wave layout below is 2 x 2 quarters of a 128 x 128 tile");

// ---- pack: packed[k'][cb][ca] of the compute dtype from weight (Cout, Cin, 27) ----------------------------------------------
// forward: cb = co, ca = ci, k' = k.  mirrored: cb = ci, ca = co, k' = 26 - k.
template <int DT>
__global__ __launch_bounds__(CV_BLOCK) void conv3d_pack_kernel(const void* w, int w_dtype, void* packed_, int Cin, int Cout, int mirrored,
                                                               int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int CA = mirrored ? Cout : Cin, CB = mirrored ? Cin : Cout;
    const int ca = (int)(t % CA), cb = (int)((t / CA) % CB), kp = (int)(t / ((int64_t)CA * CB));
    const int co = mirrored ? ca : cb, ci = mirrored ? cb : ca, k = mirrored ? CV_TAPS - 1 - kp : kp;
    ((typename El<DT>::type*)packed_)[t] = down<DT>(load1(w, ((int64_t)co * Cin + ci) * CV_TAPS + k, w_dtype));
}

// ---- the product kernel ---------------------------------------------------------------------------------------------------------
struct ProdP {
    const void* a;           // (B, D, H, W, CA) dense rows
    const void* w;           // packed (27, CB, CA)
    const void* bias;        // CB values of bias_dtype, or NULL
    const void* addend;      // (B, D, H, W, CB) dense rows of the compute dtype, or NULL
    void* out;               // (B, D, H, W, CB) dense rows
    int32_t bias_dtype, D, H, W, CA, CB, nbz, nby, nbx;
};

template <int DT>
__global__ __launch_bounds__(CV_BLOCK) void conv3d_product_kernel(const ProdP p) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE, KC = El<DT>::KC;
    __shared__ uint4 sA[CV_HROWS * CV_ROWV];                           // the brick with its halo, KC channels per row
    __shared__ uint4 sW[CV_STAGE_TAPS * CV_TN * CV_ROWV];              // [tap of the stage][output channel], KC per row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    // the brick of this workgroup: coordinates, never a flattened row index
    uint32_t id = blockIdx.x;
    const int bx = id % p.nbx; id /= p.nbx;
    const int by = id % p.nby; id /= p.nby;
    const int bz = id % p.nbz;
    const int64_t b = id / p.nbz;
    const int z0 = bz * CV_BD, y0 = by * CV_BH, x0 = bx * CV_BW;
    const int col0 = blockIdx.y * CV_TN;
    const E* A = (const E*)p.a;
    const E* Wp = (const E*)p.w;

    int hb[4];        // halo row of this lane's voxel of tile i under tap (0, 0, 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = wm + 16 * i + l16;
        hb[i] = ((v / (CV_BH * CV_BW)) * CV_HH + (v / CV_BW) % CV_BH) * CV_HW + v % CV_BW;
    }
    typename El<DT>::acc acc[4][4];      // [channel tile][voxel tile]: D rows = output channels, D columns = voxels
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = typename El<DT>::acc{0, 0, 0, 0};

    for (int c0 = 0; c0 < p.CA; c0 += KC) {
        for (int v = tid; v < CV_HROWS * 4; v += CV_BLOCK) {
            const int r = v >> 2, q = v & 3, c = c0 + q * VE;
            const int z = z0 + r / (CV_HH * CV_HW) - 1, y = y0 + (r / CV_HW) % CV_HH - 1, x = x0 + r % CV_HW - 1;
            uint4 val = make_uint4(0, 0, 0, 0);
            if ((uint32_t)z < (uint32_t)p.D && (uint32_t)y < (uint32_t)p.H && (uint32_t)x < (uint32_t)p.W && c < p.CA)
                val = *reinterpret_cast<const uint4*>(A + (((b * p.D + z) * p.H + y) * p.W + x) * p.CA + c);
            sA[r * CV_ROWV + q] = val;
        }
        for (int g = 0; g < CV_TAPS / CV_STAGE_TAPS; ++g) {          // g = kd 3 + kh; the stage's taps are kw = 0, 1, 2
            for (int v = tid; v < CV_STAGE_TAPS * CV_TN * 4; v += CV_BLOCK) {
                const int t = v / (CV_TN * 4), r = (v >> 2) % CV_TN, q = v & 3, co = col0 + r, c = c0 + q * VE;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (co < p.CB && c < p.CA)
                    val = *reinterpret_cast<const uint4*>(Wp + ((int64_t)(g * CV_STAGE_TAPS + t) * p.CB + co) * p.CA + c);
                sW[(t * CV_TN + r) * CV_ROWV + q] = val;
            }
            __syncthreads();
            const int goff = ((g / 3) * CV_HH + g % 3) * CV_HW;
#pragma unroll
            for (int t = 0; t < CV_STAGE_TAPS; ++t) {
                uint4 fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fb[i] = sA[(hb[i] + goff + t) * CV_ROWV + quad];
#pragma unroll
                for (int j = 0; j < 4; ++j) fa[j] = sW[(t * CV_TN + wn + 16 * j + a_row<DT>(l16)) * CV_ROWV + quad];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) mma_row<DT>(fa[j], fb[i], acc[j][i]);
            }
            __syncthreads();
        }
    }

    // D: column = lane & 15 (voxel), rows 4 quad .. + 3 (output channels): one packed store of 4 channels per tile
    E* out = (E*)p.out;
    const E* addend = (const E*)p.addend;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = wm + 16 * i + l16;
        const int z = z0 + v / (CV_BH * CV_BW), y = y0 + (v / CV_BW) % CV_BH, x = x0 + v % CV_BW;
        if (z >= p.D || y >= p.H || x >= p.W) continue;
        const int64_t row = ((b * p.D + z) * p.H + y) * p.W + x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = col0 + wn + 16 * j + 4 * quad;
            if (co >= p.CB) continue;       // CB is a multiple of 8: the 4 channels are in or out together
            // bias and addend join the sum in the accumulator's own precision (f32; f64 for f32 operands): one rounding below
            typename El<DT>::acc sum = acc[j][i];
            if (p.bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] += up<DT>(down<DT>(load1(p.bias, co + e, p.bias_dtype)));
            }
            if (addend) {
                const E* src = addend + row * p.CB + co;
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] += up<DT>(src[e]);
            }
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = (float)sum[e];
            E* dst = out + row * p.CB + co;
            if constexpr (DT == GDR_NORM_F32) {
                *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
                const uint32_t lo = (uint32_t)down<DT>(r[0]) | ((uint32_t)down<DT>(r[1]) << 16);
                const uint32_t hi = (uint32_t)down<DT>(r[2]) | ((uint32_t)down<DT>(r[3]) << 16);
                *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
            }
        }
    }
}

// ---- grad_weight ------------------------------------------------------------------------------------------------------------------
// part[slab][k][co][ci] = sum over the slab's voxels r of g[r][co] x[r + offset_k][ci]; blockIdx = (tap, ci tile + tiles co tile, slab)
struct GwP {
    const void* x; const void* g; void* part;      // partials: f32, f64 for f32 operands
    int64_t n, slab_rows;      // voxels in all, voxels per slab (a multiple of CV_GT)
    int32_t D, H, W, CI, CO, ci_tiles;
};

template <int DT>
__global__ __launch_bounds__(CV_BLOCK) void conv3d_gw_kernel(const GwP p) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE, KC = El<DT>::KC, LDW = CV_GT + VE, VPR = CV_GT / VE;
    __shared__ __attribute__((aligned(16))) E sX[CV_GT * LDW];     // [ci][voxel]
    __shared__ __attribute__((aligned(16))) E sG[CV_GT * LDW];     // [co][voxel]
    __shared__ int64_t sSrc[CV_GT];                                // the shifted row of each voxel of the step, or -1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int k = blockIdx.x, ci0 = (blockIdx.y % p.ci_tiles) * CV_GT, co0 = (blockIdx.y / p.ci_tiles) * CV_GT;
    const int dz = k / 9 - 1, dy = (k / 3) % 3 - 1, dx = k % 3 - 1;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const E* X = (const E*)p.x;
    const E* G = (const E*)p.g;
    const int64_t r_begin = (int64_t)blockIdx.z * p.slab_rows;
    const int64_t r_end = r_begin + p.slab_rows < p.n ? r_begin + p.slab_rows : p.n;
    using Acc = typename El<DT>::acc;
    Acc acc[2][2];      // [ci tile][co tile]: D rows = input channels, D columns = output channels
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Acc{0, 0, 0, 0};
    for (int64_t r0 = r_begin; r0 < r_end; r0 += CV_GT) {
        int64_t src = -1;
        if (tid < CV_GT) {
            const int64_t r = r0 + tid;
            if (r < r_end) {
                // the voxel's coordinates; the shifted one is checked per axis, so the flat shift stays inside the batch item
                const uint32_t u = (uint32_t)r;
                const int x = u % p.W, y = (u / p.W) % p.H, z = (u / p.W / p.H) % p.D;
                const int nz = z + dz, ny = y + dy, nx = x + dx;
                if ((uint32_t)nz < (uint32_t)p.D && (uint32_t)ny < (uint32_t)p.H && (uint32_t)nx < (uint32_t)p.W)
                    src = r + ((int64_t)dz * p.H + dy) * p.W + dx;
            }
            sSrc[tid] = src;
        }
        if (!__syncthreads_or(src >= 0)) continue;      // no voxel of the step has this neighbour (uniform over the workgroup)
        for (int v = tid; v < CV_GT * VPR; v += CV_BLOCK) {
            const int r = v / VPR, cl = (v % VPR) * VE;
            const int64_t s = sSrc[r];
            union { uint4 v; E e[VE]; } ux, ug;
            ux.v = make_uint4(0, 0, 0, 0);
            ug.v = make_uint4(0, 0, 0, 0);
            if (s >= 0) {
                if (ci0 + cl < p.CI) ux.v = *reinterpret_cast<const uint4*>(X + s * p.CI + ci0 + cl);
                if (co0 + cl < p.CO) ug.v = *reinterpret_cast<const uint4*>(G + (r0 + r) * p.CO + co0 + cl);
            }
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                sX[(cl + e) * LDW + r] = ux.e[e];
                sG[(cl + e) * LDW + r] = ug.e[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < CV_GT / KC; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint4 a = *reinterpret_cast<const uint4*>(sX + (wm + 16 * i + a_row<DT>(l16)) * LDW + s * KC + quad * VE);
                    const uint4 bb = *reinterpret_cast<const uint4*>(sG + (wn + 16 * j + l16) * LDW + s * KC + quad * VE);
                    mma_row<DT>(a, bb, acc[i][j]);
                }
        __syncthreads();
    }
    // D: column = lane & 15 (co), rows 4 quad .. + 3 (ci): one vector of 4 per tile
    using P = typename std::conditional<DT == GDR_NORM_F32, double, float>::type;
    P* out = (P*)p.part + (int64_t)blockIdx.z * CV_TAPS * p.CO * p.CI;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = co0 + wn + 16 * j + l16;
        if (co >= p.CO) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ci = ci0 + wm + 16 * i + 4 * quad;
            if (ci >= p.CI) continue;
            *reinterpret_cast<Acc*>(out + ((int64_t)k * p.CO + co) * p.CI + ci) = acc[i][j];
        }
    }
}

// gw (Cout, Cin, 27) of gw_dtype = the slabs' partials added in slab order, rounded once
template <typename P>
__global__ __launch_bounds__(CV_BLOCK) void conv3d_gw_fold_kernel(const P* part, void* gw, int gw_dtype, int CI, int CO, int slabs,
                                                                  int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int ci = (int)(t % CI), co = (int)((t / CI) % CO), k = (int)(t / ((int64_t)CI * CO));
    P s = 0;
    for (int b = 0; b < slabs; ++b) s += part[(int64_t)b * total + t];
    store1(gw, ((int64_t)co * CI + ci) * CV_TAPS + k, gw_dtype, (float)s);
}

// ---- grad_bias: per-block column sums, then one launch adds the partials in order -------------------------------------------
template <int DT>
__global__ __launch_bounds__(CV_BLOCK) void conv3d_bias_part_kernel(const void* go_, double* part, int64_t n, int C) {
    const typename El<DT>::type* go = (const typename El<DT>::type*)go_;
    const int64_t rows = (n + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * rows;
    const int64_t r1 = r0 + rows < n ? r0 + rows : n;
    for (int c = threadIdx.x; c < C; c += CV_BLOCK) {
        double s = 0.0;       // (f64: the sum is rounded once, in the second launch)
        for (int64_t r = r0; r < r1; ++r) s += up<DT>(go[r * C + c]);
        part[(int64_t)blockIdx.x * C + c] = s;
    }
}

__global__ __launch_bounds__(CV_BLOCK) void conv3d_bias_sum_kernel(const double* part, void* out, int out_dtype, int blocks, int C) {
    const int c = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(int64_t)b * C + c];
    store1(out, c, out_dtype, (float)s);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
bool bad_channels(int32_t C) { return C < 8 || C > GDR_CONV3D_MAX_CHANNELS || C % 8; }

// voxels of a (B, D, H, W) volume, or -1 beyond the envelope
int64_t voxels_of(int64_t B, int32_t D, int32_t H, int32_t W) {
    const int64_t lim = (INT64_C(1) << 31) - 1;
    int64_t n = B;
    for (int32_t s : {D, H, W}) {
        if (n > lim / s) return -1;
        n *= s;
    }
    return n;
}

int slabs_of(int64_t n) { return gdr::slabs_of(n, CV_SLAB_MIN, CV_MAX_SLABS); }

int bias_blocks_of(int64_t n) {
    const int64_t b = (n + 63) / 64;
    return b < 1 ? 1 : (b > CV_BIAS_BLOCKS ? CV_BIAS_BLOCKS : (int)b);
}

#define GDR_CONV3D_DT(KERNEL, ...)                                                                       \
    do {                                                                                                 \
        if (dtype == GDR_NORM_F16) hipLaunchKernelGGL(KERNEL<GDR_NORM_F16>, __VA_ARGS__);             \
        else if (dtype == GDR_NORM_BF16) hipLaunchKernelGGL(KERNEL<GDR_NORM_BF16>, __VA_ARGS__);      \
        else hipLaunchKernelGGL(KERNEL<GDR_NORM_F32>, __VA_ARGS__);                                      \
    } while (0)

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_conv3d_workspace_bytes(int32_t what, int32_t dtype, int64_t voxels, int32_t Cin, int32_t Cout) {
    if (bad_dtype(dtype)) { invalid_arg("conv3d_workspace_bytes: unknown dtype"); return 0; }
    if (voxels < 0) { invalid_arg("conv3d_workspace_bytes: voxels must be >= 0"); return 0; }
    if (bad_channels(Cin) || bad_channels(Cout) || voxels > (INT64_C(1) << 31) - 1) {
        unsupported("conv3d_workspace_bytes: Cin and Cout must be multiples of 8 in 8..GDR_CONV3D_MAX_CHANNELS and voxels below 2^31");
        return 0;
    }
    const size_t w = (size_t)CV_TAPS * Cin * Cout;
    switch (what) {
        case GDR_CONV3D_WS_PACKED: return align_up(w * esize(dtype));
        case GDR_CONV3D_WS_GRAD_WEIGHT: return align_up((size_t)slabs_of(voxels) * w * (dtype == GDR_NORM_F32 ? sizeof(double) : sizeof(float)));
        case GDR_CONV3D_WS_GRAD_BIAS: return align_up((size_t)bias_blocks_of(voxels) * Cout * sizeof(double));
    }
    invalid_arg("conv3d_workspace_bytes: unknown workspace kind");
    return 0;
}

int gdr_conv3d_pack_weight(const void* weight, int32_t weight_dtype, int32_t Cin, int32_t Cout, int32_t mirrored, void* packed,
                           int32_t dtype, void* stream) {
    if (bad_dtype(weight_dtype) || bad_dtype(dtype)) return invalid_arg("conv3d_pack_weight: unknown dtype");
    if (bad_channels(Cin) || bad_channels(Cout))
        return unsupported("conv3d_pack_weight: Cin and Cout must be multiples of 8 in 8..GDR_CONV3D_MAX_CHANNELS");
    if (!weight || !packed) return invalid_arg("conv3d_pack_weight: NULL argument");
    if (misaligned(weight, esize(weight_dtype) - 1) || misaligned(packed, 15))
        return unsupported("conv3d_pack_weight: the weight must be aligned to its element and the packed buffer to 16 bytes");
    const int64_t total = (int64_t)CV_TAPS * Cin * Cout;
    GDR_CONV3D_DT(conv3d_pack_kernel, dim3(div_up(total, CV_BLOCK)), dim3(CV_BLOCK), 0, (hipStream_t)stream, weight, weight_dtype, packed,
                  Cin, Cout, mirrored ? 1 : 0, total);
    return launch_status("conv3d_pack_kernel");
}

int gdr_conv3d_forward(const void* x, int32_t dtype, const void* packed, const void* bias, int32_t bias_dtype, const void* addend,
                       int64_t B, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* out, void* stream) {
    if (bad_dtype(dtype) || (bias && bad_dtype(bias_dtype))) return invalid_arg("conv3d_forward: unknown dtype");
    if (B < 0 || D < 1 || H < 1 || W < 1) return invalid_arg("conv3d_forward: B must be >= 0 and D, H, W >= 1");
    if (bad_channels(Cin) || bad_channels(Cout))
        return unsupported("conv3d_forward: Cin and Cout must be multiples of 8 in 8..GDR_CONV3D_MAX_CHANNELS");
    const int64_t n = voxels_of(B, D, H, W);
    if (n < 0) return unsupported("conv3d_forward: B D H W must be below 2^31");
    if (n == 0) return GDR_OK;
    if (!x || !packed || !out) return invalid_arg("conv3d_forward: NULL argument");
    if (misaligned(x, 15) || misaligned(packed, 15) || misaligned(out, 15) || misaligned(addend, 15) ||
        misaligned(bias, esize(bias_dtype) - 1))
        return unsupported("conv3d_forward: every row buffer must start on 16 bytes");
    ProdP p = {};
    p.a = x; p.w = packed; p.bias = bias; p.addend = addend; p.out = out; p.bias_dtype = bias_dtype;
    p.D = D; p.H = H; p.W = W; p.CA = Cin; p.CB = Cout;
    p.nbz = div_up(D, CV_BD); p.nby = div_up(H, CV_BH); p.nbx = div_up(W, CV_BW);
    const int64_t bricks = B * p.nbz * p.nby * p.nbx;      // <= B D H W < 2^31
    GDR_CONV3D_DT(conv3d_product_kernel, dim3((uint32_t)bricks, div_up(Cout, CV_TN)), dim3(CV_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("conv3d_product_kernel");
}

int gdr_conv3d_grad_weight(const void* x, const void* grad_out, int32_t dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t Cin,
                           int32_t Cout, void* workspace, size_t workspace_bytes, void* grad_weight, int32_t grad_weight_dtype,
                           void* stream) {
    if (bad_dtype(dtype) || bad_dtype(grad_weight_dtype)) return invalid_arg("conv3d_grad_weight: unknown dtype");
    if (B < 0 || D < 1 || H < 1 || W < 1) return invalid_arg("conv3d_grad_weight: B must be >= 0 and D, H, W >= 1");
    if (bad_channels(Cin) || bad_channels(Cout))
        return unsupported("conv3d_grad_weight: Cin and Cout must be multiples of 8 in 8..GDR_CONV3D_MAX_CHANNELS");
    const int64_t n = voxels_of(B, D, H, W);
    if (n < 0) return unsupported("conv3d_grad_weight: B D H W must be below 2^31");
    if (!workspace || !grad_weight || (n && (!x || !grad_out))) return invalid_arg("conv3d_grad_weight: NULL argument");
    if (misaligned(x, 15) || misaligned(grad_out, 15) || misaligned(workspace, 255) ||
        misaligned(grad_weight, esize(grad_weight_dtype) - 1))
        return unsupported("conv3d_grad_weight: every row buffer must start on 16 bytes and the workspace on 256");
    if (workspace_bytes < gdr_conv3d_workspace_bytes(GDR_CONV3D_WS_GRAD_WEIGHT, dtype, n, Cin, Cout))
        return workspace_too_small("conv3d_grad_weight: workspace smaller than gdr_conv3d_workspace_bytes");
    const hipStream_t st = (hipStream_t)stream;
    const int slabs = slabs_of(n);
    GwP p = {};
    p.x = x; p.g = grad_out; p.part = workspace; p.n = n;
    p.slab_rows = (int64_t)align_up((size_t)((n + slabs - 1) / slabs), CV_GT);
    p.D = D; p.H = H; p.W = W; p.CI = Cin; p.CO = Cout; p.ci_tiles = div_up(Cin, CV_GT);
    GDR_CONV3D_DT(conv3d_gw_kernel, dim3(CV_TAPS, p.ci_tiles * div_up(Cout, CV_GT), slabs), dim3(CV_BLOCK), 0, st, p);
    if (const int rc = launch_status("conv3d_gw_kernel")) return rc;
    const int64_t total = (int64_t)CV_TAPS * Cin * Cout;
    if (dtype == GDR_NORM_F32)
        hipLaunchKernelGGL(conv3d_gw_fold_kernel<double>, dim3(div_up(total, CV_BLOCK)), dim3(CV_BLOCK), 0, st, (const double*)workspace,
                           grad_weight, grad_weight_dtype, Cin, Cout, slabs, total);
    else
        hipLaunchKernelGGL(conv3d_gw_fold_kernel<float>, dim3(div_up(total, CV_BLOCK)), dim3(CV_BLOCK), 0, st, (const float*)workspace,
                           grad_weight, grad_weight_dtype, Cin, Cout, slabs, total);
    return launch_status("conv3d_gw_fold_kernel");
}

int gdr_conv3d_grad_bias(const void* grad_out, int32_t dtype, int64_t voxels, int32_t Cout, void* workspace, size_t workspace_bytes,
                         void* grad_bias, int32_t grad_bias_dtype, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(grad_bias_dtype)) return invalid_arg("conv3d_grad_bias: unknown dtype");
    if (voxels < 0) return invalid_arg("conv3d_grad_bias: voxels must be >= 0");
    if (bad_channels(Cout) || voxels > (INT64_C(1) << 31) - 1)
        return unsupported("conv3d_grad_bias: Cout must be a multiple of 8 in 8..GDR_CONV3D_MAX_CHANNELS and voxels below 2^31");
    if (!workspace || !grad_bias || (voxels && !grad_out)) return invalid_arg("conv3d_grad_bias: NULL argument");
    if (misaligned(grad_out, 15) || misaligned(workspace, 255) || misaligned(grad_bias, esize(grad_bias_dtype) - 1))
        return unsupported("conv3d_grad_bias: grad_out must start on 16 bytes and the workspace on 256");
    if (workspace_bytes < gdr_conv3d_workspace_bytes(GDR_CONV3D_WS_GRAD_BIAS, dtype, voxels, 8, Cout))
        return workspace_too_small("conv3d_grad_bias: workspace smaller than gdr_conv3d_workspace_bytes");
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = bias_blocks_of(voxels);
    double* part = (double*)workspace;
    GDR_CONV3D_DT(conv3d_bias_part_kernel, dim3(blocks), dim3(CV_BLOCK), 0, st, grad_out, part, voxels, Cout);
    hipLaunchKernelGGL(conv3d_bias_sum_kernel, dim3(div_up(Cout, CV_BLOCK)), dim3(CV_BLOCK), 0, st, (const double*)part, grad_bias,
                       grad_bias_dtype, blocks, Cout);
    return launch_status("conv3d bias kernels");
}

}  // extern "C"

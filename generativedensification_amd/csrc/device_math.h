// device_math.h — per-Gaussian device helpers shared by preprocess.hip (3DGS path) and preprocess_surfel.hip
// (2DGS path): camera block, SH basis + gradient (expression trees identical to the oracle's), quaternion ->
// rotation, the adaptor activations that can be folded into K1/K9 with their derivatives, and the per-Gaussian
// arithmetic that K1 / K9 of both paths have in common (to_view, view_dir, sh_colour, sh_backward, tile_rect,
// quat_grad, the tile sums).  Every single-view and multi-view kernel calls these, and the path-specific helpers at
// the top of preprocess.hip (cov3d_of, project, cov2d_det, splat_radius, ndc2pix, conic_of, conic_grad_of, cov2d_grad,
// the record stores) and of preprocess_surfel.hip (surfel_normal, surfel_aabb, write_surfel_rec): an expression tree
// with ONE definition is what keeps single-view and multi-view results equal bit for bit.  (The multi-view 3DGS K9 and
// the surfel K9s kernels still write out part of their per-view chain; the comments above them say which part and why.
// Prefer helpers that return a scalar or a float3 / float4 and are called where the lines stood: those compile to the
// written-out code, helpers handing back structs or arrays have not.)  Include inside a translation unit
// compiled with -ffp-contract=off when integer intermediates must match the oracle bit for bit.
#pragma once
#include "gdr_common.h"

namespace gdr {
namespace {

#define SH_C2_0 1.0925484305920792f
#define SH_C2_1 -1.0925484305920792f
#define SH_C2_2 0.31539156525252005f
#define SH_C2_3 -1.0925484305920792f
#define SH_C2_4 0.5462742152960396f
#define SH_C3_0 -0.5900435899266435f
#define SH_C3_1 2.890611442640554f
#define SH_C3_2 -0.4570457994644658f
#define SH_C3_3 0.3731763325901154f
#define SH_C3_4 -0.4570457994644658f
#define SH_C3_5 1.445305721320277f
#define SH_C3_6 -0.5900435899266435f
#define SH_C0 0.28209479177387814f
#define SH_C1 0.4886025119029199f

struct Cam {
    float v[16];
    float p[16];
    float c[3];
};

__device__ __forceinline__ void load_cam(Cam& cam, const float* __restrict__ view,
                                         const float* __restrict__ proj,
                                         const float* __restrict__ campos) {
#pragma unroll
    for (int k = 0; k < 16; ++k) { cam.v[k] = view[k]; cam.p[k] = proj[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) cam.c[k] = campos ? campos[k] : 0.f;
}

// SH basis values b_k(x,y,z); expression trees identical to oracle sh_basis().
template <int DEG>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float* b) {
    b[0] = SH_C0;
    if (DEG >= 1) {
        b[1] = -SH_C1 * y;
        b[2] = SH_C1 * z;
        b[3] = -SH_C1 * x;
    }
    if (DEG >= 2) {
        float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = SH_C2_0 * xy;
        b[5] = SH_C2_1 * yz;
        b[6] = SH_C2_2 * (2.f * zz - xx - yy);
        b[7] = SH_C2_3 * xz;
        b[8] = SH_C2_4 * (xx - yy);
        if (DEG >= 3) {
            b[9] = SH_C3_0 * y * (3.f * xx - yy);
            b[10] = SH_C3_1 * xy * z;
            b[11] = SH_C3_2 * y * (4.f * zz - xx - yy);
            b[12] = SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy);
            b[13] = SH_C3_4 * x * (4.f * zz - xx - yy);
            b[14] = SH_C3_5 * z * (xx - yy);
            b[15] = SH_C3_6 * x * (xx - 3.f * yy);
        }
    }
}

template <int DEG>
__device__ __forceinline__ void sh_basis_grad(float x, float y, float z, float* bx, float* by,
                                              float* bz) {
    constexpr int NB = (DEG + 1) * (DEG + 1);
#pragma unroll
    for (int k = 0; k < NB; ++k) bx[k] = by[k] = bz[k] = 0.f;
    if (DEG >= 1) {
        by[1] = -SH_C1;
        bz[2] = SH_C1;
        bx[3] = -SH_C1;
    }
    if (DEG >= 2) {
        float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        bx[4] = SH_C2_0 * y; by[4] = SH_C2_0 * x;
        by[5] = SH_C2_1 * z; bz[5] = SH_C2_1 * y;
        bx[6] = SH_C2_2 * (-2.f * x); by[6] = SH_C2_2 * (-2.f * y); bz[6] = SH_C2_2 * (4.f * z);
        bx[7] = SH_C2_3 * z; bz[7] = SH_C2_3 * x;
        bx[8] = SH_C2_4 * (2.f * x); by[8] = SH_C2_4 * (-2.f * y);
        if (DEG >= 3) {
            bx[9] = SH_C3_0 * (6.f * xy); by[9] = SH_C3_0 * (3.f * xx - 3.f * yy);
            bx[10] = SH_C3_1 * yz; by[10] = SH_C3_1 * xz; bz[10] = SH_C3_1 * xy;
            bx[11] = SH_C3_2 * (-2.f * xy); by[11] = SH_C3_2 * (4.f * zz - xx - 3.f * yy); bz[11] = SH_C3_2 * (8.f * yz);
            bx[12] = SH_C3_3 * (-6.f * xz); by[12] = SH_C3_3 * (-6.f * yz); bz[12] = SH_C3_3 * (6.f * zz - 3.f * xx - 3.f * yy);
            bx[13] = SH_C3_4 * (4.f * zz - 3.f * xx - yy); by[13] = SH_C3_4 * (-2.f * xy); bz[13] = SH_C3_4 * (8.f * xz);
            bx[14] = SH_C3_5 * (2.f * xz); by[14] = SH_C3_5 * (-2.f * yz); bz[14] = SH_C3_5 * (xx - yy);
            bx[15] = SH_C3_6 * (3.f * xx - 3.f * yy); by[15] = SH_C3_6 * (-6.f * xy);
        }
    }
}

__device__ __forceinline__ void quat_to_R(float r, float x, float y, float z, float* R) {
    R[0] = 1.f - 2.f * (y * y + z * z);
    R[1] = 2.f * (x * y - r * z);
    R[2] = 2.f * (x * z + r * y);
    R[3] = 2.f * (x * y + r * z);
    R[4] = 1.f - 2.f * (x * x + z * z);
    R[5] = 2.f * (y * z - r * x);
    R[6] = 2.f * (x * z - r * y);
    R[7] = 2.f * (y * z + r * x);
    R[8] = 1.f - 2.f * (x * x + y * y);
}

// Activations of the render adaptor (lightning/renderer.py:225-230: sigmoid / exp / F.normalize),
// optionally folded into K1/K9 (gdr_inputs.flags) so the caller's raw tensors are read once.
__device__ __forceinline__ float act_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float4 act_normalize(float4 q, float* inv_norm) {
    const float n = sqrtf((q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w));
    const float inv = 1.f / fmaxf(n, 1e-12f);  // F.normalize(eps=1e-12)
    *inv_norm = inv;
    return make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
}
// their derivatives: d exp(x) = exp(x) = s, and d (q / |q|) = (I - q^ q^T) / |q| for the normalised q^ and inv_n = 1 / |q|
__device__ __forceinline__ float act_exp_grad(float d, float s) { return d * s; }
__device__ __forceinline__ float4 act_normalize_grad(float4 q, float4 d, float inv_n) {
    const float dot = (q.x * d.x + q.y * d.y) + (q.z * d.z + q.w * d.w);
    return make_float4((d.x - q.x * dot) * inv_n, (d.y - q.y * dot) * inv_n, (d.z - q.z * dot) * inv_n,
                       (d.w - q.w * dot) * inv_n);
}

// ---- per-Gaussian arithmetic of K1 / K9, defined ONCE for the single-view and the multi-view kernels of both paths ----
// Values in, values out: the kernels keep their loads and stores, and where one kernel assigns a term that another
// accumulates, the helper returns the term and the caller assigns or adds it (x = t and x += t differ in the sign of a
// zero, and a pre-summed pair of terms rounds differently from two additions onto a running sum).

// world -> view space of a mean
__device__ __forceinline__ float3 to_view(const Cam& cam, float x, float y, float z) {
    return make_float3(cam.v[0] * x + cam.v[4] * y + cam.v[8] * z + cam.v[12],
                       cam.v[1] * x + cam.v[5] * y + cam.v[9] * z + cam.v[13],
                       cam.v[2] * x + cam.v[6] * y + cam.v[10] * z + cam.v[14]);
}

// unit vector from the camera to a mean; returns 1 / distance
__device__ __forceinline__ float view_dir(const Cam& cam, float x, float y, float z, float (&u)[3]) {
    const float dx = x - cam.c[0], dy = y - cam.c[1], dz = z - cam.c[2];
    const float inv = 1.f / sqrtf((dx * dx + dy * dy) + dz * dz);
    u[0] = dx * inv; u[1] = dy * inv; u[2] = dz * inv;
    return inv;
}

// SH row -> clamped colour in direction u; returns the clamp bits (bit ch: channel ch was negative)
template <int DEG>
__device__ __forceinline__ uint32_t sh_colour(const float (&u)[3], const float (&sh)[3 * (DEG + 1) * (DEG + 1)],
                                              float (&rgb)[3]) {
    constexpr int NB = (DEG + 1) * (DEG + 1);
    float bk[NB];
    sh_basis<DEG>(u[0], u[1], u[2], bk);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = bk[0] * sh[ch];
#pragma unroll
    for (int k = 1; k < NB; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = rgb[ch] + bk[k] * sh[3 * k + ch];
    uint32_t clampbits = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        rgb[ch] = rgb[ch] + 0.5f;
        if (rgb[ch] < 0.f) clampbits |= (1u << ch);
        rgb[ch] = fmaxf(rgb[ch], 0.f);
    }
    return clampbits;
}

// SH backward of one view (A.5-iv): basis bk and clamp-masked colour gradient g (dL/dsh[k][ch] = bk[k] g[ch], which the
// caller stores or sums), and the terms dm that the direction's dependence on the mean adds to dL/dmean
template <int DEG>
__device__ __forceinline__ void sh_backward(const float (&u)[3], float inv, const float (&sh)[3 * (DEG + 1) * (DEG + 1)],
                                            float gr, float gg, float gb, uint32_t cl,
                                            float (&bk)[(DEG + 1) * (DEG + 1)], float (&g)[3], float (&dm)[3]) {
    constexpr int NB = (DEG + 1) * (DEG + 1);
    float bx[NB], by[NB], bz[NB];
    sh_basis<DEG>(u[0], u[1], u[2], bk);
    sh_basis_grad<DEG>(u[0], u[1], u[2], bx, by, bz);
    g[0] = (cl & 1u) ? 0.f : gr; g[1] = (cl & 2u) ? 0.f : gg; g[2] = (cl & 4u) ? 0.f : gb;
    float ddx = 0.f, ddy = 0.f, ddz = 0.f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float sg = sh[3 * k + ch] * g[ch];
            ddx += bx[k] * sg;
            ddy += by[k] * sg;
            ddz += bz[k] * sg;
        }
    }
    const float dot = u[0] * ddx + u[1] * ddy + u[2] * ddz;
    dm[0] = (ddx - u[0] * dot) * inv;
    dm[1] = (ddy - u[1] * dot) * inv;
    dm[2] = (ddz - u[2] * dot) * inv;
}

// tile rectangle [x, z) x [y, w) covered by the square of half-side r around (cx, cy); returns the number of tiles
__device__ __forceinline__ uint32_t tile_rect(float cx, float cy, int r, int gx, int gy, int4& rect) {
    const float rf = (float)r;
    rect.x = min(gx, max(0, (int)((cx - rf) / (float)GDR_TILE)));
    rect.y = min(gy, max(0, (int)((cy - rf) / (float)GDR_TILE)));
    rect.z = min(gx, max(0, (int)((cx + rf + (float)(GDR_TILE - 1)) / (float)GDR_TILE)));
    rect.w = min(gy, max(0, (int)((cy + rf + (float)(GDR_TILE - 1)) / (float)GDR_TILE)));
    return (uint32_t)((rect.z - rect.x) * (rect.w - rect.y));
}

// dL/dq (r, x, y, z) from dL/dR of quat_to_R
__device__ __forceinline__ float4 quat_grad(float4 q, const float (&dR)[9]) {
    const float qr = q.x, qx = q.y, qy = q.z, qz = q.w;
#define G_(r_, c_) dR[3 * (r_) + (c_)]
    float4 d;
    d.x = 2.f * (-qz * G_(0, 1) + qy * G_(0, 2) + qz * G_(1, 0) - qx * G_(1, 2) - qy * G_(2, 0) + qx * G_(2, 1));
    d.y = 2.f * (qy * G_(0, 1) + qz * G_(0, 2) + qy * G_(1, 0) - 2.f * qx * G_(1, 1) - qr * G_(1, 2) + qz * G_(2, 0) + qr * G_(2, 1) - 2.f * qx * G_(2, 2));
    d.z = 2.f * (-2.f * qy * G_(0, 0) + qx * G_(0, 1) + qr * G_(0, 2) + qx * G_(1, 0) + qz * G_(1, 2) - qr * G_(2, 0) + qz * G_(2, 1) - 2.f * qy * G_(2, 2));
    d.w = 2.f * (-2.f * qz * G_(0, 0) - qr * G_(0, 1) + qx * G_(0, 2) + qr * G_(1, 0) - 2.f * qz * G_(1, 1) + qy * G_(1, 2) + qx * G_(2, 0) + qy * G_(2, 1));
#undef G_
    return d;
}

// tiles_touched of a view: wave sum -> wsum[wave]; after a __syncthreads() ONE thread publishes the block's sum (which
// feeds the scan, K2) and takes the block's slice of the view's duplicate list
__device__ __forceinline__ void wave_tiles_sum(uint32_t tiles, uint32_t (&wsum)[GDR_BLOCK / GDR_WAVE]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tiles += __shfl_xor(tiles, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = tiles;
}
__device__ __forceinline__ void publish_block_sum(const uint32_t (&wsum)[GDR_BLOCK / GDR_WAVE],
                                                  uint32_t* block_sums, uint32_t* block_offs, uint32_t* num_rendered) {
    const uint32_t bs = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    block_sums[blockIdx.x] = bs;
    block_offs[blockIdx.x] = bs ? atomicAdd(num_rendered, bs) : 0u;
}


// ---- coalesced access to per-Gaussian rows of ROWF floats (the SH block: 3 (deg+1)^2) -------------------------
// One thread owns one Gaussian, so its row (192 bytes at degree 3) is a stride-ROWF access pattern: every wave-level
// load touches 64 different cache lines and the lines are re-fetched from L2 several times before a lane has consumed
// them (PMC on K9: 45 M L2 hits for 15 M misses).  Instead the workgroup copies its 256 consecutive rows — one
// contiguous 48 KB span — with fully coalesced float4 accesses through LDS.  Row stride in LDS = ROWF + 4 or + 8
// floats, chosen so that (stride / 4) is odd: 16-byte row reads/writes of consecutive lanes then rotate through all
// banks.
template <int ROWF>
struct RowStage {
    static constexpr int Q = ROWF / 4;                               // float4 per row
    static constexpr int STRIDE = ROWF + ((Q % 2 == 0) ? 4 : 8);     // floats
    static constexpr int LDS_FLOATS = GDR_BLOCK * STRIDE;
};

// global rows [row0, row0 + nrows) -> LDS (all GDR_BLOCK threads call it; nrows <= GDR_BLOCK)
template <int ROWF>
__device__ __forceinline__ void stage_rows_in(const float* __restrict__ g, int row0, int nrows, float* lds) {
    constexpr int Q = RowStage<ROWF>::Q, STRIDE = RowStage<ROWF>::STRIDE;
    const float4* src = reinterpret_cast<const float4*>(g + (size_t)row0 * ROWF);
    const int total = nrows * Q;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const int idx = (int)threadIdx.x + GDR_BLOCK * j;
        if (idx < total) {
            const int row = idx / Q, c = idx - row * Q;
            *reinterpret_cast<float4*>(lds + row * STRIDE + 4 * c) = src[idx];
        }
    }
}

// The same copy in two steps, for a caller that has loads of its own to issue while the rows are on their way.  As one
// step (stage_rows_in) every float4 is loaded, waited for and written inside a branch of its own before the next one is
// loaded: ROWF / 4 memory latencies in a row (12 at degree 3) at the head of every workgroup.  Here nothing is branched
// on: a thread whose float4 lies past the end of the span copies the span's last float4 again (same value to the same
// LDS address as its owner), so stage_rows_load is ROWF / 4 loads back to back and stage_rows_store waits for each only
// where it is written.  Those duplicate LDS writes are deliberate: several lanes store one value to one address, which
// the hardware serialises, and only the last workgroup of a launch has such lanes (up to ROWF / 4 redundant writes per
// lane there).  The multi-view K9 uses this pair; the multi-view K1 at degree 1, the single-view K9 and
// preprocess_surfel.hip still call stage_rows_in and should gain the same way (not done here: not measured).
template <int ROWF>
__device__ __forceinline__ void stage_rows_load(const float* __restrict__ g, int row0, int nrows,
                                                float4 (&t)[RowStage<ROWF>::Q]) {
    constexpr int Q = RowStage<ROWF>::Q;
    const float4* src = reinterpret_cast<const float4*>(g + (size_t)row0 * ROWF);
    const int last = nrows * Q - 1;
#pragma unroll
    for (int j = 0; j < Q; ++j) t[j] = src[min((int)threadIdx.x + GDR_BLOCK * j, last)];
}
template <int ROWF>
__device__ __forceinline__ void stage_rows_store(const float4 (&t)[RowStage<ROWF>::Q], int nrows, float* lds) {
    constexpr int Q = RowStage<ROWF>::Q, STRIDE = RowStage<ROWF>::STRIDE;
    const int last = nrows * Q - 1;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const int idx = min((int)threadIdx.x + GDR_BLOCK * j, last);
        const int row = idx / Q, c = idx - row * Q;
        *reinterpret_cast<float4*>(lds + row * STRIDE + 4 * c) = t[j];
    }
}

// LDS -> global rows (optionally added to what is there), same mapping
template <int ROWF>
__device__ __forceinline__ void stage_rows_out(float* __restrict__ g, int row0, int nrows, const float* lds,
                                               bool accumulate) {
    constexpr int Q = RowStage<ROWF>::Q, STRIDE = RowStage<ROWF>::STRIDE;
    float4* dst = reinterpret_cast<float4*>(g + (size_t)row0 * ROWF);
    const int total = nrows * Q;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const int idx = (int)threadIdx.x + GDR_BLOCK * j;
        if (idx < total) {
            const int row = idx / Q, c = idx - row * Q;
            float4 v = *reinterpret_cast<const float4*>(lds + row * STRIDE + 4 * c);
            if (accumulate) {
                const float4 o = dst[idx];
                v = make_float4(v.x + o.x, v.y + o.y, v.z + o.z, v.w + o.w);
            }
            dst[idx] = v;
        }
    }
}

}  // namespace
}  // namespace gdr

// preprocess.hip — per-Gaussian stages of the rasterizer for gfx950.
//   K1  preprocess forward : project, EWA 2D covariance, conic, radius, tile rect,
//                            SH -> RGB, block partial sums of tiles_touched
//   K8/K9 preprocess backward: conic/mean2D/colour/depth partials -> means3D, SH,
//                            scales, rotations (or cov3D)
//   K10 mark_visible
// Behaviour: SURVEY.md Appendix A.1 / A.5 (the un-vendored CUDA rasterizer the reference
// installs from third_party/diff-gaussian-rasterization, /root/reference/.gitmodules:1-3).
//
// This translation unit is compiled with -ffp-contract=off and IEEE divide/sqrt: every
// float operation rounds exactly once, in the order written, so that radii, tile rects,
// depth key bits and therefore the whole sorted (tile,depth) list are bit-identical to
// the CPU oracle (oracle/gdr_oracle.c, built with the same contraction setting).
// These kernels are HBM-bound (236 B read + ~90 B written per Gaussian at SH degree 3);
// the extra VALU ops from not fusing multiply-adds are hidden behind memory.
#include <stdlib.h>

#include "gdr_common.h"
#include "device_math.h"

#pragma clang fp contract(off)

namespace gdr {

namespace {

// conservative half-extent (pixels) of {alpha >= 1/255} for conic (cx,cy,cz) and opacity o:
// exact bounding box of the ellipse power >= -ln(255 o), widened by 0.2 % + 0.02 px.  K6/K7 only
// use it to skip entries that would fail the alpha test at every pixel of a 4x4 block.
__device__ __forceinline__ float2 alpha_extent(const float4 co) {
    const float t = 255.f * co.w;
    if (!(t > 1.f)) return make_float2(-1.f, -1.f);  // alpha <= o < 1/255 everywhere (also NaN)
    const float det = co.x * co.z - co.y * co.y;
    if (!(det > 0.f)) return make_float2(1e30f, 1e30f);  // degenerate: never cull
    const float tau2 = 2.f * __logf(t) / det;            // 2 ln(255 o) / det(conic)
    return make_float2(sqrtf(tau2 * co.z) * 1.002f + 0.02f, sqrtf(tau2 * co.x) * 1.002f + 0.02f);
}
__device__ __forceinline__ void write_rec(float4* __restrict__ rec, int i, float2 pxy, float depth, float4 con_o,
                                          float4 rgbd) {
    const float2 ext = alpha_extent(con_o);
    rec[4 * i + 0] = make_float4(pxy.x, pxy.y, depth, 0.f);
    rec[4 * i + 1] = con_o;
    rec[4 * i + 2] = rgbd;
    rec[4 * i + 3] = make_float4(ext.x, ext.y, 0.f, 0.f);
}

// EWA projection pieces shared by forward and backward (Appendix A.1-4).
struct Ewa {
    float tx, ty, tz, xmul, ymul;
    float A0[3], A1[3], v0[3], v1[3];
    float a, b, c;
};

__device__ __forceinline__ void ewa(const Cam& cam, float pvx, float pvy, float pvz,
                                    const float* c6, float focal_x, float focal_y, float tanx,
                                    float tany, Ewa& e) {
    const float limx = 1.3f * tanx, limy = 1.3f * tany;
    float txtz = pvx / pvz, tytz = pvy / pvz;
    e.tz = pvz;
    e.tx = fminf(limx, fmaxf(-limx, txtz)) * pvz;
    e.ty = fminf(limy, fmaxf(-limy, tytz)) * pvz;
    e.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    e.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    float J00 = focal_x / pvz, J02 = -(focal_x * e.tx) / (pvz * pvz);
    float J11 = focal_y / pvz, J12 = -(focal_y * e.ty) / (pvz * pvz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e.A0[k] = J00 * cam.v[4 * k + 0] + J02 * cam.v[4 * k + 2];
        e.A1[k] = J11 * cam.v[4 * k + 1] + J12 * cam.v[4 * k + 2];
    }
    const float S[9] = {c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        e.v0[r] = (S[3 * r] * e.A0[0] + S[3 * r + 1] * e.A0[1]) + S[3 * r + 2] * e.A0[2];
        e.v1[r] = (S[3 * r] * e.A1[0] + S[3 * r + 1] * e.A1[1]) + S[3 * r + 2] * e.A1[2];
    }
    e.a = ((e.A0[0] * e.v0[0] + e.A0[1] * e.v0[1]) + e.A0[2] * e.v0[2]) + 0.3f;
    e.b = (e.A0[0] * e.v1[0] + e.A0[1] * e.v1[1]) + e.A0[2] * e.v1[2];
    e.c = ((e.A1[0] * e.v1[0] + e.A1[1] * e.v1[1]) + e.A1[2] * e.v1[2]) + 0.3f;
}

// The rest of the 3DGS per-Gaussian arithmetic, each expression tree defined once for the single-view and the multi-view
// kernels (what the surfel path shares as well is in device_math.h).

// cov3D (upper triangle) = (R S)(R S)^T from the activated quaternion and scales
__device__ __forceinline__ void cov3d_of(float4 q, float sc0, float sc1, float sc2, float scale_modifier, float (&c6)[6]) {
    float R[9], Mm[9];
    quat_to_R(q.x, q.y, q.z, q.w, R);
    const float s[3] = {scale_modifier * sc0, scale_modifier * sc1, scale_modifier * sc2};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) Mm[r * 3 + k] = R[r * 3 + k] * s[k];
#define SIG(a_, b_) ((Mm[a_ * 3 + 0] * Mm[b_ * 3 + 0] + Mm[a_ * 3 + 1] * Mm[b_ * 3 + 1]) + Mm[a_ * 3 + 2] * Mm[b_ * 3 + 2])
    c6[0] = SIG(0, 0); c6[1] = SIG(0, 1); c6[2] = SIG(0, 2);
    c6[3] = SIG(1, 1); c6[4] = SIG(1, 2); c6[5] = SIG(2, 2);
#undef SIG
}

// homogeneous projection of a mean: clip x, clip y and 1 / (clip w + 1e-7)
__device__ __forceinline__ float3 project(const Cam& cam, float x, float y, float z) {
    const float hx = cam.p[0] * x + cam.p[4] * y + cam.p[8] * z + cam.p[12];
    const float hy = cam.p[1] * x + cam.p[5] * y + cam.p[9] * z + cam.p[13];
    const float hw = cam.p[3] * x + cam.p[7] * y + cam.p[11] * z + cam.p[15];
    return make_float3(hx, hy, 1.0f / (hw + 0.0000001f));
}

// integer radius of the 3-sigma circle around a 2D covariance (a b; b c) of determinant det (A.1-4)
__device__ __forceinline__ int splat_radius(float a, float c, float det) {
    const float mid = 0.5f * (a + c);
    const float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
    const float lambda1 = mid + disc, lambda2 = mid - disc;
    const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
    return (int)my_radius;
}
// NDC coordinate -> pixel coordinate on an axis of S pixels
__device__ __forceinline__ float ndc2pix(float v, int S) { return ((v + 1.0f) * (float)S - 1.0f) * 0.5f; }

// determinant of the 2D covariance, and its inverse matrix (the conic) from 1 / determinant
__device__ __forceinline__ float cov2d_det(const Ewa& e) { return e.a * e.c - e.b * e.b; }
__device__ __forceinline__ float3 conic_of(const Ewa& e, float det_inv) {
    return make_float3(e.c * det_inv, -e.b * det_inv, e.a * det_inv);
}
// K1 strings these together itself (project, ewa, cov2d_det, splat_radius, ndc2pix, tile_rect, conic_of), in the same
// order in the single-view and the multi-view kernel.  One helper that returned the whole splat in a struct cost the
// multi-view kernels 2 to 7 VGPRs and about 1 % of their time at degree 3; these scalar pieces compile to the code the
// written-out block did.

// dL/dconic as K7 leaves it -> true partials (the exact factors -1/2, -1, -1/2 are K9's to apply); .w (dL/ddepth) as is
__device__ __forceinline__ float4 conic_grad_of(float4 g) { return make_float4(g.x * -0.5f, -g.y, g.z * -0.5f, g.w); }
// dL/dconic -> dL/d(a, b, c) of the 2D covariance of determinant det != 0
__device__ __forceinline__ float3 cov2d_grad(float a, float b, float c, float det, float4 gconic) {
    const float d2 = 1.f / (det * det);
    return make_float3(d2 * (-c * c * gconic.x + b * c * gconic.y - b * b * gconic.z),
                       d2 * (2.f * b * c * gconic.x - (a * c + b * b) * gconic.y + 2.f * a * b * gconic.z),
                       d2 * (-b * b * gconic.x + a * b * gconic.y - a * a * gconic.z));
}

// One view's chain from the gradient record back to the covariance and the mean (A.5-i..iii).  g2: dL/dmean2D;
// gconic: dL/dconic as K7 leaves it (the exact factors -1/2, -1, -1/2 are applied here).
// has_cov is false where the 2D covariance is singular: dcov is then NOT a term (the caller leaves its own untouched).
// The mean gets two terms from here, through the EWA Jacobian and through the projected centre, which the caller assigns
// or adds ONE AFTER THE OTHER; the depth term (risk R1 switch GDR_IN_NO_DEPTH_TO_MEAN) is the caller's.
struct ConicGrad {
    bool has_cov;
    float dcov[6];
    float dmean_ewa[3], dmean_proj[3];
};
__device__ __forceinline__ void conic_backward(const Cam& cam, float x, float y, float z, const float (&c6)[6],
                                               float focal_x, float focal_y, float tanx, float tany, float4 g2,
                                               float4 gconic, ConicGrad& o) {
    gconic = conic_grad_of(gconic);
    const float3 pv = to_view(cam, x, y, z);
    Ewa e;
    ewa(cam, pv.x, pv.y, pv.z, c6, focal_x, focal_y, tanx, tany, e);
    const float det = cov2d_det(e);
    float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
    o.has_cov = det * det != 0.f;
    if (o.has_cov) {
        const float3 d = cov2d_grad(e.a, e.b, e.c, det, gconic);
        dL_da = d.x; dL_db = d.y; dL_dc = d.z;
        const float* A0 = e.A0;
        const float* A1 = e.A1;
        o.dcov[0] = A0[0] * A0[0] * dL_da + A0[0] * A1[0] * dL_db + A1[0] * A1[0] * dL_dc;
        o.dcov[3] = A0[1] * A0[1] * dL_da + A0[1] * A1[1] * dL_db + A1[1] * A1[1] * dL_dc;
        o.dcov[5] = A0[2] * A0[2] * dL_da + A0[2] * A1[2] * dL_db + A1[2] * A1[2] * dL_dc;
        o.dcov[1] = 2.f * A0[0] * A0[1] * dL_da + (A0[0] * A1[1] + A0[1] * A1[0]) * dL_db + 2.f * A1[0] * A1[1] * dL_dc;
        o.dcov[2] = 2.f * A0[0] * A0[2] * dL_da + (A0[0] * A1[2] + A0[2] * A1[0]) * dL_db + 2.f * A1[0] * A1[2] * dL_dc;
        o.dcov[4] = 2.f * A0[1] * A0[2] * dL_da + (A0[1] * A1[2] + A0[2] * A1[1]) * dL_db + 2.f * A1[1] * A1[2] * dL_dc;
    }
    float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dA0 = 2.f * dL_da * e.v0[k] + dL_db * e.v1[k];
        const float dA1 = 2.f * dL_dc * e.v1[k] + dL_db * e.v0[k];
        dJ00 += dA0 * cam.v[4 * k + 0];
        dJ02 += dA0 * cam.v[4 * k + 2];
        dJ11 += dA1 * cam.v[4 * k + 1];
        dJ12 += dA1 * cam.v[4 * k + 2];
    }
    const float tz1 = 1.f / e.tz, tz2 = tz1 * tz1, tz3 = tz2 * tz1;
    const float dtx = e.xmul * (-focal_x * tz2 * dJ02);
    const float dty = e.ymul * (-focal_y * tz2 * dJ12);
    const float dtz = -focal_x * tz2 * dJ00 - focal_y * tz2 * dJ11 +
                      (2.f * focal_x * e.tx) * tz3 * dJ02 + (2.f * focal_y * e.ty) * tz3 * dJ12;
    const float3 mh = project(cam, x, y, z);
    const float m_w = mh.z;
    const float mul1 = mh.x * m_w * m_w, mul2 = mh.y * m_w * m_w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.dmean_ewa[k] = cam.v[4 * k + 0] * dtx + cam.v[4 * k + 1] * dty + cam.v[4 * k + 2] * dtz;
        o.dmean_proj[k] = (cam.p[4 * k + 0] * m_w - cam.p[4 * k + 3] * mul1) * g2.x +
                          (cam.p[4 * k + 1] * m_w - cam.p[4 * k + 3] * mul2) * g2.y;
    }
}

// dL/dcov3D -> dL/dscale, dL/dquaternion (A.5-v), through the folded activations where flags has them (sc*: the
// activated scales, q: the normalised quaternion with inv_n = 1 / |raw q|)
__device__ __forceinline__ void cov3d_backward(float4 q, float inv_n, float sc0, float sc1, float sc2, float scale_modifier,
                                               const float (&dcov)[6], uint32_t flags, float (&dscale)[3], float4& drot) {
    float R[9];
    quat_to_R(q.x, q.y, q.z, q.w, R);
    const float s[3] = {scale_modifier * sc0, scale_modifier * sc1, scale_modifier * sc2};
    const float Gs[9] = {dcov[0], 0.5f * dcov[1], 0.5f * dcov[2], 0.5f * dcov[1], dcov[3],
                         0.5f * dcov[4], 0.5f * dcov[2], 0.5f * dcov[4], dcov[5]};
    float dR[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float ds = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int l = 0; l < 3; ++l) acc += Gs[3 * r + l] * (R[3 * l + k] * s[k]);
            const float dM = 2.f * acc;
            ds += R[3 * r + k] * dM;
            dR[3 * r + k] = s[k] * dM;
        }
        dscale[k] = scale_modifier * ds;
    }
    drot = quat_grad(q, dR);
    if (flags & GDR_IN_RAW_SCALES) {
        dscale[0] = act_exp_grad(dscale[0], sc0); dscale[1] = act_exp_grad(dscale[1], sc1); dscale[2] = act_exp_grad(dscale[2], sc2);
    }
    if (flags & GDR_IN_RAW_ROTATIONS) drot = act_normalize_grad(q, drot, inv_n);
}

// A lane's render record into its slot of the workgroup's OUT slice (REC_STRIDE floats per slot: (stride / 4) odd, so
// the 16-byte accesses of consecutive lanes rotate through the banks) ...
constexpr int REC_STRIDE = 20;
__device__ __forceinline__ void stage_rec(float* rec_out, float2 pxy, float depth, float4 con_o, float4 rgbd) {
    const float2 ext = alpha_extent(con_o);
    float* mine = rec_out + (int)threadIdx.x * REC_STRIDE;
    *reinterpret_cast<float4*>(mine) = make_float4(pxy.x, pxy.y, depth, 0.f);
    *reinterpret_cast<float4*>(mine + 4) = con_o;
    *reinterpret_cast<float4*>(mine + 8) = rgbd;
    *reinterpret_cast<float4*>(mine + 12) = make_float4(ext.x, ext.y, 0.f, 0.f);
}
// ... and the wave's 64 records (4 KB contiguous in the view's record array) out of it: four coalesced 1 KB stores per
// wave instead of 64-line-stride float4 stores per lane.  Every lane of the wave calls it, past the end of the rows too.
__device__ __forceinline__ void store_wave_recs(const float* rec_out, float4* g_rec, int N) {
    const int wave0 = (int)(threadIdx.x & ~63u), lane = (int)(threadIdx.x & 63u);
    const int first = blockIdx.x * GDR_BLOCK + wave0;          // first Gaussian of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int nrec = min(GDR_WAVE, N - first);                   // (<= 0 for a wave past the end)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = lane + GDR_WAVE * j;                       // float4 index inside the wave's 4 KB span
        const int r = q >> 2, c = q & 3;
        if (r < nrec) g_rec[4 * (size_t)first + q] = *reinterpret_cast<const float4*>(rec_out + (wave0 + r) * REC_STRIDE + 4 * c);
    }
}

// ---------------------------------------------------------------------------------
// K1
// ---------------------------------------------------------------------------------
template <int DEG>
__global__ __launch_bounds__(GDR_BLOCK) void preprocess_fwd_kernel(
    int N, int M, const float* __restrict__ means3D, const float* __restrict__ scales,
    float scale_modifier, const float* __restrict__ rotations, const float* __restrict__ opacities,
    const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ cov3D_precomp, const float* __restrict__ view,
    const float* __restrict__ proj, const float* __restrict__ campos, int W, int H, float tanx,
    float tany, float focal_x, float focal_y, int32_t* __restrict__ radii, float* __restrict__ g_depths,
    float4* __restrict__ g_rec,
    float* __restrict__ g_cov3D, int4* __restrict__ g_rect, uint32_t* __restrict__ g_tiles,
    uint8_t* __restrict__ g_clamped, uint32_t* __restrict__ block_sums, uint32_t flags,
    uint32_t* __restrict__ block_offs, uint32_t* __restrict__ num_rendered) {
    Cam cam;
    load_cam(cam, view, proj, campos);
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    const int gx = (W + GDR_TILE - 1) / GDR_TILE, gy = (H + GDR_TILE - 1) / GDR_TILE;
    __shared__ float rec_out[GDR_BLOCK * REC_STRIDE];

    uint32_t tiles = 0;
    if (i < N) {
        int rad = 0;
        float depth = 0.f;
        float2 pxy = make_float2(0.f, 0.f);
        float4 con_o = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 rgbd = make_float4(0.f, 0.f, 0.f, 0.f);
        int4 rect = make_int4(0, 0, 0, 0);
        uint32_t clampbits = 0;
        float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

        const float px_ = means3D[3 * i], py_ = means3D[3 * i + 1], pz_ = means3D[3 * i + 2];
        const float3 pv = to_view(cam, px_, py_, pz_);
        // cov3D of EVERY Gaussian, also of those this view culls: a render group's multi-view K8+K9 reads ONE view's copy
        // for all its views, and a Gaussian behind this camera's near plane may be visible to the next one
        if (cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * i + k];
        } else {
            float4 q = reinterpret_cast<const float4*>(rotations)[i];
            float sc0 = scales[3 * i], sc1 = scales[3 * i + 1], sc2 = scales[3 * i + 2];
            if (flags & GDR_IN_RAW_ROTATIONS) { float inv_n; q = act_normalize(q, &inv_n); }
            if (flags & GDR_IN_RAW_SCALES) { sc0 = expf(sc0); sc1 = expf(sc1); sc2 = expf(sc2); }
            cov3d_of(q, sc0, sc1, sc2, scale_modifier, c6);
        }
        bool ok = pv.z > 0.2f;  // near cull (A.1-1); no x/y frustum test when prefiltered=False
        if (ok) {
            const float3 ph = project(cam, px_, py_, pz_);
            const float ppx = ph.x * ph.z, ppy = ph.y * ph.z;

            Ewa e;
            ewa(cam, pv.x, pv.y, pv.z, c6, focal_x, focal_y, tanx, tany, e);
            const float det = cov2d_det(e);
            ok = det != 0.f;
            if (ok) {
                const float det_inv = 1.f / det;
                const int r_i = splat_radius(e.a, e.c, det);
                const float sx = ndc2pix(ppx, W), sy = ndc2pix(ppy, H);
                tiles = tile_rect(sx, sy, r_i, gx, gy, rect);
                ok = tiles != 0;
                if (ok) {
                    rad = r_i;
                    depth = pv.z;
                    pxy = make_float2(sx, sy);
                    const float op = (flags & GDR_IN_RAW_OPACITY) ? act_sigmoid(opacities[i]) : opacities[i];
                    const float3 conic = conic_of(e, det_inv);
                    con_o = make_float4(conic.x, conic.y, conic.z, op);
                    if (colors_precomp) {
                        rgbd.x = colors_precomp[3 * i];
                        rgbd.y = colors_precomp[3 * i + 1];
                        rgbd.z = colors_precomp[3 * i + 2];
                    } else {
                        constexpr int NB = (DEG + 1) * (DEG + 1);
                        const float* sh_g = shs + (size_t)i * M * 3;
                        float sh[NB * 3], u[3], rgb[3];
                        view_dir(cam, px_, py_, pz_, u);
#pragma unroll
                        for (int k = 0; k < NB * 3; ++k) sh[k] = sh_g[k];
                        clampbits = sh_colour<DEG>(u, sh, rgb);
                        rgbd.x = rgb[0]; rgbd.y = rgb[1]; rgbd.z = rgb[2];
                    }
                    rgbd.w = depth;
                } else {
                    rect = make_int4(0, 0, 0, 0);
                }
            }
            if (!ok) { tiles = 0; }
        }
        radii[i] = rad;
        g_depths[i] = depth;
        stage_rec(rec_out, pxy, depth, con_o, rgbd);
        if (!cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; ++k) g_cov3D[6 * i + k] = c6[k];
        }
        g_rect[i] = rect;
        g_tiles[i] = tiles;
        g_clamped[i] = (uint8_t)clampbits;
    }
    store_wave_recs(rec_out, g_rec, N);
    __shared__ uint32_t wsum[GDR_BLOCK / GDR_WAVE];
    wave_tiles_sum(tiles, wsum);
    __syncthreads();
    if (threadIdx.x == 0) publish_block_sum(wsum, block_sums, block_offs, num_rendered);
}

// ---------------------------------------------------------------------------------
// K8 + K9 fused: one pass over the Gaussians.
// grad_rec layout per Gaussian (16 floats = one 64-byte line, accumulated by K7):
//   [0..3] dL/dmean2D x, y (signed, NDC units), sum|x-term|, sum|y-term|
//   [4..6] dL/dconic.x, .y, .z (true partials)   [7] dL/ddepth
//   [8..10] dL/dcolour r, g, b                   [11] dL/dopacity     [12..15] unused
// ---------------------------------------------------------------------------------
// STAGED (shs given, M == NB, degrees 1 and 3): SH rows in / SH-gradient rows out through LDS, coalesced
// (device_math.h RowStage); one barrier after body() for every thread
template <int DEG, bool STAGED>
__global__ __launch_bounds__(GDR_BLOCK) void preprocess_bwd_kernel(
    int N, int M, const float* __restrict__ means3D, const int32_t* __restrict__ radii,
    const float* __restrict__ shs, const uint8_t* __restrict__ g_clamped,
    const float* __restrict__ scales, const float* __restrict__ rotations, float scale_modifier,
    const float* __restrict__ cov3D, int cov_precomp, int colors_precomp,
    const float* __restrict__ view, const float* __restrict__ proj,
    const float* __restrict__ campos, int W, int H, float tanx, float tany, float focal_x,
    float focal_y, const float4* __restrict__ grad_rec, float4* __restrict__ dL_dmean2D,
    float* __restrict__ dL_dopacity, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dcov3D, float* __restrict__ dL_dsh,
    float* __restrict__ dL_dcolors, float* __restrict__ dL_dscale, float4* __restrict__ dL_drot,
    const float4* __restrict__ g_rec, uint32_t flags, int accumulate) {
    Cam cam;
    load_cam(cam, view, proj, campos);
    constexpr int NB = (DEG + 1) * (DEG + 1);
    constexpr int ROWF = 3 * NB;
    using RS = RowStage<STAGED ? ROWF : 4>;
    __shared__ float lds_rows[STAGED ? RS::LDS_FLOATS : 1];
    const int row0 = blockIdx.x * GDR_BLOCK, nrows = min(GDR_BLOCK, N - row0);
    const int i = row0 + threadIdx.x;
    float* my_row = lds_rows + (STAGED ? (int)threadIdx.x * RS::STRIDE : 0);
    if (STAGED) {
        stage_rows_in<STAGED ? ROWF : 4>(shs, row0, nrows, lds_rows);
        __syncthreads();
    }
    auto zero_row = [&]() {
        if (STAGED) {
#pragma unroll
            for (int c = 0; c < ROWF / 4; ++c) *reinterpret_cast<float4*>(my_row + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto body = [&]() __attribute__((always_inline)) {
    if (i >= N) return;
    const bool vis = radii[i] > 0;
    if (accumulate && !vis) { zero_row(); return; }  // += 0 everywhere: nothing to do for a culled Gaussian
    float dmean[3] = {0.f, 0.f, 0.f};
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dscale[3] = {0.f, 0.f, 0.f};
    float4 drot = make_float4(0.f, 0.f, 0.f, 0.f);
    float* dsh = dL_dsh ? dL_dsh + (size_t)i * M * 3 : nullptr;

    if (vis) {
        const float px_ = means3D[3 * i], py_ = means3D[3 * i + 1], pz_ = means3D[3 * i + 2];
        const float4 g2 = grad_rec[4 * i];          // mean2D x, y, |x|, |y|
        const float4 gconic = grad_rec[4 * i + 1];  // conic.xyz (K7 leaves the exact factors -1/2, -1, -1/2 to us), ddepth
        const float4 gcolor = grad_rec[4 * i + 2];  // rgb, opacity
        {
            float dop = gcolor.w;
            if (flags & GDR_IN_RAW_OPACITY) {  // d sigmoid = o (1 - o), o as stored by K1
                const float o = g_rec[4 * i + 1].w;
                dop = dop * (o * (1.f - o));
            }
            if (accumulate) {
                const float4 old = dL_dmean2D[i];
                dL_dmean2D[i] = make_float4(old.x + g2.x, old.y + g2.y, old.z + g2.z, old.w + g2.w);
                dL_dopacity[i] += dop;
            } else {
                dL_dmean2D[i] = g2;
                dL_dopacity[i] = dop;
            }
        }
        float c6[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) c6[k] = cov3D[6 * i + k];

        ConicGrad cg;
        conic_backward(cam, px_, py_, pz_, c6, focal_x, focal_y, tanx, tany, g2, gconic, cg);
        if (cg.has_cov) {
#pragma unroll
            for (int k = 0; k < 6; ++k) dcov[k] = cg.dcov[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dmean[k] = cg.dmean_ewa[k];
            dmean[k] += cg.dmean_proj[k];
            if (!(flags & GDR_IN_NO_DEPTH_TO_MEAN)) dmean[k] += cam.v[4 * k + 2] * gconic.w;
        }
        if (!colors_precomp) {
            const uint32_t cl = g_clamped[i];
            const float* sh_g = shs + (size_t)i * M * 3;
            float sh[NB * 3];
            if (STAGED) {
#pragma unroll
                for (int c = 0; c < ROWF / 4; ++c) {
                    const float4 t = *reinterpret_cast<const float4*>(my_row + 4 * c);
                    sh[4 * c] = t.x; sh[4 * c + 1] = t.y; sh[4 * c + 2] = t.z; sh[4 * c + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NB * 3; ++k) sh[k] = sh_g[k];
            }
            float u[3], bk[NB], g[3], dm[3];
            const float inv = view_dir(cam, px_, py_, pz_, u);
            sh_backward<DEG>(u, inv, sh, gcolor.x, gcolor.y, gcolor.z, cl, bk, g, dm);
            // dL/dsh[k][ch] = b_k g_ch: written (or added) as whole 16-byte chunks when the SH row
            // of a Gaussian is 16-byte aligned (M*12 % 16 == 0: deg 1 and 3), else scalar
            if (STAGED) {  // the gradient row replaces the SH row this thread owns; written out coalesced after body()
#pragma unroll
                for (int c = 0; c < ROWF / 4; ++c)
                    *reinterpret_cast<float4*>(my_row + 4 * c) =
                        make_float4(bk[(4 * c) / 3] * g[(4 * c) % 3], bk[(4 * c + 1) / 3] * g[(4 * c + 1) % 3],
                                    bk[(4 * c + 2) / 3] * g[(4 * c + 2) % 3], bk[(4 * c + 3) / 3] * g[(4 * c + 3) % 3]);
            } else if ((3 * NB) % 4 == 0 && M == NB) {
                float4* d4 = reinterpret_cast<float4*>(dsh);
#pragma unroll
                for (int c = 0; c < (3 * NB) / 4; ++c) {
                    float4 v = make_float4(bk[(4 * c) / 3] * g[(4 * c) % 3], bk[(4 * c + 1) / 3] * g[(4 * c + 1) % 3],
                                           bk[(4 * c + 2) / 3] * g[(4 * c + 2) % 3], bk[(4 * c + 3) / 3] * g[(4 * c + 3) % 3]);
                    if (accumulate) {
                        const float4 o = d4[c];
                        v = make_float4(v.x + o.x, v.y + o.y, v.z + o.z, v.w + o.w);
                    }
                    d4[c] = v;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NB; ++k)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        if (accumulate) dsh[3 * k + ch] += bk[k] * g[ch];
                        else dsh[3 * k + ch] = bk[k] * g[ch];
                    }
                if (!accumulate)
                    for (int k = NB; k < M; ++k)
                        for (int ch = 0; ch < 3; ++ch) dsh[3 * k + ch] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) dmean[k] += dm[k];
        } else if (dL_dcolors) {
            if (accumulate) {
                dL_dcolors[3 * i] += gcolor.x; dL_dcolors[3 * i + 1] += gcolor.y; dL_dcolors[3 * i + 2] += gcolor.z;
            } else {
                dL_dcolors[3 * i] = gcolor.x; dL_dcolors[3 * i + 1] = gcolor.y; dL_dcolors[3 * i + 2] = gcolor.z;
            }
        }
        // cov3D -> scale / quaternion (A.5-v)
        if (!cov_precomp) {
            float4 q = reinterpret_cast<const float4*>(rotations)[i];
            float sc0 = scales[3 * i], sc1 = scales[3 * i + 1], sc2 = scales[3 * i + 2];
            float inv_n = 1.f;
            if (flags & GDR_IN_RAW_ROTATIONS) q = act_normalize(q, &inv_n);
            if (flags & GDR_IN_RAW_SCALES) { sc0 = expf(sc0); sc1 = expf(sc1); sc2 = expf(sc2); }
            cov3d_backward(q, inv_n, sc0, sc1, sc2, scale_modifier, dcov, flags, dscale, drot);
        }
    } else {
        dL_dmean2D[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        dL_dopacity[i] = 0.f;
        zero_row();
        if (dsh && !STAGED)
            for (int k = 0; k < 3 * M; ++k) dsh[k] = 0.f;
        if (colors_precomp && dL_dcolors) {
            dL_dcolors[3 * i] = 0.f; dL_dcolors[3 * i + 1] = 0.f; dL_dcolors[3 * i + 2] = 0.f;
        }
    }
    if (accumulate) {
        dL_dmeans3D[3 * i] += dmean[0];
        dL_dmeans3D[3 * i + 1] += dmean[1];
        dL_dmeans3D[3 * i + 2] += dmean[2];
        if (cov_precomp) {
            if (dL_dcov3D)
#pragma unroll
                for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] += dcov[k];
        } else {
            dL_dscale[3 * i] += dscale[0];
            dL_dscale[3 * i + 1] += dscale[1];
            dL_dscale[3 * i + 2] += dscale[2];
            const float4 old = dL_drot[i];
            dL_drot[i] = make_float4(old.x + drot.x, old.y + drot.y, old.z + drot.z, old.w + drot.w);
        }
        return;
    }
    dL_dmeans3D[3 * i] = dmean[0];
    dL_dmeans3D[3 * i + 1] = dmean[1];
    dL_dmeans3D[3 * i + 2] = dmean[2];
    if (cov_precomp) {
        if (dL_dcov3D)
#pragma unroll
            for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] = dcov[k];
    } else {
        dL_dscale[3 * i] = dscale[0];
        dL_dscale[3 * i + 1] = dscale[1];
        dL_dscale[3 * i + 2] = dscale[2];
        dL_drot[i] = drot;
    }
    };
    body();
    if (STAGED) {
        __syncthreads();
        stage_rows_out<STAGED ? ROWF : 4>(dL_dsh, row0, nrows, lds_rows, accumulate != 0);
    }
}


// =================================================================================
// Multi-view variants: the callers render V views of ONE Gaussian set back to
// back (network.py:826-838).  One thread still owns one Gaussian but loops over the views, so
// the view-independent work is done once: inputs (236 B at SH degree 3) are read once instead
// of V times, cov3D is computed/stored once, and in the backward the per-view partial
// gradients are summed in registers and every output is written once (no read-modify-write
// passes, no V-fold SH gradient traffic).
// K1: per-view arithmetic IS the single-view kernel's.  Both call the same helpers in the same
// order (cov3d_of, project, ewa, cov2d_det, splat_radius, ndc2pix, conic_of, stage_rec /
// store_wave_recs above; to_view, tile_rect, view_dir, sh_colour and the tile sums in
// device_math.h), so integer intermediates are bit-identical by construction.
// K9: shares to_view, ewa, project, conic_grad_of, cov2d_grad, view_dir, sh_backward and quat_grad
// with the single-view kernel (which reaches them through conic_backward / cov3d_backward).  The
// rest of its per-view chain (cov2D -> cov3D terms, EWA Jacobian -> mean, scale / rotation
// Jacobian, the normalisation derivative) is still written out here, expression for expression
// that of conic_backward / cov3d_backward: calling those two, or any helper that hands back an
// array, moved the register allocation of the degree-1 instantiations from 119 / 121 to 128..142
// VGPRs, over the 128 that four waves per SIMD allow (see the dispatch note in
// launch_preprocess_bwd_views); helpers that return a scalar or a float3 / float4 left it alone.
// =================================================================================
struct FwdView {
    const float* view; const float* proj; const float* campos;
    float tanx, tany, fx, fy;
    int32_t* radii; float* depths; float4* rec; int4* rect;
    uint32_t* tiles; uint8_t* clamped; uint32_t* block_sums; uint32_t* block_offs; uint32_t* num_rendered;
};
struct FwdViewsArgs { int V; FwdView v[GDR_MAX_VIEWS]; };

// STAGED (M == NB and 3 NB a multiple of 4: degrees 1 and 3; round 5): the per-Gaussian rows move through LDS with
// coalesced global accesses, as K9's do (device_math.h RowStage).  A thread owns a Gaussian, so its SH row (192 bytes at
// degree 3) and the 64-byte render record it writes per view are stride accesses: every wave-level float4 load / store touches
// 64 different cache lines.  IN: the workgroup copies its 256 consecutive SH rows (one contiguous 48 KB span) into LDS with
// lane-contiguous float4 loads, every thread takes its row into registers, and the same LDS then serves OUT: each wave
// transposes its 64 records (a contiguous 4 KB span per view) through a wave-private slice and stores them as four fully
// coalesced 1 KB float4 stores.  Arithmetic untouched: same values, same bits.
template <int DEG, bool STAGED = false>
__global__ __launch_bounds__(GDR_BLOCK) void preprocess_fwd_views_kernel(
    int N, int M, const float* __restrict__ means3D, const float* __restrict__ scales,
    float scale_modifier, const float* __restrict__ rotations, const float* __restrict__ opacities,
    const float* __restrict__ shs, int W, int H, float* __restrict__ g_cov3D, uint32_t flags,
    const FwdViewsArgs a) {
    __shared__ uint32_t wsum[GDR_MAX_VIEWS][GDR_BLOCK / GDR_WAVE];
    constexpr int NB = (DEG + 1) * (DEG + 1);
    constexpr int ROWF = 3 * NB;
    using RS = RowStage<STAGED ? ROWF : 4>;
    // IN staging only where the rows are small (degree 1: 12 floats, 20 KB per workgroup).  At degree 3 the 53 KB it takes
    // leave two workgroups per CU instead of three and K1 runs 30 % SLOWER than with the strided loads (same-box A/B,
    // profiles/r05_ab_k1_staged.txt: C4 286 -> 378 us, C2 46 -> 54 us): the OUT staging alone is kept there.
    constexpr bool STAGE_SH = STAGED && DEG == 1;
    constexpr int LDS_FLOATS = STAGED ? (STAGE_SH && RS::LDS_FLOATS > GDR_BLOCK * REC_STRIDE ? RS::LDS_FLOATS : GDR_BLOCK * REC_STRIDE) : 1;
    __shared__ float lds_rows[LDS_FLOATS];
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    const int gx = (W + GDR_TILE - 1) / GDR_TILE, gy = (H + GDR_TILE - 1) / GDR_TILE;
    const bool valid = i < N;
    float px_ = 0.f, py_ = 0.f, pz_ = 0.f, op = 0.f;
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float sh[NB * 3];
    bool sh_loaded = false;
    if (STAGE_SH) {
        const int row0 = blockIdx.x * GDR_BLOCK;
        stage_rows_in<STAGED ? ROWF : 4>(shs, row0, min(GDR_BLOCK, N - row0), lds_rows);
        __syncthreads();
        if (valid) {
            const float* my_row = lds_rows + (int)threadIdx.x * RS::STRIDE;
#pragma unroll
            for (int c = 0; c < ROWF / 4; ++c) {
                const float4 t = *reinterpret_cast<const float4*>(my_row + 4 * c);
                sh[4 * c] = t.x; sh[4 * c + 1] = t.y; sh[4 * c + 2] = t.z; sh[4 * c + 3] = t.w;
            }
        }
        sh_loaded = true;
        __syncthreads();     // the rows are in registers: the LDS is the waves' OUT slices from here on
    }
    if (valid) {
        px_ = means3D[3 * i]; py_ = means3D[3 * i + 1]; pz_ = means3D[3 * i + 2];
        op = (flags & GDR_IN_RAW_OPACITY) ? act_sigmoid(opacities[i]) : opacities[i];
        float4 q = reinterpret_cast<const float4*>(rotations)[i];
        float sc0 = scales[3 * i], sc1 = scales[3 * i + 1], sc2 = scales[3 * i + 2];
        if (flags & GDR_IN_RAW_ROTATIONS) { float inv_n; q = act_normalize(q, &inv_n); }
        if (flags & GDR_IN_RAW_SCALES) { sc0 = expf(sc0); sc1 = expf(sc1); sc2 = expf(sc2); }
        cov3d_of(q, sc0, sc1, sc2, scale_modifier, c6);
#pragma unroll
        for (int k = 0; k < 6; ++k) g_cov3D[6 * i + k] = c6[k];
    }
    for (int v = 0; v < a.V; ++v) {
        const FwdView& fv = a.v[v];
        Cam cam;
        load_cam(cam, fv.view, fv.proj, fv.campos);
        uint32_t tiles = 0;
        if (valid) {
            int rad = 0;
            float depth = 0.f;
            float2 pxy = make_float2(0.f, 0.f);
            float4 con_o = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 rgbd = make_float4(0.f, 0.f, 0.f, 0.f);
            int4 rect = make_int4(0, 0, 0, 0);
            uint32_t clampbits = 0;
            const float3 pv = to_view(cam, px_, py_, pz_);
            bool ok = pv.z > 0.2f;
            if (ok) {
                const float3 ph = project(cam, px_, py_, pz_);
                const float ppx = ph.x * ph.z, ppy = ph.y * ph.z;
                Ewa e;
                ewa(cam, pv.x, pv.y, pv.z, c6, fv.fx, fv.fy, fv.tanx, fv.tany, e);
                const float det = cov2d_det(e);
                ok = det != 0.f;
                if (ok) {
                    const float det_inv = 1.f / det;
                    const int r_i = splat_radius(e.a, e.c, det);
                    const float sx = ndc2pix(ppx, W), sy = ndc2pix(ppy, H);
                    tiles = tile_rect(sx, sy, r_i, gx, gy, rect);
                    ok = tiles != 0;
                    if (ok) {
                        rad = r_i;
                        depth = pv.z;
                        pxy = make_float2(sx, sy);
                        const float3 conic = conic_of(e, det_inv);
                        con_o = make_float4(conic.x, conic.y, conic.z, op);
                        if (!sh_loaded) {  // first view in which this Gaussian is visible
                            const float* src = shs + (size_t)i * M * 3;
                            if ((M * 3) % 4 == 0) {
#pragma unroll
                                for (int c = 0; c < (NB * 3) / 4; ++c) {
                                    const float4 t = reinterpret_cast<const float4*>(src)[c];
                                    sh[4 * c] = t.x; sh[4 * c + 1] = t.y; sh[4 * c + 2] = t.z; sh[4 * c + 3] = t.w;
                                }
#pragma unroll
                                for (int k = ((NB * 3) / 4) * 4; k < NB * 3; ++k) sh[k] = src[k];
                            } else {
#pragma unroll
                                for (int k = 0; k < NB * 3; ++k) sh[k] = src[k];
                            }
                            sh_loaded = true;
                        }
                        float u[3], rgb[3];
                        view_dir(cam, px_, py_, pz_, u);
                        clampbits = sh_colour<DEG>(u, sh, rgb);
                        rgbd = make_float4(rgb[0], rgb[1], rgb[2], depth);
                    } else {
                        rect = make_int4(0, 0, 0, 0);
                    }
                }
                if (!ok) tiles = 0;
            }
            fv.radii[i] = rad;
            fv.depths[i] = depth;
            if (!STAGED) write_rec(fv.rec, i, pxy, depth, con_o, rgbd);
            fv.rect[i] = rect;
            fv.tiles[i] = tiles;
            fv.clamped[i] = (uint8_t)clampbits;
            if (STAGED) stage_rec(lds_rows, pxy, depth, con_o, rgbd);
        }
        if (STAGED) {
            store_wave_recs(lds_rows, fv.rec, N);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();                             // the slice is free for the next view
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        wave_tiles_sum(tiles, wsum[v]);
    }
    __syncthreads();
    if ((int)threadIdx.x < a.V) {
        const FwdView& fv = a.v[threadIdx.x];
        publish_block_sum(wsum[threadIdx.x], fv.block_sums, fv.block_offs, fv.num_rendered);
    }
}

struct BwdView {
    const float* view; const float* proj; const float* campos;
    float tanx, tany, fx, fy;
    const int32_t* radii; const uint8_t* clamped; const float4* grad_rec;
};
struct BwdViewsArgs { int V; BwdView v[GDR_MAX_VIEWS]; };

// STAGED (M == NB and 3 NB a multiple of 4: degrees 1 and 3): SH rows in, SH gradient rows out through LDS with
// coalesced accesses (device_math.h RowStage)
template <int DEG, bool STAGED, bool PREFETCH = false>
__global__ __launch_bounds__(GDR_BLOCK) void preprocess_bwd_views_kernel(
    int N, int M, const float* __restrict__ means3D, const float* __restrict__ shs,
    const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ opacities, float scale_modifier, const float* __restrict__ cov3D, int W,
    int H, uint32_t flags, int accumulate, float4* __restrict__ dL_dmean2D,
    float* __restrict__ dL_dopacity, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dsh,
    float* __restrict__ dL_dscale, float4* __restrict__ dL_drot, const BwdViewsArgs a) {
    constexpr int NB = (DEG + 1) * (DEG + 1);
    constexpr int ROWF = 3 * NB;
    using RS = RowStage<STAGED ? ROWF : 4>;
    __shared__ float lds_rows[STAGED ? RS::LDS_FLOATS : 1];
    const int row0 = blockIdx.x * GDR_BLOCK;
    const int nrows = min(GDR_BLOCK, N - row0);
    const int i = row0 + threadIdx.x;
    const bool in_range = i < N;
    if (!STAGED && !in_range) return;
    // The loads that depend on no other are written in front of the first wait: the workgroup's SH rows (STAGED), this
    // Gaussian's mean and covariance and, with PREFETCH, its radius in every view.  In the gfx950 code the rows and the
    // radii are in flight together in front of the barrier (one memory latency instead of ROWF / 4 + 1); the compiler
    // sinks the mean / covariance loads behind the barrier into the in_range block, where they share a second latency with
    // the first view's record.  A lane past the end reads Gaussian N - 1 and uses nothing of it.
    const int il = min(i, N - 1);
    float4 rows_in[RowStage<STAGED ? ROWF : 4>::Q];
    if (STAGED) stage_rows_load<STAGED ? ROWF : 4>(shs, row0, nrows, rows_in);
    const float px_ = means3D[3 * il], py_ = means3D[3 * il + 1], pz_ = means3D[3 * il + 2];
    float c6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov3D[6 * il + k];
    // the view index is clamped, not branched on (a branch would make every load wait for the one before it): views
    // past V read view V - 1 again and are masked out below
    int rad_v[PREFETCH ? GDR_MAX_VIEWS : 1];
    if (PREFETCH) {
#pragma unroll
        for (int v = 0; v < GDR_MAX_VIEWS; ++v) rad_v[v] = a.v[min(v, a.V - 1)].radii[il];
    }
    if (STAGED) {
        stage_rows_store<STAGED ? ROWF : 4>(rows_in, nrows, lds_rows);
        __syncthreads();
    }
    float* my_row = lds_rows + (STAGED ? (int)threadIdx.x * RS::STRIDE : 0);
    if (in_range) {
    float dmean[3] = {0.f, 0.f, 0.f};
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 dm2 = make_float4(0.f, 0.f, 0.f, 0.f);
    float dop = 0.f;
    float dsh[NB * 3];
#pragma unroll
    for (int k = 0; k < NB * 3; ++k) dsh[k] = 0.f;
    bool any_vis = false;
    const float* sh_g = shs + (size_t)i * M * 3;
    auto sh = [&](int idx) -> float { return STAGED ? my_row[idx] : sh_g[idx]; };

    // The gradient record of view v+1 is fetched while view v is processed.  Which views see this Gaussian is known
    // before the loop (rad_v above -> vis_mask), so a view's record loads wait for nothing and the only dependent load
    // chain left in the loop is record -> arithmetic.
    uint32_t vis_mask = 0u;
    if (PREFETCH) {
#pragma unroll
        for (int v = 0; v < GDR_MAX_VIEWS; ++v)
            if (v < a.V && rad_v[v] > 0) vis_mask |= 1u << v;
    }
    float4 n_g2 = make_float4(0.f, 0.f, 0.f, 0.f), n_gconic = n_g2, n_gcolor = n_g2;
    uint32_t n_cl = 0u;
    auto fetch_view = [&](int v) __attribute__((always_inline)) {
        const BwdView& b = a.v[v];
        if ((vis_mask >> v) & 1u) {
            n_g2 = b.grad_rec[4 * i]; n_gconic = b.grad_rec[4 * i + 1]; n_gcolor = b.grad_rec[4 * i + 2];
            n_cl = b.clamped[i];
        }
    };
    if (PREFETCH) fetch_view(0);
    for (int v = 0; v < a.V; ++v) {
        const BwdView& bv = a.v[v];
        bool vis;
        float4 g2, gconic, gcolor;
        uint32_t cl_v = 0u;
        if (PREFETCH) {
            vis = (vis_mask >> v) & 1u; g2 = n_g2; gconic = n_gconic; gcolor = n_gcolor; cl_v = n_cl;
            if (v + 1 < a.V) fetch_view(v + 1);
        } else {
            vis = bv.radii[i] > 0;
        }
        if (!vis) continue;
        any_vis = true;
        Cam cam;
        load_cam(cam, bv.view, bv.proj, bv.campos);
        if (!PREFETCH) {
            g2 = bv.grad_rec[4 * i]; gconic = bv.grad_rec[4 * i + 1]; gcolor = bv.grad_rec[4 * i + 2];
            cl_v = bv.clamped[i];
        }
        gconic = conic_grad_of(gconic);
        dm2 = make_float4(dm2.x + g2.x, dm2.y + g2.y, dm2.z + g2.z, dm2.w + g2.w);
        dop += gcolor.w;
        const float3 pv = to_view(cam, px_, py_, pz_);
        Ewa e;
        ewa(cam, pv.x, pv.y, pv.z, c6, bv.fx, bv.fy, bv.tanx, bv.tany, e);
        const float ea = e.a, eb = e.b, ec = e.c;
        const float det = ea * ec - eb * eb;
        float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
        if (det * det != 0.f) {
            const float3 d = cov2d_grad(ea, eb, ec, det, gconic);
            dL_da = d.x; dL_db = d.y; dL_dc = d.z;
            const float* A0 = e.A0;
            const float* A1 = e.A1;
            dcov[0] += A0[0] * A0[0] * dL_da + A0[0] * A1[0] * dL_db + A1[0] * A1[0] * dL_dc;
            dcov[3] += A0[1] * A0[1] * dL_da + A0[1] * A1[1] * dL_db + A1[1] * A1[1] * dL_dc;
            dcov[5] += A0[2] * A0[2] * dL_da + A0[2] * A1[2] * dL_db + A1[2] * A1[2] * dL_dc;
            dcov[1] += 2.f * A0[0] * A0[1] * dL_da + (A0[0] * A1[1] + A0[1] * A1[0]) * dL_db + 2.f * A1[0] * A1[1] * dL_dc;
            dcov[2] += 2.f * A0[0] * A0[2] * dL_da + (A0[0] * A1[2] + A0[2] * A1[0]) * dL_db + 2.f * A1[0] * A1[2] * dL_dc;
            dcov[4] += 2.f * A0[1] * A0[2] * dL_da + (A0[1] * A1[2] + A0[2] * A1[1]) * dL_db + 2.f * A1[1] * A1[2] * dL_dc;
        }
        float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float dA0 = 2.f * dL_da * e.v0[k] + dL_db * e.v1[k];
            const float dA1 = 2.f * dL_dc * e.v1[k] + dL_db * e.v0[k];
            dJ00 += dA0 * cam.v[4 * k + 0];
            dJ02 += dA0 * cam.v[4 * k + 2];
            dJ11 += dA1 * cam.v[4 * k + 1];
            dJ12 += dA1 * cam.v[4 * k + 2];
        }
        const float tz1 = 1.f / e.tz, tz2 = tz1 * tz1, tz3 = tz2 * tz1;
        const float dtx = e.xmul * (-bv.fx * tz2 * dJ02);
        const float dty = e.ymul * (-bv.fy * tz2 * dJ12);
        const float dtz = -bv.fx * tz2 * dJ00 - bv.fy * tz2 * dJ11 + (2.f * bv.fx * e.tx) * tz3 * dJ02 +
                          (2.f * bv.fy * e.ty) * tz3 * dJ12;
        const float3 mh = project(cam, px_, py_, pz_);
        const float m_w = mh.z;
        const float mul1 = mh.x * m_w * m_w, mul2 = mh.y * m_w * m_w;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dmean[k] += cam.v[4 * k + 0] * dtx + cam.v[4 * k + 1] * dty + cam.v[4 * k + 2] * dtz;
            dmean[k] += (cam.p[4 * k + 0] * m_w - cam.p[4 * k + 3] * mul1) * g2.x +
                        (cam.p[4 * k + 1] * m_w - cam.p[4 * k + 3] * mul2) * g2.y;
            if (!(flags & GDR_IN_NO_DEPTH_TO_MEAN)) dmean[k] += cam.v[4 * k + 2] * gconic.w;  // risk R1 switch
        }
        {   // SH backward
            float shr[NB * 3];  // this view's copy of the SH row: 16-byte LDS reads when staged
            if (STAGED) {
#pragma unroll
                for (int c = 0; c < ROWF / 4; ++c) {
                    const float4 t = *reinterpret_cast<const float4*>(my_row + 4 * c);
                    shr[4 * c] = t.x; shr[4 * c + 1] = t.y; shr[4 * c + 2] = t.z; shr[4 * c + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NB * 3; ++k) shr[k] = sh(k);
            }
            float u[3], bk[NB], g[3], dm[3];
            const float inv = view_dir(cam, px_, py_, pz_, u);
            sh_backward<DEG>(u, inv, shr, gcolor.x, gcolor.y, gcolor.z, cl_v, bk, g, dm);
#pragma unroll
            for (int k = 0; k < NB; ++k)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dsh[3 * k + ch] += bk[k] * g[ch];
#pragma unroll
            for (int k = 0; k < 3; ++k) dmean[k] += dm[k];
        }
    }
    if (!STAGED && accumulate && !any_vis) return;
    float dscale[3] = {0.f, 0.f, 0.f};
    float4 drot = make_float4(0.f, 0.f, 0.f, 0.f);
    if (any_vis) {
        if (flags & GDR_IN_RAW_OPACITY) {
            const float o = act_sigmoid(opacities[i]);
            dop = dop * (o * (1.f - o));
        }
        float4 q = reinterpret_cast<const float4*>(rotations)[i];
        float sc0 = scales[3 * i], sc1 = scales[3 * i + 1], sc2 = scales[3 * i + 2];
        float inv_n = 1.f;
        if (flags & GDR_IN_RAW_ROTATIONS) q = act_normalize(q, &inv_n);
        if (flags & GDR_IN_RAW_SCALES) { sc0 = expf(sc0); sc1 = expf(sc1); sc2 = expf(sc2); }
        float R[9];
        quat_to_R(q.x, q.y, q.z, q.w, R);
        const float s[3] = {scale_modifier * sc0, scale_modifier * sc1, scale_modifier * sc2};
        const float Gs[9] = {dcov[0], 0.5f * dcov[1], 0.5f * dcov[2], 0.5f * dcov[1], dcov[3],
                             0.5f * dcov[4], 0.5f * dcov[2], 0.5f * dcov[4], dcov[5]};
        float dR[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float ds = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float acc = 0.f;
#pragma unroll
                for (int l = 0; l < 3; ++l) acc += Gs[3 * r + l] * (R[3 * l + k] * s[k]);
                const float dM = 2.f * acc;
                ds += R[3 * r + k] * dM;
                dR[3 * r + k] = s[k] * dM;
            }
            dscale[k] = scale_modifier * ds;
        }
        drot = quat_grad(q, dR);
        if (flags & GDR_IN_RAW_SCALES) { dscale[0] *= sc0; dscale[1] *= sc1; dscale[2] *= sc2; }
        if (flags & GDR_IN_RAW_ROTATIONS) {
            const float dot = (q.x * drot.x + q.y * drot.y) + (q.z * drot.z + q.w * drot.w);
            drot = make_float4((drot.x - q.x * dot) * inv_n, (drot.y - q.y * dot) * inv_n,
                               (drot.z - q.z * dot) * inv_n, (drot.w - q.w * dot) * inv_n);
        }
    }
    float* o_sh = dL_dsh + (size_t)i * M * 3;
    if (STAGED && accumulate && !any_vis) {
        // nothing to add for this Gaussian (zeros go through the staged SH rows below)
    } else {
    if (accumulate) {
        const float4 om = dL_dmean2D[i];
        dm2 = make_float4(dm2.x + om.x, dm2.y + om.y, dm2.z + om.z, dm2.w + om.w);
        dop += dL_dopacity[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) { dmean[k] += dL_dmeans3D[3 * i + k]; dscale[k] += dL_dscale[3 * i + k]; }
        const float4 orot = dL_drot[i];
        drot = make_float4(drot.x + orot.x, drot.y + orot.y, drot.z + orot.z, drot.w + orot.w);
    }
    dL_dmean2D[i] = dm2;
    dL_dopacity[i] = dop;
#pragma unroll
    for (int k = 0; k < 3; ++k) { dL_dmeans3D[3 * i + k] = dmean[k]; dL_dscale[3 * i + k] = dscale[k]; }
    dL_drot[i] = drot;
    }
    if (STAGED) {
        // every lane is past its last read of its SH row (it owns that row exclusively): overwrite it with the gradient
#pragma unroll
        for (int c = 0; c < ROWF / 4; ++c)
            *reinterpret_cast<float4*>(my_row + 4 * c) = make_float4(dsh[4 * c], dsh[4 * c + 1], dsh[4 * c + 2], dsh[4 * c + 3]);
    } else if ((M * 3) % 4 == 0 && M == NB) {
        float4* d4 = reinterpret_cast<float4*>(o_sh);
#pragma unroll
        for (int c = 0; c < (3 * NB) / 4; ++c) {
            float4 t = make_float4(dsh[4 * c], dsh[4 * c + 1], dsh[4 * c + 2], dsh[4 * c + 3]);
            if (accumulate) {
                const float4 o = d4[c];
                t = make_float4(t.x + o.x, t.y + o.y, t.z + o.z, t.w + o.w);
            }
            d4[c] = t;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NB * 3; ++k) {
            if (accumulate) o_sh[k] += dsh[k];
            else o_sh[k] = dsh[k];
        }
        if (!accumulate)
            for (int k = NB * 3; k < M * 3; ++k) o_sh[k] = 0.f;
    }
    }  // in_range
    if (STAGED) {
        __syncthreads();
        stage_rows_out<STAGED ? ROWF : 4>(dL_dsh, row0, nrows, lds_rows, accumulate != 0);
    }
}

__global__ __launch_bounds__(GDR_BLOCK) void mark_visible_kernel(int N, const float* __restrict__ means3D,
                                                                  const float* __restrict__ view,
                                                                  uint8_t* __restrict__ present) {
    const int i = blockIdx.x * GDR_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float z = view[2] * means3D[3 * i] + view[6] * means3D[3 * i + 1] + view[10] * means3D[3 * i + 2] + view[14];
    present[i] = z > 0.2f ? 1 : 0;
}

}  // namespace

#define LAUNCH_DEG(KID, KERNEL, deg, grid, st, ...)                                          \
    switch (deg) {                                                                          \
        case 0: GDR_LAUNCH(KID, KERNEL<0>, dim3(grid), dim3(GDR_BLOCK), st, __VA_ARGS__); break; \
        case 1: GDR_LAUNCH(KID, KERNEL<1>, dim3(grid), dim3(GDR_BLOCK), st, __VA_ARGS__); break; \
        case 2: GDR_LAUNCH(KID, KERNEL<2>, dim3(grid), dim3(GDR_BLOCK), st, __VA_ARGS__); break; \
        default: GDR_LAUNCH(KID, KERNEL<3>, dim3(grid), dim3(GDR_BLOCK), st, __VA_ARGS__); break; \
    }

hipError_t launch_preprocess_fwd(const gdr_settings* s, const gdr_inputs* in, const gdr_geom* g,
                                 int32_t* radii, hipStream_t st) {
    const int N = in->N;
    if (N == 0) return hipSuccess;
    const int W = s->image_width, H = s->image_height;
    const float focal_x = (float)W / (2.f * s->tanfovx), focal_y = (float)H / (2.f * s->tanfovy);
    const int grid = div_up(N, GDR_BLOCK);
    const int deg = in->shs ? s->sh_degree : 0;
    LAUNCH_DEG(GDR_K_PREPROCESS_FWD, preprocess_fwd_kernel, deg, grid, st, N, in->M, in->means3D, in->scales,
               s->scale_modifier, in->rotations, in->opacities, in->shs, in->colors_precomp,
               in->cov3D_precomp, s->viewmatrix, s->projmatrix, s->campos, W, H, s->tanfovx,
               s->tanfovy, focal_x, focal_y, radii, g->depths, (float4*)g->rec, g->cov3D, (int4*)g->rect,
               g->tiles_touched, g->clamped, g->block_sums, in->flags, g->block_offs, g->num_rendered);
    return hipGetLastError();
}

hipError_t launch_preprocess_bwd(const gdr_settings* s, const gdr_inputs* in, const gdr_geom* g,
                                 const int32_t* radii, const gdr_grad_outputs* go, hipStream_t st) {
    const int N = in->N;
    if (N == 0) return hipSuccess;
    const int W = s->image_width, H = s->image_height;
    const float focal_x = (float)W / (2.f * s->tanfovx), focal_y = (float)H / (2.f * s->tanfovy);
    const int grid = div_up(N, GDR_BLOCK);
    const int deg = in->shs ? s->sh_degree : 0;
    const float* cov3D = in->cov3D_precomp ? in->cov3D_precomp : g->cov3D;
#define GDR_K9(DEG_, ST_) GDR_LAUNCH(GDR_K_PREPROCESS_BWD, (preprocess_bwd_kernel<DEG_, ST_>), dim3(grid), dim3(GDR_BLOCK), st, N, in->M, in->means3D, radii, in->shs, \
               g->clamped, in->scales, in->rotations, s->scale_modifier, cov3D, \
               in->cov3D_precomp ? 1 : 0, in->colors_precomp ? 1 : 0, s->viewmatrix, \
               s->projmatrix, s->campos, W, H, s->tanfovx, s->tanfovy, focal_x, focal_y, \
               (const float4*)go->scratch, (float4*)go->dL_dmeans2D, go->dL_dopacities, go->dL_dmeans3D, \
               go->dL_dcov3D, go->dL_dshs, go->dL_dcolors, go->dL_dscales, \
               (float4*)go->dL_drotations, (const float4*)g->rec, in->flags, go->accumulate)
    {
        const int nb_ = (deg + 1) * (deg + 1);
        const bool staged = in->shs && go->dL_dshs && in->M == nb_ && (3 * nb_) % 4 == 0;
        switch (deg) {
            case 0: GDR_K9(0, false); break;
            case 1: if (staged) GDR_K9(1, true); else GDR_K9(1, false); break;
            case 2: GDR_K9(2, false); break;
            default: if (staged) GDR_K9(3, true); else GDR_K9(3, false); break;
        }
    }
#undef GDR_K9
    return hipGetLastError();
}

hipError_t launch_preprocess_fwd_views(int V, const gdr_settings* s, const gdr_inputs* in,
                                       const gdr_geom* geoms, int32_t* const* radii, hipStream_t st) {
    const int N = in->N;
    if (N == 0) return hipSuccess;
    const int W = s[0].image_width, H = s[0].image_height;
    FwdViewsArgs a;
    a.V = V;
    for (int v = 0; v < V; ++v) {
        FwdView& f = a.v[v];
        f.view = s[v].viewmatrix; f.proj = s[v].projmatrix; f.campos = s[v].campos;
        f.tanx = s[v].tanfovx; f.tany = s[v].tanfovy;
        f.fx = (float)W / (2.f * s[v].tanfovx); f.fy = (float)H / (2.f * s[v].tanfovy);
        f.radii = radii[v]; f.depths = geoms[v].depths; f.rec = (float4*)geoms[v].rec;
        f.rect = (int4*)geoms[v].rect; f.tiles = geoms[v].tiles_touched; f.clamped = geoms[v].clamped;
        f.block_sums = geoms[v].block_sums; f.block_offs = geoms[v].block_offs;
        f.num_rendered = geoms[v].num_rendered;
    }
    const int grid = div_up(N, GDR_BLOCK);
    const int deg = s[0].sh_degree, nb = (deg + 1) * (deg + 1);
    static const bool stage = getenv("GDR_K1_STAGED") ? atoi(getenv("GDR_K1_STAGED")) != 0 : true;   // (developer A/B)
    const bool staged = stage && in->M == nb && (3 * nb) % 4 == 0 && (deg == 1 || deg == 3);
#define GDR_K1V(DEG_, ST_)                                                                                              \
    GDR_LAUNCH(GDR_K_PREPROCESS_FWD, (preprocess_fwd_views_kernel<DEG_, ST_>), dim3(grid), dim3(GDR_BLOCK), st, N, in->M,    \
               in->means3D, in->scales, s[0].scale_modifier, in->rotations, in->opacities, in->shs, W, H, geoms[0].cov3D,   \
               in->flags, a)
    if (staged && deg == 3) GDR_K1V(3, true);
    else if (staged && deg == 1) GDR_K1V(1, true);
    else
        LAUNCH_DEG(GDR_K_PREPROCESS_FWD, preprocess_fwd_views_kernel, s[0].sh_degree, grid, st, N, in->M,
                   in->means3D, in->scales, s[0].scale_modifier, in->rotations, in->opacities, in->shs, W, H,
                   geoms[0].cov3D, in->flags, a);
#undef GDR_K1V
    return hipGetLastError();
}

hipError_t launch_preprocess_bwd_views(int V, const gdr_settings* s, const gdr_inputs* in,
                                       const gdr_geom* geoms, const int32_t* const* radii,
                                       float* const* grad_recs, const gdr_grad_outputs* go,
                                       hipStream_t st) {
    const int N = in->N;
    if (N == 0) return hipSuccess;
    const int W = s[0].image_width, H = s[0].image_height;
    BwdViewsArgs a;
    a.V = V;
    for (int v = 0; v < V; ++v) {
        BwdView& b = a.v[v];
        b.view = s[v].viewmatrix; b.proj = s[v].projmatrix; b.campos = s[v].campos;
        b.tanx = s[v].tanfovx; b.tany = s[v].tanfovy;
        b.fx = (float)W / (2.f * s[v].tanfovx); b.fy = (float)H / (2.f * s[v].tanfovy);
        b.radii = radii[v]; b.clamped = geoms[v].clamped; b.grad_rec = (const float4*)grad_recs[v];
    }
    const int grid = div_up(N, GDR_BLOCK);
    // record prefetch (see the kernel): degree 3 only, where K9 runs at 2 waves per SIMD and a view's record has to be on
    // its way while the view before is worked on; at degree 1 the extra registers cost a wave per SIMD (132 / 130 VGPRs
    // unstaged / staged with it against 121 / 119 without: 3 waves instead of 4; round 5 measured C3 82 -> 90 us with it)
    static const bool prefetch = getenv("GDR_K9_PREFETCH") ? atoi(getenv("GDR_K9_PREFETCH")) != 0 : true;
#define GDR_K9V(DEG_, ST_)                                                                                  \
    if (prefetch && V > 1 && DEG_ == 3)                                                                     \
        GDR_LAUNCH(GDR_K_PREPROCESS_BWD, (preprocess_bwd_views_kernel<DEG_, ST_, true>), dim3(grid), dim3(GDR_BLOCK), st, N,  \
               in->M, in->means3D, in->shs, in->scales, in->rotations, in->opacities, s[0].scale_modifier,     \
               geoms[0].cov3D, W, H, in->flags, go->accumulate, (float4*)go->dL_dmeans2D, go->dL_dopacities,   \
               go->dL_dmeans3D, go->dL_dshs, go->dL_dscales, (float4*)go->dL_drotations, a);                  \
    else                                                                                                    \
    GDR_LAUNCH(GDR_K_PREPROCESS_BWD, (preprocess_bwd_views_kernel<DEG_, ST_>), dim3(grid), dim3(GDR_BLOCK), st, N,  \
               in->M, in->means3D, in->shs, in->scales, in->rotations, in->opacities, s[0].scale_modifier,     \
               geoms[0].cov3D, W, H, in->flags, go->accumulate, (float4*)go->dL_dmeans2D, go->dL_dopacities,   \
               go->dL_dmeans3D, go->dL_dshs, go->dL_dscales, (float4*)go->dL_drotations, a)
    const int deg = s[0].sh_degree, nb = (deg + 1) * (deg + 1);
    const bool staged = in->M == nb && (3 * nb) % 4 == 0;
    switch (deg) {
        case 0: GDR_K9V(0, false); break;
        case 1: if (staged) GDR_K9V(1, true); else GDR_K9V(1, false); break;
        case 2: GDR_K9V(2, false); break;
        default: if (staged) GDR_K9V(3, true); else GDR_K9V(3, false); break;
    }
#undef GDR_K9V
    return hipGetLastError();
}

hipError_t launch_mark_visible(int N, const float* means3D, const float* view, uint8_t* present,
                               hipStream_t st) {
    if (N == 0) return hipSuccess;
    GDR_LAUNCH(GDR_K_MARK_VISIBLE, mark_visible_kernel, dim3(div_up(N, GDR_BLOCK)), dim3(GDR_BLOCK), st, N,
                       means3D, view, present);
    return hipGetLastError();
}

}  // namespace gdr

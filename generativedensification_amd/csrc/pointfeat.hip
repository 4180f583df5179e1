// pointfeat.hip — projected bilinear sampling of point and volume features (include/gdr.h gdr_point_feats_*,
// gdr_sample_views_*): what the reference computes with tensor ops between its coarse and fine render calls in
// Network.get_point_feats, and for the feature volume in Network.build_feat_vol (lightning/network.py): `projection`,
// two `cat`s, one `einsum` copy, F.grid_sample and the |depth - z| channel.
//
// Arithmetic, per view v and point p (all f32; the projection, its backward and the taps are proj_taps.h's):
//   q = R_v p + t_v (w2c[v][:3,:3], w2c[v][:3,3]);  h = K_v q;  x = h0 / h2, y = h1 / h2, z = h2.
//   The reference normalises (xy + 0.5) / (W, H) * 2 - 1 and samples with align_corners=False, which un-normalises back to
//   the pixel index (x, y): the sample is taken at (x, y) directly.  Neighbours floor(x) + {0, 1}, floor(y) + {0, 1}, weights
//   from the fractional parts, summed in grid_sample's order (y0x0, y0x1, y1x0, y1x1).  A neighbour outside [0, W) x [0, H)
//   contributes nothing and receives no gradient.
//   A (point, view) pair is degenerate when h2 == 0 or x or y is not finite or lies outside +-2^30: it samples zeros, sends no
//   gradient to the images and none to the point through x and y; the z path (|0 - z|, the z output) is unchanged.  A point
//   behind the camera (h2 < 0) is not degenerate: it projects mirrored, as upstream.
//
// point_feats: out (N, V, 8) = ref rgb, render rgb, acc, |depth sample - z|, read from the four sources where they are
//   (element strides).  Forward: one thread per (point, view) pair, two 16-byte stores.  d|.| uses sign(0) = 0.
// sample_views: out (V, C, N) and z (V, N).  Forward: lanes over points (coalesced (V, C, N) writes), blockIdx.y = view,
//   blockIdx.z = a block of PF_CHUNK channels, so a 16^3 grid with hundreds of channels still fills the chip.
// Backward (both): image gradients are float atomics (one global_atomic_add_f32 each, no return) into the caller's zero-filled
//   dense tensors, issued only for the tensors that are given.  The point gradient is summed over views (and channels) inside
//   one thread and written with plain stores: bitwise reproducible.  With the point gradient wanted a thread owns a point and
//   walks every view; sample_views without it spreads views and channel blocks over the grid like the forward.
#include "gdr_common.h"
#include "host_util.h"
#include "proj_taps.h"

namespace gdr {
namespace {

constexpr int PF_BLOCK = 256;
constexpr int PF_CHUNK = 32;          // channels per workgroup row of sample_views
// values of the four neighbours of one channel plane (zero outside); off[t] = element offset of neighbour t in the plane
__device__ __forceinline__ void gather4(const float* __restrict__ plane, const int64_t* off, const Taps& t, float* val) {
    for (int i = 0; i < 4; ++i) {
        const float v = plane[off[i]];
        val[i] = t.in[i] ? v : 0.f;
    }
}

__device__ __forceinline__ float blend4(const float* val, const Taps& t) {
    float s = val[0] * (t.wx[0] * t.wy[0]);
    s += val[1] * (t.wx[1] * t.wy[0]);
    s += val[2] * (t.wx[0] * t.wy[1]);
    s += val[3] * (t.wx[1] * t.wy[1]);
    return s;
}

// d(sample)/dx and d(sample)/dy of one channel, times its upstream gradient, added to (gx, gy)
__device__ __forceinline__ void blend4_bwd(const float* val, const Taps& t, float g, float& gx, float& gy) {
    gx += g * ((val[1] - val[0]) * t.wy[0] + (val[3] - val[2]) * t.wy[1]);
    gy += g * ((val[2] - val[0]) * t.wx[0] + (val[3] - val[1]) * t.wx[1]);
}

__device__ __forceinline__ void tap_offsets(const Taps& t, int64_t sh, int64_t sw, int64_t* off) {
    for (int i = 0; i < 4; ++i) off[i] = (int64_t)t.yc[i >> 1] * sh + (int64_t)t.xc[i & 1] * sw;
}

__device__ __forceinline__ float sign0(float a) { return a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f); }

struct FeatP {
    const float *ref, *img, *acc, *dep, *pts, *w2c, *ixt;
    int64_t ref_s[4], img_s[4], acc_s[3], dep_s[3], pts_s[2];
    int64_t N;
    int32_t V, H, W;
    float* out;              // forward: (N, V, 8)
    const float* gout;       // backward: (N, V, 8) dense
    float *g_ref, *g_img, *g_acc, *g_dep, *g_pts;   // dense, in the sources' shapes; NULL = not wanted
};

__global__ __launch_bounds__(PF_BLOCK) void point_feats_fwd_kernel(const FeatP p) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;     // pair = n * V + v
    if (i >= p.N * p.V) return;
    const int64_t n = i / p.V;
    const int v = (int)(i - n * p.V);
    const float* pt = p.pts + n * p.pts_s[0];
    const Cam cam = load_cam(p.w2c, p.ixt, v);
    const Proj pr = project(cam, pt[0], pt[p.pts_s[1]], pt[2 * p.pts_s[1]]);
    const Taps t = make_taps(pr, p.H, p.W);
    int64_t off[4];
    float val[4], o[8];
    tap_offsets(t, p.ref_s[2], p.ref_s[3], off);
    for (int c = 0; c < 3; ++c) {
        gather4(p.ref + v * p.ref_s[0] + c * p.ref_s[1], off, t, val);
        o[c] = blend4(val, t);
    }
    tap_offsets(t, p.img_s[1], p.img_s[2], off);
    for (int c = 0; c < 3; ++c) {
        gather4(p.img + v * p.img_s[0] + c * p.img_s[3], off, t, val);
        o[3 + c] = blend4(val, t);
    }
    tap_offsets(t, p.acc_s[1], p.acc_s[2], off);
    gather4(p.acc + v * p.acc_s[0], off, t, val);
    o[6] = blend4(val, t);
    tap_offsets(t, p.dep_s[1], p.dep_s[2], off);
    gather4(p.dep + v * p.dep_s[0], off, t, val);
    o[7] = fabsf(blend4(val, t) - pr.z);
    float4* dst = reinterpret_cast<float4*>(p.out + i * 8);
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
}

// add g * w[t] to the inside neighbours of one dense (H, W, step) plane
__device__ __forceinline__ void scatter4(float* plane, const Taps& t, int W, int step, float g) {
    for (int i = 0; i < 4; ++i)
        if (t.in[i]) atomicAdd(plane + ((int64_t)t.yc[i >> 1] * W + t.xc[i & 1]) * step, g * (t.wx[i & 1] * t.wy[i >> 1]));
}

__global__ __launch_bounds__(PF_BLOCK) void point_feats_bwd_kernel(const FeatP p) {
    const int64_t n = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (n >= p.N) return;
    const float* pt = p.pts + n * p.pts_s[0];
    const float px = pt[0], py = pt[p.pts_s[1]], pz = pt[2 * p.pts_s[1]];
    const int64_t HW = (int64_t)p.H * p.W;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    for (int v = 0; v < p.V; ++v) {
        const Cam cam = load_cam(p.w2c, p.ixt, v);
        const Proj pr = project(cam, px, py, pz);
        const Taps t = make_taps(pr, p.H, p.W);
        const float* g = p.gout + (n * p.V + v) * 8;
        int64_t off[4];
        float val[4];
        tap_offsets(t, p.dep_s[1], p.dep_s[2], off);
        gather4(p.dep + v * p.dep_s[0], off, t, val);
        const float gd = g[7] * sign0(blend4(val, t) - pr.z);      // gradient at the depth sample; -gd at z
        if (p.g_ref)
            for (int c = 0; c < 3; ++c) scatter4(p.g_ref + (v * 3 + c) * HW, t, p.W, 1, g[c]);
        if (p.g_img)
            for (int c = 0; c < 3; ++c) scatter4(p.g_img + v * HW * 3 + c, t, p.W, 3, g[3 + c]);
        if (p.g_acc) scatter4(p.g_acc + v * HW, t, p.W, 1, g[6]);
        if (p.g_dep) scatter4(p.g_dep + v * HW, t, p.W, 1, gd);
        if (p.g_pts) {
            float gx = 0.f, gy = 0.f;
            if (pr.ok) {
                blend4_bwd(val, t, gd, gx, gy);
                tap_offsets(t, p.ref_s[2], p.ref_s[3], off);
                for (int c = 0; c < 3; ++c) {
                    gather4(p.ref + v * p.ref_s[0] + c * p.ref_s[1], off, t, val);
                    blend4_bwd(val, t, g[c], gx, gy);
                }
                tap_offsets(t, p.img_s[1], p.img_s[2], off);
                for (int c = 0; c < 3; ++c) {
                    gather4(p.img + v * p.img_s[0] + c * p.img_s[3], off, t, val);
                    blend4_bwd(val, t, g[3 + c], gx, gy);
                }
                tap_offsets(t, p.acc_s[1], p.acc_s[2], off);
                gather4(p.acc + v * p.acc_s[0], off, t, val);
                blend4_bwd(val, t, g[6], gx, gy);
            }
            project_bwd(cam, pr, gx, gy, -gd, dx, dy, dz);
        }
    }
    if (p.g_pts) {
        p.g_pts[n * 3 + 0] = dx;
        p.g_pts[n * 3 + 1] = dy;
        p.g_pts[n * 3 + 2] = dz;
    }
}

struct ViewsP {
    const float *img, *pts, *w2c, *ixt;
    int64_t img_s[4], pts_s[2];
    int64_t N;
    int32_t V, C, H, W;
    int32_t views_per_row, chunk;    // a thread walks views [y * views_per_row, ...) and channels [z * chunk, ...)
    float *out, *z;                  // forward: (V, C, N), (V, N)
    const float *gout, *gz;          // backward: dense; gz may be NULL
    float *g_img, *g_pts;            // dense (V, C, H, W), (N, 3); NULL = not wanted
};

__global__ __launch_bounds__(PF_BLOCK) void sample_views_fwd_kernel(const ViewsP p) {
    const int64_t n = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (n >= p.N) return;
    const int v = blockIdx.y;
    const int c0 = blockIdx.z * p.chunk, c1 = min(c0 + p.chunk, p.C);
    const float* pt = p.pts + n * p.pts_s[0];
    const Cam cam = load_cam(p.w2c, p.ixt, v);
    const Proj pr = project(cam, pt[0], pt[p.pts_s[1]], pt[2 * p.pts_s[1]]);
    const Taps t = make_taps(pr, p.H, p.W);
    if (c0 == 0) p.z[(int64_t)v * p.N + n] = pr.z;
    int64_t off[4];
    tap_offsets(t, p.img_s[2], p.img_s[3], off);
    const float* plane = p.img + v * p.img_s[0] + c0 * p.img_s[1];
    float* dst = p.out + ((int64_t)v * p.C + c0) * p.N + n;
    for (int c = c0; c < c1; ++c, plane += p.img_s[1], dst += p.N) {
        float val[4];
        gather4(plane, off, t, val);
        *dst = blend4(val, t);
    }
}

__global__ __launch_bounds__(PF_BLOCK) void sample_views_bwd_kernel(const ViewsP p) {
    const int64_t n = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (n >= p.N) return;
    const int v0 = blockIdx.y * p.views_per_row, v1 = min(v0 + p.views_per_row, p.V);
    const int c0 = blockIdx.z * p.chunk, c1 = min(c0 + p.chunk, p.C);
    const float* pt = p.pts + n * p.pts_s[0];
    const float px = pt[0], py = pt[p.pts_s[1]], pz = pt[2 * p.pts_s[1]];
    const int64_t HW = (int64_t)p.H * p.W;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    for (int v = v0; v < v1; ++v) {
        const Cam cam = load_cam(p.w2c, p.ixt, v);
        const Proj pr = project(cam, px, py, pz);
        const Taps t = make_taps(pr, p.H, p.W);
        float gx = 0.f, gy = 0.f;
        if (pr.ok) {
            int64_t off[4];
            tap_offsets(t, p.img_s[2], p.img_s[3], off);
            const float* plane = p.img + v * p.img_s[0] + c0 * p.img_s[1];
            const float* g = p.gout + ((int64_t)v * p.C + c0) * p.N + n;
            float* gplane = p.g_img ? p.g_img + ((int64_t)v * p.C + c0) * HW : nullptr;
            for (int c = c0; c < c1; ++c, plane += p.img_s[1], g += p.N) {
                const float gc = *g;
                if (gplane) { scatter4(gplane, t, p.W, 1, gc); gplane += HW; }
                if (p.g_pts) {
                    float val[4];
                    gather4(plane, off, t, val);
                    blend4_bwd(val, t, gc, gx, gy);
                }
            }
        }
        if (p.g_pts) project_bwd(cam, pr, gx, gy, p.gz ? p.gz[(int64_t)v * p.N + n] : 0.f, dx, dy, dz);
    }
    if (p.g_pts) {
        p.g_pts[n * 3 + 0] = dx;
        p.g_pts[n * 3 + 1] = dy;
        p.g_pts[n * 3 + 2] = dz;
    }
}

const char* pf_check(const gdr_pointfeat_args* a, bool channels) {
    if (!a) return "pointfeat: NULL args";
    if (a->N < 0 || a->N > GDR_PF_MAX_POINTS) return "pointfeat: N must be in 0..2^31-1";
    if (a->V < 1 || a->V > GDR_PF_MAX_VIEWS) return "pointfeat: V must be in 1..GDR_PF_MAX_VIEWS";
    if (a->H < 1 || a->H > GDR_PF_MAX_SIDE || a->W < 1 || a->W > GDR_PF_MAX_SIDE) return "pointfeat: H, W must be in 1..GDR_PF_MAX_SIDE";
    if (channels && (a->C < 1 || a->C > GDR_PF_MAX_CHANNELS)) return "pointfeat: C must be in 1..GDR_PF_MAX_CHANNELS";
    return nullptr;
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_point_feats_forward(const gdr_pointfeat_args* a, const float* img_ref, const int64_t* img_ref_strides, const float* image,
                            const int64_t* image_strides, const float* acc_map, const int64_t* acc_map_strides,
                            const float* depth, const int64_t* depth_strides, const float* points, const int64_t* points_strides,
                            const float* w2cs, const float* ixts, float* out, void* stream) {
    if (const char* why = pf_check(a, false)) return invalid_arg(why);
    if (!img_ref_strides || !image_strides || !acc_map_strides || !depth_strides || !points_strides)
        return invalid_arg("point_feats_forward: NULL strides");
    if (a->N == 0) return GDR_OK;
    if (!img_ref || !image || !acc_map || !depth || !points || !w2cs || !ixts || !out)
        return invalid_arg("point_feats_forward: NULL argument");
    if (misaligned(img_ref, 3) || misaligned(image, 3) || misaligned(acc_map, 3) || misaligned(depth, 3) || misaligned(points, 3) ||
        misaligned(w2cs, 3) || misaligned(ixts, 3) || misaligned(out, 15))
        return invalid_arg("point_feats_forward: unaligned buffer (out needs 16 bytes)");
    FeatP p = {};
    p.ref = img_ref; p.img = image; p.acc = acc_map; p.dep = depth; p.pts = points; p.w2c = w2cs; p.ixt = ixts; p.out = out;
    for (int i = 0; i < 4; ++i) { p.ref_s[i] = img_ref_strides[i]; p.img_s[i] = image_strides[i]; }
    for (int i = 0; i < 3; ++i) { p.acc_s[i] = acc_map_strides[i]; p.dep_s[i] = depth_strides[i]; }
    p.pts_s[0] = points_strides[0]; p.pts_s[1] = points_strides[1];
    p.N = a->N; p.V = a->V; p.H = a->H; p.W = a->W;
    hipLaunchKernelGGL(point_feats_fwd_kernel, dim3(div_up(a->N * a->V, PF_BLOCK)), dim3(PF_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("point_feats_fwd_kernel");
}

int gdr_point_feats_backward(const gdr_pointfeat_args* a, const float* grad_out, const float* img_ref,
                             const int64_t* img_ref_strides, const float* image, const int64_t* image_strides,
                             const float* acc_map, const int64_t* acc_map_strides, const float* depth,
                             const int64_t* depth_strides, const float* points, const int64_t* points_strides, const float* w2cs,
                             const float* ixts, float* grad_img_ref, float* grad_image, float* grad_acc_map, float* grad_depth,
                             float* grad_points, void* stream) {
    if (const char* why = pf_check(a, false)) return invalid_arg(why);
    if (!img_ref_strides || !image_strides || !acc_map_strides || !depth_strides || !points_strides)
        return invalid_arg("point_feats_backward: NULL strides");
    if (a->N == 0) return GDR_OK;
    if (!grad_img_ref && !grad_image && !grad_acc_map && !grad_depth && !grad_points) return GDR_OK;   // nothing is wanted
    if (!grad_out || !depth || !points || !w2cs || !ixts) return invalid_arg("point_feats_backward: NULL argument");
    if (grad_points && (!img_ref || !image || !acc_map))
        return invalid_arg("point_feats_backward: the point gradient reads every source");
    if (misaligned(grad_out, 3) || misaligned(img_ref, 3) || misaligned(image, 3) || misaligned(acc_map, 3) || misaligned(depth, 3) ||
        misaligned(points, 3) || misaligned(w2cs, 3) || misaligned(ixts, 3) || misaligned(grad_img_ref, 3) ||
        misaligned(grad_image, 3) || misaligned(grad_acc_map, 3) || misaligned(grad_depth, 3) || misaligned(grad_points, 3))
        return invalid_arg("point_feats_backward: unaligned buffer");
    FeatP p = {};
    p.ref = img_ref; p.img = image; p.acc = acc_map; p.dep = depth; p.pts = points; p.w2c = w2cs; p.ixt = ixts; p.gout = grad_out;
    p.g_ref = grad_img_ref; p.g_img = grad_image; p.g_acc = grad_acc_map; p.g_dep = grad_depth; p.g_pts = grad_points;
    for (int i = 0; i < 4; ++i) { p.ref_s[i] = img_ref_strides[i]; p.img_s[i] = image_strides[i]; }
    for (int i = 0; i < 3; ++i) { p.acc_s[i] = acc_map_strides[i]; p.dep_s[i] = depth_strides[i]; }
    p.pts_s[0] = points_strides[0]; p.pts_s[1] = points_strides[1];
    p.N = a->N; p.V = a->V; p.H = a->H; p.W = a->W;
    hipLaunchKernelGGL(point_feats_bwd_kernel, dim3(div_up(a->N, PF_BLOCK)), dim3(PF_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("point_feats_bwd_kernel");
}

int gdr_sample_views_forward(const gdr_pointfeat_args* a, const float* images, const int64_t* images_strides, const float* points,
                             const int64_t* points_strides, const float* w2cs, const float* ixts, float* out, float* z,
                             void* stream) {
    if (const char* why = pf_check(a, true)) return invalid_arg(why);
    if (!images_strides || !points_strides) return invalid_arg("sample_views_forward: NULL strides");
    if (a->N == 0) return GDR_OK;
    if (!images || !points || !w2cs || !ixts || !out || !z) return invalid_arg("sample_views_forward: NULL argument");
    if (misaligned(images, 3) || misaligned(points, 3) || misaligned(w2cs, 3) || misaligned(ixts, 3) || misaligned(out, 3) ||
        misaligned(z, 3))
        return invalid_arg("sample_views_forward: unaligned buffer");
    ViewsP p = {};
    p.img = images; p.pts = points; p.w2c = w2cs; p.ixt = ixts; p.out = out; p.z = z;
    for (int i = 0; i < 4; ++i) p.img_s[i] = images_strides[i];
    p.pts_s[0] = points_strides[0]; p.pts_s[1] = points_strides[1];
    p.N = a->N; p.V = a->V; p.C = a->C; p.H = a->H; p.W = a->W;
    p.views_per_row = 1; p.chunk = PF_CHUNK;
    hipLaunchKernelGGL(sample_views_fwd_kernel, dim3(div_up(a->N, PF_BLOCK), a->V, div_up(a->C, PF_CHUNK)), dim3(PF_BLOCK), 0,
                       (hipStream_t)stream, p);
    return launch_status("sample_views_fwd_kernel");
}

int gdr_sample_views_backward(const gdr_pointfeat_args* a, const float* grad_out, const float* grad_z, const float* images,
                              const int64_t* images_strides, const float* points, const int64_t* points_strides,
                              const float* w2cs, const float* ixts, float* grad_images, float* grad_points, void* stream) {
    if (const char* why = pf_check(a, true)) return invalid_arg(why);
    if (!images_strides || !points_strides) return invalid_arg("sample_views_backward: NULL strides");
    if (a->N == 0) return GDR_OK;
    if (!grad_images && !grad_points) return GDR_OK;   // nothing is wanted
    if (!grad_out || !points || !w2cs || !ixts) return invalid_arg("sample_views_backward: NULL argument");
    if (grad_points && !images) return invalid_arg("sample_views_backward: the point gradient reads the images");
    if (misaligned(grad_out, 3) || misaligned(grad_z, 3) || misaligned(images, 3) || misaligned(points, 3) || misaligned(w2cs, 3) ||
        misaligned(ixts, 3) || misaligned(grad_images, 3) || misaligned(grad_points, 3))
        return invalid_arg("sample_views_backward: unaligned buffer");
    ViewsP p = {};
    p.img = images; p.pts = points; p.w2c = w2cs; p.ixt = ixts; p.gout = grad_out; p.gz = grad_z;
    p.g_img = grad_images; p.g_pts = grad_points;
    for (int i = 0; i < 4; ++i) p.img_s[i] = images_strides[i];
    p.pts_s[0] = points_strides[0]; p.pts_s[1] = points_strides[1];
    p.N = a->N; p.V = a->V; p.C = a->C; p.H = a->H; p.W = a->W;
    // the point gradient is one thread's sum over every view and channel; without it the views and channel blocks spread
    p.views_per_row = grad_points ? a->V : 1;
    p.chunk = grad_points ? a->C : PF_CHUNK;
    hipLaunchKernelGGL(sample_views_bwd_kernel, dim3(div_up(a->N, PF_BLOCK), div_up(a->V, p.views_per_row), div_up(a->C, p.chunk)),
                       dim3(PF_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("sample_views_bwd_kernel");
}

}  // extern "C"

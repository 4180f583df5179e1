// viewattn.hip — the core of a single-query cross attention whose key / value projections are folded into the query and the
// output (include/gdr.h gdr_viewattn_*; the fold is generativedensification_amd/viewattn.py fold_attention_weights):
//
//   forward   s[n, h, v] = scale * <t[n, h], cond[n, v]>,  p = softmax_v(s),  u[n, h] = sum_v p[n, h, v] * cond[n, v]
//   backward  dp_v = <dU_h, cond_v>,  ds_v = p_v * (dp_v - sum_w p_w dp_w),  dt_h = scale * sum_v ds_v * cond_v,
//             dcond_v = sum_h (p_v * dU_h + scale * ds_v * t_h)
//
// t (N, H, Ck) is the query of a point moved into the key space, cond (N, V, Ck) its V raw view features: no projected key or
// value exists anywhere, and the core holds no weights.  Everything is computed in f32 whatever the storage types; the
// maximum is subtracted before expf (the accurate one); the backward recomputes p from t and cond (nothing is saved but the
// inputs).  No atomics: every output element has one writer and every sum a fixed order, so two runs are bitwise equal.  No
// entry point allocates or synchronises.
//
// Mapping: one lane per (point, head).  A point is held by a group of HP lanes, HP the power of two that covers H (lanes
// h >= H idle), so the heads of a point are adjacent lanes and a wave reads 64 / HP consecutive rows of t: contiguous memory
// when the rows are dense.  A workgroup of 256 threads holds 256 / HP points.  The V rows of cond are read by every lane of
// the group at the same address (one broadcast access per row piece).  Up to VA_HOLD = 4 views (the decoder has 2..4) they
// stay in registers and are read once, and every loop over views is unrolled; beyond that the `many` kernels walk the views in
// rolled loops and read cond once per pass (two passes forward, three backward: from L1 after the first).  The sum over heads
// of dcond is an xor butterfly inside the group (row_io.h group_sum), which gives every lane the same bits; lane v % HP writes
// view v.  With V = 1 the forward is p = 1 exactly and u = cond[n, 0] bit for bit, and ds = 0 exactly.
//
// dp_v - sum_w p_w dp_w is never computed in that form: near a one-hot row it cancels two numbers of the size of dp and keeps
// their rounding, which then reaches dcond multiplied by scale * t.  The held kernels take sum_w p_w (dp_v - dp_w), the many
// kernels (dp_v - pivot) - sum_w p_w (dp_w - pivot) with pivot = dp of the first view that has the largest s; both use
// sum_w p_w = 1 and add only small terms there.
//
// Bounds: a group leaves whole when its point is >= N; lanes h >= H load and store nothing and add zeros to the head sum; no
// index depends on a loaded value, so non-finite inputs give unspecified values and never an access outside the buffers.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"

namespace gdr {
namespace {

constexpr int VA_BLOCK = 256;
constexpr int VA_HOLD = 4;                         // views held in registers
constexpr int64_t VA_MAX_ROWS = (int64_t)1 << 27;

struct VaP {
    const void* t; const void* cond; const void* grad; void* out; void* dt; void* dcond;
    int64_t N, t_stride, cond_stride, out_stride, grad_stride;
    int32_t H, V, hp_shift, t_dt, cond_dt, out_dt, grad_dt;
    float scale;
};

// the point and head of this lane: a point's HP lanes are adjacent and never straddle a wave
__device__ __forceinline__ void lane_of(const VaP& p, int64_t& n, int& h) {
    const int64_t gid = (int64_t)blockIdx.x * VA_BLOCK + threadIdx.x;
    n = gid >> p.hp_shift;
    h = (int)(gid & ((1 << p.hp_shift) - 1));
}

// ---- V <= VA_HOLD: cond in registers, read once -------------------------------------------------------------------------------
template <int CK>
__device__ __forceinline__ void hold_cond(const VaP& p, int64_t n, float (&c)[VA_HOLD][CK]) {
#pragma unroll
    for (int v = 0; v < VA_HOLD; ++v) {
        if (v < p.V) load_row<CK>(p.cond, n * p.cond_stride + (int64_t)v * CK, p.cond_dt, c[v]);
        else {
#pragma unroll
            for (int k = 0; k < CK; ++k) c[v][k] = 0.f;
        }
    }
}

// s -> p in place over the first V entries: max, expf of the differences, their sum in ascending v, one division
__device__ __forceinline__ void softmax(float (&s)[VA_HOLD], int V) {
    float m = s[0];
#pragma unroll
    for (int v = 1; v < VA_HOLD; ++v)
        if (v < V) m = fmaxf(m, s[v]);
    float l = 0.f;
#pragma unroll
    for (int v = 0; v < VA_HOLD; ++v)
        if (v < V) { s[v] = expf(s[v] - m); l += s[v]; }
    const float inv = 1.0f / l;
#pragma unroll
    for (int v = 0; v < VA_HOLD; ++v)
        if (v < V) s[v] *= inv;
}

template <int CK>
__global__ __launch_bounds__(VA_BLOCK) void viewattn_fwd_kernel(const VaP p) {
    int64_t n;
    int h;
    lane_of(p, n, h);
    if (n >= p.N || h >= p.H) return;              // (no cross-lane traffic in the forward)
    const int V = p.V;
    float t[CK], c[VA_HOLD][CK], s[VA_HOLD], u[CK];
    load_row<CK>(p.t, n * p.t_stride + (int64_t)h * CK, p.t_dt, t);
    hold_cond<CK>(p, n, c);
#pragma unroll
    for (int v = 0; v < VA_HOLD; ++v) s[v] = v < V ? p.scale * dot<CK>(t, c[v]) : 0.f;
    softmax(s, V);
#pragma unroll
    for (int k = 0; k < CK; ++k) u[k] = s[0] * c[0][k];
#pragma unroll
    for (int v = 1; v < VA_HOLD; ++v) {
        if (v < V) {
#pragma unroll
            for (int k = 0; k < CK; ++k) u[k] = fmaf(s[v], c[v][k], u[k]);
        }
    }
    store_row<CK>(p.out, n * p.out_stride + (int64_t)h * CK, p.out_dt, u);
}

template <int CK>
__global__ __launch_bounds__(VA_BLOCK) void viewattn_bwd_kernel(const VaP p) {
    const int hp = 1 << p.hp_shift;
    int64_t n;
    int h;
    lane_of(p, n, h);
    if (n >= p.N) return;                          // (whole groups leave: the butterflies stay inside a group)
    const bool on = h < p.H;
    const int V = p.V;
    float t[CK], g[CK], c[VA_HOLD][CK], s[VA_HOLD], dp[VA_HOLD], dt[CK];
    if (on) {
        load_row<CK>(p.t, n * p.t_stride + (int64_t)h * CK, p.t_dt, t);
        load_row<CK>(p.grad, n * p.grad_stride + (int64_t)h * CK, p.grad_dt, g);
    } else {
#pragma unroll
        for (int k = 0; k < CK; ++k) t[k] = g[k] = 0.f;
    }
    hold_cond<CK>(p, n, c);
#pragma unroll
    for (int v = 0; v < VA_HOLD; ++v) {
        s[v] = v < V ? p.scale * dot<CK>(t, c[v]) : 0.f;
        dp[v] = v < V ? dot<CK>(g, c[v]) : 0.f;
    }
    softmax(s, V);
#pragma unroll
    for (int k = 0; k < CK; ++k) dt[k] = 0.f;
#pragma unroll
    for (int v = 0; v < VA_HOLD; ++v) {
        if (v < V) {                                // (uniform over the wave: V is a kernel argument)
            // dp_v - sum_w p_w dp_w as sum_w p_w (dp_v - dp_w) (sum_w p_w = 1): near a one-hot row the first form cancels
            // two numbers of the size of dp and keeps their rounding, the second adds small terms; V = 1 gives 0 exactly
            float spread = 0.f;
#pragma unroll
            for (int w = 0; w < VA_HOLD; ++w)
                if (w < V) spread = fmaf(s[w], dp[v] - dp[w], spread);
            const float ds = s[v] * spread;
            const float sds = p.scale * ds;
            float dc[CK];
#pragma unroll
            for (int k = 0; k < CK; ++k) {
                dt[k] = fmaf(ds, c[v][k], dt[k]);
                dc[k] = group_sum(on ? fmaf(sds, t[k], s[v] * g[k]) : 0.f, hp);
            }
            if (h == (v & (hp - 1))) store_row<CK>(p.dcond, (n * V + v) * CK, p.cond_dt, dc);
        }
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < CK; ++k) dt[k] *= p.scale;
        store_row<CK>(p.dt, (n * p.H + h) * CK, p.t_dt, dt);
    }
}

// ---- V > VA_HOLD: rolled loops over the views, cond read once per pass (from L1 after the first) -----------------------------
template <int CK>
__global__ __launch_bounds__(VA_BLOCK) void viewattn_fwd_many_kernel(const VaP p) {
    int64_t n;
    int h;
    lane_of(p, n, h);
    if (n >= p.N || h >= p.H) return;
    const int V = p.V;
    const int64_t cbase = n * p.cond_stride;
    float t[CK], c[CK], u[CK];
    load_row<CK>(p.t, n * p.t_stride + (int64_t)h * CK, p.t_dt, t);
    float m = -INFINITY;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        load_row<CK>(p.cond, cbase + (int64_t)v * CK, p.cond_dt, c);
        m = fmaxf(m, p.scale * dot<CK>(t, c));
    }
    float l = 0.f;
#pragma unroll
    for (int k = 0; k < CK; ++k) u[k] = 0.f;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        load_row<CK>(p.cond, cbase + (int64_t)v * CK, p.cond_dt, c);
        const float e = expf(p.scale * dot<CK>(t, c) - m);
        l += e;
#pragma unroll
        for (int k = 0; k < CK; ++k) u[k] = fmaf(e, c[k], u[k]);
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int k = 0; k < CK; ++k) u[k] *= inv;
    store_row<CK>(p.out, n * p.out_stride + (int64_t)h * CK, p.out_dt, u);
}

template <int CK>
__global__ __launch_bounds__(VA_BLOCK) void viewattn_bwd_many_kernel(const VaP p) {
    const int hp = 1 << p.hp_shift;
    int64_t n;
    int h;
    lane_of(p, n, h);
    if (n >= p.N) return;
    const bool on = h < p.H;
    const int V = p.V;
    const int64_t cbase = n * p.cond_stride;
    float t[CK], g[CK], c[CK], dt[CK], dc[CK];
    if (on) {
        load_row<CK>(p.t, n * p.t_stride + (int64_t)h * CK, p.t_dt, t);
        load_row<CK>(p.grad, n * p.grad_stride + (int64_t)h * CK, p.grad_dt, g);
    } else {
#pragma unroll
        for (int k = 0; k < CK; ++k) t[k] = g[k] = 0.f;
    }
    // pass 1: the maximum of s, and dp of the first view that reaches it as the pivot.  dp_v - sum_w p_w dp_w is taken as
    // (dp_v - pivot) - sum_w p_w (dp_w - pivot): near a one-hot row both parts are small, where the plain form cancels two
    // numbers of the size of dp and keeps their rounding
    float m = -INFINITY, pivot = 0.f;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        load_row<CK>(p.cond, cbase + (int64_t)v * CK, p.cond_dt, c);
        const float s = p.scale * dot<CK>(t, c);
        if (s > m) { m = s; pivot = dot<CK>(g, c); }
    }
    // pass 2: the normaliser and the p-weighted mean of dp - pivot
    float l = 0.f, a = 0.f;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        load_row<CK>(p.cond, cbase + (int64_t)v * CK, p.cond_dt, c);
        const float e = expf(p.scale * dot<CK>(t, c) - m);
        l += e;
        a = fmaf(e, dot<CK>(g, c) - pivot, a);
    }
    const float inv = 1.0f / l, mean = a * inv;
#pragma unroll
    for (int k = 0; k < CK; ++k) dt[k] = 0.f;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {                   // (uniform trip count: the butterflies meet whole groups)
        load_row<CK>(p.cond, cbase + (int64_t)v * CK, p.cond_dt, c);
        const float pv = expf(p.scale * dot<CK>(t, c) - m) * inv;
        const float ds = pv * ((dot<CK>(g, c) - pivot) - mean);
        const float sds = p.scale * ds;
#pragma unroll
        for (int k = 0; k < CK; ++k) {
            dt[k] = fmaf(ds, c[k], dt[k]);
            dc[k] = group_sum(on ? fmaf(sds, t[k], pv * g[k]) : 0.f, hp);
        }
        if (h == (v & (hp - 1))) store_row<CK>(p.dcond, (n * V + v) * CK, p.cond_dt, dc);
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < CK; ++k) dt[k] *= p.scale;
        store_row<CK>(p.dt, (n * p.H + h) * CK, p.t_dt, dt);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

int check_shape(int64_t N, int32_t H, int32_t Ck, int32_t V, float scale) {
    if (N < 0 || H < 1 || V < 1 || Ck < 1) return invalid_arg("viewattn: N must be >= 0 and H, Ck, V >= 1");
    if (!(scale == scale)) return invalid_arg("viewattn: scale is NaN");
    if (Ck != 4 && Ck != 8 && Ck != 16) return unsupported("viewattn: Ck must be 4, 8 or 16");
    if (H > GDR_VIEWATTN_MAX_HEADS) return unsupported("viewattn: H must be at most GDR_VIEWATTN_MAX_HEADS");
    if (V > GDR_VIEWATTN_MAX_VIEWS) return unsupported("viewattn: V must be at most GDR_VIEWATTN_MAX_VIEWS");
    if (N > VA_MAX_ROWS) return unsupported("viewattn: N must be at most 2^27");
    return GDR_OK;
}

int32_t head_shift(int32_t H) {
    int32_t sh = 0;
    while ((1 << sh) < H) ++sh;
    return sh;
}

// one launch of HELD<Ck> (V <= VA_HOLD) or MANY<Ck> over (N << hp_shift) lanes
#define VA_LAUNCH(HELD, MANY)                                                                                                    \
    do {                                                                                                                         \
        const dim3 grid((uint32_t)(((p.N << p.hp_shift) + VA_BLOCK - 1) / VA_BLOCK));                                            \
        const bool held = p.V <= VA_HOLD;                                                                                        \
        if (Ck == 4) {                                                                                                           \
            if (held) hipLaunchKernelGGL(HELD<4>, grid, dim3(VA_BLOCK), 0, st, p);                                               \
            else hipLaunchKernelGGL(MANY<4>, grid, dim3(VA_BLOCK), 0, st, p);                                                    \
        } else if (Ck == 8) {                                                                                                    \
            if (held) hipLaunchKernelGGL(HELD<8>, grid, dim3(VA_BLOCK), 0, st, p);                                               \
            else hipLaunchKernelGGL(MANY<8>, grid, dim3(VA_BLOCK), 0, st, p);                                                    \
        } else {                                                                                                                 \
            if (held) hipLaunchKernelGGL(HELD<16>, grid, dim3(VA_BLOCK), 0, st, p);                                              \
            else hipLaunchKernelGGL(MANY<16>, grid, dim3(VA_BLOCK), 0, st, p);                                                   \
        }                                                                                                                        \
    } while (0)

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_viewattn_forward(const void* t, int64_t t_stride, int32_t t_dtype, const void* cond, int64_t cond_stride, int32_t cond_dtype,
                         int64_t N, int32_t H, int32_t Ck, int32_t V, float scale, void* out, int64_t out_stride, int32_t out_dtype,
                         void* stream) {
    if (const int rc = check_shape(N, H, Ck, V, scale)) return rc;
    if (bad_dtype(t_dtype) || bad_dtype(cond_dtype) || bad_dtype(out_dtype)) return invalid_arg("viewattn_forward: unknown dtype");
    if (N == 0) return GDR_OK;
    if (!t || !cond || !out) return invalid_arg("viewattn_forward: NULL argument");
    if (bad_rows(t, t_stride, (int64_t)H * Ck) || bad_rows(cond, cond_stride, (int64_t)V * Ck) || bad_rows(out, out_stride, (int64_t)H * Ck))
        return unsupported("viewattn_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    VaP p = {};
    p.t = t; p.cond = cond; p.out = out;
    p.N = N; p.t_stride = t_stride; p.cond_stride = cond_stride; p.out_stride = out_stride;
    p.H = H; p.V = V; p.hp_shift = head_shift(H); p.t_dt = t_dtype; p.cond_dt = cond_dtype; p.out_dt = out_dtype; p.scale = scale;
    const hipStream_t st = (hipStream_t)stream;
    VA_LAUNCH(viewattn_fwd_kernel, viewattn_fwd_many_kernel);
    return launch_status("viewattn_fwd_kernel");
}

int gdr_viewattn_backward(const void* grad_out, int64_t grad_out_stride, int32_t grad_out_dtype, const void* t, int64_t t_stride,
                          int32_t t_dtype, const void* cond, int64_t cond_stride, int32_t cond_dtype, int64_t N, int32_t H, int32_t Ck,
                          int32_t V, float scale, void* grad_t, void* grad_cond, void* stream) {
    if (const int rc = check_shape(N, H, Ck, V, scale)) return rc;
    if (bad_dtype(t_dtype) || bad_dtype(cond_dtype) || bad_dtype(grad_out_dtype)) return invalid_arg("viewattn_backward: unknown dtype");
    if (N == 0) return GDR_OK;
    if (!grad_out || !t || !cond || !grad_t || !grad_cond) return invalid_arg("viewattn_backward: NULL argument");
    if (bad_rows(t, t_stride, (int64_t)H * Ck) || bad_rows(cond, cond_stride, (int64_t)V * Ck) ||
        bad_rows(grad_out, grad_out_stride, (int64_t)H * Ck) || misaligned(grad_t, 15) || misaligned(grad_cond, 15))
        return unsupported("viewattn_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    VaP p = {};
    p.t = t; p.cond = cond; p.grad = grad_out; p.dt = grad_t; p.dcond = grad_cond;
    p.N = N; p.t_stride = t_stride; p.cond_stride = cond_stride; p.grad_stride = grad_out_stride;
    p.H = H; p.V = V; p.hp_shift = head_shift(H); p.t_dt = t_dtype; p.cond_dt = cond_dtype; p.grad_dt = grad_out_dtype; p.scale = scale;
    const hipStream_t st = (hipStream_t)stream;
    VA_LAUNCH(viewattn_bwd_kernel, viewattn_bwd_many_kernel);
    return launch_status("viewattn_bwd_kernel");
}

}  // extern "C"

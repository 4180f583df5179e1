// groupattn.hip — the group cross attention of the volume transformer and the two LayerNorms that carry the volume into patch
// order and back (include/gdr.h gdr_groupattn_*; the module is generativedensification_amd/groupattn.py):
//
//   core      s[m, h, i, j] = scale * <q[m, i, h], k[m, j, h]>,  p = softmax_j(s),  out[m, i, h] = sum_j p[m, h, i, j] * v[m, j, h]
//   backward  dp_ij = <g[m, i, h], v[m, j, h]>,  ds_ij = p_ij * (dp_ij - sum_w p_iw dp_iw),
//             dq_i = scale * sum_j ds_ij k_j,  dk_j = scale * sum_i ds_ij q_i,  dv_j = sum_i p_ij g_i
//   norms     a LayerNorm over the C channels of a row, with the rows of a (B, D, H, W, C) volume gathered into patch order
//             (patchify: the raw rows leave as well) or the normalised rows scattered back (unpatchify).  Patch row
//             r = (b G + g) bs^3 + l, g = (gd Gh + gh) Gw + gw, l = (z bs + y) bs + x, is voxel (gd bs + z, gh bs + y, gw bs + x).
//
// Everything is computed in f32 whatever the storage types; the maximum is subtracted before expf; the backward recomputes p
// and the row statistics (nothing is saved but the inputs).  No atomics: every output element has one writer and every sum a
// fixed order, so two runs are bitwise equal.  No entry point allocates or synchronises.
//
// Mapping of the core: one lane per (group, query, head) with the head fastest, so a wave reads consecutive pieces of
// consecutive q rows (contiguous when the rows are dense), and the lanes that share a key read it at the same address in the
// same instruction.  The query row is multiplied by scale once, so a score is a plain dot product.  k and v are walked in
// rolled loops (once for the maximum, once for the sums; the second walk is served by L1).  The backward gives a workgroup `upw` whole groups (about GA_ITEMS query lanes) and runs two phases over them.
// Phase A, a lane per (group, query, head): the maximum, 1 / l, the pivot and the mean of dp - pivot go to LDS (16 bytes per
// lane) and dq leaves.  Phase B, a lane per (group, key, head): it walks the group's queries in ascending order, rebuilds
// p_ij and ds_ij from the LDS record and sums dk and dv in registers, in blocks of GA_SUM queries.  The q and g rows it reads were read by phase A of the
// same workgroup.  dp_ij - sum_w p_iw dp_iw is taken as (dp_ij - pivot) - mean(dp - pivot), pivot = dp of the first key that
// has the largest s (csrc/viewattn.hip explains why); with one key p = 1 and ds = 0 exactly.
//
// Mapping of the norms: csrc/norm.hip's, a row per group of LC lanes (row_io.h row_shape, row_stats; ln_rows.h for the row
// load, the backward's tail, the LDS sum and the fold).  The backward gives a workgroup GDR_GROUPATTN_NORM_ROWS consecutive
// patch rows, keeps the weight / bias sums of a group's rows in registers, adds the groups through LDS pairwise (sum_groups<true>,
// both vectors behind one barrier) and leaves one partial pair per workgroup; the fold launch (ln_fold_kernel<true>) adds the
// partials (16 lanes per column, each a run of workgroups in ascending order, then those 16 pairwise).
//
// Bounds: every lane checks its item against the counts of its workgroup; the row map is a bijection of [0, B D H W) (the
// host checks that D, H, W are multiples of bs); no index depends on a loaded value, so non-finite inputs give unspecified
// values and never an access outside the buffers.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "ln_rows.h"

namespace gdr {
namespace {

constexpr int GA_BLOCK = 256;
constexpr int GA_ITEMS = 512;                      // query lanes a backward workgroup aims at (one group at least)
constexpr int GA_SUM = 8;                          // queries per block of the dk / dv sums
constexpr int64_t GA_MAX_GROUPS = (int64_t)1 << 24;

struct GaP {
    const void* q; const void* k; const void* v; const void* grad; void* out; void* dq; void* dk; void* dv;
    int64_t M, q_stride, k_stride, v_stride, grad_stride;
    int32_t Lq, Lk, H, upw, q_dt, k_dt, v_dt, out_dt, grad_dt;
    float scale;
};

// a query row times scale, once: the score is then a plain dot product, every site gives the same bits and s - max is exactly
// 0 at the maximum (scale * dot(q, k) - max would be contracted into fma(scale, dot, -max), which returns the rounding residual
// of the product instead); dk = sum ds * (scale q) takes the same row
template <int DH>
__device__ __forceinline__ void scaled(float (&q)[DH], float scale) {
#pragma unroll
    for (int e = 0; e < DH; ++e) q[e] *= scale;
}

template <int DH>
__global__ __launch_bounds__(GA_BLOCK) void groupattn_fwd_kernel(const GaP p) {
    const int64_t idx = (int64_t)blockIdx.x * GA_BLOCK + threadIdx.x;
    const int64_t row = idx / p.H;                 // m Lq + i
    if (row >= p.M * p.Lq) return;                 // (no cross-lane traffic in the forward)
    const int col = (int)(idx - row * p.H) * DH, Lk = p.Lk;
    const int64_t krow = row / p.Lq * Lk;
    float q[DH], c[DH], u[DH];
    load_row<DH>(p.q, row * p.q_stride + col, p.q_dt, q);
    scaled<DH>(q, p.scale);
    float mx = -INFINITY;
#pragma unroll 1
    for (int j = 0; j < Lk; ++j) {
        load_row<DH>(p.k, (krow + j) * p.k_stride + col, p.k_dt, c);
        mx = fmaxf(mx, dot<DH>(q, c));
    }
    float l = 0.f;
#pragma unroll
    for (int e = 0; e < DH; ++e) u[e] = 0.f;
#pragma unroll 1
    for (int j = 0; j < Lk; ++j) {
        load_row<DH>(p.k, (krow + j) * p.k_stride + col, p.k_dt, c);
        const float ex = expf(dot<DH>(q, c) - mx);
        l += ex;
        load_row<DH>(p.v, (krow + j) * p.v_stride + col, p.v_dt, c);
#pragma unroll
        for (int e = 0; e < DH; ++e) u[e] = fmaf(ex, c[e], u[e]);
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int e = 0; e < DH; ++e) u[e] *= inv;
    store_row<DH>(p.out, row * ((int64_t)p.H * DH) + col, p.out_dt, u);
}

template <int DH>
__global__ __launch_bounds__(GA_BLOCK) void groupattn_bwd_kernel(const GaP p) {
    extern __shared__ __attribute__((aligned(16))) float4 rec[];       // per query lane: max, 1 / l, pivot, mean of dp - pivot
    const int H = p.H, Lq = p.Lq, Lk = p.Lk, qi = Lq * H, ki = Lk * H;
    const int64_t E = (int64_t)H * DH, m0 = (int64_t)blockIdx.x * p.upw;
    const int nu = (int)(p.M - m0 < p.upw ? p.M - m0 : p.upw);         // groups of this workgroup (>= 1 by the grid)
    // phase A: a lane per (group, query, head)
    for (int t = threadIdx.x; t < nu * qi; t += GA_BLOCK) {
        const int u = t / qi, r = t - u * qi, i = r / H, col = (r - i * H) * DH;
        const int64_t row = (m0 + u) * Lq + i, krow = (m0 + u) * Lk;
        float q[DH], g[DH], c[DH], dq[DH];
        load_row<DH>(p.q, row * p.q_stride + col, p.q_dt, q);
        load_row<DH>(p.grad, row * p.grad_stride + col, p.grad_dt, g);
        scaled<DH>(q, p.scale);
        float mx = -INFINITY, pivot = 0.f;
#pragma unroll 1
        for (int j = 0; j < Lk; ++j) {
            load_row<DH>(p.k, (krow + j) * p.k_stride + col, p.k_dt, c);
            const float s = dot<DH>(q, c);
            if (s > mx) {
                mx = s;
                load_row<DH>(p.v, (krow + j) * p.v_stride + col, p.v_dt, c);
                pivot = dot<DH>(g, c);
            }
        }
        float l = 0.f, a = 0.f;
#pragma unroll 1
        for (int j = 0; j < Lk; ++j) {
            load_row<DH>(p.k, (krow + j) * p.k_stride + col, p.k_dt, c);
            const float ex = expf(dot<DH>(q, c) - mx);
            l += ex;
            load_row<DH>(p.v, (krow + j) * p.v_stride + col, p.v_dt, c);
            a = fmaf(ex, dot<DH>(g, c) - pivot, a);
        }
        const float inv = 1.0f / l, mean = a * inv;
#pragma unroll
        for (int e = 0; e < DH; ++e) dq[e] = 0.f;
#pragma unroll 1
        for (int j = 0; j < Lk; ++j) {
            load_row<DH>(p.v, (krow + j) * p.v_stride + col, p.v_dt, c);
            const float dp = dot<DH>(g, c);
            load_row<DH>(p.k, (krow + j) * p.k_stride + col, p.k_dt, c);
            const float pv = expf(dot<DH>(q, c) - mx) * inv;
            const float ds = pv * ((dp - pivot) - mean);
#pragma unroll
            for (int e = 0; e < DH; ++e) dq[e] = fmaf(ds, c[e], dq[e]);
        }
#pragma unroll
        for (int e = 0; e < DH; ++e) dq[e] *= p.scale;
        store_row<DH>(p.dq, row * E + col, p.q_dt, dq);
        rec[t] = make_float4(mx, inv, pivot, mean);
    }
    __syncthreads();
    // phase B: a lane per (group, key, head); the queries of the group in ascending order
    for (int t = threadIdx.x; t < nu * ki; t += GA_BLOCK) {
        const int u = t / ki, r = t - u * ki, j = r / H, h = r - j * H, col = h * DH;
        const int64_t row0 = (m0 + u) * Lq, krow = (m0 + u) * Lk + j;
        float c[DH], w[DH], q[DH], g[DH], dk[DH], dv[DH];
        load_row<DH>(p.k, krow * p.k_stride + col, p.k_dt, c);
        load_row<DH>(p.v, krow * p.v_stride + col, p.v_dt, w);
#pragma unroll
        for (int e = 0; e < DH; ++e) dk[e] = dv[e] = 0.f;
        // blocks of GA_SUM queries are summed on their own and then added: a chain of 64 additions onto one growing sum
        // carries about twice the rounding of 8 + 8
#pragma unroll 1
        for (int i0 = 0; i0 < Lq; i0 += GA_SUM) {
            const int i1 = i0 + GA_SUM < Lq ? i0 + GA_SUM : Lq;
            float bk[DH], bv[DH];
#pragma unroll
            for (int e = 0; e < DH; ++e) bk[e] = bv[e] = 0.f;
#pragma unroll 1
            for (int i = i0; i < i1; ++i) {
                load_row<DH>(p.q, (row0 + i) * p.q_stride + col, p.q_dt, q);
                load_row<DH>(p.grad, (row0 + i) * p.grad_stride + col, p.grad_dt, g);
                scaled<DH>(q, p.scale);
                const float4 st = rec[(u * Lq + i) * H + h];
                const float pv = expf(dot<DH>(q, c) - st.x) * st.y;
                const float ds = pv * ((dot<DH>(g, w) - st.z) - st.w);
#pragma unroll
                for (int e = 0; e < DH; ++e) {
                    bk[e] = fmaf(ds, q[e], bk[e]);
                    bv[e] = fmaf(pv, g[e], bv[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < DH; ++e) { dk[e] += bk[e]; dv[e] += bv[e]; }
        }
        store_row<DH>(p.dk, krow * E + col, p.k_dt, dk);
        store_row<DH>(p.dv, krow * E + col, p.v_dt, dv);
    }
}

// ---- the row-map LayerNorms --------------------------------------------------------------------------------------------------
constexpr int RM_BLOCK = LN_BLOCK;
constexpr int RM_ROWS = GDR_GROUPATTN_NORM_ROWS;
constexpr int64_t RM_MAX_ROWS = INT64_C(0x7fffffff);

// unpatch = 0: x and dx are the volume (read / written through the map), out, copy and both gradients are in patch order;
// unpatch = 1: x and dx are in patch order, out and grad are the volume
struct RmP {
    const void* x; const void* weight; const void* bias; const void* grad; const void* grad_copy; void* out; void* copy; void* dx;
    float* part;                      // (workgroups, 2, C): dweight, dbias of a workgroup's rows
    int64_t N;
    int32_t D, H, W, bs, C, lc_shift, unpatch, x_dt, copy_dt, w_dt, b_dt, out_dt, grad_dt, gcopy_dt;
    float eps;
};

// the voxel row of patch row r
__device__ __forceinline__ int64_t voxel_row(const RmP& p, int64_t r) {
    const int bs = p.bs, b3 = bs * bs * bs, Gh = p.H / bs, Gw = p.W / bs;
    const int64_t G = (int64_t)(p.D / bs) * Gh * Gw, pg = r / b3, b = pg / G;
    const int l = (int)(r - pg * b3), g = (int)(pg - b * G);
    const int x = l % bs, y = l / bs % bs, z = l / (bs * bs), gw = g % Gw, gh = g / Gw % Gh, gd = g / (Gw * Gh);
    return ((b * p.D + gd * bs + z) * p.H + gh * bs + y) * p.W + gw * bs + x;
}

// x as the patches hold it: rounded to their type when that differs from the volume's (the norm is the norm of the patches)
__device__ __forceinline__ void round8(float (&x)[8], int x_dt, int copy_dt) {
    if (copy_dt == x_dt || copy_dt == GDR_NORM_F32) return;
#pragma unroll
    for (int v = 0; v < 8; ++v) x[v] = up_any(down_any(x[v], copy_dt), copy_dt);
}

template <int K>
__global__ __launch_bounds__(RM_BLOCK) void rowmap_norm_fwd_kernel(const RmP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (RM_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N) return;                        // (whole groups leave: the butterflies stay inside a group)
    const int64_t vox = voxel_row(p, row), src = p.unpatch ? row : vox, dst = p.unpatch ? vox : row;
    float x[K][8];
    bool on[K];
    pieces_on<K>(l, lc, p.C, on);
    load_row<K>(p.x, src * p.C, p.x_dt, on, l, lc, x);
    if (p.copy) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
                store8(p.copy, row * p.C + piece_c0(l, lc, k), p.copy_dt, x[k]);
                round8(x[k], p.x_dt, p.copy_dt);
            }
    }
    float mean, rstd;
    row_stats<K>(x, on, lc, 1.0f / (float)p.C, p.eps, mean, rstd);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!on[k]) continue;
        const int c0 = piece_c0(l, lc, k);
        float y[8], a[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) y[v] = (x[k][v] - mean) * rstd;
        if (p.weight) {
            load8(p.weight, c0, p.w_dt, a);
#pragma unroll
            for (int v = 0; v < 8; ++v) y[v] *= a[v];
        }
        if (p.bias) {
            load8(p.bias, c0, p.b_dt, a);
#pragma unroll
            for (int v = 0; v < 8; ++v) y[v] += a[v];
        }
        store8(p.out, dst * p.C + c0, p.out_dt, y);
    }
}

// xh the normalised row, g the gradient of the normalised output, means over the C channels:
//   dxh = g * weight;  dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)) + grad_copy;  dweight = sum g * xh;  dbias = sum g
template <int K>
__global__ __launch_bounds__(RM_BLOCK) void rowmap_norm_bwd_kernel(const RmP p) {
    __shared__ float sh[4096 * K];                 // (256 / LC) groups x 2 x C channels: C <= 8 LC K
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift, G = RM_BLOCK >> p.lc_shift;
    const int64_t a = (int64_t)blockIdx.x * RM_ROWS, e = a + RM_ROWS < p.N ? a + RM_ROWS : p.N;
    const int C = p.C;
    const float inv_c = 1.0f / (float)C;
    bool on[K];
    float sc[K][8], accw[K][8], accb[K][8];
    pieces_on<K>(l, lc, C, on);
    fill_row<K>(accw, 0.f);
    fill_row<K>(accb, 0.f);
    fill_row<K>(sc, 1.f);
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k] && p.weight) load8(p.weight, piece_c0(l, lc, k), p.w_dt, sc[k]);
    for (int64_t r = a + grp; r < e; r += G) {     // at most RM_ROWS / G rows, the same rows in every lane of a group
        const int64_t vox = voxel_row(p, r), xr = p.unpatch ? r : vox, gr = p.unpatch ? vox : r;
        float x[K][8], g[K][8];
        load_row<K>(p.x, xr * C, p.x_dt, on, l, lc, x);
        if (p.grad) load_row<K>(p.grad, gr * C, p.grad_dt, on, l, lc, g);
        else fill_row<K>(g, 0.f);
        if (!p.unpatch) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) round8(x[k], p.x_dt, p.copy_dt);
        }
        float mean, rstd;
        row_stats<K>(x, on, lc, inv_c, p.eps, mean, rstd);
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    x[k][v] = (x[k][v] - mean) * rstd;                 // xh
                    const float gx = g[k][v] * x[k][v];
                    accw[k][v] += gx;
                    accb[k][v] += g[k][v];
                    g[k][v] *= sc[k][v];                               // dxh
                    m1 += g[k][v];
                    m2 += gx * sc[k][v];
                }
            }
        ln_dx<K>(g, x, on, m1, m2, lc, inv_c, rstd);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
                const int c0 = piece_c0(l, lc, k);
                if (p.grad_copy) {
                    float gc[8];
                    load8(p.grad_copy, r * C + c0, p.gcopy_dt, gc);
#pragma unroll
                    for (int v = 0; v < 8; ++v) g[k][v] += gc[v];
                }
                store8(p.dx, xr * C + c0, p.x_dt, g[k]);
            }
    }
    put_sums<K>(sh + grp * 2 * C, accw, on, l, lc);        // one LDS pass for the two vectors
    put_sums<K>(sh + grp * 2 * C + C, accb, on, l, lc);
    sum_groups<true>(sh, 2 * C, G, p.part + (int64_t)blockIdx.x * 2 * C);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int check_core(int64_t M, int32_t Lq, int32_t Lk, int32_t H, int32_t Dh, float scale) {
    if (M < 0 || Lq < 1 || Lk < 1 || H < 1 || Dh < 1) return invalid_arg("groupattn: M must be >= 0 and Lq, Lk, H, Dh >= 1");
    if (!(scale == scale)) return invalid_arg("groupattn: scale is NaN");
    if (Dh != 8 && Dh != 16 && Dh != 32) return unsupported("groupattn: Dh must be 8, 16 or 32");
    if (H > GDR_GROUPATTN_MAX_HEADS) return unsupported("groupattn: H must be at most GDR_GROUPATTN_MAX_HEADS");
    if (Lq > GDR_GROUPATTN_MAX_QUERIES) return unsupported("groupattn: Lq must be at most GDR_GROUPATTN_MAX_QUERIES");
    if (Lk > GDR_GROUPATTN_MAX_KEYS) return unsupported("groupattn: Lk must be at most GDR_GROUPATTN_MAX_KEYS");
    if (M > GA_MAX_GROUPS) return unsupported("groupattn: M must be at most 2^24");
    return GDR_OK;
}

#define GA_LAUNCH(KERNEL, GRID, LDS)                                                                                             \
    do {                                                                                                                         \
        if (Dh == 8) hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(GA_BLOCK), LDS, st, p);                                            \
        else if (Dh == 16) hipLaunchKernelGGL(KERNEL<16>, GRID, dim3(GA_BLOCK), LDS, st, p);                                     \
        else hipLaunchKernelGGL(KERNEL<32>, GRID, dim3(GA_BLOCK), LDS, st, p);                                                   \
    } while (0)

// the shape of a volume and its patches: *rows = B D H W
int check_volume(int64_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t bs, float eps, int64_t* rows) {
    if (B < 0 || D < 1 || H < 1 || W < 1 || bs < 1) return invalid_arg("groupattn norm: B must be >= 0 and D, H, W, bs >= 1");
    if (!(eps >= 0.f)) return invalid_arg("groupattn norm: eps must be >= 0");
    if (bs > GDR_GROUPATTN_MAX_BLOCK) return unsupported("groupattn norm: bs must be at most GDR_GROUPATTN_MAX_BLOCK");
    if (D % bs || H % bs || W % bs) return invalid_arg("groupattn norm: D, H and W must be multiples of bs");
    if (C < 8 || C > GDR_NORM_MAX_CHANNELS || C % 8) return unsupported("groupattn norm: C must be a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS");
    int64_t voxels = (int64_t)D * H;               // (two int32 factors fit; the third only once these are below 2^31)
    if (voxels > RM_MAX_ROWS || (voxels *= W) > RM_MAX_ROWS || (B && voxels > RM_MAX_ROWS / B))
        return unsupported("groupattn norm: B D H W must be below 2^31");
    *rows = B * voxels;
    return GDR_OK;
}

int norm_forward(int unpatch, const void* x, int32_t x_dtype, int32_t copy_dtype, const void* weight, int32_t weight_dtype, const void* bias,
                 int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t bs, float eps, void* copy, void* out,
                 int32_t out_dtype, void* stream) {
    int64_t N;
    if (const int rc = check_volume(B, D, H, W, C, bs, eps, &N)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(copy_dtype) || bad_dtype(out_dtype) || (weight && bad_dtype(weight_dtype)) || (bias && bad_dtype(bias_dtype)))
        return invalid_arg("groupattn norm forward: unknown dtype");
    if (N == 0) return GDR_OK;
    if (!x || !out || (!unpatch && !copy)) return invalid_arg("groupattn norm forward: NULL argument");
    if (misaligned(x, 15) || misaligned(out, 15) || misaligned(copy, 15) || misaligned(weight, 15) || misaligned(bias, 15))
        return unsupported("groupattn norm forward: every buffer must start on 16 bytes");
    RmP p = {};
    p.x = x; p.weight = weight; p.bias = bias; p.out = out; p.copy = copy;
    p.N = N; p.D = D; p.H = H; p.W = W; p.bs = bs; p.C = C; p.unpatch = unpatch;
    p.x_dt = x_dtype; p.copy_dt = copy_dtype; p.w_dt = weight_dtype; p.b_dt = bias_dtype; p.out_dt = out_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = RM_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((N + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    LN_LAUNCH_K(rowmap_norm_fwd_kernel, K, grid, st, p);
    return launch_status("groupattn rowmap_norm_fwd_kernel");
}

size_t norm_workspace(int64_t N, int64_t C) { return align_up((size_t)((N + RM_ROWS - 1) / RM_ROWS) * 2 * (size_t)C * 4); }

int norm_backward(int unpatch, const void* grad_out, int32_t grad_dtype, const void* grad_copy, int32_t grad_copy_dtype, const void* x,
                  int32_t x_dtype, int32_t copy_dtype, const void* weight, int32_t weight_dtype, int32_t bias_dtype, int64_t B, int32_t D, int32_t H,
                  int32_t W, int32_t C, int32_t bs, float eps, void* workspace, size_t workspace_bytes, void* grad_x, void* grad_weight,
                  void* grad_bias, void* stream) {
    int64_t N;
    if (const int rc = check_volume(B, D, H, W, C, bs, eps, &N)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(copy_dtype) || (grad_out && bad_dtype(grad_dtype)) || (grad_copy && bad_dtype(grad_copy_dtype)) ||
        ((weight || grad_weight) && bad_dtype(weight_dtype)) || (grad_bias && bad_dtype(bias_dtype)))
        return invalid_arg("groupattn norm backward: unknown dtype");
    if (!workspace || (N && (!x || !grad_x))) return invalid_arg("groupattn norm backward: NULL argument");
    if (misaligned(x, 15) || misaligned(grad_out, 15) || misaligned(grad_copy, 15) || misaligned(weight, 15) || misaligned(grad_x, 15) ||
        misaligned(grad_weight, 3) || misaligned(grad_bias, 3) || misaligned(workspace, 255))
        return unsupported("groupattn norm backward: every row buffer must start on 16 bytes and the workspace on 256");
    if (workspace_bytes < norm_workspace(N, C)) return workspace_too_small("groupattn norm backward: workspace smaller than gdr_groupattn_norm_backward_bytes");
    RmP p = {};
    p.x = x; p.weight = weight; p.grad = grad_out; p.grad_copy = grad_copy; p.dx = grad_x; p.part = (float*)workspace;
    p.N = N; p.D = D; p.H = H; p.W = W; p.bs = bs; p.C = C; p.unpatch = unpatch;
    p.x_dt = x_dtype; p.copy_dt = copy_dtype; p.w_dt = weight_dtype; p.b_dt = bias_dtype; p.grad_dt = grad_dtype; p.gcopy_dt = grad_copy_dtype; p.eps = eps;
    const int64_t nparts = (N + RM_ROWS - 1) / RM_ROWS;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const hipStream_t st = (hipStream_t)stream;
    if (nparts) LN_LAUNCH_K(rowmap_norm_bwd_kernel, K, dim3((uint32_t)nparts), st, p);
    if (grad_weight || grad_bias) launch_ln_fold<true>(p.part, nparts, C, grad_weight, weight_dtype, grad_bias, bias_dtype, st);
    return launch_status("groupattn rowmap_norm_bwd kernels");
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_groupattn_forward(const void* q, int64_t q_stride, int32_t q_dtype, const void* k, int64_t k_stride, int32_t k_dtype,
                          const void* v, int64_t v_stride, int32_t v_dtype, int64_t M, int32_t Lq, int32_t Lk, int32_t H, int32_t Dh,
                          float scale, void* out, int32_t out_dtype, void* stream) {
    if (const int rc = check_core(M, Lq, Lk, H, Dh, scale)) return rc;
    if (bad_dtype(q_dtype) || bad_dtype(k_dtype) || bad_dtype(v_dtype) || bad_dtype(out_dtype)) return invalid_arg("groupattn_forward: unknown dtype");
    if (M == 0) return GDR_OK;
    if (!q || !k || !v || !out) return invalid_arg("groupattn_forward: NULL argument");
    const int64_t E = (int64_t)H * Dh;
    if (bad_rows(q, q_stride, E) || bad_rows(k, k_stride, E) || bad_rows(v, v_stride, E) || misaligned(out, 15))
        return unsupported("groupattn_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    GaP p = {};
    p.q = q; p.k = k; p.v = v; p.out = out;
    p.M = M; p.q_stride = q_stride; p.k_stride = k_stride; p.v_stride = v_stride;
    p.Lq = Lq; p.Lk = Lk; p.H = H; p.q_dt = q_dtype; p.k_dt = k_dtype; p.v_dt = v_dtype; p.out_dt = out_dtype; p.scale = scale;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((uint32_t)((M * Lq * H + GA_BLOCK - 1) / GA_BLOCK));           // at most 2^28 workgroups
    GA_LAUNCH(groupattn_fwd_kernel, grid, 0);
    return launch_status("groupattn_fwd_kernel");
}

int gdr_groupattn_backward(const void* grad_out, int64_t grad_out_stride, int32_t grad_out_dtype, const void* q, int64_t q_stride,
                           int32_t q_dtype, const void* k, int64_t k_stride, int32_t k_dtype, const void* v, int64_t v_stride,
                           int32_t v_dtype, int64_t M, int32_t Lq, int32_t Lk, int32_t H, int32_t Dh, float scale, void* grad_q,
                           void* grad_k, void* grad_v, void* stream) {
    if (const int rc = check_core(M, Lq, Lk, H, Dh, scale)) return rc;
    if (bad_dtype(q_dtype) || bad_dtype(k_dtype) || bad_dtype(v_dtype) || bad_dtype(grad_out_dtype)) return invalid_arg("groupattn_backward: unknown dtype");
    if (M == 0) return GDR_OK;
    if (!grad_out || !q || !k || !v || !grad_q || !grad_k || !grad_v) return invalid_arg("groupattn_backward: NULL argument");
    const int64_t E = (int64_t)H * Dh;
    if (bad_rows(q, q_stride, E) || bad_rows(k, k_stride, E) || bad_rows(v, v_stride, E) || bad_rows(grad_out, grad_out_stride, E) ||
        misaligned(grad_q, 15) || misaligned(grad_k, 15) || misaligned(grad_v, 15))
        return unsupported("groupattn_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    GaP p = {};
    p.q = q; p.k = k; p.v = v; p.grad = grad_out; p.dq = grad_q; p.dk = grad_k; p.dv = grad_v;
    p.M = M; p.q_stride = q_stride; p.k_stride = k_stride; p.v_stride = v_stride; p.grad_stride = grad_out_stride;
    p.Lq = Lq; p.Lk = Lk; p.H = H; p.q_dt = q_dtype; p.k_dt = k_dtype; p.v_dt = v_dtype; p.grad_dt = grad_out_dtype; p.scale = scale;
    const int qi = Lq * H;                         // query lanes of a group: at most 4096, 64 KiB of LDS records
    p.upw = GA_ITEMS / qi > 1 ? GA_ITEMS / qi : 1;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((uint32_t)((M + p.upw - 1) / p.upw));
    const size_t lds = (size_t)p.upw * qi * sizeof(float4);
    GA_LAUNCH(groupattn_bwd_kernel, grid, lds);
    return launch_status("groupattn_bwd_kernel");
}

int gdr_groupattn_patchify_norm_forward(const void* vol, int32_t vol_dtype, const void* weight, int32_t weight_dtype, const void* bias,
                                        int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t bs, float eps,
                                        void* patches, int32_t patches_dtype, void* normed, int32_t normed_dtype, void* stream) {
    return norm_forward(0, vol, vol_dtype, patches_dtype, weight, weight_dtype, bias, bias_dtype, B, D, H, W, C, bs, eps, patches, normed,
                        normed_dtype, stream);
}

int gdr_groupattn_norm_unpatchify_forward(const void* patches, int32_t patches_dtype, const void* weight, int32_t weight_dtype,
                                          const void* bias, int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C,
                                          int32_t bs, float eps, void* vol, int32_t vol_dtype, void* stream) {
    return norm_forward(1, patches, patches_dtype, patches_dtype, weight, weight_dtype, bias, bias_dtype, B, D, H, W, C, bs, eps, nullptr, vol, vol_dtype,
                        stream);
}

size_t gdr_groupattn_norm_backward_bytes(int64_t rows, int32_t C) {
    if (rows < 0 || rows > RM_MAX_ROWS || C < 8 || C > GDR_NORM_MAX_CHANNELS || C % 8) {
        set_error("groupattn norm backward: rows must be in 0..2^31 - 1 and C a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS", hipSuccess);
        return 0;
    }
    return norm_workspace(rows, C) + 256;          // (never 0 for valid arguments)
}

int gdr_groupattn_patchify_norm_backward(const void* grad_normed, int32_t grad_normed_dtype, const void* grad_patches,
                                         int32_t grad_patches_dtype, const void* vol, int32_t vol_dtype, int32_t patches_dtype, const void* weight,
                                         int32_t weight_dtype, int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C,
                                         int32_t bs, float eps, void* workspace, size_t workspace_bytes, void* grad_vol, void* grad_weight,
                                         void* grad_bias, void* stream) {
    return norm_backward(0, grad_normed, grad_normed_dtype, grad_patches, grad_patches_dtype, vol, vol_dtype, patches_dtype, weight, weight_dtype,
                         bias_dtype, B, D, H, W, C, bs, eps, workspace, workspace_bytes, grad_vol, grad_weight, grad_bias, stream);
}

int gdr_groupattn_norm_unpatchify_backward(const void* grad_vol, int32_t grad_vol_dtype, const void* patches, int32_t patches_dtype,
                                           const void* weight, int32_t weight_dtype, int32_t bias_dtype, int64_t B, int32_t D, int32_t H,
                                           int32_t W, int32_t C, int32_t bs, float eps, void* workspace, size_t workspace_bytes,
                                           void* grad_patches, void* grad_weight, void* grad_bias, void* stream) {
    return norm_backward(1, grad_vol, grad_vol_dtype, nullptr, GDR_NORM_F32, patches, patches_dtype, patches_dtype, weight, weight_dtype, bias_dtype, B,
                         D, H, W, C, bs, eps, workspace, workspace_bytes, grad_patches, grad_weight, grad_bias, stream);
}

}  // extern "C"

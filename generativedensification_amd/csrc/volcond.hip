// volcond.hip — the conditioning of the volume transformer between the image encoder and the first GroupAttBlock
// (include/gdr.h gdr_volcond_*): what the reference computes with tensor ops in Network.build_feat_vol, the view_embed concat of
// Network.forward and the cond regrouping at the head of VolTransformer.forward (lightning/network.py).
//
//   ray_sh   rays (n, 6) = (origin o, direction d) -> (n, 32) f32: dh = d / max(|d|, 1e-12), m = o x dh, out = [Y(dh), Y(m)], Y the
//            16 real spherical harmonics of degree <= 3 as polynomials of (x, y, z) (Y_l^m at l (l + 1) + m, Condon-Shortley
//            phase), evaluated on m although m is no unit vector; optionally SiLU of every entry.
//   modln    out[r] = (layer_norm(x[r]) * weight + bias) * (1 + scale[r]) + shift[r], shift = ss[r, :C], scale = ss[r, C:].
//            backward, xh the normalised row, g = grad_out, y = xh * weight + bias, means over the C channels:
//              dshift = g;  dscale = g * y;  dy = g * (1 + scale);  dweight = sum_r dy * xh;  dbias = sum_r dy;
//              dxh = dy * weight;  dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh))
//   sample   cond[row(b, v, n), :C] = the bilinear sample of rows[b V + v] (h, w, C channels-last) at the projection of grid
//            point n into view b V + v, cond[row, C:] = view_embed[v]; row(b, v, n) puts the r^3 points (d, h, w order) into
//            g^3 blocks of bs^3: ((((b g + gz) g + gy) g + gx) V + v) bs^3 + (iz bs + iy) bs + ix.
//            Projection: q = R p + t, hc = K q, x = hc0 / hc2, y = hc1 / hc2 in the pixels of the (img_h, img_w) image the
//            intrinsics refer to; the token map is sampled at u = (x + 0.5) w / img_w - 0.5, v = (y + 0.5) h / img_h - 0.5,
//            computed as grid_sample(align_corners=False) does from the normalised coordinate.  Neighbours floor + {0, 1},
//            summed in grid_sample's order (y0x0, y0x1, y1x0, y1x1); a neighbour outside the map contributes nothing.  A pair
//            with hc2 == 0, or a position that is not finite or outside +-2^30, samples zeros; hc2 < 0 projects mirrored.
//            The forward saves, per (view, point, tap), the texel index (or the sentinel B V h w for a tap outside) and the
//            weight.  The backward sorts the entries by texel (gdr_serial_sort: stable, so a texel's entries stay in ascending
//            point order) and one lane group per texel sums weight * grad_cond row over its run, lanes over channels.
//            dview_embed[v] is the sum of grad_cond[row, C:] over b and n ascending: 64 contiguous ranges, then those in order.
//
// Everything is f32 arithmetic whatever the storage types.  No atomics: every output element has one writer and every sum a
// fixed order, so two runs are bitwise equal.  No entry point allocates or synchronises.
//
// modln's row load, backward tail, LDS sum of the groups and fold (ln_fold_kernel<false>) are ln_rows.h's, shared with norm.hip
// and groupattn.hip; make_taps and the 2^30 bound are proj_taps.h's, shared with pointfeat.hip.
//
// Bounds: every row index is checked against its count; texel coordinates are clamped into the map before an address is formed;
// the searches of the backward stop after 32 steps and the entry indices they read come from the sort, which returns a
// permutation of [0, entries).
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "ln_rows.h"
#include "proj_taps.h"

namespace gdr {
namespace {

constexpr int VC_BLOCK = LN_BLOCK;
constexpr int VC_ROWS = GDR_VOLCOND_SLAB_ROWS;

// ---- ray_sh ------------------------------------------------------------------------------------------------------------------
// sqrt(1 / 4 pi); sqrt(3 / 4 pi); sqrt(15 / 4 pi), sqrt(5 / 16 pi), sqrt(15 / 16 pi); sqrt(35 / 32 pi), sqrt(105 / 4 pi),
// sqrt(21 / 32 pi), sqrt(7 / 16 pi), sqrt(105 / 16 pi)
constexpr float SH0 = 0.28209479177387814f;
constexpr float SH1 = 0.4886025119029199f;
constexpr float SH2A = 1.0925484305920792f, SH2B = 0.31539156525252005f, SH2C = 0.5462742152960396f;
constexpr float SH3A = 0.5900435899266435f, SH3B = 2.890611442640554f, SH3C = 0.4570457994644658f, SH3D = 0.3731763325901154f,
                SH3E = 1.445305721320277f;

__device__ __forceinline__ void sh16(float x, float y, float z, float* o) {
    const float x2 = x * x, y2 = y * y, z2 = z * z;
    o[0] = SH0;
    o[1] = -SH1 * y;
    o[2] = SH1 * z;
    o[3] = -SH1 * x;
    o[4] = SH2A * (x * y);
    o[5] = -SH2A * (y * z);
    o[6] = SH2B * (3.f * z2 - 1.f);
    o[7] = -SH2A * (x * z);
    o[8] = SH2C * (x2 - y2);
    o[9] = -SH3A * y * (3.f * x2 - y2);
    o[10] = SH3B * (x * y) * z;
    o[11] = -SH3C * y * (5.f * z2 - 1.f);
    o[12] = SH3D * z * (5.f * z2 - 3.f);
    o[13] = -SH3C * x * (5.f * z2 - 1.f);
    o[14] = SH3E * z * (x2 - y2);
    o[15] = -SH3A * x * (x2 - 3.f * y2);
}

__global__ __launch_bounds__(VC_BLOCK) void ray_sh_kernel(const void* __restrict__ rays, int dt, int64_t n, int silu,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * VC_BLOCK + threadIdx.x;
    if (i >= n) return;
    float r[6];
    for (int k = 0; k < 6; ++k) r[k] = load1(rays, i * 6 + k, dt);
    const float len = sqrtf(r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
    const float den = fmaxf(len, 1e-12f);
    const float dx = r[3] / den, dy = r[4] / den, dz = r[5] / den;
    const float mx = r[1] * dz - r[2] * dy, my = r[2] * dx - r[0] * dz, mz = r[0] * dy - r[1] * dx;
    float o[32];
    sh16(dx, dy, dz, o);
    sh16(mx, my, mz, o + 16);
    if (silu)
        for (int k = 0; k < 32; ++k) o[k] = o[k] / (1.f + expf(-o[k]));
    float4* dst = reinterpret_cast<float4*>(out + i * 32);
    for (int k = 0; k < 8; ++k) dst[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}

// ---- modln -------------------------------------------------------------------------------------------------------------------
struct ModP {
    const void *x, *ss, *weight, *bias, *grad;
    void *out, *dx, *dss;
    float* part;                      // (slabs, 2, C): dweight, dbias of a slab
    int64_t R, x_stride, x_inner, x_outer, ss_stride, grad_stride;
    int32_t C, lc_shift, x_dt, ss_dt, w_dt, b_dt, out_dt;
    float eps;
};

// x is (outer, inner, C) through two strides: row = o * inner + i lies at o * x_outer + i * x_stride
__device__ __forceinline__ int64_t x_offset(const ModP& p, int64_t row) {
    const int64_t o = row / p.x_inner;
    return o * p.x_outer + (row - o * p.x_inner) * p.x_stride;
}

template <int K>
__device__ __forceinline__ void load_affine(const ModP& p, const bool (&on)[K], int l, int lc, float (&w)[K][8], float (&b)[K][8]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int v = 0; v < 8; ++v) { w[k][v] = 1.f; b[k][v] = 0.f; }
        if (on[k]) {
            if (p.weight) load8(p.weight, piece_c0(l, lc, k), p.w_dt, w[k]);
            if (p.bias) load8(p.bias, piece_c0(l, lc, k), p.b_dt, b[k]);
        }
    }
}

template <int K>
__global__ __launch_bounds__(VC_BLOCK) void modln_fwd_kernel(const ModP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (VC_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.R) return;                        // (whole groups leave: the butterflies stay inside a group)
    float x[K][8], w[K][8], b[K][8];
    bool on[K];
    pieces_on<K>(l, lc, p.C, on);
    load_row<K>(p.x, x_offset(p, row), p.x_dt, on, l, lc, x);
    load_affine<K>(p, on, l, lc, w, b);
    float mean, rstd;
    row_stats<K>(x, on, lc, 1.0f / (float)p.C, p.eps, mean, rstd);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!on[k]) continue;
        const int c0 = piece_c0(l, lc, k);
        float sh[8], sc[8], y[8];
        load8(p.ss, row * p.ss_stride + c0, p.ss_dt, sh);
        load8(p.ss, row * p.ss_stride + p.C + c0, p.ss_dt, sc);
#pragma unroll
        for (int v = 0; v < 8; ++v) y[v] = ((x[k][v] - mean) * rstd * w[k][v] + b[k][v]) * (1.f + sc[v]) + sh[v];
        store8(p.out, row * p.C + c0, p.out_dt, y);
    }
}

// a workgroup takes the VC_ROWS rows of slab blockIdx.x; its groups take them in turn and keep dweight / dbias of their rows in
// registers; behind the rows the sums of the groups are added through LDS in group order into the slab's partial
template <int K>
__global__ __launch_bounds__(VC_BLOCK) void modln_bwd_kernel(const ModP p) {
    __shared__ float lds[2048 * K];                // (256 / LC) groups x C channels: C <= 8 LC K
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift, G = VC_BLOCK >> p.lc_shift;
    const int64_t j = blockIdx.x, a = j * VC_ROWS, e = a + VC_ROWS < p.R ? a + VC_ROWS : p.R;
    const int C = p.C;
    const float inv_c = 1.0f / (float)C;
    bool on[K];
    pieces_on<K>(l, lc, C, on);
    float w[K][8], b[K][8], aw[K][8], ab[K][8];
    load_affine<K>(p, on, l, lc, w, b);
    fill_row<K>(aw, 0.f);
    fill_row<K>(ab, 0.f);
    for (int64_t r = a + grp; r < e; r += G) {
        float x[K][8], g[K][8];
        load_row<K>(p.x, x_offset(p, r), p.x_dt, on, l, lc, x);
        load_row<K>(p.grad, r * p.grad_stride, p.out_dt, on, l, lc, g);
        float mean, rstd;
        row_stats<K>(x, on, lc, inv_c, p.eps, mean, rstd);
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
                const int c0 = piece_c0(l, lc, k);
                float sc[8], ds[8];
                load8(p.ss, r * p.ss_stride + C + c0, p.ss_dt, sc);
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    x[k][v] = (x[k][v] - mean) * rstd;                 // xh
                    ds[v] = g[k][v] * (x[k][v] * w[k][v] + b[k][v]);   // dscale
                }
                if (p.dss) {
                    store8(p.dss, r * 2 * C + c0, p.ss_dt, g[k]);      // dshift
                    store8(p.dss, r * 2 * C + C + c0, p.ss_dt, ds);
                }
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const float dy = g[k][v] * (1.f + sc[v]);
                    aw[k][v] += dy * x[k][v];
                    ab[k][v] += dy;
                    g[k][v] = dy * w[k][v];                            // dxh
                    m1 += g[k][v];
                    m2 += g[k][v] * x[k][v];
                }
            }
        if (p.dx) {                                // (the same in every thread)
            ln_dx<K>(g, x, on, m1, m2, lc, inv_c, rstd);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) store8(p.dx, r * C + piece_c0(l, lc, k), p.x_dt, g[k]);
        }
    }
    if (!p.part) return;                           // (the same in every thread)
    put_sums<K>(lds + grp * C, aw, on, l, lc);
    sum_groups<false>(lds, C, G, p.part + j * 2 * C);
    __syncthreads();
    put_sums<K>(lds + grp * C, ab, on, l, lc);
    sum_groups<false>(lds, C, G, p.part + (j * 2 + 1) * C);
}

// ---- sample ------------------------------------------------------------------------------------------------------------------
struct SampP {
    const void *rows, *ve, *grad;
    const float *pts, *w2c, *ixt;
    void *cond, *drows, *dve;
    int64_t* keys; float* wts;                     // forward: written (NULL = not wanted); backward: read
    const int64_t* order;
    int64_t N, pairs, entries, texels, ve_stride;  // N = r^3, pairs = B V N, entries = 4 pairs, texels = B V h w
    int32_t B, V, h, w, C, E, r, g, bs, img_h, img_w, lc_shift, rows_dt, ve_dt, cond_dt;
};

// the cond row of point n of view v of batch element b
__device__ __forceinline__ int64_t cond_row(const SampP& p, int b, int v, int64_t n) {
    const int r = p.r, bs = p.bs, g = p.g;
    const int x = (int)(n % r), y = (int)((n / r) % r), z = (int)(n / ((int64_t)r * r));
    const int64_t blk = (((int64_t)b * g + z / bs) * g + y / bs) * g + x / bs;
    return (blk * p.V + v) * ((int64_t)bs * bs * bs) + ((z % bs) * bs + y % bs) * bs + x % bs;
}

// the four neighbours of point n in view bv of the (h, w) map (proj_taps.h make_taps); a degenerate pair has none inside.  The
// projection is proj_taps.h project's arithmetic written out: called from there the compiler fuses other products of the matrix
// rows into FMAs, and the samples and saved weights move in the last bit.
__device__ __forceinline__ Taps project_taps(const SampP& p, int bv, int64_t n) {
    const float* m = p.w2c + (int64_t)bv * 16;
    const float* k = p.ixt + (int64_t)bv * 9;
    const float px = p.pts[n * 3], py = p.pts[n * 3 + 1], pz = p.pts[n * 3 + 2];
    const float q0 = m[0] * px + m[1] * py + m[2] * pz + m[3];
    const float q1 = m[4] * px + m[5] * py + m[6] * pz + m[7];
    const float q2 = m[8] * px + m[9] * py + m[10] * pz + m[11];
    const float h0 = k[0] * q0 + k[1] * q1 + k[2] * q2;
    const float h1 = k[3] * q0 + k[4] * q1 + k[5] * q2;
    const float h2 = k[6] * q0 + k[7] * q1 + k[8] * q2;
    bool ok = h2 != 0.f;
    float x = ok ? h0 / h2 : 0.f, y = ok ? h1 / h2 : 0.f;
    ok = ok && fabsf(x) <= PT_MAX_POS && fabsf(y) <= PT_MAX_POS;       // (false for NaN and inf)
    // the pixel of the (img_h, img_w) image -> normalised -> the position in the (h, w) map, as grid_sample un-normalises
    float u = (((x + 0.5f) / (float)p.img_w * 2.f - 1.f + 1.f) * (float)p.w - 1.f) / 2.f;
    float v = (((y + 0.5f) / (float)p.img_h * 2.f - 1.f + 1.f) * (float)p.h - 1.f) / 2.f;
    ok = ok && fabsf(u) <= PT_MAX_POS && fabsf(v) <= PT_MAX_POS;
    if (!ok) u = v = 0.f;
    const Proj pr = {u, v, h2, ok};
    return make_taps(pr, p.h, p.w);
}

// one group of LC lanes per (view, point) pair, lanes over channels
__global__ __launch_bounds__(VC_BLOCK) void sample_fwd_kernel(const SampP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t pair = (int64_t)blockIdx.x * (VC_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (pair >= p.pairs) return;
    const int bv = (int)(pair / p.N);
    const int64_t n = pair - (int64_t)bv * p.N;
    const int b = bv / p.V, v = bv - b * p.V;
    const Taps t = project_taps(p, bv, n);
    float wt[4];
    int64_t tex[4];
    for (int i = 0; i < 4; ++i) {
        wt[i] = t.wx[i & 1] * t.wy[i >> 1];
        tex[i] = ((int64_t)bv * p.h + t.yc[i >> 1]) * p.w + t.xc[i & 1];
    }
    if (p.keys && l < 4) {
        p.keys[pair * 4 + l] = t.in[l] ? tex[l] : p.texels;
        p.wts[pair * 4 + l] = wt[l];
    }
    const int64_t row = cond_row(p, b, v, n), W = p.C + p.E;
    for (int c0 = l * 8; c0 < p.C; c0 += lc * 8) {
        float acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.f;
        for (int i = 0; i < 4; ++i) {
            if (!t.in[i]) continue;                // (the same in every lane of the group)
            float val[8];
            load8(p.rows, tex[i] * p.C + c0, p.rows_dt, val);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += val[q] * wt[i];
        }
        store8(p.cond, row * W + c0, p.cond_dt, acc);
    }
    for (int c0 = l * 8; c0 < p.E; c0 += lc * 8) {
        float val[8];
        load8(p.ve, v * p.ve_stride + c0, p.ve_dt, val);
        store8(p.cond, row * W + p.C + c0, p.cond_dt, val);
    }
}

// the first j in [0, entries) with key[order[j]] >= want (entries if there is none)
__device__ __forceinline__ int64_t lower_bound(const SampP& p, int64_t want) {
    int64_t lo = 0, hi = p.entries;
    for (int k = 0; k < 32 && lo < hi; ++k) {
        const int64_t mid = (lo + hi) >> 1;
        int64_t e = p.order[mid];
        e = e < 0 ? 0 : (e >= p.entries ? p.entries - 1 : e);
        if (p.keys[e] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one group of LC lanes per texel: the sum of weight * grad_cond row over the texel's run of sorted entries
__global__ __launch_bounds__(VC_BLOCK) void sample_bwd_kernel(const SampP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t tex = (int64_t)blockIdx.x * (VC_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (tex >= p.texels) return;
    const int64_t j0 = lower_bound(p, tex), j1 = lower_bound(p, tex + 1), W = p.C + p.E;
    for (int c0 = l * 8; c0 < p.C; c0 += lc * 8) {
        float acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.f;
        // four entries at a time: their index, weight and row loads are independent; the sum keeps the entries' order
        for (int64_t j = j0; j < j1; j += 4) {
            float wt[4], g[4][8];
            int64_t off[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int64_t e = j + q < j1 ? p.order[j + q] : 0;
                e = e < 0 ? 0 : (e >= p.entries ? p.entries - 1 : e);
                const int64_t pair = e >> 2;
                const int bv = (int)(pair / p.N);
                const int b = bv / p.V;
                wt[q] = p.wts[e];
                off[q] = cond_row(p, b, bv - b * p.V, pair - (int64_t)bv * p.N) * W + c0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) load8(p.grad, off[q], p.cond_dt, g[q]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j + q < j1) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) acc[v] += g[q][v] * wt[q];
                }
        }
        store8(p.drows, tex * p.C + c0, p.rows_dt, acc);
    }
}

// dve[v, c] = the sum over (b, n) ascending of grad_cond[row(b, v, n), C + c]: 64 contiguous ranges, then those in order.  One
// workgroup per (view, 4 columns); a lane keeps four loads in flight and adds them in order.
constexpr int VC_VE_LANES = 64;
constexpr int VC_VE_CH = VC_BLOCK / VC_VE_LANES;

__global__ __launch_bounds__(VC_BLOCK) void sample_ve_kernel(const SampP p, uint32_t ctiles) {
    __shared__ float sh[VC_VE_LANES][VC_VE_CH];
    const int tid = threadIdx.x, ch = tid & (VC_VE_CH - 1), fl = tid / VC_VE_CH;
    const int v = blockIdx.x / ctiles, c = (int)(blockIdx.x % ctiles) * VC_VE_CH + ch;
    const int64_t W = p.C + p.E;
    float acc = 0.f;
    if (c < p.E) {
        const int64_t T = (int64_t)p.B * p.N, per = (T + VC_VE_LANES - 1) / VC_VE_LANES;
        const int64_t t0 = fl * per, t1 = t0 + per < T ? t0 + per : T;
        for (int64_t t = t0; t < t1; t += 4) {
            float val[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t tq = t + q < t1 ? t + q : t;
                const int b = (int)(tq / p.N);
                val[q] = load1(p.grad, cond_row(p, b, v, tq - (int64_t)b * p.N) * W + p.C + c, p.cond_dt);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (t + q < t1) acc += val[q];
        }
    }
    sh[fl][ch] = acc;
    __syncthreads();
    if (fl != 0 || c >= p.E) return;
    for (int i = 1; i < VC_VE_LANES; ++i) acc += sh[i][ch];
    store1(p.dve, (int64_t)v * p.E + c, p.ve_dt, acc);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
constexpr int64_t VC_MAX_ROWS = INT64_C(0x7fffffff);

int check_modln(int64_t R, int64_t C) {
    if (R < 0) return invalid_arg("volcond_modln: R must be >= 0");
    if (R > VC_MAX_ROWS) return unsupported("volcond_modln: R must be below 2^31");
    if (C < 8 || C > GDR_NORM_MAX_CHANNELS || C % 8) return unsupported("volcond_modln: C must be a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS");
    return GDR_OK;
}

int check_sample(const gdr_volcond_sample_args* a) {
    if (!a) return invalid_arg("volcond_sample: NULL args");
    if (a->B < 1 || a->V < 1 || a->r < 1 || a->n_group < 1 || a->img_h < 1 || a->img_w < 1 || a->h < 1 || a->w < 1 || a->E < 0)
        return invalid_arg("volcond_sample: B, V, r, n_group, h, w, img_h, img_w must be >= 1 and E >= 0");
    if (a->r % a->n_group) return invalid_arg("volcond_sample: n_group must divide r");
    if (a->C < 8 || a->C > GDR_VOLCOND_MAX_CHANNELS || a->C % 8) return unsupported("volcond_sample: C must be a multiple of 8 in 8..GDR_VOLCOND_MAX_CHANNELS");
    if (a->E % 8 || a->E > GDR_VOLCOND_MAX_CHANNELS) return unsupported("volcond_sample: E must be 0 or a multiple of 8 up to GDR_VOLCOND_MAX_CHANNELS");
    if (a->h > GDR_VOLCOND_MAX_SIDE || a->w > GDR_VOLCOND_MAX_SIDE) return unsupported("volcond_sample: h, w must be at most GDR_VOLCOND_MAX_SIDE");
    if (a->r > 1024) return unsupported("volcond_sample: r must be at most 1024");
    const int64_t N = (int64_t)a->r * a->r * a->r, bv = (int64_t)a->B * a->V;
    if (bv > GDR_VOLCOND_MAX_ENTRIES / 4 || N > GDR_VOLCOND_MAX_ENTRIES / 4 / bv)
        return unsupported("volcond_sample: 4 B V r^3 must be at most GDR_VOLCOND_MAX_ENTRIES");
    if (bv * a->h * a->w > VC_MAX_ROWS) return unsupported("volcond_sample: B V h w must be below 2^31");
    return GDR_OK;
}

void fill_sample(SampP& p, const gdr_volcond_sample_args* a) {
    p.B = a->B; p.V = a->V; p.h = a->h; p.w = a->w; p.C = a->C; p.E = a->E; p.r = a->r; p.g = a->n_group; p.bs = a->r / a->n_group;
    p.img_h = a->img_h; p.img_w = a->img_w;
    p.N = (int64_t)a->r * a->r * a->r;
    p.pairs = p.N * a->B * a->V; p.entries = p.pairs * 4; p.texels = (int64_t)a->B * a->V * a->h * a->w;
    int K;                                         // (C may need more than two pieces: the kernels loop over them)
    row_shape(a->C, &p.lc_shift, &K);
}

struct SampWs { size_t order, inverse, sort, sort_bytes, bytes; };

SampWs sample_workspace(int64_t entries) {
    SampWs w;
    w.order = 0;
    w.inverse = align_up((size_t)entries * 8);
    w.sort = w.inverse + align_up((size_t)entries * 8);
    w.sort_bytes = gdr_serial_sort_bytes(1, entries);
    w.bytes = w.sort + align_up(w.sort_bytes);
    return w;
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_volcond_ray_sh(const void* rays, int32_t rays_dtype, int64_t n, int32_t silu, float* out, void* stream) {
    if (n < 0) return invalid_arg("volcond_ray_sh: n must be >= 0");
    if (n > VC_MAX_ROWS / 32) return unsupported("volcond_ray_sh: 32 n must be below 2^31");
    if (bad_dtype(rays_dtype)) return invalid_arg("volcond_ray_sh: unknown dtype");
    if (n == 0) return GDR_OK;
    if (!rays || !out) return invalid_arg("volcond_ray_sh: NULL argument");
    if (misaligned(rays, (unsigned)esize(rays_dtype) - 1) || misaligned(out, 15)) return invalid_arg("volcond_ray_sh: unaligned buffer (out needs 16 bytes)");
    hipLaunchKernelGGL(ray_sh_kernel, dim3((uint32_t)div_up(n, VC_BLOCK)), dim3(VC_BLOCK), 0, (hipStream_t)stream, rays, rays_dtype, n,
                       silu ? 1 : 0, out);
    return launch_status("volcond ray_sh_kernel");
}

int gdr_volcond_modln_forward(const void* x, int64_t x_stride, int64_t x_inner, int64_t x_outer_stride, int32_t x_dtype, const void* shift_scale, int64_t ss_stride,
                              int32_t ss_dtype, const void* weight, int32_t weight_dtype, const void* bias, int32_t bias_dtype,
                              int64_t R, int32_t C, float eps, void* out, int32_t out_dtype, void* stream) {
    if (const int rc = check_modln(R, C)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(ss_dtype) || bad_dtype(out_dtype) || (weight && bad_dtype(weight_dtype)) || (bias && bad_dtype(bias_dtype)))
        return invalid_arg("volcond_modln_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("volcond_modln_forward: eps must be >= 0");
    if (R == 0) return GDR_OK;
    if (!x || !shift_scale || !out) return invalid_arg("volcond_modln_forward: NULL argument");
    if (bad_rows(x, x_stride, C) || x_inner < 1 || x_outer_stride < 0 || x_outer_stride % 8 || bad_rows(shift_scale, ss_stride, 2 * (int64_t)C) || misaligned(out, 15) || misaligned(weight, 15) ||
        misaligned(bias, 15))
        return invalid_arg("volcond_modln_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    ModP p = {};
    p.x = x; p.ss = shift_scale; p.weight = weight; p.bias = bias; p.out = out;
    p.R = R; p.x_stride = x_stride; p.x_inner = x_inner; p.x_outer = x_outer_stride; p.ss_stride = ss_stride;
    p.C = C; p.x_dt = x_dtype; p.ss_dt = ss_dtype; p.w_dt = weight_dtype; p.b_dt = bias_dtype; p.out_dt = out_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = VC_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((R + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    LN_LAUNCH_K(modln_fwd_kernel, K, grid, st, p);
    return launch_status("volcond modln_fwd_kernel");
}

size_t gdr_volcond_modln_backward_bytes(int64_t R, int32_t C) {
    if (check_modln(R, C)) return 0;
    return align_up((size_t)((R + VC_ROWS - 1) / VC_ROWS) * 2 * (size_t)C * 4) + 256;   // (never 0 for valid arguments)
}

int gdr_volcond_modln_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* x, int64_t x_stride,
                               int64_t x_inner, int64_t x_outer_stride, int32_t x_dtype, const void* shift_scale, int64_t ss_stride, int32_t ss_dtype, const void* weight,
                               int32_t weight_dtype, const void* bias, int32_t bias_dtype, int64_t R, int32_t C, float eps,
                               void* workspace, size_t workspace_bytes, void* grad_x, void* grad_shift_scale, void* grad_weight,
                               void* grad_bias, void* stream) {
    if (const int rc = check_modln(R, C)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(ss_dtype) || bad_dtype(grad_dtype) || ((weight || grad_weight) && bad_dtype(weight_dtype)) ||
        ((bias || grad_bias) && bad_dtype(bias_dtype)))
        return invalid_arg("volcond_modln_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("volcond_modln_backward: eps must be >= 0");
    if (!grad_x && !grad_shift_scale && !grad_weight && !grad_bias) return GDR_OK;   // nothing is wanted
    const bool params = grad_weight || grad_bias;
    if ((params && !workspace) || (R && (!grad_out || !x || !shift_scale))) return invalid_arg("volcond_modln_backward: NULL argument");
    if ((R && (bad_rows(x, x_stride, C) || x_inner < 1 || x_outer_stride < 0 || x_outer_stride % 8 || bad_rows(shift_scale, ss_stride, 2 * (int64_t)C) || bad_rows(grad_out, grad_stride, C))) ||
        misaligned(grad_x, 15) || misaligned(grad_shift_scale, 15) || misaligned(weight, 15) || misaligned(bias, 15) ||
        misaligned(grad_weight, (unsigned)esize(weight_dtype) - 1) || misaligned(grad_bias, (unsigned)esize(bias_dtype) - 1) ||
        misaligned(workspace, 255))
        return invalid_arg("volcond_modln_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    const int64_t slabs = (R + VC_ROWS - 1) / VC_ROWS;
    if (params && workspace_bytes < align_up((size_t)slabs * 2 * (size_t)C * 4))
        return workspace_too_small("volcond_modln_backward: workspace smaller than gdr_volcond_modln_backward_bytes");
    ModP p = {};
    p.x = x; p.ss = shift_scale; p.weight = weight; p.bias = bias; p.grad = grad_out;
    p.dx = grad_x; p.dss = grad_shift_scale; p.part = params ? (float*)workspace : nullptr;
    p.R = R; p.x_stride = x_stride; p.x_inner = x_inner; p.x_outer = x_outer_stride; p.ss_stride = ss_stride; p.grad_stride = grad_stride;
    p.C = C; p.x_dt = x_dtype; p.ss_dt = ss_dtype; p.w_dt = weight_dtype; p.b_dt = bias_dtype; p.out_dt = grad_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const hipStream_t st = (hipStream_t)stream;
    if (slabs) LN_LAUNCH_K(modln_bwd_kernel, K, dim3((uint32_t)slabs), st, p);
    if (params) launch_ln_fold<false>(p.part, slabs, C, grad_weight, weight_dtype, grad_bias, bias_dtype, st);
    return launch_status("volcond modln_bwd kernels");
}

int gdr_volcond_sample_forward(const gdr_volcond_sample_args* a, const void* rows, int32_t rows_dtype, const float* points,
                               const float* w2cs, const float* ixts, const void* view_embed, int64_t ve_stride, int32_t ve_dtype,
                               void* cond, int32_t cond_dtype, int64_t* keys, float* weights, void* stream) {
    if (const int rc = check_sample(a)) return rc;
    if (bad_dtype(rows_dtype) || bad_dtype(cond_dtype) || (a->E && bad_dtype(ve_dtype))) return invalid_arg("volcond_sample_forward: unknown dtype");
    if (!rows || !points || !w2cs || !ixts || !cond || (a->E && !view_embed) || (!keys != !weights))
        return invalid_arg("volcond_sample_forward: NULL argument");
    if (misaligned(rows, 15) || misaligned(cond, 15) || misaligned(points, 3) || misaligned(w2cs, 3) || misaligned(ixts, 3) ||
        misaligned(keys, 7) || misaligned(weights, 3) || (a->E && (bad_rows(view_embed, ve_stride, a->E))))
        return invalid_arg("volcond_sample_forward: unaligned buffer (rows, cond and view_embed rows need 16 bytes)");
    SampP p = {};
    fill_sample(p, a);
    p.rows = rows; p.pts = points; p.w2c = w2cs; p.ixt = ixts; p.ve = view_embed; p.ve_stride = ve_stride; p.cond = cond;
    p.keys = keys; p.wts = weights; p.rows_dt = rows_dtype; p.ve_dt = ve_dtype; p.cond_dt = cond_dtype;
    const int64_t groups = VC_BLOCK >> p.lc_shift;
    hipLaunchKernelGGL(sample_fwd_kernel, dim3((uint32_t)div_up(p.pairs, groups)), dim3(VC_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("volcond sample_fwd_kernel");
}

size_t gdr_volcond_sample_backward_bytes(const gdr_volcond_sample_args* a) {
    if (check_sample(a)) return 0;
    const int64_t entries = (int64_t)a->r * a->r * a->r * a->B * a->V * 4;
    return sample_workspace(entries).bytes + 256;
}

int gdr_volcond_sample_backward(const gdr_volcond_sample_args* a, const void* grad_cond, int32_t grad_dtype, const int64_t* keys,
                                const float* weights, void* workspace, size_t workspace_bytes, void* grad_rows, int32_t rows_dtype,
                                void* grad_view_embed, int32_t ve_dtype, void* stream) {
    if (const int rc = check_sample(a)) return rc;
    if (bad_dtype(grad_dtype) || (grad_rows && bad_dtype(rows_dtype)) || (grad_view_embed && bad_dtype(ve_dtype)))
        return invalid_arg("volcond_sample_backward: unknown dtype");
    if (!grad_rows && !grad_view_embed) return GDR_OK;   // nothing is wanted
    if (!grad_cond || (grad_rows && (!keys || !weights || !workspace))) return invalid_arg("volcond_sample_backward: NULL argument");
    if (grad_view_embed && !a->E) return invalid_arg("volcond_sample_backward: grad_view_embed without view_embed columns");
    if (misaligned(grad_cond, 15) || misaligned(grad_rows, 15) || misaligned(grad_view_embed, (unsigned)esize(ve_dtype) - 1) ||
        misaligned(keys, 7) || misaligned(weights, 3) || misaligned(workspace, 255))
        return invalid_arg("volcond_sample_backward: unaligned buffer");
    SampP p = {};
    fill_sample(p, a);
    p.grad = grad_cond; p.cond_dt = grad_dtype; p.drows = grad_rows; p.rows_dt = rows_dtype; p.dve = grad_view_embed; p.ve_dt = ve_dtype;
    p.keys = const_cast<int64_t*>(keys); p.wts = const_cast<float*>(weights);
    const hipStream_t st = (hipStream_t)stream;
    if (grad_rows) {
        const SampWs ws = sample_workspace(p.entries);
        if (workspace_bytes < ws.bytes) return workspace_too_small("volcond_sample_backward: workspace smaller than gdr_volcond_sample_backward_bytes");
        char* base = (char*)workspace;
        int bits = 1;
        while (bits < 63 && (INT64_C(1) << bits) <= p.texels) ++bits;
        if (const int rc = gdr_serial_sort(keys, 1, p.entries, bits, base + ws.sort, ws.sort_bytes, (int64_t*)(base + ws.order),
                                           (int64_t*)(base + ws.inverse), stream))
            return rc;
        p.order = (const int64_t*)(base + ws.order);
        const int64_t groups = VC_BLOCK >> p.lc_shift;
        hipLaunchKernelGGL(sample_bwd_kernel, dim3((uint32_t)div_up(p.texels, groups)), dim3(VC_BLOCK), 0, st, p);
    }
    if (grad_view_embed) {
        const uint32_t ctiles = (uint32_t)((a->E + VC_VE_CH - 1) / VC_VE_CH);
        hipLaunchKernelGGL(sample_ve_kernel, dim3((uint32_t)a->V * ctiles), dim3(VC_BLOCK), 0, st, p, ctiles);
    }
    return launch_status("volcond sample_bwd kernels");
}

}  // extern "C"

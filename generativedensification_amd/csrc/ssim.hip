// ssim.hip — fused SSIM / MS-SSIM, forward and backward (include/gdr.h gdr_ssim_*), the image-similarity half of the
// training loss MSE + 0.5 (1 - MS-SSIM) and the SSIM of the evaluation.
//
// Specification (a restatement of the published algorithm of pytorch_msssim 1.x; not pinned against that package):
//   window   g[i] = exp(-(i - k/2)^2 / (2 sigma^2)), i = 0..k-1, normalised to sum 1 (the caller passes it, k odd <= 15).
//            Applied separably, first along H then along W, VALID (no padding): an h x w map gives (h-k+1) x (w-k+1).
//   terms    mu_x = G*X, mu_y = G*Y, s_xx = G*(X X) - mu_x^2, s_yy = G*(Y Y) - mu_y^2, s_xy = G*(X Y) - mu_x mu_y,
//            cs = (2 s_xy + C2) / (s_xx + s_yy + C2), ssim_map = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs;
//            per (batch, channel) plane: ssim = mean(ssim_map), cs = mean(cs_map) over the valid region.
//   ssim     per plane ssim, relu'd when nonnegative (GDR_SSIM_NONNEG).
//   ms_ssim  L levels with weights w_l: at levels 0..L-2 keep relu(cs), then 2x2 average-pool X and Y with padding
//            size % 2 per axis and count_include_pad (output j averages inputs 2j - pad and 2j - pad + 1, out-of-range
//            inputs read as 0, divisor always 4); the last level keeps relu(ssim); value = prod_l v_l^w_l per plane.
//   backward d value / d X (and Y) as torch autograd through the formulas above; a plane where relu clamps a level gets
//            an exactly zero gradient (torch: pow / prod give the clamped entry an infinite factor that relu's mask zeroes).
//
// Structure, per level l (sizes h_l x w_l, valid region hv x wv = (h_l-k+1) x (w_l-k+1), P = B*C planes):
//   forward   ssim_tile_kernel<K, false>: a 16 x 64 tile of the valid region plus a (k-1) halo of X and Y in LDS, the five
//             moments blurred along H then W, per-block sums of ssim_map and cs (fixed order) into partials[l][p][tile];
//             ssim_pool_kernel writes the pooled X, Y of level l+1 into the workspace (kept for backward).
//             ssim_finalize_kernel: one block per plane sums the partials of every level in a fixed order (bitwise
//             reproducible, no float atomics), applies relu / pow / prod and writes the plane's value and, per level,
//             coef[p][l] = d value / d mean_l.
//   backward  coarsest level first.  ssim_tile_kernel<K, true> recomputes the moments of the tile and writes, per valid
//             pixel, G * d f / d(mu_x, mu_y, E_xx = E_yy, E_xy) (G = upstream grad x coef / (hv wv), f = cs_map or
//             ssim_map) as one float4; ssim_grad_kernel<K> applies the transposed (full-extent) blur to the four maps and
//             forms dX = T(a_x) + 2X T(b) + Y T(c) (dY symmetric) plus the transposed 2x2 pool of level l+1's gradient.
// Level 0 reads X, Y and writes dX, dY through arbitrary element strides (the caller's permuted NHWC view is read in place);
// the pyramid levels are dense fp32 planes.  No host synchronisation; every launch on the caller's stream.
#include <algorithm>

#include "gdr_common.h"
#include "host_util.h"

namespace gdr {
namespace {

constexpr int SS_TX = 64;                    // tile width (valid-region pixels forward, input pixels in ssim_grad_kernel)
constexpr int SS_TY = 16;                    // tile height
constexpr int SS_ROWS = SS_TY * SS_TX / GDR_BLOCK;   // outputs per thread (one column, SS_ROWS rows 4 apart)

struct SsWin { float g[GDR_SSIM_MAX_WIN]; };

// one image level: element (p, y, x) of plane p = b*C + c at base + b*s[0] + c*s[1] + y*s[2] + x*s[3]
struct SsPlane {
    const float* base; int64_t s[4]; int C;
    __device__ __forceinline__ int64_t off(int p, int y, int x) const {
        return (int64_t)(p / C) * s[0] + (int64_t)(p % C) * s[1] + (int64_t)y * s[2] + (int64_t)x * s[3];
    }
    __device__ __forceinline__ float at(int p, int y, int x) const { return base[off(p, y, x)]; }
};

struct SsOut {
    float* base; int64_t s[4]; int C;
    __device__ __forceinline__ float& at(int p, int y, int x) const {
        return base[(int64_t)(p / C) * s[0] + (int64_t)(p % C) * s[1] + (int64_t)y * s[2] + (int64_t)x * s[3]];
    }
};

// block-wide sum of two values in a fixed order (wave shuffles, then the 4 wave sums in index order)
__device__ __forceinline__ float2 block_sum2(float a, float b, float2* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(a, b);
    __syncthreads();
    return make_float2((red[0].x + red[1].x) + (red[2].x + red[3].x), (red[0].y + red[1].y) + (red[2].y + red[3].y));
}

// Forward (BWD = false): per-block sums of ssim_map and cs_map over the tile -> part[(p * tiles + tile) * 2 + {0, 1}].
// Backward (BWD = true): per valid pixel G * d f / d(mu_x, mu_y, E_xx, E_xy) -> cmap[(p * hv + y) * wv + x] with
// G = go[p] * coef[p * L + l] / (hv * wv) and f = ssim_map on the last level (last != 0), cs_map below it.
template <int K, bool BWD>
__global__ __launch_bounds__(GDR_BLOCK) void ssim_tile_kernel(SsPlane X, SsPlane Y, int h, int w, SsWin win, float C1,
                                                              float C2, int last, float* __restrict__ part,
                                                              const float* __restrict__ go, const float* __restrict__ coef,
                                                              int L, int l, float4* __restrict__ cmap) {
    constexpr int IW = SS_TX + K - 1, IH = SS_TY + K - 1;
    __shared__ float sx[IH][IW], sy[IH][IW];
    __shared__ float sv[5][SS_TY][IW];
    __shared__ float2 red[GDR_BLOCK / GDR_WAVE];
    const int hv = h - K + 1, wv = w - K + 1;
    const int p = blockIdx.z, x0 = blockIdx.x * SS_TX, y0 = blockIdx.y * SS_TY;
    for (int i = threadIdx.x; i < IH * IW; i += GDR_BLOCK) {
        const int r = i / IW, c = i - r * IW, gy = y0 + r, gx = x0 + c;
        const bool in = gy < h && gx < w;
        sx[r][c] = in ? X.at(p, gy, gx) : 0.f;
        sy[r][c] = in ? Y.at(p, gy, gx) : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_TY * IW; i += GDR_BLOCK) {   // along H
        const int r = i / IW, c = i - r * IW;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const float g = win.g[t], a = sx[r + t][c], b = sy[r + t][c];
            m[0] = fmaf(g, a, m[0]);
            m[1] = fmaf(g, b, m[1]);
            m[2] = fmaf(g, a * a, m[2]);
            m[3] = fmaf(g, b * b, m[3]);
            m[4] = fmaf(g, a * b, m[4]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) sv[k][r][c] = m[k];
    }
    __syncthreads();
    const int c = threadIdx.x & (SS_TX - 1), x = x0 + c;
    float s_ssim = 0.f, s_cs = 0.f, G = 0.f;
    if (BWD) G = go[p] * coef[p * L + l] / ((float)hv * (float)wv);
#pragma unroll
    for (int j = 0; j < SS_ROWS; ++j) {
        const int r = (threadIdx.x >> 6) + j * (GDR_BLOCK / SS_TX), y = y0 + r;
        if (y >= hv || x >= wv) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {   // along W
            const float g = win.g[t];
#pragma unroll
            for (int k = 0; k < 5; ++k) m[k] = fmaf(g, sv[k][r][c + t], m[k]);
        }
        const float mx = m[0], my = m[1];
        const float sxx = m[2] - mx * mx, syy = m[3] - my * my, sxy = m[4] - mx * my;
        const float A1 = 2.f * mx * my + C1, B1 = mx * mx + my * my + C1;
        const float A2 = 2.f * sxy + C2, B2 = sxx + syy + C2;
        const float cs = A2 / B2, lum = A1 / B1;
        if (!BWD) {
            s_ssim += lum * cs;
            s_cs += cs;
        } else {
            // f = cs:       df/dmx = (2 mx cs - 2 my) / B2, df/dE_xx = df/dE_yy = -cs / B2, df/dE_xy = 2 / B2
            // f = lum * cs: lum * (the above) + cs * dlum/dmx, dlum/dmx = (2 my - 2 mx lum) / B1
            const float inv2 = 1.f / B2;
            float ax = (2.f * mx * cs - 2.f * my) * inv2, ay = (2.f * my * cs - 2.f * mx) * inv2;
            float b = -cs * inv2, cc = 2.f * inv2;
            if (last) {
                const float inv1 = 1.f / B1;
                ax = lum * ax + cs * (2.f * my - 2.f * mx * lum) * inv1;
                ay = lum * ay + cs * (2.f * mx - 2.f * my * lum) * inv1;
                b *= lum;
                cc *= lum;
            }
            cmap[((int64_t)p * hv + y) * wv + x] = make_float4(G * ax, G * ay, G * b, G * cc);
        }
    }
    if (!BWD) {
        const float2 s = block_sum2(s_ssim, s_cs, red);
        if (threadIdx.x == 0) {
            const int tile = blockIdx.y * gridDim.x + blockIdx.x;
            const int64_t o = ((int64_t)p * gridDim.x * gridDim.y + tile) * 2;
            part[o] = s.x;
            part[o + 1] = s.y;
        }
    }
}

// dX (and dY when DY) of one level over a 16 x 64 tile of its INPUT pixels: the transposed blur of the four coefficient
// maps (read with a (k-1) halo up and left, zero outside the valid region), combined with X, Y, plus the transposed 2x2
// pool of the coarser level's gradient (dnext, dense (P, h2, w2); NULL on the coarsest level).
template <int K, bool DY>
__global__ __launch_bounds__(GDR_BLOCK) void ssim_grad_kernel(SsPlane X, SsPlane Y, int h, int w, SsWin win,
                                                              const float4* __restrict__ cmap,
                                                              const float* __restrict__ dnx, const float* __restrict__ dny,
                                                              SsOut dX, SsOut dY) {
    constexpr int IW = SS_TX + K - 1, IH = SS_TY + K - 1;
    __shared__ float sc[4][IH][IW];
    __shared__ float sv[4][SS_TY][IW];
    const int hv = h - K + 1, wv = w - K + 1;
    const int p = blockIdx.z, x0 = blockIdx.x * SS_TX, y0 = blockIdx.y * SS_TY;
    // local (r, c) holds valid-region pixel (y0 - (K-1) + r, x0 - (K-1) + c)
    for (int i = threadIdx.x; i < IH * IW; i += GDR_BLOCK) {
        const int r = i / IW, c = i - r * IW, gy = y0 - (K - 1) + r, gx = x0 - (K - 1) + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < hv && gx >= 0 && gx < wv) v = cmap[((int64_t)p * hv + gy) * wv + gx];
        sc[0][r][c] = v.x;
        sc[1][r][c] = v.y;
        sc[2][r][c] = v.z;
        sc[3][r][c] = v.w;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_TY * IW; i += GDR_BLOCK) {   // transposed along H: out(y) = sum_t g[t] in(y - t)
        const int r = i / IW, c = i - r * IW;
        float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const float g = win.g[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = fmaf(g, sc[k][r + (K - 1) - t][c], m[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sv[k][r][c] = m[k];
    }
    __syncthreads();
    const int c = threadIdx.x & (SS_TX - 1), x = x0 + c;
    const int padx = w & 1, pady = h & 1, w2 = (w + padx) >> 1, h2 = (h + pady) >> 1;
#pragma unroll
    for (int j = 0; j < SS_ROWS; ++j) {
        const int r = (threadIdx.x >> 6) + j * (GDR_BLOCK / SS_TX), y = y0 + r;
        if (y >= h || x >= w) continue;
        float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {   // transposed along W
            const float g = win.g[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = fmaf(g, sv[k][r][c + (K - 1) - t], m[k]);
        }
        const float a = X.at(p, y, x), b = Y.at(p, y, x);
        float gx = m[0] + 2.f * a * m[2] + b * m[3];
        float gy = m[1] + 2.f * b * m[2] + a * m[3];
        if (dnx) {
            const int64_t o = ((int64_t)p * h2 + ((y + pady) >> 1)) * w2 + ((x + padx) >> 1);
            gx += 0.25f * dnx[o];
            if (DY) gy += 0.25f * dny[o];
        }
        dX.at(p, y, x) = gx;
        if (DY) dY.at(p, y, x) = gy;
    }
}

// 2x2 average pool, padding (h % 2, w % 2), count_include_pad: out (P, h2, w2) dense
__global__ __launch_bounds__(GDR_BLOCK) void ssim_pool_kernel(SsPlane X, SsPlane Y, int P, int h, int w,
                                                              float* __restrict__ ox, float* __restrict__ oy) {
    const int padx = w & 1, pady = h & 1, w2 = (w + padx) >> 1, h2 = (h + pady) >> 1;
    const int64_t n = (int64_t)P * h2 * w2;
    for (int64_t i = (int64_t)blockIdx.x * GDR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GDR_BLOCK) {
        const int j = (int)(i % w2), k = (int)((i / w2) % h2), p = (int)(i / ((int64_t)w2 * h2));
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * k - pady + dy, x = 2 * j - padx + dx;
                if (y >= 0 && y < h && x >= 0 && x < w) {
                    sa += X.at(p, y, x);
                    sb += Y.at(p, y, x);
                }
            }
        }
        ox[i] = 0.25f * sa;
        oy[i] = 0.25f * sb;
    }
}

struct SsLevels {
    int h[GDR_SSIM_MAX_LEVELS], w[GDR_SSIM_MAX_LEVELS], tiles[GDR_SSIM_MAX_LEVELS];
    int64_t part_off[GDR_SSIM_MAX_LEVELS];   // floats into the partials
    double count[GDR_SSIM_MAX_LEVELS];       // valid pixels per plane
};

// one block per plane: the partials of every level summed in a fixed order (double), then relu / pow / prod
__global__ __launch_bounds__(GDR_BLOCK) void ssim_finalize_kernel(const float* __restrict__ part, SsLevels lv, int L,
                                                                  int mode, SsWin wts, float* __restrict__ out,
                                                                  float* __restrict__ coef) {
    __shared__ double red[2][GDR_BLOCK];
    __shared__ float mean[GDR_SSIM_MAX_LEVELS];
    const int p = blockIdx.x;
    for (int l = 0; l < L; ++l) {
        const int T = lv.tiles[l];
        const float* q = part + lv.part_off[l] + (int64_t)p * T * 2;
        double a = 0.0, b = 0.0;
        for (int t = threadIdx.x; t < T; t += GDR_BLOCK) {
            a += (double)q[2 * t];
            b += (double)q[2 * t + 1];
        }
        red[0][threadIdx.x] = a;
        red[1][threadIdx.x] = b;
        __syncthreads();
        for (int s = GDR_BLOCK / 2; s > 0; s >>= 1) {
            if (threadIdx.x < s) {
                red[0][threadIdx.x] += red[0][threadIdx.x + s];
                red[1][threadIdx.x] += red[1][threadIdx.x + s];
            }
            __syncthreads();
        }
        // ms_ssim keeps cs below the last level and ssim on it; ssim() has one level
        if (threadIdx.x == 0) mean[l] = (float)((l == L - 1 ? red[0][0] : red[1][0]) / lv.count[l]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float m[GDR_SSIM_MAX_LEVELS];
    for (int l = 0; l < L; ++l) m[l] = mean[l];
    if (mode != GDR_SSIM_MS) {
        const float v = m[0];
        out[p] = (mode == GDR_SSIM_NONNEG && !(v > 0.f)) ? 0.f : v;
        coef[p] = (mode == GDR_SSIM_NONNEG && !(v > 0.f)) ? 0.f : 1.f;
        return;
    }
    float pw[GDR_SSIM_MAX_LEVELS], prod = 1.f;
    for (int l = 0; l < L; ++l) {
        pw[l] = powf(fmaxf(m[l], 0.f), wts.g[l]);
        prod *= pw[l];
    }
    out[p] = prod;
    for (int l = 0; l < L; ++l) {
        float others = 1.f;
        for (int k = 0; k < L; ++k)
            if (k != l) others *= pw[k];
        coef[p * L + l] = m[l] > 0.f ? others * wts.g[l] * powf(m[l], wts.g[l] - 1.f) : 0.f;
    }
}

}  // namespace
}  // namespace gdr

// ---- host side -------------------------------------------------------------------------------------------------------
using namespace gdr;

namespace {

struct SsLayout {
    int L, K, P;
    SsLevels lv;
    // forward workspace (kept for backward): pooled pyramid of levels 1..L-1, partials, per-(plane, level) coefficients
    size_t px[GDR_SSIM_MAX_LEVELS], py[GDR_SSIM_MAX_LEVELS], part, coef, ws_bytes;
    // backward scratch: the float4 coefficient map (sized for level 0) and the gradient pyramids of levels 1..L-1
    size_t cmap, gx[GDR_SSIM_MAX_LEVELS], gy[GDR_SSIM_MAX_LEVELS], scratch_bytes;
};

// NULL = valid; otherwise the reason the arguments are refused
const char* ssim_layout(const gdr_ssim_args* a, int want_dy, SsLayout* o) {
    if (!a) return "NULL args";
    if (a->B <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return "B, C, H, W must be positive";
    if ((int64_t)a->B * a->C > 65535) return "B * C exceeds 65535 planes";
    if (a->win_size < 1 || a->win_size > GDR_SSIM_MAX_WIN || !(a->win_size & 1)) return "win_size must be odd, 1..15";
    if (a->mode != GDR_SSIM_PLAIN && a->mode != GDR_SSIM_NONNEG && a->mode != GDR_SSIM_MS) return "unknown mode";
    if (a->levels < 1 || a->levels > GDR_SSIM_MAX_LEVELS || (a->mode != GDR_SSIM_MS && a->levels != 1))
        return "levels must be 1 (ssim) or 1..8 (ms_ssim)";
    o->L = a->levels;
    o->K = a->win_size;
    o->P = a->B * a->C;
    size_t off = 0, part = 0;
    int h = a->H, w = a->W;
    for (int l = 0; l < o->L; ++l) {
        if (h < o->K || w < o->K) return "image smaller than the window at some level";
        o->lv.h[l] = h;
        o->lv.w[l] = w;
        const int hv = h - o->K + 1, wv = w - o->K + 1;
        o->lv.tiles[l] = div_up(wv, SS_TX) * div_up(hv, SS_TY);
        o->lv.count[l] = (double)hv * (double)wv;
        o->lv.part_off[l] = (int64_t)part;
        part += (size_t)o->P * o->lv.tiles[l] * 2;
        o->px[l] = o->py[l] = 0;
        if (l > 0) {
            const size_t n = align_up((size_t)o->P * h * w * sizeof(float));
            o->px[l] = off;
            o->py[l] = off + n;
            off += 2 * n;
        }
        h = (h + (h & 1)) >> 1;
        w = (w + (w & 1)) >> 1;
    }
    o->part = off;
    off += align_up(part * sizeof(float));
    o->coef = off;
    off += align_up((size_t)o->P * o->L * sizeof(float));
    o->ws_bytes = off;
    off = 0;
    o->cmap = off;
    off += align_up((size_t)o->P * (a->H - o->K + 1) * (a->W - o->K + 1) * sizeof(float4));
    for (int l = 0; l < o->L; ++l) {
        o->gx[l] = o->gy[l] = 0;
        if (l == 0) continue;
        const size_t n = align_up((size_t)o->P * o->lv.h[l] * o->lv.w[l] * sizeof(float));
        o->gx[l] = off;
        off += n;
        if (want_dy) {
            o->gy[l] = off;
            off += n;
        }
    }
    o->scratch_bytes = off;
    return nullptr;
}

SsPlane plane(const float* base, const int64_t* s, int C) {
    SsPlane p;
    p.base = base;
    for (int i = 0; i < 4; ++i) p.s[i] = s[i];
    p.C = C;
    return p;
}

SsPlane dense(const float* base, int h, int w) {
    const int64_t s[4] = {(int64_t)h * w, 0, w, 1};
    return plane(base, s, 1);   // plane p at p * h * w
}

SsWin window(const gdr_ssim_args* a) {
    SsWin g = {};
    for (int t = 0; t < a->win_size; ++t) g.g[t] = a->win[t];
    return g;
}

#define GDR_SSIM_DISPATCH(K, CALL)                                                                                        \
    switch (K) {                                                                                                          \
        case 1: CALL(1); break;                                                                                           \
        case 3: CALL(3); break;                                                                                           \
        case 5: CALL(5); break;                                                                                           \
        case 7: CALL(7); break;                                                                                           \
        case 9: CALL(9); break;                                                                                           \
        case 11: CALL(11); break;                                                                                         \
        case 13: CALL(13); break;                                                                                         \
        default: CALL(15); break;                                                                                         \
    }

}  // namespace

extern "C" {

size_t gdr_ssim_workspace_bytes(const gdr_ssim_args* a) {
    SsLayout o;
    if (const char* why = ssim_layout(a, 0, &o)) { invalid_arg(why); return 0; }
    return o.ws_bytes;
}

size_t gdr_ssim_scratch_bytes(const gdr_ssim_args* a, int32_t want_dy) {
    SsLayout o;
    if (const char* why = ssim_layout(a, want_dy, &o)) { invalid_arg(why); return 0; }
    return o.scratch_bytes;
}

int gdr_ssim_forward(const gdr_ssim_args* a, const float* X, const int64_t* x_strides, const float* Y,
                     const int64_t* y_strides, void* workspace, float* out, void* stream) {
    SsLayout o;
    if (const char* why = ssim_layout(a, 0, &o)) return invalid_arg(why);
    if (!X || !Y || !x_strides || !y_strides || !workspace || !out) return invalid_arg("ssim_forward: NULL argument");
    if (misaligned(workspace, 255)) return invalid_arg("ssim_forward: workspace unaligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* part = (float*)(ws + o.part);
    const SsWin win = window(a);
    SsPlane x = plane(X, x_strides, a->C), y = plane(Y, y_strides, a->C);
    for (int l = 0; l < o.L; ++l) {
        const int h = o.lv.h[l], w = o.lv.w[l];
        const dim3 grid(div_up(w - o.K + 1, SS_TX), div_up(h - o.K + 1, SS_TY), o.P);
        float* pl = part + o.lv.part_off[l];
#define GDR_SSIM_FWD(KK)                                                                                                  \
    hipLaunchKernelGGL((ssim_tile_kernel<KK, false>), grid, dim3(GDR_BLOCK), 0, st, x, y, h, w, win, a->C1, a->C2,        \
                       (int)(l == o.L - 1), pl, (const float*)nullptr, (const float*)nullptr, o.L, l, (float4*)nullptr)
        GDR_SSIM_DISPATCH(o.K, GDR_SSIM_FWD)
#undef GDR_SSIM_FWD
        if (int rc = launch_status("ssim_tile_kernel")) return rc;
        if (l + 1 < o.L) {
            const int h2 = o.lv.h[l + 1], w2 = o.lv.w[l + 1];
            float* nx = (float*)(ws + o.px[l + 1]);
            float* ny = (float*)(ws + o.py[l + 1]);
            const int grid_p = (int)std::min<int64_t>(div_up((int64_t)o.P * h2 * w2, GDR_BLOCK), 8192);
            hipLaunchKernelGGL(ssim_pool_kernel, dim3(grid_p), dim3(GDR_BLOCK), 0, st, x, y, o.P, h, w, nx, ny);
            if (int rc = launch_status("ssim_pool_kernel")) return rc;
            x = dense(nx, h2, w2);
            y = dense(ny, h2, w2);
        }
    }
    SsWin wts = {};
    for (int l = 0; l < o.L; ++l) wts.g[l] = a->weights[l];
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(o.P), dim3(GDR_BLOCK), 0, st, (const float*)part, o.lv, o.L, a->mode,
                       wts, out, (float*)(ws + o.coef));
    return launch_status("ssim_finalize_kernel");
}

int gdr_ssim_backward(const gdr_ssim_args* a, const float* X, const int64_t* x_strides, const float* Y,
                      const int64_t* y_strides, const void* workspace, const float* grad_out, float* dX,
                      const int64_t* dx_strides, float* dY, const int64_t* dy_strides, void* scratch, void* stream) {
    SsLayout o;
    const bool want_dy = dY != nullptr;
    if (const char* why = ssim_layout(a, want_dy, &o)) return invalid_arg(why);
    if (!X || !Y || !x_strides || !y_strides || !workspace || !grad_out || !dX || !dx_strides || !scratch ||
        (want_dy && !dy_strides))
        return invalid_arg("ssim_backward: NULL argument");
    if (misaligned(workspace, 255) || misaligned(scratch, 255)) return invalid_arg("ssim_backward: workspace unaligned");
    hipStream_t st = (hipStream_t)stream;
    const char* ws = (const char*)workspace;
    char* sc = (char*)scratch;
    const float* coef = (const float*)(ws + o.coef);
    float4* cmap = (float4*)(sc + o.cmap);
    const SsWin win = window(a);
    for (int l = o.L - 1; l >= 0; --l) {
        const int h = o.lv.h[l], w = o.lv.w[l];
        const SsPlane x = l ? dense((const float*)(ws + o.px[l]), h, w) : plane(X, x_strides, a->C);
        const SsPlane y = l ? dense((const float*)(ws + o.py[l]), h, w) : plane(Y, y_strides, a->C);
        const dim3 gv(div_up(w - o.K + 1, SS_TX), div_up(h - o.K + 1, SS_TY), o.P);
#define GDR_SSIM_COEF(KK)                                                                                                 \
    hipLaunchKernelGGL((ssim_tile_kernel<KK, true>), gv, dim3(GDR_BLOCK), 0, st, x, y, h, w, win, a->C1, a->C2,           \
                       (int)(l == o.L - 1), (float*)nullptr, grad_out, coef, o.L, l, cmap)
        GDR_SSIM_DISPATCH(o.K, GDR_SSIM_COEF)
#undef GDR_SSIM_COEF
        if (int rc = launch_status("ssim_tile_kernel (backward)")) return rc;
        const float* dnx = l + 1 < o.L ? (const float*)(sc + o.gx[l + 1]) : nullptr;
        const float* dny = l + 1 < o.L && want_dy ? (const float*)(sc + o.gy[l + 1]) : nullptr;
        SsOut ox, oy;
        if (l == 0) {
            ox.base = dX;
            for (int i = 0; i < 4; ++i) ox.s[i] = dx_strides[i];
            ox.C = a->C;
            oy.base = dY;
            for (int i = 0; i < 4; ++i) oy.s[i] = want_dy ? dy_strides[i] : 0;
            oy.C = a->C;
        } else {
            const SsPlane px = dense((const float*)(sc + o.gx[l]), h, w), py = dense((const float*)(sc + o.gy[l]), h, w);
            ox.base = (float*)px.base;
            oy.base = want_dy ? (float*)py.base : nullptr;
            for (int i = 0; i < 4; ++i) ox.s[i] = oy.s[i] = px.s[i];
            ox.C = oy.C = px.C;
        }
        const dim3 gi(div_up(w, SS_TX), div_up(h, SS_TY), o.P);
#define GDR_SSIM_GRAD(KK)                                                                                                 \
    if (want_dy)                                                                                                          \
        hipLaunchKernelGGL((ssim_grad_kernel<KK, true>), gi, dim3(GDR_BLOCK), 0, st, x, y, h, w, win,                     \
                           (const float4*)cmap, dnx, dny, ox, oy);                                                        \
    else                                                                                                                  \
        hipLaunchKernelGGL((ssim_grad_kernel<KK, false>), gi, dim3(GDR_BLOCK), 0, st, x, y, h, w, win,                    \
                           (const float4*)cmap, dnx, dny, ox, oy)
        GDR_SSIM_DISPATCH(o.K, GDR_SSIM_GRAD)
#undef GDR_SSIM_GRAD
        if (int rc = launch_status("ssim_grad_kernel")) return rc;
    }
    return GDR_OK;
}

}  // extern "C"

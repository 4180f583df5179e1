// norm.hip — the two row normalisations of the point decoder that sit between its kernels (include/gdr.h gdr_norm_*):
//
//   ada    out[i] = scale[b] * (feat[i] - mean_i) * rstd_i for row i of segment b (offset[b - 1] <= i < offset[b], offset[-1] = 0),
//          mean / biased variance over the C channels, rstd = 1 / sqrt(var + eps); rows behind offset[B - 1] are zero.  The
//          reference's AdaLayerNorm: gather_csr(affine(global_feat), [0, offset]) * layer_norm(feat).
//          backward, xh the normalised row, g = grad_out, means over the C channels:
//            dxh = g * scale[b];  dfeat[i] = rstd_i * (dxh - mean(dxh) - xh * mean(dxh * xh));  dscale[b] = sum_i g[i] * xh[i]
//   pe     out[r] = layer_norm([sin(f_k x[r, j]) at 3k + j, cos(f_k x[r, j]) at 3F + 3k + j, feat[r / S]]), no affine, over the
//          W = 6F + C entries: UpscaleModule's gather_csr + positional_encoding + cat + LayerNorm.
//          backward, dz = rstd * (g - mean(g) - zh * mean(g * zh)):
//            dx[r, j] = sum_k f_k * (cos * dz_sin - sin * dz_cos);  dfeat[p] = sum over the S children of dz_feat
//
// Everything is computed in f32 whatever the storage types, and the statistics are recomputed in the backward (nothing is
// saved but the inputs).  No atomics: every output element has one writer and every sum a fixed order, so two runs are
// bitwise equal.  No entry point allocates or synchronises.
//
// Mapping: a row is held by a group of LC lanes, LC the power of two in 8..64 that covers C / 8; lane l holds the 8 channels
// behind 8 * l (and, at C > 512, the 8 behind 8 * (l + 64)): one 16-byte access per lane for 16-bit rows, two for f32 rows.  A
// workgroup of 256 threads holds 256 / LC groups.  Row sums are xor butterflies inside the group, which give every lane the
// same bits.  Mean first, then the squared deviations (two passes over registers).
//   ada forward   one row per group.
//   ada backward  a workgroup takes GDR_NORM_ROWS consecutive rows and walks them by pieces (the maximal ranges that lie in
//                 one segment, found by all threads alike); the groups take the rows of a piece in turn and keep the dscale sum
//                 of their rows in registers; behind a piece the sums of the groups are added through LDS in group order.  A
//                 segment that lies inside the workgroup's rows is finished there (f32, in the workspace), one that crosses
//                 the border leaves a head (slot 0) or a tail (slot 1) partial.  The fold launch adds the partials of every
//                 segment in ascending order (16 lane rows per channel, then those 16 in order) and writes dscale.
//   pe            one parent per group, its S children in turn: feat is read once, the trig values (lane l takes the
//                 (k, j) pairs l, l + LC, ...: one sincosf for two columns) and the normalised row go through an LDS row, so
//                 the result leaves in aligned 8-element pieces although the feat part starts at column 6F.  dfeat is summed
//                 over the children in registers; dx over k by lanes 0..2 from an LDS row, k ascending.
//
// The pieces of a lane, the zero-filled row load, the backward's tail behind the element loop, the LDS sum of the groups and
// the dispatch on the pieces per lane are ln_rows.h's, shared with groupattn.hip's and volcond.hip's norms; ada's fold is
// segmented and stays here.
//
// Bounds: offset values are clamped to [0, N] where they are read; the searches stop after 16 steps; a piece consumes at
// least one row; every row index is checked against N or P.  A malformed offset gives unspecified values and never an access
// outside the buffers.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "ln_rows.h"

namespace gdr {
namespace {

constexpr int NM_BLOCK = LN_BLOCK;
constexpr int NM_ROWS = GDR_NORM_ROWS;
constexpr int NM_TRIG = 6 * GDR_NORM_MAX_FREQS;      // trig columns of a pe row at most
constexpr int NM_PE_EXTRA = NM_TRIG + NM_TRIG / 2;   // LDS floats of a group in the pe backward beside the gradient row

// idx: an even element index from a base aligned to two elements
__device__ __forceinline__ void load2(const void* base, int64_t idx, int dt, float& a, float& b) {
    if (dt == GDR_NORM_F32) {
        const float2 v = *reinterpret_cast<const float2*>((const float*)base + idx);
        a = v.x; b = v.y;
    } else {
        const uint32_t v = *reinterpret_cast<const uint32_t*>((const uint16_t*)base + idx);
        a = up_any((uint16_t)(v & 0xffffu), dt); b = up_any((uint16_t)(v >> 16), dt);
    }
}
__device__ __forceinline__ int64_t clamp_end(const int64_t* __restrict__ offset, int i, int64_t N) {
    const int64_t v = offset[i];
    return v < 0 ? 0 : (v > N ? N : v);
}

// the number of segment ends <= row: the segment that holds `row`, B if it lies behind the last one (ends non-decreasing)
__device__ __forceinline__ int seg_of_row(const int64_t* __restrict__ offset, int B, int64_t N, int64_t row) {
    int lo = 0, hi = B;
    for (int k = 0; k < 16 && lo < hi; ++k) {
        const int mid = (lo + hi) >> 1;
        if (clamp_end(offset, mid, N) <= row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- ada ---------------------------------------------------------------------------------------------------------------------
struct AdaP {
    const void* feat; const void* scale; const int64_t* offset; const void* grad; void* out; void* dfeat; void* dscale;
    float* ws_seg; float* ws_part;
    int64_t N, feat_stride, scale_stride, grad_stride;
    int32_t B, C, lc_shift, feat_dt, scale_dt, out_dt;
    float eps;
};

template <int K>
__global__ __launch_bounds__(NM_BLOCK) void ada_fwd_kernel(const AdaP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N) return;                        // (whole groups leave: the butterflies stay inside a group)
    float x[K][8];
    bool on[K];
    pieces_on<K>(l, lc, p.C, on);
    load_row<K>(p.feat, row * p.feat_stride, p.feat_dt, on, l, lc, x);
    const int b = seg_of_row(p.offset, p.B, p.N, row);
    float mean, rstd;
    row_stats<K>(x, on, lc, 1.0f / (float)p.C, p.eps, mean, rstd);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!on[k]) continue;
        const int c0 = piece_c0(l, lc, k);
        float y[8];
        if (b < p.B) {
            float sc[8];
            load8(p.scale, (int64_t)b * p.scale_stride + c0, p.scale_dt, sc);
#pragma unroll
            for (int v = 0; v < 8; ++v) y[v] = sc[v] * ((x[k][v] - mean) * rstd);
        } else {
#pragma unroll
            for (int v = 0; v < 8; ++v) y[v] = 0.f;
        }
        store8(p.out, row * p.C + c0, p.out_dt, y);
    }
}

template <int K>
__global__ __launch_bounds__(NM_BLOCK) void ada_bwd_kernel(const AdaP p) {
    __shared__ float sh[2048 * K];                 // (256 / LC) groups x C channels: C <= 8 LC K
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift, G = NM_BLOCK >> p.lc_shift;
    const int64_t N = p.N, j = blockIdx.x, a = j * NM_ROWS, e = a + NM_ROWS < N ? a + NM_ROWS : N;
    const int C = p.C;
    const float inv_c = 1.0f / (float)C;
    bool on[K];
    pieces_on<K>(l, lc, C, on);
    int64_t row = a;
    // (everything that steers the loop is the same in all threads of the workgroup)
    for (int it = 0; it < NM_ROWS && row < e; ++it) {
        const int b = seg_of_row(p.offset, p.B, N, row);
        if (b >= p.B) {                            // behind the last segment: zero gradient
            float z[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) z[v] = 0.f;
            for (int64_t r = row + grp; r < e; r += G)
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (on[k]) store8(p.dfeat, r * C + piece_c0(l, lc, k), p.feat_dt, z);
            break;
        }
        const int64_t st = b ? clamp_end(p.offset, b - 1, N) : 0, en = clamp_end(p.offset, b, N);
        int64_t r1 = en < e ? en : e;
        if (r1 <= row) r1 = row + 1;               // (ends that are not monotone: one row on)
        float sc[K][8], acc[K][8];
        fill_row<K>(acc, 0.f);
        load_row<K>(p.scale, (int64_t)b * p.scale_stride, p.scale_dt, on, l, lc, sc);
        for (int64_t r = row + grp; r < r1; r += G) {      // at most GDR_NORM_ROWS / G rows
            float x[K][8], g[K][8];
            load_row<K>(p.feat, r * p.feat_stride, p.feat_dt, on, l, lc, x);
            load_row<K>(p.grad, r * p.grad_stride, p.out_dt, on, l, lc, g);
            float mean, rstd;
            row_stats<K>(x, on, lc, inv_c, p.eps, mean, rstd);
            float m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        x[k][v] = (x[k][v] - mean) * rstd;             // xh
                        const float gx = g[k][v] * x[k][v];
                        acc[k][v] += gx;
                        g[k][v] *= sc[k][v];                           // dxh
                        m1 += g[k][v];
                        m2 += gx * sc[k][v];
                    }
                }
            ln_dx<K>(g, x, on, m1, m2, lc, inv_c, rstd);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) store8(p.dfeat, r * C + piece_c0(l, lc, k), p.feat_dt, g[k]);
        }
        put_sums<K>(sh + grp * C, acc, on, l, lc);
        sum_groups<false>(sh, C, G, (st >= a && en <= e) ? p.ws_seg + (int64_t)b * C : p.ws_part + (j * 2 + (st < a ? 0 : 1)) * C);
        __syncthreads();
        row = r1;
    }
}

// dscale[b, c]: 0 for an empty segment, the finished sum of a segment that lies in one workgroup's rows, else the partials of
// its workgroups in ascending order.  One workgroup per (segment, 16 channels).
__global__ __launch_bounds__(NM_BLOCK) void ada_fold_kernel(const AdaP p, uint32_t ctiles) {
    __shared__ float sh[LN_FOLD_LANES][LN_FOLD_CH];
    const int tid = threadIdx.x, ch = tid & (LN_FOLD_CH - 1), fl = tid / LN_FOLD_CH;
    const int b = blockIdx.x / ctiles, c = (int)(blockIdx.x % ctiles) * LN_FOLD_CH + ch, C = p.C;
    const int64_t N = p.N;
    const int64_t st = b ? clamp_end(p.offset, b - 1, N) : 0, en = clamp_end(p.offset, b, N);
    float acc = 0.f;
    if (en > st && c < C) {
        const int64_t j0 = st / NM_ROWS, j1 = (en - 1) / NM_ROWS;
        if (j0 == j1) {
            if (fl == 0) acc = p.ws_seg[(int64_t)b * C + c];
        } else {
            const int64_t T = j1 - j0 + 1, per = (T + LN_FOLD_LANES - 1) / LN_FOLD_LANES;
            const int64_t t0 = fl * per, t1 = t0 + per < T ? t0 + per : T;
#pragma unroll 4
            for (int64_t t = t0; t < t1; ++t) acc += p.ws_part[((j0 + t) * 2 + (t == 0 ? 1 : 0)) * C + c];
        }
    }
    sh[fl][ch] = acc;
    __syncthreads();
    if (fl != 0 || c >= C) return;
    for (int i = 1; i < LN_FOLD_LANES; ++i) acc += sh[i][ch];
    store1(p.dscale, (int64_t)b * C + c, p.scale_dt, acc);
}

// ---- pe ----------------------------------------------------------------------------------------------------------------------
struct PeP {
    const void* x; const void* feat; const void* freq; const void* grad; void* out; void* dx; void* dfeat;
    int64_t P, feat_stride, out_stride, grad_stride;
    int32_t S, C, F, lc_shift, x_dt, feat_dt, freq_dt, out_dt;
    float eps;
};

// the trig values of row r into zt (sin at t, cos at 3F + t for the lane's pairs t = 3k + j); returns the lane's share of their sum
__device__ __forceinline__ float pe_trig(const PeP& p, int64_t r, int l, int lc, float* __restrict__ zt) {
    const int T = 3 * p.F;
    float s = 0.f;
    for (int t = l; t < T; t += lc) {
        const int k = t / 3, jj = t - 3 * k;
        const float arg = load1(p.freq, k, p.freq_dt) * load1(p.x, r * 3 + jj, p.x_dt);
        float sn, cs;
        sincosf(arg, &sn, &cs);
        zt[t] = sn; zt[T + t] = cs;
        s += sn + cs;
    }
    return s;
}

// mean and rstd of the row [zt (the lane's own trig entries), xf]
template <int K>
__device__ __forceinline__ void pe_stats(const PeP& p, const float* __restrict__ zt, const float (&xf)[K][8], const bool (&on)[K],
                                         float trig_sum, float feat_sum, int l, int lc, float inv_w, float& mean, float& rstd) {
    const int T = 3 * p.F;
    mean = group_sum(trig_sum + feat_sum, lc) * inv_w;
    float q = 0.f;
    for (int t = l; t < T; t += lc) {
        const float a = zt[t] - mean, b = zt[T + t] - mean;
        q += a * a + b * b;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) {
#pragma unroll
            for (int v = 0; v < 8; ++v) { const float d = xf[k][v] - mean; q += d * d; }
        }
    rstd = 1.0f / sqrtf(group_sum(q, lc) * inv_w + p.eps);
}

template <int K>
__global__ __launch_bounds__(NM_BLOCK) void pe_fwd_kernel(const PeP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift;
    const int C = p.C, T = 3 * p.F, W = 2 * T + C, Wp = (W + 7) & ~7;
    const int64_t parent = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + grp;
    const bool active = parent < p.P;              // (idle groups stay for the barriers and touch no global memory)
    float* z = lds + grp * Wp;
    const float inv_w = 1.0f / (float)W;
    float xf[K][8];
    bool on[K];
    float feat_sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (l + k * lc) * 8;
        on[k] = active && c0 < C;
#pragma unroll
        for (int v = 0; v < 8; ++v) xf[k][v] = 0.f;
        if (on[k]) load8(p.feat, parent * p.feat_stride + c0, p.feat_dt, xf[k]);
#pragma unroll
        for (int v = 0; v < 8; ++v) feat_sum += xf[k][v];
    }
    for (int s = 0; s < p.S; ++s) {
        const int64_t r = parent * p.S + s;
        const float trig_sum = active ? pe_trig(p, r, l, lc, z) : 0.f;
        float mean, rstd;
        pe_stats<K>(p, z, xf, on, trig_sum, feat_sum, active ? l : T, lc, inv_w, mean, rstd);
        if (active) {
            for (int t = l; t < T; t += lc) {
                z[t] = (z[t] - mean) * rstd;
                z[T + t] = (z[T + t] - mean) * rstd;
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) z[2 * T + (l + k * lc) * 8 + v] = (xf[k][v] - mean) * rstd;
                }
            for (int c = W + l; c < Wp; c += lc) z[c] = 0.f;           // the padding of the row stride is written as zeros
        }
        __syncthreads();
        if (active)
            for (int q = l; q < Wp / 8; q += lc) {
                float y[8];
#pragma unroll
                for (int v = 0; v < 8; ++v) y[v] = z[q * 8 + v];
                store8(p.out, r * p.out_stride + q * 8, p.out_dt, y);
            }
        __syncthreads();
    }
}

// GV = 8: the gradient rows start on 16 bytes and have a stride that is a multiple of 8; GV = 2: on two elements, even stride
template <int K, int GV>
__global__ __launch_bounds__(NM_BLOCK) void pe_bwd_kernel(const PeP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift;
    const int C = p.C, T = 3 * p.F, W = 2 * T + C, Wp = (W + 7) & ~7;
    const int64_t parent = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + grp;
    const bool active = parent < p.P;
    float* zt = lds + grp * (Wp + NM_PE_EXTRA);    // trig values, then the gradient row, then the dx terms
    float* gr = zt + NM_TRIG;
    float* ct = gr + Wp;
    const float inv_w = 1.0f / (float)W;
    float xf[K][8], acc[K][8];
    bool on[K];
    float feat_sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (l + k * lc) * 8;
        on[k] = active && c0 < C;
#pragma unroll
        for (int v = 0; v < 8; ++v) { xf[k][v] = 0.f; acc[k][v] = 0.f; }
        if (on[k]) load8(p.feat, parent * p.feat_stride + c0, p.feat_dt, xf[k]);
#pragma unroll
        for (int v = 0; v < 8; ++v) feat_sum += xf[k][v];
    }
    for (int s = 0; s < p.S; ++s) {
        const int64_t r = parent * p.S + s;
        const float trig_sum = active ? pe_trig(p, r, l, lc, zt) : 0.f;
        if (active) {
            if constexpr (GV == 8) {
                for (int q = l; q * 8 < W; q += lc) {
                    if (q * 8 + 8 <= W) {
                        float y[8];
                        load8(p.grad, r * p.grad_stride + q * 8, p.out_dt, y);
#pragma unroll
                        for (int v = 0; v < 8; ++v) gr[q * 8 + v] = y[v];
                    } else {                       // the last piece of a row: only what the row holds
                        for (int c = q * 8; c < W; ++c) gr[c] = load1(p.grad, r * p.grad_stride + c, p.out_dt);
                    }
                }
            } else {
                for (int i = l; i * 2 < W; i += lc)                    // (W is even)
                    load2(p.grad, r * p.grad_stride + i * 2, p.out_dt, gr[i * 2], gr[i * 2 + 1]);
            }
        }
        float mean, rstd;
        pe_stats<K>(p, zt, xf, on, trig_sum, feat_sum, active ? l : T, lc, inv_w, mean, rstd);
        __syncthreads();
        float m1 = 0.f, m2 = 0.f;
        if (active) {
            for (int t = l; t < T; t += lc) {
                const float gs = gr[t], gc = gr[T + t];
                m1 += gs + gc;
                m2 += gs * ((zt[t] - mean) * rstd) + gc * ((zt[T + t] - mean) * rstd);
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        const float g = gr[2 * T + (l + k * lc) * 8 + v];
                        m1 += g;
                        m2 += g * ((xf[k][v] - mean) * rstd);
                    }
                }
        }
        m1 = group_sum(m1, lc) * inv_w;
        m2 = group_sum(m2, lc) * inv_w;
        if (active) {
            for (int t = l; t < T; t += lc) {
                const float sn = zt[t], cs = zt[T + t];
                const float ds = rstd * (gr[t] - m1 - (sn - mean) * rstd * m2);
                const float dc = rstd * (gr[T + t] - m1 - (cs - mean) * rstd * m2);
                ct[t] = load1(p.freq, t / 3, p.freq_dt) * (cs * ds - sn * dc);
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
#pragma unroll
                    for (int v = 0; v < 8; ++v)
                        acc[k][v] += rstd * (gr[2 * T + (l + k * lc) * 8 + v] - m1 - (xf[k][v] - mean) * rstd * m2);
                }
        }
        __syncthreads();
        if (active && l < 3 && p.dx) {             // (LC >= 8)
            float d = 0.f;
            for (int k = 0; k < p.F; ++k) d += ct[3 * k + l];          // k ascending: fixed
            store1(p.dx, r * 3 + l, p.x_dt, d);
        }
        __syncthreads();
    }
    if (p.dfeat) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) store8(p.dfeat, parent * C + (l + k * lc) * 8, p.feat_dt, acc[k]);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
constexpr int64_t NM_MAX_ROWS = INT64_C(0x7fffffff);

int elem_bytes(int32_t dt) { return dt == GDR_NORM_F32 ? 4 : 2; }

// 0, or the status with the message set
int check_channels(int64_t C) {
    if (C < 8 || C > GDR_NORM_MAX_CHANNELS || C % 8) return unsupported("norm: C must be a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS");
    return GDR_OK;
}

int check_ada(int64_t N, int64_t B, int64_t C) {
    if (N < 0 || B < 1) return invalid_arg("norm_ada: N must be >= 0 and B >= 1");
    if (N > NM_MAX_ROWS) return unsupported("norm_ada: N must be below 2^31");
    if (B > GDR_NORM_MAX_SEGMENTS) return unsupported("norm_ada: B must be at most GDR_NORM_MAX_SEGMENTS");
    return check_channels(C);
}

int check_pe(int64_t P, int64_t S, int64_t C, int64_t F) {
    if (P < 0) return invalid_arg("norm_pe: P must be >= 0");
    if (F < 1 || F > GDR_NORM_MAX_FREQS) return unsupported("norm_pe: F must be in 1..GDR_NORM_MAX_FREQS");
    if (S < 1 || S > GDR_NORM_MAX_UPSCALE) return unsupported("norm_pe: S must be in 1..GDR_NORM_MAX_UPSCALE");
    if (P > NM_MAX_ROWS / S) return unsupported("norm_pe: P * S must be below 2^31");
    return check_channels(C);
}

struct AdaWs { size_t seg, part, bytes; };

AdaWs ada_workspace(int64_t N, int64_t B, int64_t C) {
    AdaWs w;
    w.seg = 0;
    w.part = align_up((size_t)B * (size_t)C * 4);
    w.bytes = w.part + align_up((size_t)((N + NM_ROWS - 1) / NM_ROWS) * 2 * (size_t)C * 4);
    return w;
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_norm_ada_forward(const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* scale, int64_t scale_stride,
                         int32_t scale_dtype, const int64_t* offset, int64_t N, int32_t B, int32_t C, float eps, void* out,
                         int32_t out_dtype, void* stream) {
    if (const int rc = check_ada(N, B, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(scale_dtype) || bad_dtype(out_dtype)) return invalid_arg("norm_ada_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_ada_forward: eps must be >= 0");
    if (N == 0) return GDR_OK;
    if (!feat || !scale || !offset || !out) return invalid_arg("norm_ada_forward: NULL argument");
    if (bad_rows(feat, feat_stride, C) || bad_rows(scale, scale_stride, C) || misaligned(out, 15) || misaligned(offset, 7))
        return invalid_arg("norm_ada_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    AdaP p = {};
    p.feat = feat; p.scale = scale; p.offset = offset; p.out = out;
    p.N = N; p.feat_stride = feat_stride; p.scale_stride = scale_stride;
    p.B = B; p.C = C; p.feat_dt = feat_dtype; p.scale_dt = scale_dtype; p.out_dt = out_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((N + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    LN_LAUNCH_K(ada_fwd_kernel, K, grid, st, p);
    return launch_status("norm ada_fwd_kernel");
}

size_t gdr_norm_ada_backward_bytes(int64_t N, int32_t B, int32_t C) {
    if (check_ada(N, B, C)) return 0;
    return ada_workspace(N, B, C).bytes + 256;     // (never 0 for valid arguments)
}

int gdr_norm_ada_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* feat, int64_t feat_stride,
                          int32_t feat_dtype, const void* scale, int64_t scale_stride, int32_t scale_dtype, const int64_t* offset,
                          int64_t N, int32_t B, int32_t C, float eps, void* workspace, size_t workspace_bytes, void* grad_feat,
                          void* grad_scale, void* stream) {
    if (const int rc = check_ada(N, B, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(scale_dtype) || bad_dtype(grad_dtype)) return invalid_arg("norm_ada_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_ada_backward: eps must be >= 0");
    if (!offset || !workspace || !grad_scale || (N && (!grad_out || !feat || !scale || !grad_feat)))
        return invalid_arg("norm_ada_backward: NULL argument");
    if ((N && (bad_rows(feat, feat_stride, C) || bad_rows(scale, scale_stride, C) || bad_rows(grad_out, grad_stride, C))) ||
        misaligned(grad_feat, 15) || misaligned(grad_scale, 15) || misaligned(offset, 7) || misaligned(workspace, 255))
        return invalid_arg("norm_ada_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    const AdaWs ws = ada_workspace(N, B, C);
    if (workspace_bytes < ws.bytes) return workspace_too_small("norm_ada_backward: workspace smaller than gdr_norm_ada_backward_bytes");
    AdaP p = {};
    p.feat = feat; p.scale = scale; p.offset = offset; p.grad = grad_out; p.dfeat = grad_feat; p.dscale = grad_scale;
    p.ws_seg = (float*)((char*)workspace + ws.seg); p.ws_part = (float*)((char*)workspace + ws.part);
    p.N = N; p.feat_stride = feat_stride; p.scale_stride = scale_stride; p.grad_stride = grad_stride;
    p.B = B; p.C = C; p.feat_dt = feat_dtype; p.scale_dt = scale_dtype; p.out_dt = grad_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t chunks = (uint32_t)((N + NM_ROWS - 1) / NM_ROWS);
    if (chunks) LN_LAUNCH_K(ada_bwd_kernel, K, dim3(chunks), st, p);
    const uint32_t ctiles = (uint32_t)((C + LN_FOLD_CH - 1) / LN_FOLD_CH);
    hipLaunchKernelGGL(ada_fold_kernel, dim3((uint32_t)B * ctiles), dim3(NM_BLOCK), 0, st, p, ctiles);
    return launch_status("norm ada_bwd kernels");
}

int gdr_norm_pe_forward(const void* x, int32_t x_dtype, const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq,
                        int32_t freq_dtype, int64_t P, int32_t S, int32_t C, int32_t F, float eps, void* out, int64_t out_stride,
                        int32_t out_dtype, void* stream) {
    if (const int rc = check_pe(P, S, C, F)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(feat_dtype) || bad_dtype(freq_dtype) || bad_dtype(out_dtype))
        return invalid_arg("norm_pe_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_pe_forward: eps must be >= 0");
    if (P == 0) return GDR_OK;
    if (!x || !feat || !freq || !out) return invalid_arg("norm_pe_forward: NULL argument");
    if (bad_rows(feat, feat_stride, C) || bad_rows(out, out_stride, 6 * F + C) || misaligned(x, elem_bytes(x_dtype) - 1) ||
        misaligned(freq, elem_bytes(freq_dtype) - 1))
        return invalid_arg("norm_pe_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    PeP p = {};
    p.x = x; p.feat = feat; p.freq = freq; p.out = out;
    p.P = P; p.feat_stride = feat_stride; p.out_stride = out_stride;
    p.S = S; p.C = C; p.F = F; p.x_dt = x_dtype; p.feat_dt = feat_dtype; p.freq_dt = freq_dtype; p.out_dt = out_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift;
    const int Wp = (6 * F + C + 7) & ~7;
    const size_t lds = (size_t)groups * Wp * sizeof(float);
    const dim3 grid((uint32_t)((P + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    if (K == 1) hipLaunchKernelGGL(pe_fwd_kernel<1>, grid, dim3(NM_BLOCK), lds, st, p);
    else hipLaunchKernelGGL(pe_fwd_kernel<2>, grid, dim3(NM_BLOCK), lds, st, p);
    return launch_status("norm pe_fwd_kernel");
}

int gdr_norm_pe_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* x, int32_t x_dtype,
                         const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype, int64_t P,
                         int32_t S, int32_t C, int32_t F, float eps, void* grad_x, void* grad_feat, void* stream) {
    if (const int rc = check_pe(P, S, C, F)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(feat_dtype) || bad_dtype(freq_dtype) || bad_dtype(grad_dtype))
        return invalid_arg("norm_pe_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_pe_backward: eps must be >= 0");
    if (P == 0) return GDR_OK;
    if (!x || !feat || !freq || !grad_out) return invalid_arg("norm_pe_backward: NULL argument");
    const int W = 6 * F + C;
    const unsigned gmask = 2 * elem_bytes(grad_dtype) - 1;
    if (bad_rows(feat, feat_stride, C) || misaligned(grad_feat, 15) || misaligned(x, elem_bytes(x_dtype) - 1) ||
        misaligned(grad_x, elem_bytes(x_dtype) - 1) || misaligned(freq, elem_bytes(freq_dtype) - 1) || grad_stride < W ||
        grad_stride % 2 || misaligned(grad_out, gmask))
        return invalid_arg("norm_pe_backward: feat rows must start on 16 bytes with a stride that is a multiple of 8; grad_out "
                           "rows on two elements with an even stride that covers the row");
    PeP p = {};
    p.x = x; p.feat = feat; p.freq = freq; p.grad = grad_out; p.dx = grad_x; p.dfeat = grad_feat;
    p.P = P; p.feat_stride = feat_stride; p.grad_stride = grad_stride;
    p.S = S; p.C = C; p.F = F; p.x_dt = x_dtype; p.feat_dt = feat_dtype; p.freq_dt = freq_dtype; p.out_dt = grad_dtype; p.eps = eps;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift;
    const int Wp = (W + 7) & ~7;
    const size_t lds = (size_t)groups * (Wp + NM_PE_EXTRA) * sizeof(float);
    const dim3 grid((uint32_t)((P + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = grad_stride % 8 == 0 && !misaligned(grad_out, 15);
    if (K == 1) {
        if (wide) hipLaunchKernelGGL((pe_bwd_kernel<1, 8>), grid, dim3(NM_BLOCK), lds, st, p);
        else hipLaunchKernelGGL((pe_bwd_kernel<1, 2>), grid, dim3(NM_BLOCK), lds, st, p);
    } else {
        if (wide) hipLaunchKernelGGL((pe_bwd_kernel<2, 8>), grid, dim3(NM_BLOCK), lds, st, p);
        else hipLaunchKernelGGL((pe_bwd_kernel<2, 2>), grid, dim3(NM_BLOCK), lds, st, p);
    }
    return launch_status("norm pe_bwd_kernel");
}

}  // extern "C"

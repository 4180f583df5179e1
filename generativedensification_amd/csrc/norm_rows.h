// norm_rows.h — the row passes of the point decoder's two normalisations, written once for norm.hip (ada, pe) and upscale.hip
// (merge, expand; internal).  The arithmetic and the mapping are described in the header of norm.hip.  A kernel here is a
// template over a small policy that says where a row comes from and where its gradients go; everything between — the
// statistics, the trig columns, the normalised row, the backward's means, the dscale partials and their fold — is this
// file's and is the same instruction sequence for every policy, so two policies that feed the same values give the same bits.
//
//   ada kernels, policy R (AdaPlain here, upscale.hip's MergeRows):
//     a unit is the S consecutive rows that share a parent (S = 1 for AdaPlain: the row itself); segments, the backward's
//     chunks of GDR_NORM_ROWS and the dscale partials count units.
//     R::children(p)                       rows of a unit
//     R::Unit, R::begin / R::end           what a group keeps for a unit across its rows in the backward
//     R::load_fwd / R::load                the row `r` of unit `u` into x (f32, pieces that are off are zero)
//     R::store / R::zero                   the gradient of row r (dy, f32) out, or zeros for a unit behind the last segment
//   pe kernels, policy X (PeGiven here, upscale.hip's ExpandX):
//     X::LDS                               floats a group keeps in LDS beside the shared layout (the host adds the same)
//     X::prepare                           once per parent, before a barrier: whatever x needs
//     X::x(p, xs, r, s, j)                 the PE argument of child s, axis j
//     X::wants_dx / X::State / X::put_dx / X::finish   where dx[r, j] (lanes 0..2, f32) goes
// Include after gdr_common.h, host_util.h, row_io.h and ln_rows.h.
#pragma once

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
// N counts units; feat / grad / out / dfeat hold N * S rows.  skip .. y_dt are MergeRows' (upscale.hip).
struct AdaP {
    const void* feat; const void* scale; const int64_t* offset; const void* grad; void* out; void* dfeat; void* dscale;
    float* ws_seg; float* ws_part;
    const void* skip; const void* keep; void* dskip;
    int64_t N, feat_stride, scale_stride, grad_stride, skip_stride;
    int32_t B, C, lc_shift, feat_dt, scale_dt, out_dt, S, skip_dt, keep_dt, y_dt;
    float eps;
};

struct AdaPlain {
    template <int K> struct Unit {};
    static __device__ __forceinline__ int children(const AdaP&) { return 1; }
    static __device__ __forceinline__ int64_t unit_of(const AdaP&, int64_t row) { return row; }
    template <int K>
    static __device__ __forceinline__ void load_fwd(const AdaP& p, int64_t r, int64_t, const bool (&on)[K], int l, int lc, float (&x)[K][8]) {
        load_row<K>(p.feat, r * p.feat_stride, p.feat_dt, on, l, lc, x);
    }
    template <int K>
    static __device__ __forceinline__ void begin(const AdaP&, int64_t, const bool (&)[K], int, int, Unit<K>&) {}
    template <int K>
    static __device__ __forceinline__ void load(const AdaP& p, int64_t r, const Unit<K>&, const bool (&on)[K], int l, int lc, float (&x)[K][8]) {
        load_row<K>(p.feat, r * p.feat_stride, p.feat_dt, on, l, lc, x);
    }
    template <int K>
    static __device__ __forceinline__ void store(const AdaP& p, int64_t r, Unit<K>&, const bool (&on)[K], int l, int lc, const float (&dy)[K][8]) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) store8(p.dfeat, r * p.C + piece_c0(l, lc, k), p.feat_dt, dy[k]);
    }
    template <int K>
    static __device__ __forceinline__ void end(const AdaP&, int64_t, const Unit<K>&, const bool (&)[K], int, int) {}
    template <int K>
    static __device__ __forceinline__ void zero(const AdaP& p, int64_t u, const bool (&on)[K], int l, int lc) {
        float z[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) z[v] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) store8(p.dfeat, u * p.C + piece_c0(l, lc, k), p.feat_dt, z);
    }
};

template <int K, class R>
__global__ __launch_bounds__(NM_BLOCK) void ada_fwd_kernel(const AdaP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N * R::children(p)) return;       // (whole groups leave: the butterflies stay inside a group)
    const int64_t unit = R::unit_of(p, row);
    float x[K][8];
    bool on[K];
    pieces_on<K>(l, lc, p.C, on);
    R::template load_fwd<K>(p, row, unit, on, l, lc, x);
    const int b = seg_of_row(p.offset, p.B, p.N, unit);
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

template <int K, class R>
__global__ __launch_bounds__(NM_BLOCK) void ada_bwd_kernel(const AdaP p) {
    __shared__ float sh[2048 * K];                 // (256 / LC) groups x C channels: C <= 8 LC K
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift, G = NM_BLOCK >> p.lc_shift;
    const int64_t N = p.N, j = blockIdx.x, a = j * NM_ROWS, e = a + NM_ROWS < N ? a + NM_ROWS : N;
    const int C = p.C, S = R::children(p);
    const float inv_c = 1.0f / (float)C;
    bool on[K];
    pieces_on<K>(l, lc, C, on);
    int64_t row = a;
    // (everything that steers the loop is the same in all threads of the workgroup)
    for (int it = 0; it < NM_ROWS && row < e; ++it) {
        const int b = seg_of_row(p.offset, p.B, N, row);
        if (b >= p.B) {                            // behind the last segment: zero gradient
            for (int64_t u = row + grp; u < e; u += G) R::template zero<K>(p, u, on, l, lc);
            break;
        }
        const int64_t st = b ? clamp_end(p.offset, b - 1, N) : 0, en = clamp_end(p.offset, b, N);
        int64_t r1 = en < e ? en : e;
        if (r1 <= row) r1 = row + 1;               // (ends that are not monotone: one row on)
        float sc[K][8], acc[K][8];
        fill_row<K>(acc, 0.f);
        load_row<K>(p.scale, (int64_t)b * p.scale_stride, p.scale_dt, on, l, lc, sc);
        for (int64_t u = row + grp; u < r1; u += G) {      // at most GDR_NORM_ROWS / G units
            typename R::template Unit<K> unit;
            R::template begin<K>(p, u, on, l, lc, unit);
            for (int s = 0; s < S; ++s) {
                const int64_t r = u * S + s;
                float x[K][8], g[K][8];
                R::template load<K>(p, r, unit, on, l, lc, x);
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
                R::template store<K>(p, r, unit, on, l, lc, g);
            }
            R::template end<K>(p, u, unit, on, l, lc);
        }
        put_sums<K>(sh + grp * C, acc, on, l, lc);
        sum_groups<false>(sh, C, G, (st >= a && en <= e) ? p.ws_seg + (int64_t)b * C : p.ws_part + (j * 2 + (st < a ? 0 : 1)) * C);
        __syncthreads();
        row = r1;
    }
}

// dscale[b, c]: 0 for an empty segment, the finished sum of a segment that lies in one workgroup's units, else the partials of
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
// grad may be NULL in the backward (a zero gradient).  t .. absolute are ExpandX's (upscale.hip).
struct PeP {
    const void* x; const void* feat; const void* freq; const void* grad; void* out; void* dx; void* dfeat;
    const void* t; const void* coord; const void* grad_ox; void* out_x; void* dt; void* dcoord;
    int64_t P, feat_stride, out_stride, grad_stride;
    int32_t S, C, F, lc_shift, x_dt, feat_dt, freq_dt, out_dt, t_dt, coord_dt, ox_dt, absolute;
    float eps, half_grid;
};

struct PeGiven {
    static constexpr int LDS = 0;
    struct State {};
    static __device__ __forceinline__ void prepare(const PeP&, int64_t, bool, int, int, float*) {}
    static __device__ __forceinline__ float x(const PeP& p, const float*, int64_t r, int, int jj) {
        return load1(p.x, r * 3 + jj, p.x_dt);
    }
    static __device__ __forceinline__ bool wants_dx(const PeP& p) { return p.dx != nullptr; }
    static __device__ __forceinline__ void put_dx(const PeP& p, const float*, State&, int64_t r, int64_t, int, int l, float d) {
        store1(p.dx, r * 3 + l, p.x_dt, d);
    }
    static __device__ __forceinline__ void finish(const PeP&, const State&, int64_t, int) {}
};

// the trig values of row r into zt (sin at t, cos at 3F + t for the lane's pairs t = 3k + j); returns the lane's share of their sum
template <class X>
__device__ __forceinline__ float pe_trig(const PeP& p, const float* __restrict__ xs, int64_t r, int s, int l, int lc,
                                         float* __restrict__ zt) {
    const int T = 3 * p.F;
    float sum = 0.f;
    for (int t = l; t < T; t += lc) {
        const int k = t / 3, jj = t - 3 * k;
        const float arg = load1(p.freq, k, p.freq_dt) * X::x(p, xs, r, s, jj);
        float sn, cs;
        sincosf(arg, &sn, &cs);
        zt[t] = sn; zt[T + t] = cs;
        sum += sn + cs;
    }
    return sum;
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

template <int K, class X>
__global__ __launch_bounds__(NM_BLOCK) void pe_fwd_kernel(const PeP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift;
    const int C = p.C, T = 3 * p.F, W = 2 * T + C, Wp = (W + 7) & ~7;
    const int64_t parent = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + grp;
    const bool active = parent < p.P;              // (idle groups stay for the barriers and touch no global memory)
    float* z = lds + grp * (Wp + X::LDS);
    float* xs = z + Wp;
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
    if constexpr (X::LDS > 0) {
        X::prepare(p, parent, active, l, lc, xs);
        __syncthreads();
    }
    for (int s = 0; s < p.S; ++s) {
        const int64_t r = parent * p.S + s;
        const float trig_sum = active ? pe_trig<X>(p, xs, r, s, l, lc, z) : 0.f;
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
template <int K, int GV, class X>
__global__ __launch_bounds__(NM_BLOCK) void pe_bwd_kernel(const PeP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift;
    const int C = p.C, T = 3 * p.F, W = 2 * T + C, Wp = (W + 7) & ~7;
    const int64_t parent = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + grp;
    const bool active = parent < p.P;
    float* zt = lds + grp * (Wp + NM_PE_EXTRA + X::LDS);   // trig values, then the gradient row, then the dx terms
    float* gr = zt + NM_TRIG;
    float* ct = gr + Wp;
    float* xs = ct + NM_TRIG / 2;
    const float inv_w = 1.0f / (float)W;
    float xf[K][8], acc[K][8];
    bool on[K];
    float feat_sum = 0.f;
    typename X::State state = {};
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
    if constexpr (X::LDS > 0) {
        X::prepare(p, parent, active, l, lc, xs);
        __syncthreads();
    }
    for (int s = 0; s < p.S; ++s) {
        const int64_t r = parent * p.S + s;
        const float trig_sum = active ? pe_trig<X>(p, xs, r, s, l, lc, zt) : 0.f;
        if (active) {
            if (!p.grad) {
                for (int c = l; c < W; c += lc) gr[c] = 0.f;
            } else if constexpr (GV == 8) {
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
        if (active && l < 3 && X::wants_dx(p)) {   // (LC >= 8)
            float d = 0.f;
            for (int k = 0; k < p.F; ++k) d += ct[3 * k + l];          // k ascending: fixed
            X::put_dx(p, xs, state, r, parent, s, l, d);
        }
        __syncthreads();
    }
    if (active && l < 3) X::finish(p, state, parent, l);
    if (p.dfeat) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) store8(p.dfeat, parent * C + (l + k * lc) * 8, p.feat_dt, acc[k]);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
constexpr int64_t NM_MAX_ROWS = INT64_C(0x7fffffff);

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

// N units
AdaWs ada_workspace(int64_t N, int64_t B, int64_t C) {
    AdaWs w;
    w.seg = 0;
    w.part = align_up((size_t)B * (size_t)C * 4);
    w.bytes = w.part + align_up((size_t)((N + NM_ROWS - 1) / NM_ROWS) * 2 * (size_t)C * 4);
    return w;
}

// the launches, from a filled parameter block (lc_shift is set here); LDS is sized from the C, F the kernels index with
template <class R>
void launch_ada_fwd(AdaP& p, hipStream_t st) {
    int K;
    row_shape(p.C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift, rows = p.N * p.S;
    const dim3 grid((uint32_t)((rows + groups - 1) / groups));
    if (K == 1) hipLaunchKernelGGL((ada_fwd_kernel<1, R>), grid, dim3(NM_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ada_fwd_kernel<2, R>), grid, dim3(NM_BLOCK), 0, st, p);
}

// the row launch, and the fold when p.dscale is set
template <class R>
void launch_ada_bwd(AdaP& p, hipStream_t st) {
    int K;
    row_shape(p.C, &p.lc_shift, &K);
    const uint32_t chunks = (uint32_t)((p.N + NM_ROWS - 1) / NM_ROWS);
    if (chunks) {
        if (K == 1) hipLaunchKernelGGL((ada_bwd_kernel<1, R>), dim3(chunks), dim3(NM_BLOCK), 0, st, p);
        else hipLaunchKernelGGL((ada_bwd_kernel<2, R>), dim3(chunks), dim3(NM_BLOCK), 0, st, p);
    }
    if (!p.dscale) return;
    const uint32_t ctiles = (uint32_t)((p.C + LN_FOLD_CH - 1) / LN_FOLD_CH);
    hipLaunchKernelGGL(ada_fold_kernel, dim3((uint32_t)p.B * ctiles), dim3(NM_BLOCK), 0, st, p, ctiles);
}

template <class X>
void launch_pe_fwd(PeP& p, hipStream_t st) {
    int K;
    row_shape(p.C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift;
    const int Wp = (6 * p.F + p.C + 7) & ~7;
    const size_t lds = (size_t)groups * (Wp + X::LDS) * sizeof(float);
    const dim3 grid((uint32_t)((p.P + groups - 1) / groups));
    if (K == 1) hipLaunchKernelGGL((pe_fwd_kernel<1, X>), grid, dim3(NM_BLOCK), lds, st, p);
    else hipLaunchKernelGGL((pe_fwd_kernel<2, X>), grid, dim3(NM_BLOCK), lds, st, p);
}

// wide: the gradient rows start on 16 bytes with a stride that is a multiple of 8 (or there are none)
template <class X>
void launch_pe_bwd(PeP& p, bool wide, hipStream_t st) {
    int K;
    row_shape(p.C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift;
    const int Wp = (6 * p.F + p.C + 7) & ~7;
    const size_t lds = (size_t)groups * (Wp + NM_PE_EXTRA + X::LDS) * sizeof(float);
    const dim3 grid((uint32_t)((p.P + groups - 1) / groups));
    if (K == 1) {
        if (wide) hipLaunchKernelGGL((pe_bwd_kernel<1, 8, X>), grid, dim3(NM_BLOCK), lds, st, p);
        else hipLaunchKernelGGL((pe_bwd_kernel<1, 2, X>), grid, dim3(NM_BLOCK), lds, st, p);
    } else {
        if (wide) hipLaunchKernelGGL((pe_bwd_kernel<2, 8, X>), grid, dim3(NM_BLOCK), lds, st, p);
        else hipLaunchKernelGGL((pe_bwd_kernel<2, 2, X>), grid, dim3(NM_BLOCK), lds, st, p);
    }
}

}  // namespace
}  // namespace gdr

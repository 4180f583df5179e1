// row_io.h — elements and rows of a run-time storage type (GDR_F16 / GDR_BF16 / GDR_F32) <-> f32 on the device: one element
// (load1 / store1: every row kernel and, through mfma_rows.h, the weights, biases and partial sums of conv3d.hip, deconv3d.hip,
// coarsehead.hip and finehead.hip), eight (load8 / store8: norm.hip, densify.hip, volcond.hip, upscale.hip and ln_rows.h), a
// head's row (load_row / store_row / dot: viewattn.hip, groupattn.hip and the gather form of attn.hip); then the lane-group
// row sum and the LayerNorm statistics of a row held by a lane group, on which ln_rows.h builds the rest of what the row
// LayerNorms share (internal; include after gdr_common.h).  A new module takes these from here.
#pragma once
#include "half_bits.h"

namespace gdr {

// one element.  (up_any / down_any written out: called as functions here, the compiler lays out the MFMA kernels' bias and
// weight loops differently, and those are the kernels whose time was tuned)
__device__ __forceinline__ float load1(const void* base, int64_t idx, int dt) {
    if (dt == GDR_F32) return ((const float*)base)[idx];
    const uint16_t b = ((const uint16_t*)base)[idx];
    return dt == GDR_BF16 ? up16<true>(b) : up16<false>(b);
}
__device__ __forceinline__ void store1(void* base, int64_t idx, int dt, float x) {
    if (dt == GDR_F32) ((float*)base)[idx] = x;
    else ((uint16_t*)base)[idx] = dt == GDR_BF16 ? down16<true>(x) : down16<false>(x);
}

// idx: an element index that is a multiple of 8 from a 16-byte aligned base.  The dtype is picked per element, not once
// around half_bits.h's unpack8 / pack8: that form gives the same bits, but the compiler then keeps both conversions of a row
// alive across the branch, and five row kernels (ada_bwd<2>, rowmap_norm_bwd<2>, modln_bwd<1>, sample_fwd,
// viewattn_fwd_many<16>) lose a wave per SIMD to the extra registers (EXPERIMENTS.md, typed rows).
__device__ __forceinline__ void load8(const void* base, int64_t idx, int dt, float (&x)[8]) {
    if (dt == GDR_F32) {
        const float4* p = reinterpret_cast<const float4*>((const float*)base + idx);
        const float4 a = p[0], b = p[1];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
        union { uint4 raw; uint16_t e[8]; } u;
        u.raw = *reinterpret_cast<const uint4*>((const uint16_t*)base + idx);
#pragma unroll
        for (int v = 0; v < 8; ++v) x[v] = up_any(u.e[v], dt);
    }
}
__device__ __forceinline__ void store8(void* base, int64_t idx, int dt, const float (&x)[8]) {
    if (dt == GDR_F32) {
        float4* p = reinterpret_cast<float4*>((float*)base + idx);
        p[0] = make_float4(x[0], x[1], x[2], x[3]);
        p[1] = make_float4(x[4], x[5], x[6], x[7]);
    } else {
        union { uint4 raw; uint16_t e[8]; } u;
#pragma unroll
        for (int v = 0; v < 8; ++v) u.e[v] = down_any(x[v], dt);
        *reinterpret_cast<uint4*>((uint16_t*)base + idx) = u.raw;
    }
}

// N = 4 or a multiple of 8 elements from / to element index idx, a multiple of min(N, 8) from a 16-byte aligned base
template <int N>
__device__ __forceinline__ void load_row(const void* base, int64_t idx, int dt, float (&x)[N]) {
    static_assert(N == 4 || N % 8 == 0, "a row is 4 or a multiple of 8 elements");
    if constexpr (N == 4) {
        if (dt == GDR_F32) {
            const float4 a = *reinterpret_cast<const float4*>((const float*)base + idx);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
        } else {
            union { uint2 raw; uint16_t e[4]; } u;
            u.raw = *reinterpret_cast<const uint2*>((const uint16_t*)base + idx);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = up_any(u.e[k], dt);
        }
    } else {
#pragma unroll
        for (int q = 0; q < N / 8; ++q) {
            float y[8];
            load8(base, idx + 8 * q, dt, y);
#pragma unroll
            for (int k = 0; k < 8; ++k) x[8 * q + k] = y[k];
        }
    }
}
template <int N>
__device__ __forceinline__ void store_row(void* base, int64_t idx, int dt, const float (&x)[N]) {
    static_assert(N == 4 || N % 8 == 0, "a row is 4 or a multiple of 8 elements");
    if constexpr (N == 4) {
        if (dt == GDR_F32) {
            *reinterpret_cast<float4*>((float*)base + idx) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
            union { uint2 raw; uint16_t e[4]; } u;
#pragma unroll
            for (int k = 0; k < 4; ++k) u.e[k] = down_any(x[k], dt);
            *reinterpret_cast<uint2*>((uint16_t*)base + idx) = u.raw;
        }
    } else {
#pragma unroll
        for (int q = 0; q < N / 8; ++q) {
            float y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = x[8 * q + k];
            store8(base, idx + 8 * q, dt, y);
        }
    }
}

// <a, b> as one fma chain in ascending order
template <int N>
__device__ __forceinline__ float dot(const float (&a)[N], const float (&b)[N]) {
    float s = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < N; ++k) s = fmaf(a[k], b[k], s);
    return s;
}

// the sum over the LC lanes of a group, the same bits in every lane (lc = LC)
__device__ __forceinline__ float group_sum(float v, int lc) {
    for (int m = lc >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, GDR_WAVE);
    return v;
}

// mean and rstd of the row a group holds in x (lanes / pieces that are off hold zeros)
template <int K>
__device__ __forceinline__ void row_stats(const float (&x)[K][8], const bool (&on)[K], int lc, float inv_c, float eps, float& mean,
                                          float& rstd) {
    // around the row's first value: a constant row then has mean = that value and variance 0 exactly, whatever the value
    const float pivot = __shfl(x[0][0], (int)(threadIdx.x & (GDR_WAVE - 1)) & ~(lc - 1), GDR_WAVE);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) {
#pragma unroll
            for (int v = 0; v < 8; ++v) s += x[k][v] - pivot;
        }
    mean = pivot + group_sum(s, lc) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) {
#pragma unroll
            for (int v = 0; v < 8; ++v) { const float d = x[k][v] - mean; q += d * d; }
        }
    rstd = 1.0f / sqrtf(group_sum(q, lc) * inv_c + eps);
}

// lanes per row (as a shift, 8..64 lanes) and 8-channel pieces per lane, for C a multiple of 8 in 8..1024
static inline void row_shape(int C, int32_t* lc_shift, int* K) {
    const int vecs = C / 8;
    int sh = 3;
    while (sh < 6 && (1 << sh) < vecs) ++sh;
    *lc_shift = sh;
    *K = vecs > (1 << sh) ? 2 : 1;
}

}  // namespace gdr

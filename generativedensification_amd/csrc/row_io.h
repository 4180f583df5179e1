// row_io.h — elements of a runtime storage type (GDR_NORM_F16 / BF16 / F32) <-> f32 on the device, the lane-group row sum and
// the LayerNorm statistics of a row held by a lane group, as norm.hip, densify.hip, viewattn.hip, groupattn.hip and volcond.hip
// use them; ln_rows.h builds the rest of what the three row LayerNorms share on top of this (internal; include after
// gdr_common.h).
#pragma once
#include "half_bits.h"

namespace gdr {

__device__ __forceinline__ float up_any(uint16_t b, int dt) { return dt == GDR_NORM_BF16 ? up16<true>(b) : up16<false>(b); }
__device__ __forceinline__ uint16_t down_any(float f, int dt) { return dt == GDR_NORM_BF16 ? down16<true>(f) : down16<false>(f); }

// idx: an element index that is a multiple of 8 from a 16-byte aligned base
__device__ __forceinline__ void load8(const void* base, int64_t idx, int dt, float (&x)[8]) {
    if (dt == GDR_NORM_F32) {
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
    if (dt == GDR_NORM_F32) {
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
__device__ __forceinline__ float load1(const void* base, int64_t idx, int dt) {
    return dt == GDR_NORM_F32 ? ((const float*)base)[idx] : up_any(((const uint16_t*)base)[idx], dt);
}
__device__ __forceinline__ void store1(void* base, int64_t idx, int dt, float x) {
    if (dt == GDR_NORM_F32) ((float*)base)[idx] = x;
    else ((uint16_t*)base)[idx] = down_any(x, dt);
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

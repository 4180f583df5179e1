// half_bits.h — an element of a storage type (GDR_F16 / GDR_BF16 / GDR_F32) <-> f32 on the device (internal).  up16 / down16
// are the ONE statement of the 16-bit conversions; everything else here only picks between them: by a compile-time dtype
// (up<DT> / down<DT>: the MFMA row kernels behind mfma_rows.h, subm_conv.hip, segment.hip), by a run-time one (up_any /
// down_any / round_any: the row kernels behind row_io.h), or eight words of a compile-time dtype at a time (unpack8 / pack8:
// attn.hip's global and LDS rows).  So no two modules can drift apart in how they round.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gdr.h"

namespace gdr {

template <bool BF>
__device__ __forceinline__ float up16(uint16_t b) {
    if constexpr (BF) return __uint_as_float((uint32_t)b << 16);
    else return (float)__builtin_bit_cast(_Float16, b);
}

template <bool BF>
__device__ __forceinline__ uint16_t down16(float f) {   // round to nearest even
    if constexpr (BF) {
        uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    } else {
        return __builtin_bit_cast(uint16_t, (_Float16)f);
    }
}

// the storage type of a compile-time dtype DT
template <int DT> struct Stored {
    using type = typename std::conditional<DT == GDR_F32, float, uint16_t>::type;
    static constexpr int VE = 16 / (int)sizeof(type);       // elements per 16-byte vector
};

template <int DT> __device__ __forceinline__ float up(typename Stored<DT>::type v) {
    if constexpr (DT == GDR_F32) return v;
    else return up16<DT == GDR_BF16>(v);
}

template <int DT> __device__ __forceinline__ typename Stored<DT>::type down(float f) {   // round to nearest even
    if constexpr (DT == GDR_F32) return f;
    else return down16<DT == GDR_BF16>(f);
}

// a 16-bit word of the run-time dtype dt (GDR_F16 / GDR_BF16)
__device__ __forceinline__ float up_any(uint16_t b, int dt) { return dt == GDR_BF16 ? up16<true>(b) : up16<false>(b); }
__device__ __forceinline__ uint16_t down_any(float f, int dt) { return dt == GDR_BF16 ? down16<true>(f) : down16<false>(f); }
// v as an element of storage type dt holds it
__device__ __forceinline__ float round_any(float v, int dt) { return dt == GDR_F32 ? v : up_any(down_any(v, dt), dt); }

// eight 16-bit words in one 16-byte vector <-> x[0 .. 7]
template <bool BF>
__device__ __forceinline__ void unpack8(const uint4 w, float* x) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x[2 * e] = up16<BF>((uint16_t)(u[e] & 0xffffu));
        x[2 * e + 1] = up16<BF>((uint16_t)(u[e] >> 16));
    }
}

template <bool BF>
__device__ __forceinline__ uint4 pack8(const float* x) {
    uint32_t u[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = (uint32_t)down16<BF>(x[2 * e]) | ((uint32_t)down16<BF>(x[2 * e + 1]) << 16);
    return make_uint4(u[0], u[1], u[2], u[3]);
}

}  // namespace gdr

// half_bits.h — f16 / bf16 storage words <-> f32 on the device (internal).  The ONE statement of this conversion: attn.hip
// and subm_conv.hip both round through it, so the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace gdr

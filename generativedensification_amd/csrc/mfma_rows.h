// mfma_rows.h — the MFMA matters the dense row-GEMM kernels (conv3d.hip, deconv3d.hip, coarsehead.hip, finehead.hip) share on
// the device (internal): the tile shapes and accumulator of a compute dtype, the A row a lane feeds, and one 16 x 16 MFMA
// step over the sum elements of a 64-byte LDS row pair.  Elements and their conversions are half_bits.h's and row_io.h's.
// What only the two heads share sits on top of this in head_rows.h.  Include after gdr_common.h and row_io.h.
#pragma once

namespace gdr {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// DT: GDR_F16, GDR_BF16, GDR_F32
template <int DT> struct El : Stored<DT> {
    static constexpr int KC = 4 * Stored<DT>::VE;           // sum elements per LDS row
    using acc = typename std::conditional<DT == GDR_F32, f64x4, f32x4>::type;      // one 16 x 16 tile's share of a lane
};

// The A row (an output channel of the tile) whose fragment lane l16 supplies.  The f32-input MFMAs return rows 4 quad .. + 3 in
// a lane's four registers, the f64 one rows quad, quad + 4, quad + 8, quad + 12: feeding channel 4 (m % 4) + m / 4 as A row m
// makes those the channels 4 quad .. + 3 again, so every dtype shares one epilogue.
template <int DT> __device__ __forceinline__ int a_row(int l16) {
    if constexpr (DT == GDR_F32) return 4 * (l16 & 3) + (l16 >> 2);
    else return l16;
}

// D += A B for one 16 x 16 tile over the KC sum elements of one LDS row pair; a / b: this lane's 16 bytes of its A row and
// B column.  16 bits: lane (l16, quad) holds k = 8 quad .. + 7, one 16x16x32 step into f32.  f32: it holds k = 4 quad .. + 3
// and step s takes element s from every lane, so the four steps cover k = 4 quad + s: a permutation of the sum, the same for
// A and B.  The f32 operands go through the f64 MFMA: a product of two f32 is exact in f64 and the sum keeps 53 bits, so the
// one rounding of the epilogue is the only one that shows (an f32 fma chain over 27 CA terms misses the accuracy bar against
// a convolution that accumulates in f64).
template <int DT> __device__ __forceinline__ void mma_row(const uint4& a, const uint4& b, typename El<DT>::acc& acc) {
    if constexpr (DT == GDR_F32) {
        const f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fa[s], (double)fb[s], acc, 0, 0, 0);
    } else if constexpr (DT == GDR_F16) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
}

}  // namespace gdr

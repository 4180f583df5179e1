// serial_bits.h — the word-parallel bit arithmetic of the point serialization (serialize.hip): Morton interleave and the
// Hilbert walk of Skilling ("Programming the Hilbert curve", 2004) on whole integers.  Plain C++ with no device intrinsics.
#pragma once
#include <stdint.h>

#ifndef GDR_HD
#define GDR_HD __host__ __device__ __forceinline__
#endif

namespace gdr {

// bit i of v (i < 21) -> bit 3i
GDR_HD uint64_t serial_spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | (x << 32)) & UINT64_C(0x001f00000000ffff);
    x = (x | (x << 16)) & UINT64_C(0x001f0000ff0000ff);
    x = (x | (x << 8)) & UINT64_C(0x100f00f00f00f00f);
    x = (x | (x << 4)) & UINT64_C(0x10c30c30c30c30c3);
    x = (x | (x << 2)) & UINT64_C(0x1249249249249249);
    return x;
}

// bit 3i of x -> bit i
GDR_HD uint32_t serial_compact3(uint64_t x) {
    x &= UINT64_C(0x1249249249249249);
    x = (x ^ (x >> 2)) & UINT64_C(0x10c30c30c30c30c3);
    x = (x ^ (x >> 4)) & UINT64_C(0x100f00f00f00f00f);
    x = (x ^ (x >> 8)) & UINT64_C(0x001f0000ff0000ff);
    x = (x ^ (x >> 16)) & UINT64_C(0x001f00000000ffff);
    x = (x ^ (x >> 32)) & UINT64_C(0x00000000001fffff);
    return (uint32_t)x;
}

// per bit level from the most significant: a, then b, then c
GDR_HD uint64_t serial_interleave3(uint32_t a, uint32_t b, uint32_t c) {
    return (serial_spread3(a) << 2) | (serial_spread3(b) << 1) | serial_spread3(c);
}

// one (level, dimension) step of the walk, dimension d != 0: its own inverse
#define GDR_SERIAL_STEP(X0, XD, Q, P)            \
    do {                                         \
        if ((XD) & (Q)) (X0) ^= (P);             \
        else {                                   \
            const uint32_t t_ = ((X0) ^ (XD)) & (P); \
            (X0) ^= t_;                          \
            (XD) ^= t_;                          \
        }                                        \
    } while (0)

// a, b, c < 2^depth: the Hilbert index of the cell, 3 * depth bits
GDR_HD uint64_t serial_hilbert_encode(uint32_t a, uint32_t b, uint32_t c, int depth) {
    for (uint32_t q = 1u << (depth - 1); q > 1; q >>= 1) {   // (the last level has no lower bits)
        const uint32_t p = q - 1;
        if (a & q) a ^= p;                                   // dimension 0 against itself: only the inversion is left
        GDR_SERIAL_STEP(a, b, q, p);
        GDR_SERIAL_STEP(a, c, q, p);
    }
    uint64_t h = serial_interleave3(a, b, c);
    h ^= h >> 1; h ^= h >> 2; h ^= h >> 4; h ^= h >> 8; h ^= h >> 16; h ^= h >> 32;   // prefix XOR from the top: Gray -> binary
    return h;
}

// h < 2^(3 * depth) -> the cell
GDR_HD void serial_hilbert_decode(uint64_t h, int depth, uint32_t* a_, uint32_t* b_, uint32_t* c_) {
    h ^= h >> 1;                                             // binary -> Gray
    uint32_t a = serial_compact3(h >> 2), b = serial_compact3(h >> 1), c = serial_compact3(h);
    for (uint32_t q = 2; q < (1u << depth); q <<= 1) {       // the walk backwards: levels from the least significant, dims 2, 1, 0
        const uint32_t p = q - 1;
        GDR_SERIAL_STEP(a, c, q, p);
        GDR_SERIAL_STEP(a, b, q, p);
        if (a & q) a ^= p;
    }
    *a_ = a; *b_ = b; *c_ = c;
}

}  // namespace gdr

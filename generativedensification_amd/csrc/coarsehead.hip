// coarsehead.hip — the coarse Gaussian head (gfx950), forward and every gradient: the reference's Decoder.forward_coarse
// (lightning/network.py: mlp_coarse = Linear(C, C), ReLU, Linear(C, C), ReLU, Linear(C, K P), `.float()`, the five-way split, the
// two shifts and 2 sigmoid - 1 on the offsets) and the three lines of Network.forward behind it (the offset Gaussian centres
// and the opacity mask), from the dense (rows, C) voxel rows csrc/deconv3d.hip hands on.  Public ABI: include/gdr.h
// gdr_coarsehead_*.
//
// Semantics, restated (tests/coarsehead_ref.py holds the f64 statement).  P = 3 + sh_dim + 1 + 3 + 4, row r, element e = r K + k:
//   h1 = relu(rd(x W1^T + b1)),  h2 = relu(rd(h1 W2^T + b2)),  v = h2 W3^T + b3      rd: one rounding to the compute dtype; v is
//                                                                                     never rounded to 16 bits
//   column j = k P + c of v:  c < 3: offset[e][c] = 2 sigmoid(v) - 1;  c < 3 + sh_dim: sh[e][c - 3] = v;
//     c = 3 + sh_dim: opacity[e] = v + opacity_shift;  the next 3: scaling[e] = v + scaling_shift;  the last 4: rotation[e] = v
//   centers[e] = group_centers[r % N] + offset[e] half_cell;   mask[e] = sigmoid(opacity[e]) > threshold
//   backward: dv (offset columns) = (g_offset + g_centers half_cell) (1 - o)(1 + o) / 2 with o the saved offset; the other
//     columns pass through; dz3 = rd(dv);  dz2 = rd([h2 > 0] dz3 W3);  dz1 = rd([h1 > 0] dz2 W2);  grad_x = rd(dz1 W1);
//     grad_W3 = dz3^T h2, grad_W2 = dz2^T h1, grad_W1 = dz1^T x;  grad_b = the column sums of dz.
//
// Structure (256 threads = 4 waves; D rows are channels, D columns data rows, as in conv3d.hip and deconv3d.hip).
//   pack: one launch rounds the three weights to the compute dtype into one zero-padded buffer: [out][in] for the products of
//     the forward direction, [in][out] for those of the backward; both sides padded to whole sum chunks, so no product
//     guards an index.
//   forward: a workgroup owns HEAD_ROWS = 64 consecutive rows, wave w the 16 rows of tile w.  The rows are staged in LDS, every
//     layer reads its operand rows from LDS and leaves its rounded, gated result in LDS for the next; the weight fragments are
//     read from the packed buffer (global memory: every workgroup reads the same < 30 KB at C = 80).  The last layer's
//     epilogue leaves the (64, K P) values and the centres in an fp32 LDS stage, and the workgroup copies each of the five
//     (seven) outputs out as one contiguous run.
//   backward: a workgroup owns a slab of rows and walks it `step` rows at a time (64, 32 or 16: what fits LDS).  Per step it
//     recomputes h1 and h2, gathers dz3 from the upstream gradients, and runs dz3 -> dz2 -> dz1 -> grad_x, the (row tile,
//     channel tile) pairs of every product dealt round to the 4 waves.  Every activation is also left transposed ([channel][row])
//     so that the row is the MFMA's sum index of the weight gradients: a wave keeps HEAD_TPW 16 x 16 tiles of the three
//     grad_W in registers over the whole slab (blockIdx.y selects which, when there are more than 4 HEAD_TPW), thread c the
//     column sums of channel c; one partial set per slab; a second launch adds them, 16 segments of the slabs per element in
//     slab order, then the 16 segment sums.  No atomics.
// What this file has in common with finehead.hip (the geometry, the tile product, the x-row staging, grad_x, the weight-gradient
// tile bookkeeping, the fold, the backward's LDS carve) is head_rows.h.
// Tile sizes, the step and where the weights sit are unmeasured choices.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "mfma_rows.h"
#include "head_rows.h"

namespace gdr {
namespace {

constexpr int CH_MAX_SLABS = 1024;
constexpr int CH_SLAB_MIN = GDR_COARSEHEAD_SLAB_MIN;

// the shape and its padded sizes
struct Geo {
    int32_t C, K, sh, P, KP;
    int32_t Cpad, Opad;      // C and K P rounded up to whole sum chunks (32 elements of 16 bits, 16 of f32)
    int32_t C16, O16;        // ... to whole 16 x 16 tiles
};

Geo geo_of(int dtype, int C, int K, int sh) {
    Geo g;
    const int kc = dtype == GDR_NORM_F32 ? 16 : 32;
    g.C = C; g.K = K; g.sh = sh; g.P = 3 + sh + 1 + 3 + 4; g.KP = K * g.P;
    g.Cpad = round_up(C, kc); g.Opad = round_up(g.KP, kc); g.C16 = round_up(C, 16); g.O16 = round_up(g.KP, 16);
    return g;
}

// element offsets of the packed buffers.  forward: W1 [Cpad][Cpad], W2 [Cpad][Cpad], W3 [Opad][Cpad], all [out][in].
// backward: W1, W2 as above, then W1t [Cpad][Cpad], W2t [Cpad][Cpad], W3t [Cpad][Opad], all [in][out].
__host__ __device__ inline int64_t sq_of(const Geo& g) { return (int64_t)g.Cpad * g.Cpad; }
__host__ __device__ inline int64_t w3_of(const Geo& g) { return (int64_t)g.Opad * g.Cpad; }
__host__ __device__ inline int64_t packed_elems(const Geo& g, bool backward) { return backward ? 4 * sq_of(g) + w3_of(g) : 2 * sq_of(g) + w3_of(g); }

// elements of one partial set: grad_W1, grad_W2 (C, C), grad_W3 (K P, C), grad_b1, grad_b2 (C), grad_b3 (K P)
__host__ __device__ inline int64_t partial_elems(const Geo& g) { return 2 * (int64_t)g.C * g.C + (int64_t)g.KP * g.C + 2 * g.C + g.KP; }

// relu of the pre-activation rounded to the compute dtype
template <int DT> __device__ __forceinline__ typename El<DT>::type relu_rd(Sc<DT> z) {
    const typename El<DT>::type r = down<DT>((float)z);
    return up<DT>(r) > 0.0f ? r : down<DT>(0.0f);
}

// ---- pack -------------------------------------------------------------------------------------------------------------------------
struct PackP {
    const void* w[3];
    int32_t w_dtype[3];
    void* packed;
    Geo g;
    int32_t backward;
    int64_t total;
};

template <int DT>
__global__ __launch_bounds__(HEAD_BLOCK) void coarsehead_pack_kernel(const PackP p) {
    int64_t i = (int64_t)blockIdx.x * HEAD_BLOCK + threadIdx.x;
    if (i >= p.total) return;
    const int64_t at = i, sq = sq_of(p.g);
    const int C = p.g.C, KP = p.g.KP, Cpad = p.g.Cpad, Opad = p.g.Opad;
    float v = 0.0f;
    if (i < 2 * sq) {                               // W1, W2 [out][in]
        const int l = (int)(i / sq);
        i -= l * sq;
        const int r = (int)(i / Cpad), c = (int)(i % Cpad);
        if (r < C && c < C) v = load1(p.w[l], (int64_t)r * C + c, p.w_dtype[l]);
    } else if (!p.backward) {                       // W3 [out][in]
        i -= 2 * sq;
        const int r = (int)(i / Cpad), c = (int)(i % Cpad);
        if (r < KP && c < C) v = load1(p.w[2], (int64_t)r * C + c, p.w_dtype[2]);
    } else if (i < 4 * sq) {                        // W1t, W2t [in][out]
        i -= 2 * sq;
        const int l = (int)(i / sq);
        i -= l * sq;
        const int r = (int)(i / Cpad), c = (int)(i % Cpad);
        if (r < C && c < C) v = load1(p.w[l], (int64_t)c * C + r, p.w_dtype[l]);
    } else {                                        // W3t [in][out]
        i -= 4 * sq;
        const int r = (int)(i / Opad), c = (int)(i % Opad);
        if (r < C && c < KP) v = load1(p.w[2], (int64_t)c * C + r, p.w_dtype[2]);
    }
    ((typename El<DT>::type*)p.packed)[at] = down<DT>(v);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
struct FwdP {
    const void* x;             // (rows, C) dense
    const void* packed;
    const void* b[3];
    int32_t b_dtype[3];
    const float* gc;           // (N, 3) group centres, or NULL
    float* out[5];             // offset (E, 3), sh (E, sh), scaling (E, 3), rotation (E, 4), opacity (E, 1); E = rows K
    float* centers;            // (E, 3) or NULL
    uint8_t* mask;             // (E) or NULL
    int64_t n, N;
    double opacity_shift, scaling_shift, half_cell, threshold;
    Geo g;
    int32_t lda, sw;           // LDS row strides: the operand rows (elements), the fp32 stage (floats)
    int64_t region0;           // bytes of the first LDS region
};

// the workgroup copies columns off .. off + w - 1 of every (row, k) of the stage out as one contiguous run
__device__ __forceinline__ void copy_out(float* dst, const float* stage, int sw, int64_t e0, int count, int K, int w, int stride, int off, int tid) {
    if (!dst) return;
    dst += e0 * w;
    for (int i = tid; i < count * w; i += HEAD_BLOCK) {
        const int el = i / w, c = i - el * w, r = el / K, k = el - r * K;
        dst[i] = stage[r * sw + k * stride + off + c];
    }
}

template <int DT>
__global__ __launch_bounds__(HEAD_BLOCK) void coarsehead_forward_kernel(const FwdP p) {
    using E = typename El<DT>::type;
    using T = Sc<DT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ch_lds[];
    E* bufA = (E*)ch_lds;                              // h1; later the fp32 stage
    E* bufB = (E*)(ch_lds + p.region0);                // x, then h2
    float* stage = (float*)ch_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const Geo& g = p.g;
    const int lda = p.lda, Cpad = g.Cpad;
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;
    const E* X = (const E*)p.x;
    const E* W1 = (const E*)p.packed;
    const E* W2 = W1 + sq_of(g);
    const E* W3 = W2 + sq_of(g);

    stage_rows<DT>(X, row0, p.n, HEAD_ROWS, g.C, Cpad, bufB, lda, false, nullptr, 0, tid);
    __syncthreads();
    const int r = 16 * wave + l16;                     // this lane's row of the tile
#pragma unroll 1
    for (int layer = 0; layer < 2; ++layer) {
        const E* W = layer ? W2 : W1;
        const E* src = layer ? bufA : bufB;
        E* dst = layer ? bufB : bufA;
        for (int jt = 0; jt < Cpad / 16; ++jt) {
            typename El<DT>::acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W + (int64_t)16 * jt * Cpad, Cpad, src + 16 * wave * lda, lda, Cpad, l16, quad, acc);
            E h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                h[e] = relu_rd<DT>((T)acc[e] + bias_at<DT>(p.b[layer], p.b_dtype[layer], 16 * jt + 4 * quad + e, g.C));
            store4<DT>(dst + r * lda + 16 * jt + 4 * quad, h);
        }
        __syncthreads();
    }
    // the last layer: D rows are the K P columns.  (the stage overlays h1: every wave is past it)
    const int64_t row = row0 + r;
    const bool valid = row < p.n;
    for (int jt = 0; jt < g.O16 / 16; ++jt) {
        typename El<DT>::acc v3 = {0, 0, 0, 0};
        tile_mma<DT>(W3 + (int64_t)16 * jt * Cpad, Cpad, bufB + 16 * wave * lda, lda, Cpad, l16, quad, v3);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 16 * jt + 4 * quad + e;
            if (j >= g.KP) continue;
            const int k = j / g.P, c = j - k * g.P;
            // the epilogue in f64 for every dtype: the one rounding to f32 is then the only error it adds to the sum
            double v = (double)v3[e] + (double)bias_at<DT>(p.b[2], p.b_dtype[2], j, g.KP);
            if (c < 3) {
                v = tanh(0.5 * v);                     // = 2 sigmoid(v) - 1, without the cancellation near 0
                if (p.centers) stage[r * p.sw + g.KP + 3 * k + c] = valid ? (float)((double)p.gc[(row % p.N) * 3 + c] + v * p.half_cell) : 0.0f;
            } else if (c == 3 + g.sh) {
                v += p.opacity_shift;
            } else if (c > 3 + g.sh && c < 7 + g.sh) {
                v += p.scaling_shift;
            }
            stage[r * p.sw + j] = (float)v;
        }
    }
    __syncthreads();
    const int64_t left = p.n - row0;
    const int count = (int)(left < HEAD_ROWS ? left : HEAD_ROWS) * g.K;
    const int64_t e0 = row0 * g.K;
    copy_out(p.out[0], stage, p.sw, e0, count, g.K, 3, g.P, 0, tid);
    copy_out(p.out[1], stage, p.sw, e0, count, g.K, g.sh, g.P, 3, tid);
    copy_out(p.out[4], stage, p.sw, e0, count, g.K, 1, g.P, 3 + g.sh, tid);
    copy_out(p.out[2], stage, p.sw, e0, count, g.K, 3, g.P, 4 + g.sh, tid);
    copy_out(p.out[3], stage, p.sw, e0, count, g.K, 4, g.P, 7 + g.sh, tid);
    copy_out(p.centers, stage + g.KP, p.sw, e0, count, g.K, 3, 3, 0, tid);
    if (p.mask)
        for (int i = tid; i < count; i += HEAD_BLOCK) {
            const int rr = i / g.K, k = i - rr * g.K;
            const float op = stage[rr * p.sw + k * g.P + 3 + g.sh];
            p.mask[e0 + i] = 1.0f / (1.0f + expf(-op)) > (float)p.threshold ? 1 : 0;
        }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
struct BwdP {
    const void* x;
    const void* packed;        // the backward's packed buffer
    const void* b[2];
    int32_t b_dtype[2];
    const float* offset;       // the forward's offset output (E, 3)
    const float* gout[5];      // upstream gradients in the order of FwdP.out, each dense or NULL
    const float* gcenters;     // (E, 3) or NULL
    void* grad_x;              // (rows, C) or NULL
    void* part;                // one partial set per slab (f32; f64 for f32 rows), or NULL
    int64_t n, slab_rows;
    double half_cell;
    Geo g;
    int32_t step, lda, ldz, ldt;      // rows per step and the LDS strides (elements)
};

// dz3 of columns off .. off + w - 1 from one upstream gradient, in both layouts
template <int DT>
__device__ __forceinline__ void gather_dz3(const BwdP& p, const float* gsrc, bool is_offset, int w, int off, int64_t r0, int64_t r_end,
                                           typename El<DT>::type* RZ, typename El<DT>::type* ZT, int tid) {
    using T = Sc<DT>;
    const int K = p.g.K;
    const int64_t left = r_end - r0;
    const int count = (int)(left < p.step ? left : p.step) * K;
    const int64_t base = r0 * K * w;
    for (int i = tid; i < p.step * K * w; i += HEAD_BLOCK) {
        const int el = i / w, c = i - el * w, r = el / K, k = el - r * K;
        T gv = 0;
        if (el < count) {
            if (gsrc) gv = (T)gsrc[base + i];
            if (is_offset) {
                if (p.gcenters) gv += (T)p.gcenters[base + i] * (T)p.half_cell;
                const T o = (T)p.offset[base + i];
                gv *= ((T)1 - o) * ((T)1 + o) * (T)0.5;
            }
        }
        const typename El<DT>::type e = down<DT>((float)gv);
        const int j = k * p.g.P + off + c;
        RZ[r * p.ldz + j] = e;
        ZT[j * p.ldt + r] = e;
    }
}

template <int DT>
__global__ __launch_bounds__(HEAD_BLOCK) void coarsehead_backward_kernel(const BwdP p) {
    using E = typename El<DT>::type;
    using T = Sc<DT>;
    using Acc = typename El<DT>::acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char ch_lds[];
    const Geo& g = p.g;
    const int C = g.C, Cpad = g.Cpad, Opad = g.Opad, KP = g.KP, step = p.step, lda = p.lda, ldz = p.ldz, ldt = p.ldt, rt = step / 16;
    E* R0 = (E*)ch_lds;                  // x rows, then dz2 rows
    E* R1 = R0 + step * lda;             // h1 rows, then dz1 rows
    E* RZ = R1 + step * lda;             // dz3 rows
    E* xT = RZ + step * ldz;             // [channel][row] from here on
    E* h1T = xT + Cpad * ldt;
    E* h2T = h1T + Cpad * ldt;
    E* z1T = h2T + Cpad * ldt;
    E* z2T = z1T + Cpad * ldt;
    E* z3T = z2T + Cpad * ldt;           // [Opad][ldt]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const E* X = (const E*)p.x;
    const E* W1 = (const E*)p.packed;
    const E* W2 = W1 + sq_of(g);
    const E* W1t = W2 + sq_of(g);
    const E* W2t = W1t + sq_of(g);
    const E* W3t = W2t + sq_of(g);
    const bool sums = p.part != nullptr;
    const int64_t r_begin = (int64_t)blockIdx.x * p.slab_rows;
    const int64_t r_end = r_begin + p.slab_rows < p.n ? r_begin + p.slab_rows : p.n;

    // the weight-gradient tiles of this wave: tile t of [grad_W1 | grad_W2 | grad_W3], 16 x 16 each, (out tile, in tile) row-major
    const int c16 = g.C16 / 16, n1 = c16 * c16;
    WgTiles<DT> wg = {};
    wg.n = 3; wg.ntiles = 2 * n1 + (g.O16 / 16) * c16; wg.C = C; wg.c16 = c16;
    wg.s[0] = {z1T, xT, 0, C, 0};
    wg.s[1] = {z2T, h1T, n1, C, (int64_t)C * C};
    wg.s[2] = {z3T, h2T, 2 * n1, KP, 2 * (int64_t)C * C};
    const int t_first = (blockIdx.y * 4 + wave) * HEAD_TPW;
    Acc accW[HEAD_TPW];
#pragma unroll
    for (int i = 0; i < HEAD_TPW; ++i) accW[i] = Acc{0, 0, 0, 0};
    T db1 = 0, db2 = 0, db3 = 0;

    // the pad columns of dz3 are never written again
    for (int i = tid; i < step * (Opad - KP); i += HEAD_BLOCK) {
        const int r = i / (Opad - KP), j = KP + i - r * (Opad - KP);
        RZ[r * ldz + j] = down<DT>(0.0f);
        z3T[j * ldt + r] = down<DT>(0.0f);
    }

    for (int64_t r0 = r_begin; r0 < r_end; r0 += step) {
        stage_rows<DT>(X, r0, r_end, step, C, Cpad, R0, lda, sums, xT, ldt, tid);
        __syncthreads();
        // h1 -> R1 and h1T
        for (int pr = wave; pr < (Cpad / 16) * rt; pr += 4) {
            const int ti = pr % rt, jt = pr / rt, r = 16 * ti + l16, ch = 16 * jt + 4 * quad;
            Acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W1 + (int64_t)16 * jt * Cpad, Cpad, R0 + 16 * ti * lda, lda, Cpad, l16, quad, acc);
            E h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = relu_rd<DT>((T)acc[e] + bias_at<DT>(p.b[0], p.b_dtype[0], ch + e, C));
                h1T[(ch + e) * ldt + r] = h[e];
            }
            store4<DT>(R1 + r * lda + ch, h);
        }
        __syncthreads();
        // h2 -> h2T;  dz3 -> RZ and z3T
        for (int pr = wave; pr < (Cpad / 16) * rt; pr += 4) {
            const int ti = pr % rt, jt = pr / rt, r = 16 * ti + l16, ch = 16 * jt + 4 * quad;
            Acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W2 + (int64_t)16 * jt * Cpad, Cpad, R1 + 16 * ti * lda, lda, Cpad, l16, quad, acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) h2T[(ch + e) * ldt + r] = relu_rd<DT>((T)acc[e] + bias_at<DT>(p.b[1], p.b_dtype[1], ch + e, C));
        }
        gather_dz3<DT>(p, p.gout[0], true, 3, 0, r0, r_end, RZ, z3T, tid);
        gather_dz3<DT>(p, p.gout[1], false, g.sh, 3, r0, r_end, RZ, z3T, tid);
        gather_dz3<DT>(p, p.gout[4], false, 1, 3 + g.sh, r0, r_end, RZ, z3T, tid);
        gather_dz3<DT>(p, p.gout[2], false, 3, 4 + g.sh, r0, r_end, RZ, z3T, tid);
        gather_dz3<DT>(p, p.gout[3], false, 4, 7 + g.sh, r0, r_end, RZ, z3T, tid);
        __syncthreads();
        // dz2 = [h2 > 0] dz3 W3 -> R0 and z2T
        for (int pr = wave; pr < (Cpad / 16) * rt; pr += 4) {
            const int ti = pr % rt, jt = pr / rt, r = 16 * ti + l16, ch = 16 * jt + 4 * quad;
            Acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W3t + (int64_t)16 * jt * Opad, Opad, RZ + 16 * ti * ldz, ldz, Opad, l16, quad, acc);
            E d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d[e] = up<DT>(h2T[(ch + e) * ldt + r]) > 0.0f ? down<DT>((float)acc[e]) : down<DT>(0.0f);
                z2T[(ch + e) * ldt + r] = d[e];
            }
            store4<DT>(R0 + r * lda + ch, d);
        }
        __syncthreads();
        // dz1 = [h1 > 0] dz2 W2 -> R1 and z1T
        for (int pr = wave; pr < (Cpad / 16) * rt; pr += 4) {
            const int ti = pr % rt, jt = pr / rt, r = 16 * ti + l16, ch = 16 * jt + 4 * quad;
            Acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W2t + (int64_t)16 * jt * Cpad, Cpad, R0 + 16 * ti * lda, lda, Cpad, l16, quad, acc);
            E d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d[e] = up<DT>(h1T[(ch + e) * ldt + r]) > 0.0f ? down<DT>((float)acc[e]) : down<DT>(0.0f);
                z1T[(ch + e) * ldt + r] = d[e];
            }
            store4<DT>(R1 + r * lda + ch, d);
        }
        __syncthreads();
        // grad_x = dz1 W1
        if (p.grad_x && blockIdx.y == 0) grad_x_tiles<DT>(W1t, R1, lda, p.grad_x, r0, r_end, rt, C, g.C16, Cpad, wave, l16, quad);
        if (sums) {
            wgrad_step<DT>(wg, t_first, ldt, step, l16, quad, accW);
            if (blockIdx.y == 0) {
                if (tid < C)
                    for (int r = 0; r < step; ++r) {
                        db1 += (T)up<DT>(z1T[tid * ldt + r]);
                        db2 += (T)up<DT>(z2T[tid * ldt + r]);
                    }
                if (tid < KP)
                    for (int r = 0; r < step; ++r) db3 += (T)up<DT>(z3T[tid * ldt + r]);
            }
        }
        __syncthreads();
    }
    if (!sums) return;
    T* part = (T*)p.part + (int64_t)blockIdx.x * partial_elems(g);
    wgrad_store<DT>(wg, t_first, part, l16, quad, accW);
    if (blockIdx.y == 0) {
        T* pb = part + 2 * (int64_t)C * C + (int64_t)KP * C;
        if (tid < C) {
            pb[tid] = db1;
            pb[C + tid] = db2;
        }
        if (tid < KP) pb[2 * C + tid] = db3;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
bool bad_shape(int32_t C, int32_t K, int32_t sh) {
    if (C < 8 || C > GDR_COARSEHEAD_MAX_C || C % 8 || K < 1 || K > 4) return true;
    if (sh != 3 && sh != 12 && sh != 27 && sh != 48) return true;
    return K * (3 + sh + 1 + 3 + 4) > GDR_COARSEHEAD_MAX_OUT;
}

bool bad_rows_count(int64_t rows, int32_t K) { return rows > ((INT64_C(1) << 31) - 1) / K; }

const char* const CH_ENVELOPE = "coarsehead: C must be a multiple of 8 in 8..GDR_COARSEHEAD_MAX_C, K in 1..4, sh_dim one of 3, 12, 27, 48, "
                                "K P <= GDR_COARSEHEAD_MAX_OUT and rows K below 2^31";

int slabs_of(int64_t n) { return gdr::slabs_of(n, CH_SLAB_MIN, CH_MAX_SLABS); }

struct FwdLds { int lda, sw; size_t region0, total; };
FwdLds fwd_lds(int dtype, const Geo& g) {
    FwdLds l;
    l.lda = g.Cpad + (dtype == GDR_NORM_F32 ? 4 : 8);
    l.sw = g.KP + 3 * g.K + 1;
    const size_t rows = (size_t)HEAD_ROWS * l.lda * esize(dtype), stage = (size_t)HEAD_ROWS * l.sw * sizeof(float);
    l.region0 = align_up(rows > stage ? rows : stage, 16);
    l.total = l.region0 + rows;
    return l;
}

// the backward's steps: xT, h1T, h2T, z1T and z2T are its transposed Cpad-channel buffers
BwdLds bwd_lds(int dtype, const Geo& g) { return bwd_lds(dtype, g.Cpad, g.Opad, 5); }

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_coarsehead_workspace_bytes(int32_t what, int32_t dtype, int64_t rows, int32_t C, int32_t K, int32_t sh_dim) {
    if (bad_dtype(dtype)) { invalid_arg("coarsehead_workspace_bytes: unknown dtype"); return 0; }
    if (rows < 0) { invalid_arg("coarsehead_workspace_bytes: rows must be >= 0"); return 0; }
    if (bad_shape(C, K, sh_dim) || bad_rows_count(rows, K)) { unsupported(CH_ENVELOPE); return 0; }
    const Geo g = geo_of(dtype, C, K, sh_dim);
    switch (what) {
        case GDR_COARSEHEAD_WS_PACKED_FORWARD: return align_up((size_t)packed_elems(g, false) * esize(dtype));
        case GDR_COARSEHEAD_WS_PACKED_BACKWARD: return align_up((size_t)packed_elems(g, true) * esize(dtype));
        case GDR_COARSEHEAD_WS_PARTIALS:
            return align_up((size_t)slabs_of(rows) * partial_elems(g) * (dtype == GDR_NORM_F32 ? sizeof(double) : sizeof(float)));
    }
    invalid_arg("coarsehead_workspace_bytes: unknown workspace kind");
    return 0;
}

int gdr_coarsehead_pack(const void* w1, int32_t w1_dtype, const void* w2, int32_t w2_dtype, const void* w3, int32_t w3_dtype, int32_t C,
                        int32_t K, int32_t sh_dim, int32_t backward, void* packed, int32_t dtype, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(w1_dtype) || bad_dtype(w2_dtype) || bad_dtype(w3_dtype)) return invalid_arg("coarsehead_pack: unknown dtype");
    if (bad_shape(C, K, sh_dim)) return unsupported(CH_ENVELOPE);
    if (!w1 || !w2 || !w3 || !packed) return invalid_arg("coarsehead_pack: NULL argument");
    if (misaligned(w1, esize(w1_dtype) - 1) || misaligned(w2, esize(w2_dtype) - 1) || misaligned(w3, esize(w3_dtype) - 1) || misaligned(packed, 15))
        return unsupported("coarsehead_pack: a weight must be aligned to its element and the packed buffer to 16 bytes");
    PackP p = {};
    p.w[0] = w1; p.w[1] = w2; p.w[2] = w3; p.w_dtype[0] = w1_dtype; p.w_dtype[1] = w2_dtype; p.w_dtype[2] = w3_dtype;
    p.packed = packed; p.g = geo_of(dtype, C, K, sh_dim); p.backward = backward ? 1 : 0; p.total = packed_elems(p.g, backward != 0);
    const dim3 grid((uint32_t)div_up(p.total, (int64_t)HEAD_BLOCK));
    if (dtype == GDR_NORM_F16) hipLaunchKernelGGL(coarsehead_pack_kernel<GDR_NORM_F16>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    else if (dtype == GDR_NORM_BF16) hipLaunchKernelGGL(coarsehead_pack_kernel<GDR_NORM_BF16>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(coarsehead_pack_kernel<GDR_NORM_F32>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("coarsehead_pack_kernel");
}

int gdr_coarsehead_forward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, const void* b2, int32_t b2_dtype,
                           const void* b3, int32_t b3_dtype, int64_t rows, int64_t N, int32_t C, int32_t K, int32_t sh_dim,
                           double opacity_shift, double scaling_shift, const void* group_centers, double half_cell, double threshold,
                           void* offset, void* sh, void* scaling, void* rotation, void* opacity, void* centers, void* mask, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(b1_dtype) || bad_dtype(b2_dtype) || bad_dtype(b3_dtype)) return invalid_arg("coarsehead_forward: unknown dtype");
    if (rows < 0) return invalid_arg("coarsehead_forward: rows must be >= 0");
    if (bad_shape(C, K, sh_dim) || bad_rows_count(rows, K)) return unsupported(CH_ENVELOPE);
    if (centers && (!group_centers || N < 1 || rows % N)) return invalid_arg("coarsehead_forward: centers need group_centers (N, 3) with N dividing rows");
    if (rows == 0) return GDR_OK;
    if (!x || !packed || !b1 || !b2 || !b3 || !offset || !sh || !scaling || !rotation || !opacity) return invalid_arg("coarsehead_forward: NULL argument");
    if (misaligned(x, 15) || misaligned(packed, 15) || misaligned(b1, esize(b1_dtype) - 1) || misaligned(b2, esize(b2_dtype) - 1) ||
        misaligned(b3, esize(b3_dtype) - 1) || misaligned(group_centers, 3) || misaligned(offset, 3) || misaligned(sh, 3) || misaligned(scaling, 3) ||
        misaligned(rotation, 3) || misaligned(opacity, 3) || misaligned(centers, 3))
        return unsupported("coarsehead_forward: x and the packed buffer must start on 16 bytes, everything else on its element");
    FwdP p = {};
    p.x = x; p.packed = packed; p.b[0] = b1; p.b[1] = b2; p.b[2] = b3; p.b_dtype[0] = b1_dtype; p.b_dtype[1] = b2_dtype; p.b_dtype[2] = b3_dtype;
    p.gc = (const float*)group_centers; p.out[0] = (float*)offset; p.out[1] = (float*)sh; p.out[2] = (float*)scaling; p.out[3] = (float*)rotation;
    p.out[4] = (float*)opacity; p.centers = (float*)centers; p.mask = (uint8_t*)mask; p.n = rows; p.N = centers ? N : 1;
    p.opacity_shift = opacity_shift; p.scaling_shift = scaling_shift; p.half_cell = half_cell; p.threshold = threshold;
    p.g = geo_of(dtype, C, K, sh_dim);
    const FwdLds l = fwd_lds(dtype, p.g);
    if (l.total > HEAD_LDS_MAX) return unsupported("coarsehead_forward: the tile does not fit LDS");
    p.lda = l.lda; p.sw = l.sw; p.region0 = (int64_t)l.region0;
    GDR_HEAD_DT(coarsehead_forward_kernel, dim3((uint32_t)div_up(rows, (int64_t)HEAD_ROWS)), l.total, (hipStream_t)stream, p);
    return launch_status("coarsehead_forward_kernel");
}

int gdr_coarsehead_backward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, const void* b2, int32_t b2_dtype,
                            int64_t rows, int32_t C, int32_t K, int32_t sh_dim, const void* offset, const void* grad_offset, const void* grad_sh,
                            const void* grad_scaling, const void* grad_rotation, const void* grad_opacity, const void* grad_centers,
                            double half_cell, void* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(b1_dtype) || bad_dtype(b2_dtype)) return invalid_arg("coarsehead_backward: unknown dtype");
    if (rows < 0) return invalid_arg("coarsehead_backward: rows must be >= 0");
    if (bad_shape(C, K, sh_dim) || bad_rows_count(rows, K)) return unsupported(CH_ENVELOPE);
    if (!grad_x && !workspace) return invalid_arg("coarsehead_backward: no gradient asked for");
    if (rows && (!x || !packed || !b1 || !b2 || !offset)) return invalid_arg("coarsehead_backward: NULL argument");
    if (misaligned(x, 15) || misaligned(packed, 15) || misaligned(grad_x, 15) || misaligned(workspace, 255) || misaligned(b1, esize(b1_dtype) - 1) ||
        misaligned(b2, esize(b2_dtype) - 1) || misaligned(offset, 3) || misaligned(grad_offset, 3) || misaligned(grad_sh, 3) ||
        misaligned(grad_scaling, 3) || misaligned(grad_rotation, 3) || misaligned(grad_opacity, 3) || misaligned(grad_centers, 3))
        return unsupported("coarsehead_backward: x, grad_x and the packed buffer must start on 16 bytes, the workspace on 256");
    if (workspace && workspace_bytes < gdr_coarsehead_workspace_bytes(GDR_COARSEHEAD_WS_PARTIALS, dtype, rows, C, K, sh_dim))
        return workspace_too_small("coarsehead_backward: workspace smaller than gdr_coarsehead_workspace_bytes");
    BwdP p = {};
    p.x = x; p.packed = packed; p.b[0] = b1; p.b[1] = b2; p.b_dtype[0] = b1_dtype; p.b_dtype[1] = b2_dtype; p.offset = (const float*)offset;
    p.gout[0] = (const float*)grad_offset; p.gout[1] = (const float*)grad_sh; p.gout[2] = (const float*)grad_scaling;
    p.gout[3] = (const float*)grad_rotation; p.gout[4] = (const float*)grad_opacity; p.gcenters = (const float*)grad_centers;
    p.grad_x = grad_x; p.part = workspace; p.n = rows; p.half_cell = half_cell; p.g = geo_of(dtype, C, K, sh_dim);
    const BwdLds l = bwd_lds(dtype, p.g);
    if (l.total > HEAD_LDS_MAX) return unsupported("coarsehead_backward: the step does not fit LDS");
    p.step = l.step; p.lda = l.lda; p.ldz = l.ldz; p.ldt = l.ldt;
    const int slabs = slabs_of(rows);
    p.slab_rows = (int64_t)align_up((size_t)((rows + slabs - 1) / slabs), HEAD_ROWS);
    const int c16 = p.g.C16 / 16, ntiles = 2 * c16 * c16 + (p.g.O16 / 16) * c16;
    const int groups = workspace ? div_up(ntiles, 4 * HEAD_TPW) : 1;
    GDR_HEAD_DT(coarsehead_backward_kernel, dim3(slabs, groups), l.total, (hipStream_t)stream, p);
    return launch_status("coarsehead_backward_kernel");
}

int gdr_coarsehead_fold(const void* workspace, size_t workspace_bytes, int32_t dtype, int64_t rows, int32_t C, int32_t K, int32_t sh_dim,
                        void* grad_w1, int32_t grad_w1_dtype, void* grad_b1, int32_t grad_b1_dtype, void* grad_w2, int32_t grad_w2_dtype,
                        void* grad_b2, int32_t grad_b2_dtype, void* grad_w3, int32_t grad_w3_dtype, void* grad_b3, int32_t grad_b3_dtype,
                        void* stream) {
    FoldP p = {};                  // in the order of a partial set
    p.count = 6;
    void* const out[6] = {grad_w1, grad_w2, grad_w3, grad_b1, grad_b2, grad_b3};
    const int32_t dts[6] = {grad_w1_dtype, grad_w2_dtype, grad_w3_dtype, grad_b1_dtype, grad_b2_dtype, grad_b3_dtype};
    for (int k = 0; k < 6; ++k) { p.out[k] = out[k]; p.out_dtype[k] = dts[k]; }
    if (fold_bad_dtype(dtype, p)) return invalid_arg("coarsehead_fold: unknown dtype");
    if (rows < 0) return invalid_arg("coarsehead_fold: rows must be >= 0");
    if (bad_shape(C, K, sh_dim) || bad_rows_count(rows, K)) return unsupported(CH_ENVELOPE);
    const Geo g = geo_of(dtype, C, K, sh_dim);
    p.size[0] = p.size[1] = (int64_t)C * C; p.size[2] = (int64_t)g.KP * C; p.size[3] = p.size[4] = C; p.size[5] = g.KP;
    p.slabs = slabs_of(rows);
    return head_fold("coarsehead", workspace, workspace_bytes, gdr_coarsehead_workspace_bytes(GDR_COARSEHEAD_WS_PARTIALS, dtype, rows, C, K, sh_dim),
                     dtype, p, stream);
}

}  // extern "C"

// finehead.hip — the fine Gaussian head and the fine-set assembly (gfx950), forward and every gradient.  Public ABI:
// include/gdr.h gdr_finehead_*; the Python side is generativedensification_amd/finehead.py.
//
// 1. The head: the reference's GaussianModule / GaussianResModule `feat2attr` (lightning/point_decoder/autoencoder.py:
//    Linear(C, C), GELU, Linear(C, P), P = sh_dim + 1 + 3 + 4) on dense (rows, C) rows.  Restated (tests/finehead_ref.py holds
//    the f64 statement), rd = one rounding to the compute dtype:
//      z1 = rd(x W1^T + b1),  h = rd(gelu(z1)),  out = rd(h W2^T + b2)     gelu(z) = 0.5 z (1 + erf(z / sqrt 2)), evaluated in f32
//                                                                           (f64 for f32 rows) from the rounded z1; an f32
//                                                                           output of 16-bit rows is the sum, not rounded
//      backward: g = rd(grad_out);  dh = rd(g W2);  dz1 = rd(dh gelu'(z1)),  gelu'(z) = 0.5 (1 + erf(z / sqrt 2)) + z phi(z);
//        grad_x = rd(dz1 W1);  grad_W1 = dz1^T x, grad_b1 = column sums of dz1;  grad_W2 = g^T h, grad_b2 = column sums of g.
//    Structure (256 threads = 4 waves; D rows are channels, D columns data rows, as in coarsehead.hip):
//      pack: one launch rounds both weights to the compute dtype into one zero-padded buffer, [out][in] for the products of the
//        forward direction and [in][out] for those of the backward, padded to whole sum chunks so no product guards an index.
//      forward: a workgroup owns HEAD_ROWS = 64 consecutive rows, wave w the 16 rows of tile w.  The rows are staged in LDS, the
//        hidden row is left in LDS for the last layer and never leaves the workgroup.
//      backward: a workgroup owns a slab of rows and walks it `step` rows at a time (64, 32 or 16: what fits LDS).  Per step it
//        recomputes z1 and h, stages g, and runs dh -> dz1 -> grad_x.  x, h, dz1 and g are also left transposed
//        ([channel][row]) so that the row is the MFMA's sum index of the weight gradients: a wave keeps HEAD_TPW 16 x 16 tiles of
//        [grad_W1 | grad_W2] in registers over the whole slab and blockIdx.y selects which 4 HEAD_TPW tiles a workgroup owns
//        (every tile group recomputes the step: 5 groups at C = 256, P = 20); thread c the column sums of channel c.  One partial
//        set per slab; a second launch adds them, 16 segments of the slabs per element in slab order, then the 16 segment sums.
//        No atomics.
// 2. The assembly: lines 953-959 of the reference's Network.forward for a single-sample union.  The rows of every decoder level
//    (coord; attribute split into sh | opacity + shift | scaling + shift | rotation, converted to f32 before the add) followed by
//    the coarse Gaussians that were masked in but not selected.
//      scan (3 launches for both masks): rank_masked[i] = the number of masked rows before coarse row i (-1 where mask is 0) and
//        its inverse row_of_masked[m]; rank_rest[m] = the number of unselected rows before masked row m (-1 where selected) and
//        its inverse masked_of_rest[j].
//      assemble (1 launch): every thread owns 4 consecutive elements of one output and writes them with one 16-byte store;
//        survivor j reads masked row m = masked_of_rest[j] and coarse row row_of_masked[m], both compared with their row counts
//        before an address is formed.
//      backward (1 launch): a thread per element of every gradient wanted; a coarse row reads row rank_rest[rank_masked[i]] of the
//        upstream gradient or writes zero.
// What the head has in common with coarsehead.hip (the geometry, the tile product, the x-row staging, grad_x, the weight-gradient
// tile bookkeeping, the fold, the backward's LDS carve) is head_rows.h.
// Tile sizes, the step, the slab length and where the weights sit are unmeasured choices.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "mfma_rows.h"
#include "head_rows.h"

namespace gdr {
namespace {

constexpr int FH_MAX_SLABS = 256;
constexpr int FH_SLAB_MIN = GDR_FINEHEAD_SLAB_MIN;
constexpr int FH_CHUNK = GDR_FINEHEAD_SCAN_CHUNK;  // rows per workgroup of the scans
constexpr int FH_LEVELS = GDR_FINEHEAD_MAX_LEVELS;
static_assert(FH_CHUNK == 4 * HEAD_BLOCK, "a scan thread owns 4 rows");

// the shape and its padded sizes
struct Geo {
    int32_t C, sh, P;
    int32_t Cpad, Opad;      // C and P rounded up to whole sum chunks (32 elements of 16 bits, 16 of f32)
    int32_t C16, O16;        // ... to whole 16 x 16 tiles
};

Geo geo_of(int dtype, int C, int sh) {
    Geo g;
    const int kc = dtype == GDR_NORM_F32 ? 16 : 32;
    g.C = C; g.sh = sh; g.P = sh + 1 + 3 + 4;
    g.Cpad = round_up(C, kc); g.Opad = round_up(g.P, kc); g.C16 = round_up(C, 16); g.O16 = round_up(g.P, 16);
    return g;
}

// element offsets of the packed buffers.  forward: W1 [Cpad][Cpad], W2 [Opad][Cpad], both [out][in].
// backward: W1 as above, then W1t [Cpad][Cpad] and W2t [Cpad][Opad], both [in][out].
__host__ __device__ inline int64_t sq_of(const Geo& g) { return (int64_t)g.Cpad * g.Cpad; }
__host__ __device__ inline int64_t w2_of(const Geo& g) { return (int64_t)g.Opad * g.Cpad; }
__host__ __device__ inline int64_t packed_elems(const Geo& g, bool backward) { return backward ? 2 * sq_of(g) + w2_of(g) : sq_of(g) + w2_of(g); }

// elements of one partial set: grad_W1 (C, C), grad_W2 (P, C), grad_b1 (C), grad_b2 (P)
__host__ __device__ inline int64_t partial_elems(const Geo& g) { return (int64_t)g.C * g.C + (int64_t)g.P * g.C + g.C + g.P; }

// torch's default GELU and its derivative, in the accumulator's type
__device__ __forceinline__ float gelu_of(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ double gelu_of(double z) { return 0.5 * z * (1.0 + erf(z * 0.70710678118654752440)); }
__device__ __forceinline__ float gelu_slope(float z) {
    return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * (expf(-0.5f * z * z) * 0.39894228040143267794f);
}
__device__ __forceinline__ double gelu_slope(double z) {
    return 0.5 * (1.0 + erf(z * 0.70710678118654752440)) + z * (exp(-0.5 * z * z) * 0.39894228040143267794);
}

// ---- pack -------------------------------------------------------------------------------------------------------------------------
struct PackP {
    const void* w[2];
    int32_t w_dtype[2];
    void* packed;
    Geo g;
    int32_t backward;
    int64_t total;
};

template <int DT>
__global__ __launch_bounds__(HEAD_BLOCK) void finehead_pack_kernel(const PackP p) {
    int64_t i = (int64_t)blockIdx.x * HEAD_BLOCK + threadIdx.x;
    if (i >= p.total) return;
    const int64_t at = i, sq = sq_of(p.g);
    const int C = p.g.C, P = p.g.P, Cpad = p.g.Cpad, Opad = p.g.Opad;
    float v = 0.0f;
    if (i < sq) {                                   // W1 [out][in]
        const int r = (int)(i / Cpad), c = (int)(i % Cpad);
        if (r < C && c < C) v = load1(p.w[0], (int64_t)r * C + c, p.w_dtype[0]);
    } else if (!p.backward) {                       // W2 [out][in]
        i -= sq;
        const int r = (int)(i / Cpad), c = (int)(i % Cpad);
        if (r < P && c < C) v = load1(p.w[1], (int64_t)r * C + c, p.w_dtype[1]);
    } else if (i < 2 * sq) {                        // W1t [in][out]
        i -= sq;
        const int r = (int)(i / Cpad), c = (int)(i % Cpad);
        if (r < C && c < C) v = load1(p.w[0], (int64_t)c * C + r, p.w_dtype[0]);
    } else {                                        // W2t [in][out]
        i -= 2 * sq;
        const int r = (int)(i / Opad), c = (int)(i % Opad);
        if (r < C && c < P) v = load1(p.w[1], (int64_t)c * C + r, p.w_dtype[1]);
    }
    ((typename El<DT>::type*)p.packed)[at] = down<DT>(v);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
struct FwdP {
    const void* x;             // (rows, C) dense
    const void* packed;
    const void* b[2];
    int32_t b_dtype[2];
    void* out;                 // (rows, P) dense of out_dtype
    int32_t out_dtype;
    int64_t n;
    Geo g;
    int32_t lda;               // LDS row stride (elements)
};

template <int DT>
__global__ __launch_bounds__(HEAD_BLOCK) void finehead_forward_kernel(const FwdP p) {
    using E = typename El<DT>::type;
    using T = Sc<DT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char fh_lds[];
    E* bufX = (E*)fh_lds;                              // x
    E* bufH = bufX + HEAD_ROWS * p.lda;                  // h
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const Geo& g = p.g;
    const int lda = p.lda, Cpad = g.Cpad;
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;
    const E* X = (const E*)p.x;
    const E* W1 = (const E*)p.packed;
    const E* W2 = W1 + sq_of(g);

    stage_rows<DT>(X, row0, p.n, HEAD_ROWS, g.C, Cpad, bufX, lda, false, nullptr, 0, tid);
    __syncthreads();
    const int r = 16 * wave + l16;                     // this lane's row of the tile
    for (int jt = 0; jt < Cpad / 16; ++jt) {
        typename El<DT>::acc acc = {0, 0, 0, 0};
        tile_mma<DT>(W1 + (int64_t)16 * jt * Cpad, Cpad, bufX + 16 * wave * lda, lda, Cpad, l16, quad, acc);
        E h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const E z1 = down<DT>((float)((T)acc[e] + bias_at<DT>(p.b[0], p.b_dtype[0], 16 * jt + 4 * quad + e, g.C)));
            h[e] = down<DT>((float)gelu_of((T)up<DT>(z1)));
        }
        store4<DT>(bufH + r * lda + 16 * jt + 4 * quad, h);
    }
    __syncthreads();
    // the last layer: D rows are the P columns
    const int64_t row = row0 + r;
    for (int jt = 0; jt < g.O16 / 16; ++jt) {
        typename El<DT>::acc v2 = {0, 0, 0, 0};
        tile_mma<DT>(W2 + (int64_t)16 * jt * Cpad, Cpad, bufH + 16 * wave * lda, lda, Cpad, l16, quad, v2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 16 * jt + 4 * quad + e;
            if (row >= p.n || j >= g.P) continue;
            const T v = (T)v2[e] + bias_at<DT>(p.b[1], p.b_dtype[1], j, g.P);
            store1(p.out, row * g.P + j, p.out_dtype, (float)v);
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
struct BwdP {
    const void* x;
    const void* packed;        // the backward's packed buffer
    const void* b1;
    int32_t b1_dtype;
    const void* gout;          // (rows, P) dense of gout_dtype, or NULL (zeros)
    int32_t gout_dtype;
    void* grad_x;              // (rows, C) or NULL
    void* part;                // one partial set per slab (f32; f64 for f32 rows), or NULL
    int64_t n, slab_rows;
    Geo g;
    int32_t step, lda, ldz, ldt;      // rows per step and the LDS strides (elements)
};

template <int DT>
__global__ __launch_bounds__(HEAD_BLOCK) void finehead_backward_kernel(const BwdP p) {
    using E = typename El<DT>::type;
    using T = Sc<DT>;
    using Acc = typename El<DT>::acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char fh_lds[];
    const Geo& g = p.g;
    const int C = g.C, Cpad = g.Cpad, Opad = g.Opad, P = g.P, step = p.step, lda = p.lda, ldz = p.ldz, ldt = p.ldt, rt = step / 16;
    E* R0 = (E*)fh_lds;                  // x rows, then dz1 rows
    E* R1 = R0 + step * lda;             // z1 rows
    E* RZ = R1 + step * lda;             // g rows
    E* xT = RZ + step * ldz;             // [channel][row] from here on
    E* hT = xT + Cpad * ldt;
    E* z1T = hT + Cpad * ldt;            // dz1
    E* gT = z1T + Cpad * ldt;            // [Opad][ldt]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const E* X = (const E*)p.x;
    const E* W1 = (const E*)p.packed;
    const E* W1t = W1 + sq_of(g);
    const E* W2t = W1t + sq_of(g);
    const bool sums = p.part != nullptr;
    const int64_t r_begin = (int64_t)blockIdx.x * p.slab_rows;
    const int64_t r_end = r_begin + p.slab_rows < p.n ? r_begin + p.slab_rows : p.n;

    // the weight-gradient tiles of this wave: tile t of [grad_W1 | grad_W2], 16 x 16 each, (out tile, in tile) row-major
    const int c16 = g.C16 / 16, n1 = c16 * c16;
    WgTiles<DT> wg = {};
    wg.n = 2; wg.ntiles = n1 + (g.O16 / 16) * c16; wg.C = C; wg.c16 = c16;
    wg.s[0] = {z1T, xT, 0, C, 0};
    wg.s[1] = {gT, hT, n1, P, (int64_t)C * C};
    const int t_first = (blockIdx.y * 4 + wave) * HEAD_TPW;
    Acc accW[HEAD_TPW];
#pragma unroll
    for (int i = 0; i < HEAD_TPW; ++i) accW[i] = Acc{0, 0, 0, 0};
    T db1 = 0, db2 = 0;

    // the pad columns of g are never written again
    for (int i = tid; i < step * (Opad - P); i += HEAD_BLOCK) {
        const int r = i / (Opad - P), j = P + i - r * (Opad - P);
        RZ[r * ldz + j] = down<DT>(0.0f);
        gT[j * ldt + r] = down<DT>(0.0f);
    }

    for (int64_t r0 = r_begin; r0 < r_end; r0 += step) {
        stage_rows<DT>(X, r0, r_end, step, C, Cpad, R0, lda, sums, xT, ldt, tid);
        // g -> RZ and gT
        {
            const int64_t left = r_end - r0;
            const int count = (int)(left < step ? left : step) * P;
            const int64_t base = r0 * P;
            for (int i = tid; i < step * P; i += HEAD_BLOCK) {
                const int r = i / P, j = i - r * P;
                const E e = down<DT>(i < count && p.gout ? load1(p.gout, base + i, p.gout_dtype) : 0.0f);
                RZ[r * ldz + j] = e;
                gT[j * ldt + r] = e;
            }
        }
        __syncthreads();
        // z1 -> R1;  h -> hT
        for (int pr = wave; pr < (Cpad / 16) * rt; pr += 4) {
            const int ti = pr % rt, jt = pr / rt, r = 16 * ti + l16, ch = 16 * jt + 4 * quad;
            Acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W1 + (int64_t)16 * jt * Cpad, Cpad, R0 + 16 * ti * lda, lda, Cpad, l16, quad, acc);
            E z[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                z[e] = down<DT>((float)((T)acc[e] + bias_at<DT>(p.b1, p.b1_dtype, ch + e, C)));
                if (sums) hT[(ch + e) * ldt + r] = down<DT>((float)gelu_of((T)up<DT>(z[e])));
            }
            store4<DT>(R1 + r * lda + ch, z);
        }
        __syncthreads();
        // dz1 = rd(rd(g W2) gelu'(z1)) -> R0 and z1T
        for (int pr = wave; pr < (Cpad / 16) * rt; pr += 4) {
            const int ti = pr % rt, jt = pr / rt, r = 16 * ti + l16, ch = 16 * jt + 4 * quad;
            Acc acc = {0, 0, 0, 0};
            tile_mma<DT>(W2t + (int64_t)16 * jt * Opad, Opad, RZ + 16 * ti * ldz, ldz, Opad, l16, quad, acc);
            E d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const T dh = (T)up<DT>(down<DT>((float)acc[e]));
                d[e] = down<DT>((float)(dh * gelu_slope((T)up<DT>(R1[r * lda + ch + e]))));
                if (sums) z1T[(ch + e) * ldt + r] = d[e];
            }
            store4<DT>(R0 + r * lda + ch, d);
        }
        __syncthreads();
        // grad_x = dz1 W1
        if (p.grad_x && blockIdx.y == 0) grad_x_tiles<DT>(W1t, R0, lda, p.grad_x, r0, r_end, rt, C, g.C16, Cpad, wave, l16, quad);
        if (sums) {
            wgrad_step<DT>(wg, t_first, ldt, step, l16, quad, accW);
            if (blockIdx.y == 0) {
                if (tid < C)
                    for (int r = 0; r < step; ++r) db1 += (T)up<DT>(z1T[tid * ldt + r]);
                if (tid < P)
                    for (int r = 0; r < step; ++r) db2 += (T)up<DT>(gT[tid * ldt + r]);
            }
        }
        __syncthreads();
    }
    if (!sums) return;
    T* part = (T*)p.part + (int64_t)blockIdx.x * partial_elems(g);
    wgrad_store<DT>(wg, t_first, part, l16, quad, accW);
    if (blockIdx.y == 0) {
        T* pb = part + (int64_t)C * C + (int64_t)P * C;
        if (tid < C) pb[tid] = db1;
        if (tid < P) pb[C + tid] = db2;
    }
}

// ---- the scan of the two masks ----------------------------------------------------------------------------------------------------
// Chunks 0 .. chunksA - 1 cover the coarse rows (flag = mask), the chunksB after them the masked rows (flag = !selected).
struct ScanP {
    const uint8_t* mask;
    const uint8_t* selected;
    int64_t Nc, n_masked;
    int32_t chunksA, chunksB;
    int32_t* counts;           // per chunk: its flags, then (in place) the flags before it on its side
    int32_t* rank_masked;      // (Nc)
    int32_t* row_of_masked;    // (n_masked)
    int32_t* rank_rest;        // (n_masked)
    int32_t* masked_of_rest;   // (n_masked)
    int64_t* count;            // [0] masked rows, [1] unselected rows
};

// the 4 flags of this thread's rows of chunk `b`, as bits; row0: its first row
__device__ __forceinline__ int scan_flags(const ScanP& p, int b, int tid, int64_t& row0) {
    const bool sideA = b < p.chunksA;
    const int64_t n = sideA ? p.Nc : p.n_masked;
    const uint8_t* src = sideA ? p.mask : p.selected;
    row0 = (int64_t)(sideA ? b : b - p.chunksA) * FH_CHUNK + 4 * tid;
    int bits = 0;
    for (int k = 0; k < 4; ++k)
        if (row0 + k < n && ((src[row0 + k] != 0) == sideA)) bits |= 1 << k;
    return bits;
}

// the number of flags of the threads before this one, and (total) of the whole block
__device__ __forceinline__ int block_exclusive(int mine, int tid, int* sScan, int& total) {
    sScan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < HEAD_BLOCK; d *= 2) {
        const int add = tid >= d ? sScan[tid - d] : 0;
        __syncthreads();
        sScan[tid] += add;
        __syncthreads();
    }
    total = sScan[HEAD_BLOCK - 1];
    return sScan[tid] - mine;
}

__global__ __launch_bounds__(HEAD_BLOCK) void finehead_scan_count_kernel(const ScanP p) {
    __shared__ int sScan[HEAD_BLOCK];
    int64_t row0;
    int total;
    block_exclusive(__popc(scan_flags(p, blockIdx.x, threadIdx.x, row0)), threadIdx.x, sScan, total);
    if (threadIdx.x == 0) p.counts[blockIdx.x] = total;
}

// one block: the exclusive scan of each side's chunk counts, in place, and the two totals
__global__ __launch_bounds__(HEAD_BLOCK) void finehead_scan_bases_kernel(const ScanP p) {
    __shared__ int sScan[HEAD_BLOCK];
    const int tid = threadIdx.x;
    for (int side = 0; side < 2; ++side) {
        int32_t* c = p.counts + (side ? p.chunksA : 0);
        const int n = side ? p.chunksB : p.chunksA, per = (n + HEAD_BLOCK - 1) / HEAD_BLOCK;
        const int b0 = tid * per < n ? tid * per : n, b1 = b0 + per < n ? b0 + per : n;
        int mine = 0, total;
        for (int b = b0; b < b1; ++b) mine += c[b];
        int before = block_exclusive(mine, tid, sScan, total);
        for (int b = b0; b < b1; ++b) {
            const int v = c[b];
            c[b] = before;
            before += v;
        }
        if (tid == 0) p.count[side] = total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(HEAD_BLOCK) void finehead_scan_write_kernel(const ScanP p) {
    __shared__ int sScan[HEAD_BLOCK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool sideA = b < p.chunksA;
    int64_t row0;
    int total;
    const int bits = scan_flags(p, b, tid, row0);
    int64_t at = (int64_t)p.counts[b] + block_exclusive(__popc(bits), tid, sScan, total);
    const int64_t n = sideA ? p.Nc : p.n_masked;
    int32_t* rank = sideA ? p.rank_masked : p.rank_rest;
    int32_t* inverse = sideA ? p.row_of_masked : p.masked_of_rest;
    for (int k = 0; k < 4; ++k) {
        if (row0 + k >= n) break;
        if (bits >> k & 1) {
            rank[row0 + k] = (int32_t)at;
            if (at < p.n_masked) inverse[at] = (int32_t)(row0 + k);      // both inverses hold n_masked entries
            ++at;
        } else {
            rank[row0 + k] = -1;
        }
    }
}

// ---- the assembly -------------------------------------------------------------------------------------------------------------------
// outputs in the order centers (3), shs (sh), opacity (1), scaling (3), rotation (4)
struct AsmP {
    int32_t n_levels, attr_dtype, sh, P, vw;
    const float* coord[FH_LEVELS];
    const void* attr[FH_LEVELS];
    int64_t start[FH_LEVELS + 1];     // the first output row of each level; start[n_levels] = L
    const float* coarse[5];           // centers, (unused), opacity, scaling, rotation: (Nc, w)
    const float* shs_fine;            // (n_masked, sh)
    const int32_t* row_of_masked;
    const int32_t* masked_of_rest;
    int64_t Nc, n_masked, T;          // T = L + the survivor rows written
    float opacity_shift, scaling_shift;
    float* out[5];
    int64_t groups_end[5];            // running ends of the outputs' store groups
};

__device__ __forceinline__ int width_of(int k, int sh) { return k == 1 ? sh : (k == 2 ? 1 : (k == 4 ? 4 : 3)); }
__device__ __forceinline__ int column_of(int k, int sh) { return k == 1 ? 0 : (k == 2 ? sh : (k == 3 ? sh + 1 : sh + 4)); }      // in the attribute

__device__ __forceinline__ float assembled(const AsmP& p, int k, int w, int64_t e) {
    const int64_t row = e / w, L = p.start[p.n_levels];
    const int col = (int)(e - row * w);
    if (row < L) {
        int l = 0;
        while (row >= p.start[l + 1]) ++l;
        const int64_t rr = row - p.start[l];
        if (k == 0) return p.coord[l][rr * 3 + col];
        const float v = load1(p.attr[l], rr * p.P + column_of(k, p.sh) + col, p.attr_dtype);
        return k == 2 ? v + p.opacity_shift : (k == 3 ? v + p.scaling_shift : v);
    }
    const int64_t m = p.masked_of_rest[row - L];
    if (m < 0 || m >= p.n_masked) return 0.0f;        // (nothing maps here: a survivor count larger than the masks')
    if (k == 1) return p.shs_fine[m * p.sh + col];
    const int64_t i = p.row_of_masked[m];
    if (i < 0 || i >= p.Nc) return 0.0f;
    return p.coarse[k][i * w + col];
}

__global__ __launch_bounds__(HEAD_BLOCK) void finehead_assemble_kernel(const AsmP p) {
    const int64_t stride = (int64_t)gridDim.x * HEAD_BLOCK;
    for (int64_t gi = (int64_t)blockIdx.x * HEAD_BLOCK + threadIdx.x; gi < p.groups_end[4]; gi += stride) {
        int k = 0;
        while (gi >= p.groups_end[k]) ++k;
        const int w = width_of(k, p.sh);
        const int64_t e0 = (gi - (k ? p.groups_end[k - 1] : 0)) * p.vw, total = p.T * w;
        if (p.vw == 4 && e0 + 4 <= total) {
            *reinterpret_cast<float4*>(p.out[k] + e0) =
                make_float4(assembled(p, k, w, e0), assembled(p, k, w, e0 + 1), assembled(p, k, w, e0 + 2), assembled(p, k, w, e0 + 3));
        } else {
            for (int64_t e = e0; e < e0 + p.vw && e < total; ++e) p.out[k][e] = assembled(p, k, w, e);
        }
    }
}

struct AsmBwdP {
    int32_t n_levels, attr_dtype, sh, P;
    float* gcoord[FH_LEVELS];         // (n_l, 3) or NULL
    void* gattr[FH_LEVELS];           // (n_l, P) of attr_dtype or NULL
    int64_t start[FH_LEVELS + 1];
    const float* g[5];                // upstream: centers, shs, opacity, scaling, rotation, each (T, w) or NULL (zeros)
    float* gcoarse[5];                // centers, (unused), opacity, scaling, rotation: (Nc, w) or NULL
    float* gshs_fine;                 // (n_masked, sh) or NULL
    const int32_t* rank_masked;
    const int32_t* rank_rest;
    int64_t Nc, n_masked, n_rest;
    int64_t ends[7];                  // running ends of: level coords, level attributes, the four coarse tensors, shs_fine
};

// the upstream row of masked row m, or -1
__device__ __forceinline__ int64_t survivor_of(const AsmBwdP& p, int64_t m) {
    if (m < 0 || m >= p.n_masked) return -1;
    const int64_t j = p.rank_rest[m];
    return j >= 0 && j < p.n_rest ? p.start[p.n_levels] + j : -1;
}

__global__ __launch_bounds__(HEAD_BLOCK) void finehead_assemble_backward_kernel(const AsmBwdP p) {
    const int64_t stride = (int64_t)gridDim.x * HEAD_BLOCK;
    for (int64_t t = (int64_t)blockIdx.x * HEAD_BLOCK + threadIdx.x; t < p.ends[6]; t += stride) {
        int s = 0;
        while (t >= p.ends[s]) ++s;
        const int64_t e = t - (s ? p.ends[s - 1] : 0);
        if (s < 2) {                                  // a level's coord or attribute
            const int w = s ? p.P : 3;
            const int64_t row = e / w;
            const int c = (int)(e - row * w);
            int l = 0;
            while (row >= p.start[l + 1]) ++l;
            const int64_t rr = row - p.start[l];
            if (s == 0) {
                if (p.gcoord[l]) p.gcoord[l][rr * 3 + c] = p.g[0] ? p.g[0][row * 3 + c] : 0.0f;
            } else if (p.gattr[l]) {
                const int k = c < p.sh ? 1 : (c == p.sh ? 2 : (c < p.sh + 4 ? 3 : 4));
                const int wk = width_of(k, p.sh);
                store1(p.gattr[l], rr * p.P + c, p.attr_dtype, p.g[k] ? p.g[k][row * wk + c - column_of(k, p.sh)] : 0.0f);
            }
        } else if (s < 6) {                           // a coarse tensor
            const int k = s == 2 ? 0 : s - 1;
            if (!p.gcoarse[k]) continue;
            const int w = width_of(k, p.sh);
            const int64_t i = e / w, src = survivor_of(p, p.rank_masked[i]);
            p.gcoarse[k][e] = src >= 0 && p.g[k] ? p.g[k][src * w + (e - i * w)] : 0.0f;
        } else if (p.gshs_fine) {
            const int64_t m = e / p.sh, src = survivor_of(p, m);
            p.gshs_fine[e] = src >= 0 && p.g[1] ? p.g[1][src * p.sh + (e - m * p.sh)] : 0.0f;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
bool bad_sh(int32_t sh) { return sh != 3 && sh != 12 && sh != 27 && sh != 48; }
bool bad_shape(int32_t C, int32_t sh) { return C < 8 || C > GDR_FINEHEAD_MAX_C || C % 8 || bad_sh(sh); }
bool bad_rows_count(int64_t rows) { return rows > (INT64_C(1) << 31) - 1; }

const char* const FH_ENVELOPE = "finehead: C must be a multiple of 8 in 8..GDR_FINEHEAD_MAX_C, sh_dim one of 3, 12, 27, 48 and rows below 2^31";

int slabs_of(int64_t n) { return gdr::slabs_of(n, FH_SLAB_MIN, FH_MAX_SLABS); }

struct FwdLds { int lda; size_t total; };
FwdLds fwd_lds(int dtype, const Geo& g) {
    FwdLds l;
    l.lda = g.Cpad + (dtype == GDR_NORM_F32 ? 4 : 8);
    l.total = (size_t)2 * HEAD_ROWS * l.lda * esize(dtype);
    return l;
}

// the backward's steps: xT, hT and z1T are its transposed Cpad-channel buffers
BwdLds bwd_lds(int dtype, const Geo& g) { return bwd_lds(dtype, g.Cpad, g.Opad, 3); }

int chunks_of(int64_t n) { return (int)((n + FH_CHUNK - 1) / FH_CHUNK); }

// the grid of an elementwise kernel that strides: enough blocks for `items`, 4096 at most
dim3 strided_grid(int64_t items) {
    const int64_t blocks = (items + HEAD_BLOCK - 1) / HEAD_BLOCK;
    return dim3((uint32_t)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks)));
}

// the levels' row counts -> running first rows; false: a negative count or a total of 2^31 or more
bool level_starts(int32_t n_levels, const int64_t* rows, int64_t extra, int64_t* start) {
    start[0] = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (rows[l] < 0 || bad_rows_count(rows[l])) return false;
        start[l + 1] = start[l] + rows[l];
    }
    return !bad_rows_count(start[n_levels] + extra);
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_finehead_workspace_bytes(int32_t what, int32_t dtype, int64_t rows, int32_t C, int32_t sh_dim) {
    if (bad_dtype(dtype)) { invalid_arg("finehead_workspace_bytes: unknown dtype"); return 0; }
    if (rows < 0) { invalid_arg("finehead_workspace_bytes: rows must be >= 0"); return 0; }
    if (bad_shape(C, sh_dim) || bad_rows_count(rows)) { unsupported(FH_ENVELOPE); return 0; }
    const Geo g = geo_of(dtype, C, sh_dim);
    switch (what) {
        case GDR_FINEHEAD_WS_PACKED_FORWARD: return align_up((size_t)packed_elems(g, false) * esize(dtype));
        case GDR_FINEHEAD_WS_PACKED_BACKWARD: return align_up((size_t)packed_elems(g, true) * esize(dtype));
        case GDR_FINEHEAD_WS_PARTIALS:
            return align_up((size_t)slabs_of(rows) * partial_elems(g) * (dtype == GDR_NORM_F32 ? sizeof(double) : sizeof(float)));
    }
    invalid_arg("finehead_workspace_bytes: unknown workspace kind");
    return 0;
}

int32_t gdr_finehead_backward_step(int32_t dtype, int32_t C, int32_t sh_dim) {
    if (bad_dtype(dtype)) { invalid_arg("finehead_backward_step: unknown dtype"); return 0; }
    if (bad_shape(C, sh_dim)) { unsupported(FH_ENVELOPE); return 0; }
    return bwd_lds(dtype, geo_of(dtype, C, sh_dim)).step;
}

int gdr_finehead_pack(const void* w1, int32_t w1_dtype, const void* w2, int32_t w2_dtype, int32_t C, int32_t sh_dim, int32_t backward,
                      void* packed, int32_t dtype, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(w1_dtype) || bad_dtype(w2_dtype)) return invalid_arg("finehead_pack: unknown dtype");
    if (bad_shape(C, sh_dim)) return unsupported(FH_ENVELOPE);
    if (!w1 || !w2 || !packed) return invalid_arg("finehead_pack: NULL argument");
    if (misaligned(w1, esize(w1_dtype) - 1) || misaligned(w2, esize(w2_dtype) - 1) || misaligned(packed, 15))
        return unsupported("finehead_pack: a weight must be aligned to its element and the packed buffer to 16 bytes");
    PackP p = {};
    p.w[0] = w1; p.w[1] = w2; p.w_dtype[0] = w1_dtype; p.w_dtype[1] = w2_dtype;
    p.packed = packed; p.g = geo_of(dtype, C, sh_dim); p.backward = backward ? 1 : 0; p.total = packed_elems(p.g, backward != 0);
    const dim3 grid((uint32_t)div_up(p.total, (int64_t)HEAD_BLOCK));
    if (dtype == GDR_NORM_F16) hipLaunchKernelGGL(finehead_pack_kernel<GDR_NORM_F16>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    else if (dtype == GDR_NORM_BF16) hipLaunchKernelGGL(finehead_pack_kernel<GDR_NORM_BF16>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(finehead_pack_kernel<GDR_NORM_F32>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("finehead_pack_kernel");
}

int gdr_finehead_forward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, const void* b2, int32_t b2_dtype,
                         int64_t rows, int32_t C, int32_t sh_dim, void* out, int32_t out_dtype, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(b1_dtype) || bad_dtype(b2_dtype)) return invalid_arg("finehead_forward: unknown dtype");
    if (out_dtype != dtype && out_dtype != GDR_NORM_F32) return invalid_arg("finehead_forward: out_dtype must be the compute dtype or f32");
    if (rows < 0) return invalid_arg("finehead_forward: rows must be >= 0");
    if (bad_shape(C, sh_dim) || bad_rows_count(rows)) return unsupported(FH_ENVELOPE);
    if (rows == 0) return GDR_OK;
    if (!x || !packed || !b1 || !b2 || !out) return invalid_arg("finehead_forward: NULL argument");
    if (misaligned(x, 15) || misaligned(packed, 15) || misaligned(b1, esize(b1_dtype) - 1) || misaligned(b2, esize(b2_dtype) - 1) ||
        misaligned(out, esize(out_dtype) - 1))
        return unsupported("finehead_forward: x and the packed buffer must start on 16 bytes, everything else on its element");
    FwdP p = {};
    p.x = x; p.packed = packed; p.b[0] = b1; p.b[1] = b2; p.b_dtype[0] = b1_dtype; p.b_dtype[1] = b2_dtype;
    p.out = out; p.out_dtype = out_dtype; p.n = rows; p.g = geo_of(dtype, C, sh_dim);
    const FwdLds l = fwd_lds(dtype, p.g);
    if (l.total > HEAD_LDS_MAX) return unsupported("finehead_forward: the tile does not fit LDS");
    p.lda = l.lda;
    GDR_HEAD_DT(finehead_forward_kernel, dim3((uint32_t)div_up(rows, (int64_t)HEAD_ROWS)), l.total, (hipStream_t)stream, p);
    return launch_status("finehead_forward_kernel");
}

int gdr_finehead_backward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, int64_t rows, int32_t C,
                          int32_t sh_dim, const void* grad_out, int32_t grad_out_dtype, void* grad_x, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (bad_dtype(dtype) || bad_dtype(b1_dtype) || (grad_out && bad_dtype(grad_out_dtype))) return invalid_arg("finehead_backward: unknown dtype");
    if (rows < 0) return invalid_arg("finehead_backward: rows must be >= 0");
    if (bad_shape(C, sh_dim) || bad_rows_count(rows)) return unsupported(FH_ENVELOPE);
    if (!grad_x && !workspace) return invalid_arg("finehead_backward: no gradient asked for");
    if (rows && (!x || !packed || !b1)) return invalid_arg("finehead_backward: NULL argument");
    if (misaligned(x, 15) || misaligned(packed, 15) || misaligned(grad_x, 15) || misaligned(workspace, 255) || misaligned(b1, esize(b1_dtype) - 1) ||
        (grad_out && misaligned(grad_out, esize(grad_out_dtype) - 1)))
        return unsupported("finehead_backward: x, grad_x and the packed buffer must start on 16 bytes, the workspace on 256");
    if (workspace && workspace_bytes < gdr_finehead_workspace_bytes(GDR_FINEHEAD_WS_PARTIALS, dtype, rows, C, sh_dim))
        return workspace_too_small("finehead_backward: workspace smaller than gdr_finehead_workspace_bytes");
    BwdP p = {};
    p.x = x; p.packed = packed; p.b1 = b1; p.b1_dtype = b1_dtype; p.gout = grad_out; p.gout_dtype = grad_out ? grad_out_dtype : dtype;
    p.grad_x = grad_x; p.part = workspace; p.n = rows; p.g = geo_of(dtype, C, sh_dim);
    const BwdLds l = bwd_lds(dtype, p.g);
    if (l.total > HEAD_LDS_MAX) return unsupported("finehead_backward: the step does not fit LDS");
    p.step = l.step; p.lda = l.lda; p.ldz = l.ldz; p.ldt = l.ldt;
    const int slabs = slabs_of(rows);
    p.slab_rows = (int64_t)align_up((size_t)((rows + slabs - 1) / slabs), HEAD_ROWS);
    const int c16 = p.g.C16 / 16, ntiles = c16 * c16 + (p.g.O16 / 16) * c16;
    const int groups = workspace ? div_up(ntiles, 4 * HEAD_TPW) : 1;
    GDR_HEAD_DT(finehead_backward_kernel, dim3(slabs, groups), l.total, (hipStream_t)stream, p);
    return launch_status("finehead_backward_kernel");
}

int gdr_finehead_fold(const void* workspace, size_t workspace_bytes, int32_t dtype, int64_t rows, int32_t C, int32_t sh_dim, void* grad_w1,
                      int32_t grad_w1_dtype, void* grad_b1, int32_t grad_b1_dtype, void* grad_w2, int32_t grad_w2_dtype, void* grad_b2,
                      int32_t grad_b2_dtype, void* stream) {
    FoldP p = {};                  // in the order of a partial set
    p.count = 4;
    void* const out[4] = {grad_w1, grad_w2, grad_b1, grad_b2};
    const int32_t dts[4] = {grad_w1_dtype, grad_w2_dtype, grad_b1_dtype, grad_b2_dtype};
    for (int k = 0; k < 4; ++k) { p.out[k] = out[k]; p.out_dtype[k] = dts[k]; }
    if (fold_bad_dtype(dtype, p)) return invalid_arg("finehead_fold: unknown dtype");
    if (rows < 0) return invalid_arg("finehead_fold: rows must be >= 0");
    if (bad_shape(C, sh_dim) || bad_rows_count(rows)) return unsupported(FH_ENVELOPE);
    const Geo g = geo_of(dtype, C, sh_dim);
    p.size[0] = (int64_t)C * C; p.size[1] = (int64_t)g.P * C; p.size[2] = C; p.size[3] = g.P;
    p.slabs = slabs_of(rows);
    return head_fold("finehead", workspace, workspace_bytes, gdr_finehead_workspace_bytes(GDR_FINEHEAD_WS_PARTIALS, dtype, rows, C, sh_dim), dtype, p,
                     stream);
}

size_t gdr_finehead_scan_bytes(int64_t Nc, int64_t n_masked) {
    if (Nc < 0 || n_masked < 0) { invalid_arg("finehead_scan_bytes: row counts must be >= 0"); return 0; }
    if (bad_rows_count(Nc) || bad_rows_count(n_masked)) { unsupported("finehead_scan_bytes: row counts must be below 2^31"); return 0; }
    return align_up((size_t)(chunks_of(Nc) + chunks_of(n_masked)) * sizeof(int32_t)) + 256;      // (never 0 for valid arguments)
}

int gdr_finehead_scan(const uint8_t* mask, int64_t Nc, const uint8_t* selected, int64_t n_masked, void* workspace, size_t workspace_bytes,
                      int32_t* rank_masked, int32_t* row_of_masked, int32_t* rank_rest, int32_t* masked_of_rest, int64_t* count, void* stream) {
    if (Nc < 0 || n_masked < 0) return invalid_arg("finehead_scan: row counts must be >= 0");
    if (bad_rows_count(Nc) || bad_rows_count(n_masked)) return unsupported("finehead_scan: row counts must be below 2^31");
    if (!count || !workspace || (Nc && (!mask || !rank_masked)) || (n_masked && (!selected || !row_of_masked || !rank_rest || !masked_of_rest)))
        return invalid_arg("finehead_scan: NULL argument");
    if (misaligned(rank_masked, 3) || misaligned(row_of_masked, 3) || misaligned(rank_rest, 3) || misaligned(masked_of_rest, 3) ||
        misaligned(count, 7) || misaligned(workspace, 255))
        return invalid_arg("finehead_scan: unaligned buffer");
    if (workspace_bytes < gdr_finehead_scan_bytes(Nc, n_masked) - 256) return workspace_too_small("finehead_scan: workspace smaller than gdr_finehead_scan_bytes");
    ScanP p = {};
    p.mask = mask; p.selected = selected; p.Nc = Nc; p.n_masked = n_masked; p.chunksA = chunks_of(Nc); p.chunksB = chunks_of(n_masked);
    p.counts = (int32_t*)workspace; p.rank_masked = rank_masked; p.row_of_masked = row_of_masked; p.rank_rest = rank_rest;
    p.masked_of_rest = masked_of_rest; p.count = count;
    const int chunks = p.chunksA + p.chunksB;
    hipStream_t st = (hipStream_t)stream;
    if (chunks) hipLaunchKernelGGL(finehead_scan_count_kernel, dim3(chunks), dim3(HEAD_BLOCK), 0, st, p);
    hipLaunchKernelGGL(finehead_scan_bases_kernel, dim3(1), dim3(HEAD_BLOCK), 0, st, p);
    if (chunks) hipLaunchKernelGGL(finehead_scan_write_kernel, dim3(chunks), dim3(HEAD_BLOCK), 0, st, p);
    return launch_status("finehead scan kernels");
}

int gdr_finehead_assemble(int32_t n_levels, const void* const* coord, const void* const* attr, const int64_t* level_rows, int32_t attr_dtype,
                          int32_t sh_dim, const void* centers_coarse, const void* opacity_coarse, const void* scaling_coarse,
                          const void* rotation_coarse, int64_t Nc, const void* shs_fine, int64_t n_masked, const int32_t* row_of_masked,
                          const int32_t* masked_of_rest, int64_t n_rest, double opacity_shift, double scaling_shift, void* centers, void* shs,
                          void* opacity, void* scaling, void* rotation, void* stream) {
    if (n_levels < 0 || n_levels > FH_LEVELS) return unsupported("finehead_assemble: at most GDR_FINEHEAD_MAX_LEVELS levels");
    if (bad_dtype(attr_dtype)) return invalid_arg("finehead_assemble: unknown dtype");
    if (bad_sh(sh_dim)) return unsupported("finehead_assemble: sh_dim must be one of 3, 12, 27, 48");
    if (Nc < 0 || n_masked < 0 || n_rest < 0) return invalid_arg("finehead_assemble: row counts must be >= 0");
    if (bad_rows_count(Nc) || bad_rows_count(n_masked) || n_rest > n_masked) return unsupported("finehead_assemble: row counts must be below 2^31, n_rest at most n_masked");
    if (n_levels && (!coord || !attr || !level_rows)) return invalid_arg("finehead_assemble: NULL argument");
    AsmP p = {};
    if (!level_starts(n_levels, level_rows, n_rest, p.start)) return unsupported("finehead_assemble: level rows must be >= 0 and the output below 2^31 rows");
    p.T = p.start[n_levels] + n_rest;
    if (p.T == 0) return GDR_OK;
    void* out[5] = {centers, shs, opacity, scaling, rotation};
    const void* coarse[5] = {centers_coarse, nullptr, opacity_coarse, scaling_coarse, rotation_coarse};
    for (int k = 0; k < 5; ++k)
        if (!out[k] || misaligned(out[k], 3)) return invalid_arg("finehead_assemble: an output is NULL or not aligned to its element");
    for (int l = 0; l < n_levels; ++l) {
        if (level_rows[l] && (!coord[l] || !attr[l])) return invalid_arg("finehead_assemble: NULL level");
        if (misaligned(coord[l], 3) || misaligned(attr[l], esize(attr_dtype) - 1)) return invalid_arg("finehead_assemble: a level is not aligned to its element");
        p.coord[l] = (const float*)coord[l]; p.attr[l] = attr[l];
    }
    if (n_rest) {
        if (!row_of_masked || !masked_of_rest || !shs_fine) return invalid_arg("finehead_assemble: NULL argument");
        for (int k = 0; k < 5; ++k)
            if (k != 1 && (!coarse[k] || misaligned(coarse[k], 3))) return invalid_arg("finehead_assemble: a coarse tensor is NULL or not aligned to its element");
        if (misaligned(shs_fine, 3) || misaligned(row_of_masked, 3) || misaligned(masked_of_rest, 3)) return invalid_arg("finehead_assemble: unaligned buffer");
    }
    p.n_levels = n_levels; p.attr_dtype = attr_dtype; p.sh = sh_dim; p.P = sh_dim + 8;
    p.vw = 4;
    for (int k = 0; k < 5; ++k) {
        p.coarse[k] = (const float*)coarse[k]; p.out[k] = (float*)out[k];
        if (misaligned(out[k], 15)) p.vw = 1;
    }
    p.shs_fine = (const float*)shs_fine; p.row_of_masked = row_of_masked; p.masked_of_rest = masked_of_rest;
    p.Nc = Nc; p.n_masked = n_masked; p.opacity_shift = (float)opacity_shift; p.scaling_shift = (float)scaling_shift;
    const int widths[5] = {3, sh_dim, 1, 3, 4};
    int64_t end = 0;
    for (int k = 0; k < 5; ++k) p.groups_end[k] = end += (p.T * widths[k] + p.vw - 1) / p.vw;
    hipLaunchKernelGGL(finehead_assemble_kernel, strided_grid(end), dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("finehead_assemble_kernel");
}

int gdr_finehead_assemble_backward(int32_t n_levels, const int64_t* level_rows, int32_t attr_dtype, int32_t sh_dim, const void* grad_centers,
                                   const void* grad_shs, const void* grad_opacity, const void* grad_scaling, const void* grad_rotation,
                                   const int32_t* rank_masked, const int32_t* rank_rest, int64_t Nc, int64_t n_masked, int64_t n_rest,
                                   void* const* grad_coord, void* const* grad_attr, void* grad_centers_coarse, void* grad_opacity_coarse,
                                   void* grad_scaling_coarse, void* grad_rotation_coarse, void* grad_shs_fine, void* stream) {
    if (n_levels < 0 || n_levels > FH_LEVELS) return unsupported("finehead_assemble_backward: at most GDR_FINEHEAD_MAX_LEVELS levels");
    if (bad_dtype(attr_dtype)) return invalid_arg("finehead_assemble_backward: unknown dtype");
    if (bad_sh(sh_dim)) return unsupported("finehead_assemble_backward: sh_dim must be one of 3, 12, 27, 48");
    if (Nc < 0 || n_masked < 0 || n_rest < 0) return invalid_arg("finehead_assemble_backward: row counts must be >= 0");
    if (bad_rows_count(Nc) || bad_rows_count(n_masked) || n_rest > n_masked) return unsupported("finehead_assemble_backward: row counts must be below 2^31, n_rest at most n_masked");
    if (n_levels && (!level_rows || !grad_coord || !grad_attr)) return invalid_arg("finehead_assemble_backward: NULL argument");
    AsmBwdP p = {};
    if (!level_starts(n_levels, level_rows, n_rest, p.start)) return unsupported("finehead_assemble_backward: level rows must be >= 0 and the output below 2^31 rows");
    const void* g[5] = {grad_centers, grad_shs, grad_opacity, grad_scaling, grad_rotation};
    void* gc[5] = {grad_centers_coarse, nullptr, grad_opacity_coarse, grad_scaling_coarse, grad_rotation_coarse};
    bool coarse_wanted = grad_shs_fine != nullptr;
    for (int k = 0; k < 5; ++k) {
        if (misaligned(g[k], 3) || misaligned(gc[k], 3)) return invalid_arg("finehead_assemble_backward: a gradient is not aligned to its element");
        p.g[k] = (const float*)g[k]; p.gcoarse[k] = (float*)gc[k];
        coarse_wanted = coarse_wanted || gc[k];
    }
    if (coarse_wanted && ((Nc && !rank_masked) || (n_masked && !rank_rest))) return invalid_arg("finehead_assemble_backward: NULL rank table");
    if (misaligned(grad_shs_fine, 3) || misaligned(rank_masked, 3) || misaligned(rank_rest, 3)) return invalid_arg("finehead_assemble_backward: unaligned buffer");
    bool coords = false, attrs = false;
    for (int l = 0; l < n_levels; ++l) {
        if (misaligned(grad_coord[l], 3) || misaligned(grad_attr[l], esize(attr_dtype) - 1)) return invalid_arg("finehead_assemble_backward: a level gradient is not aligned to its element");
        p.gcoord[l] = (float*)grad_coord[l]; p.gattr[l] = grad_attr[l];
        coords = coords || (grad_coord[l] && level_rows[l]); attrs = attrs || (grad_attr[l] && level_rows[l]);
    }
    p.n_levels = n_levels; p.attr_dtype = attr_dtype; p.sh = sh_dim; p.P = sh_dim + 8;
    p.gshs_fine = (float*)grad_shs_fine; p.rank_masked = rank_masked; p.rank_rest = rank_rest; p.Nc = Nc; p.n_masked = n_masked; p.n_rest = n_rest;
    const int64_t L = p.start[n_levels];
    int64_t end = 0;
    p.ends[0] = end += coords ? L * 3 : 0;
    p.ends[1] = end += attrs ? L * p.P : 0;
    p.ends[2] = end += gc[0] ? Nc * 3 : 0;
    p.ends[3] = end += gc[2] ? Nc : 0;
    p.ends[4] = end += gc[3] ? Nc * 3 : 0;
    p.ends[5] = end += gc[4] ? Nc * 4 : 0;
    p.ends[6] = end += grad_shs_fine ? n_masked * sh_dim : 0;
    if (end == 0) return GDR_OK;
    hipLaunchKernelGGL(finehead_assemble_backward_kernel, strided_grid(end), dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("finehead_assemble_backward_kernel");
}

}  // extern "C"

// attn_tiled.hip — flash-style MFMA attention for fixed-length batches of long sequences (gfx950), forward and backward:
// what a ViT image encoder runs per layer (timm Attention.forward: 1025 tokens, head dimension 64), beyond the 256 tokens
// and the row-per-thread structure of attn.hip.  Public ABI: include/gdr.h gdr_attn_tiled_*.
//
// Semantics (tests/attn_ref.py with cu = [0, L, 2L, ...] is the f64 statement).  Per image b and head h:
//     S = scale * Q K^T (L x L),  P = softmax over the key axis of S,  O = P V,  lse_i = log sum_j exp(S_ij)
//   backward, with delta_i = sum_d dO_id O_id:  dV = P^T dO,  dS = P o (dO V^T - delta),  dQ = scale dS K,  dK = scale dS^T Q.
// q, k, v (and dout, dq, dk, dv) are (B, L, H, 64) through element strides (batch, token, head, channel), channel stride 1
// and 16-byte aligned rows: the three slices of one packed (B, L, 3, H, 64) tensor are read and written in place.
//
// Structure.  All three MFMA kernels are one scheme with the roles exchanged.  A workgroup of 4 waves owns TQ = 128
// "stationary" rows of one (b, h) (queries in forward and in the dQ kernel, keys in the dK / dV kernel), 32 per wave as two
// blocks of 16, and sweeps the other axis in tiles of TS = 64 rows staged in LDS.
//   - First products (S, and dP in backward): mfma_f32_16x16x32 with the SWEPT rows as the A operand, read from a row image in
//     LDS ([row][72]: 144-byte pitch, conflict-free 16-byte reads), and the stationary rows as the B operand, loaded once from
//     global memory into registers.  A lane then holds, for ONE stationary row (lane & 15), the values of the swept rows
//     4 quad .. 4 quad + 3 of every 16-row block (quad = lane >> 4): a softmax row lives on 4 lanes, its maximum and sum take two
//     __shfl_xor, and the row constants (running max and sum, lse, delta) are per-lane scalars.
//   - Second products (O, dQ, dK, dV, all accumulated transposed: channel x stationary row): the accumulators of two 16-row blocks,
//     rounded to the 16-bit dtype, ARE the B fragment of a k-step over 32 swept rows under the permutation
//     k = 8 quad + j  <->  swept row 16 (j >> 2) + 4 quad + (j & 3); the A operand applies the same permutation by reading
//     two 8-byte pieces from a TRANSPOSED image in LDS ([channel][68]).  Nothing of P or dS ever passes through LDS.
//   - Forward: online softmax per 64-key tile, exponentials as v_exp_f32 of log2(e)-prescaled scores; running max, running sum
//     (from the unrounded f32 P) and O in f32 registers.  Keys at or beyond L score -inf before the maximum.
//   - Backward: a small launch writes delta, from the result as two 16-bit words (out and out_lo, what out's rounding dropped:
//     K has a mean in real data, so an error of delta_i does not average out over the keys of dQ_i; from the rounded word alone
//     a correct kernel misses the dQ bar of tests/test_gpu_longattn.py at L = 1025); the key-stationary kernel keeps dK^T and
//     dV^T of its 128 keys in accumulators and sweeps the query tiles; the query-stationary kernel keeps dQ^T and sweeps the
//     key tiles.  P is recomputed from lse in both: seven products instead of five, no atomics, no hand-off between
//     workgroups, bitwise reproducible.
//   - Global loads of the next tile are issued into registers before the current tile's products and written to LDS after them.
// Rows at or beyond L are staged as zeros (never read), their statistics are set so that P is 0 or finite, and they are
// never stored.  DESIGN.md has the tile sizes against the compiler's resource report.
#include <math.h>
#include <stdio.h>

#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "mfma_rows.h"

namespace gdr {
namespace {

constexpr int TD = 64;            // head dimension
constexpr int TS = 64;            // swept rows per LDS tile
constexpr int TQ = 128;           // stationary rows per workgroup: 4 waves x 2 blocks x 16
constexpr int TW = 32;            // ... per wave
constexpr int RP = 72;            // pitch of a row image, elements
constexpr int CP = 68;            // pitch of a transposed image, elements
constexpr int TBLOCK = 256;
constexpr float LOG2E = 1.4426950408889634f;

struct Rows {            // a (B, L, H, 64) operand: channel stride 1, rows 16-byte aligned
    uint16_t* p;
    int64_t sb, st, sh;
};

struct TiledP {
    Rows q, k, v, dout, dq, dk, dv;
    uint16_t* out;       // (B, L, H, 64) dense
    uint16_t* out_lo;    // NULL or (B, L, H, 64) dense: what out's rounding dropped of the f32 result, rounded in turn
    float* lse;          // (B, H, L)
    float* delta;        // (B, H, L), backward
    int32_t B, L, H;
    float scale;
    float c;             // fl(scale * log2(e)): the scores' prescale, so that exponentials are v_exp_f32
    // c is rounded, so a score times c is off log2(e) times the scaled score by up to 6e-8 of it, the size of an f32 ulp of lse
    // in a head whose logits reach the hundreds.  lse leaves and enters the log2 domain through these two, in f64:
    double to_nat;       // scale / c (0 where scale is 0: every score is 0)
    double to_log2;      // c / scale (log2(e) where scale is 0)
};

__device__ __forceinline__ uint16_t* row_ptr(const Rows& r, int b, int t, int h) {
    return r.p + (int64_t)b * r.sb + (int64_t)t * r.st + (int64_t)h * r.sh;
}

__device__ __forceinline__ float exp2_raw(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32; 2^-inf = 0

struct Tile { uint4 x[2]; };     // a thread's share of a 64 x 64 tile: 16 bytes of rows (tid >> 3) and (tid >> 3) + 32

// rows [t0, t0 + 64) of (b, h); rows at or beyond L are zeros and are not read
__device__ __forceinline__ Tile load_tile(const Rows& src, int b, int h, int t0, int L) {
    Tile t;
    const int c = threadIdx.x & 7;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int r = t0 + (int)(threadIdx.x >> 3) + 32 * pass;
        t.x[pass] = make_uint4(0, 0, 0, 0);
        if (r < L) t.x[pass] = *reinterpret_cast<const uint4*>(row_ptr(src, b, r, h) + 8 * c);
    }
    return t;
}

// ... to the row image `img` ([row][RP]) and / or the transposed image `timg` ([channel][CP])
template <bool ROW, bool COL>
__device__ __forceinline__ void put_tile(const Tile& t, uint16_t* img, uint16_t* timg) {
    const int c = threadIdx.x & 7;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int r = (int)(threadIdx.x >> 3) + 32 * pass;
        if constexpr (ROW) *reinterpret_cast<uint4*>(img + r * RP + 8 * c) = t.x[pass];
        if constexpr (COL) {
            const uint32_t w[4] = {t.x[pass].x, t.x[pass].y, t.x[pass].z, t.x[pass].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) timg[(8 * c + e) * CP + r] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
        }
    }
}

// A fragment of a first product: row 16 blk + l16 of a row image, channels 32 ks + 8 quad .. + 7
__device__ __forceinline__ uint4 frag_rows(const uint16_t* img, int blk, int ks, int l16, int quad) {
    return *reinterpret_cast<const uint4*>(img + (16 * blk + l16) * RP + 32 * ks + 8 * quad);
}

// A fragment of a second product: channel 16 db + l16 of a transposed image, element j = swept row 32 kk + 16 (j >> 2) + 4 quad + (j & 3)
__device__ __forceinline__ uint4 frag_cols(const uint16_t* timg, int db, int kk, int l16, int quad) {
    const uint16_t* p = timg + (16 * db + l16) * CP + 32 * kk + 4 * quad;
    const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 16);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// B fragment of a first product: channels 32 ks + 8 quad .. + 7 of stationary row t (zeros at or beyond L)
__device__ __forceinline__ uint4 frag_global(const Rows& src, int b, int h, int t, int L, int ks, int quad) {
    if (t >= L) return make_uint4(0, 0, 0, 0);
    return *reinterpret_cast<const uint4*>(row_ptr(src, b, t, h) + 32 * ks + 8 * quad);
}

template <bool BF>
__device__ __forceinline__ uint32_t pack2(float a, float b) { return (uint32_t)down16<BF>(a) | ((uint32_t)down16<BF>(b) << 16); }

// two MFMA operand elements.  bf16 goes through the compiler's own conversion (v_cvt_pk_bf16_f32 on gfx950: round to nearest
// even, the bits of down16<true> for every finite value), because 16 integer roundings per lane and tile cost the bf16 kernels
// 15-20 % against the fp16 ones (BASELINE §4-vitattn); what is STORED is rounded by half_bits.h's one statement (pack2).
template <bool BF>
__device__ __forceinline__ uint32_t pack2_operand(float a, float b) {
    if constexpr (BF) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
    } else {
        return pack2<false>(a, b);
    }
}

// B fragment of a second product: the accumulators of two 16-row blocks, rounded (j 0..3 = lo, 4..7 = hi)
template <bool BF>
__device__ __forceinline__ uint4 pack_acc(const f32x4& lo, const f32x4& hi) {
    return make_uint4(pack2_operand<BF>(lo[0], lo[1]), pack2_operand<BF>(lo[2], lo[3]), pack2_operand<BF>(hi[0], hi[1]),
                      pack2_operand<BF>(hi[2], hi[3]));
}

// channels 16 db + 4 quad .. + 3 of row `dst` from a transposed accumulator, times f; `lo`: NULL, or the row that receives
// what the rounding dropped
template <bool BF>
__device__ __forceinline__ void store_acc(uint16_t* dst, int db, int quad, const f32x4& a, float f, uint16_t* lo = nullptr) {
    const float x[4] = {a[0] * f, a[1] * f, a[2] * f, a[3] * f};
    const uint32_t w0 = pack2<BF>(x[0], x[1]), w1 = pack2<BF>(x[2], x[3]);
    *reinterpret_cast<uint2*>(dst + 16 * db + 4 * quad) = make_uint2(w0, w1);
    if (lo)
        *reinterpret_cast<uint2*>(lo + 16 * db + 4 * quad) =
            make_uint2(pack2<BF>(x[0] - up16<BF>((uint16_t)w0), x[1] - up16<BF>((uint16_t)(w0 >> 16))),
                       pack2<BF>(x[2] - up16<BF>((uint16_t)w1), x[3] - up16<BF>((uint16_t)(w1 >> 16))));
}

__device__ __forceinline__ float quad_max(float v) {     // over the 4 lanes that share lane & 15
    v = fmaxf(v, __shfl_xor(v, 16, GDR_WAVE));
    return fmaxf(v, __shfl_xor(v, 32, GDR_WAVE));
}
__device__ __forceinline__ float quad_sum(float v) {     // the same bits in all 4 lanes (every step adds a pair commutatively)
    v += __shfl_xor(v, 16, GDR_WAVE);
    return v + __shfl_xor(v, 32, GDR_WAVE);
}

struct Where { int tile, h, b; };
__device__ __forceinline__ Where where(const TiledP& p) {    // a (b, h)'s workgroups are neighbours: its K / V stay in L2
    const int nt = (p.L + TQ - 1) / TQ;
    Where w;
    w.tile = blockIdx.x % nt;
    w.h = (blockIdx.x / nt) % p.H;
    w.b = blockIdx.x / (nt * p.H);
    return w;
}

template <bool BF>
__global__ __launch_bounds__(TBLOCK) void attn_tiled_fwd_kernel(const TiledP p) {
    constexpr int DT = BF ? GDR_BF16 : GDR_F16;
    __shared__ __attribute__((aligned(16))) uint16_t sK[TS * RP];
    __shared__ __attribute__((aligned(16))) uint16_t sVt[TD * CP];
    const Where w = where(p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, quad = lane >> 4;
    const int q0 = w.tile * TQ + wave * TW;
    uint4 qf[2][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[cb][ks] = frag_global(p.q, w.b, w.h, q0 + 16 * cb + l16, p.L, ks, quad);
    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};     // l: this lane's share of the row sum
    f32x4 o[2][4];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int db = 0; db < 4; ++db) o[cb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float c = p.c;
    const int nk = (p.L + TS - 1) / TS;
    Tile tk = load_tile(p.k, w.b, w.h, 0, p.L), tv = load_tile(p.v, w.b, w.h, 0, p.L);
    for (int kt = 0; kt < nk; ++kt) {
        const int k0 = kt * TS;
        __syncthreads();
        put_tile<true, false>(tk, sK, nullptr);
        put_tile<false, true>(tv, nullptr, sVt);
        __syncthreads();
        if (kt + 1 < nk) {
            tk = load_tile(p.k, w.b, w.h, k0 + TS, p.L);
            tv = load_tile(p.v, w.b, w.h, k0 + TS, p.L);
        }
        if (q0 >= p.L) continue;       // a wave without rows only stages
        f32x4 s[2][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            s[0][kb] = s[1][kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 a = frag_rows(sK, kb, ks, l16, quad);
                mma_row<DT>(a, qf[0][ks], s[0][kb]);
                mma_row<DT>(a, qf[1][ks], s[1][kb]);
            }
        }
        const bool tail = k0 + TS > p.L;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float tmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // a product of its own, never contracted into the subtraction below: the maximum's exponent is then exactly
                    // 0 and its P exactly 1, so a row that one key owns has O = V and dS = 0 to the bit (see delta)
                    float x = __fmul_rn(s[cb][kb][r], c);
                    if (tail && k0 + 16 * kb + 4 * quad + r >= p.L) x = -INFINITY;
                    s[cb][kb][r] = x;
                    tmax = fmaxf(tmax, x);
                }
            const float mn = fmaxf(m[cb], quad_max(tmax));      // finite: key k0 < L is in the tile
            const float alpha = exp2_raw(m[cb] - mn);           // first tile: 2^-inf = 0 on zeros
            m[cb] = mn;
            float sum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = exp2_raw(s[cb][kb][r] - mn);
                    s[cb][kb][r] = e;
                    sum += e;
                }
            l[cb] = l[cb] * alpha + sum;
#pragma unroll
            for (int db = 0; db < 4; ++db) o[cb][db] *= alpha;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 p0 = pack_acc<BF>(s[0][2 * kk], s[0][2 * kk + 1]), p1 = pack_acc<BF>(s[1][2 * kk], s[1][2 * kk + 1]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const uint4 a = frag_cols(sVt, db, kk, l16, quad);
                mma_row<DT>(a, p0, o[0][db]);
                mma_row<DT>(a, p1, o[1][db]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int t = q0 + 16 * cb + l16;
        const float lt = quad_sum(l[cb]);
        if (t >= p.L) continue;
        const float inv = 1.f / lt;
        const int64_t at = (((int64_t)w.b * p.L + t) * p.H + w.h) * TD;
#pragma unroll
        for (int db = 0; db < 4; ++db) store_acc<BF>(p.out + at, db, quad, o[cb][db], inv, p.out_lo ? p.out_lo + at : nullptr);
        if (quad == 0) p.lse[((int64_t)w.b * p.H + w.h) * p.L + t] = (float)((double)m[cb] * p.to_nat + (double)logf(lt));
    }
}

// delta_i = sum_d dO_id (O_id + Olo_id): a wave takes 16 rows of one (b, h) and keeps the diagonal of O dO^T, formed by the same two MFMA
// steps, with dO in the same operand, as dP = V dO^T of the backward kernels.  So where P is one key's (a sequence of one
// token: O = V), dP - delta is exactly zero, as it is in any composition of a softmax backward.
template <bool BF>
__global__ __launch_bounds__(TBLOCK) void attn_tiled_delta_kernel(const TiledP p) {
    constexpr int DT = BF ? GDR_BF16 : GDR_F16;
    const int nt = (p.L + TS - 1) / TS;
    const int tile = blockIdx.x % nt, h = (blockIdx.x / nt) % p.H, b = blockIdx.x / (nt * p.H);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, quad = lane >> 4;
    const int t = tile * TS + 16 * wave + l16;
    const Rows o = {p.out, (int64_t)p.L * p.H * TD, (int64_t)p.H * TD, TD}, lo = {p.out_lo, o.sb, o.st, o.sh};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
        mma_row<DT>(frag_global(o, b, h, t, p.L, ks, quad), frag_global(p.dout, b, h, t, p.L, ks, quad), acc);
    if (p.out_lo) {     // (after the two steps of the rounded word: with out_lo = 0 the sum is theirs, bit for bit)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            mma_row<DT>(frag_global(lo, b, h, t, p.L, ks, quad), frag_global(p.dout, b, h, t, p.L, ks, quad), acc);
    }
    // row 4 quad + r, column l16 of the 16 x 16 product: the diagonal element of row l16 sits in lane quad = l16 / 4
    const int r = l16 & 3;
    const float d = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    if (t < p.L && quad == (l16 >> 2)) p.delta[((int64_t)b * p.H + h) * p.L + t] = d;
}

// key-stationary: dK and dV of 128 keys, swept over the query tiles
template <bool BF>
__global__ __launch_bounds__(TBLOCK) void attn_tiled_bwd_kv_kernel(const TiledP p) {
    constexpr int DT = BF ? GDR_BF16 : GDR_F16;
    __shared__ __attribute__((aligned(16))) uint16_t sQ[TS * RP];
    __shared__ __attribute__((aligned(16))) uint16_t sG[TS * RP];
    __shared__ __attribute__((aligned(16))) uint16_t sQt[TD * CP];
    __shared__ __attribute__((aligned(16))) uint16_t sGt[TD * CP];
    __shared__ __attribute__((aligned(16))) float sL[TS];
    __shared__ __attribute__((aligned(16))) float sD[TS];
    const Where w = where(p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, quad = lane >> 4;
    const int j0 = w.tile * TQ + wave * TW;
    uint4 kf[2][2], vf[2][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[cb][ks] = frag_global(p.k, w.b, w.h, j0 + 16 * cb + l16, p.L, ks, quad);
            vf[cb][ks] = frag_global(p.v, w.b, w.h, j0 + 16 * cb + l16, p.L, ks, quad);
        }
    f32x4 dk[2][4], dv[2][4];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int db = 0; db < 4; ++db) dk[cb][db] = dv[cb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float c = p.c;
    const int nq = (p.L + TS - 1) / TS;
    const int64_t stat = ((int64_t)w.b * p.H + w.h) * p.L;
    // a query row at or beyond L: lse = +inf makes its P zero, and its dO row is zeros
    auto load_stat = [&](int i0, float& ls, float& dl) {
        const int i = i0 + (int)threadIdx.x;
        const bool on = threadIdx.x < TS && i < p.L;
        ls = on ? (float)((double)p.lse[stat + i] * p.to_log2) : INFINITY;
        dl = on ? p.delta[stat + i] : 0.f;
    };
    Tile tq = load_tile(p.q, w.b, w.h, 0, p.L), tg = load_tile(p.dout, w.b, w.h, 0, p.L);
    float ls, dl;
    load_stat(0, ls, dl);
    for (int qt = 0; qt < nq; ++qt) {
        const int i0 = qt * TS;
        __syncthreads();
        put_tile<true, true>(tq, sQ, sQt);
        put_tile<true, true>(tg, sG, sGt);
        if (threadIdx.x < TS) sL[threadIdx.x] = ls, sD[threadIdx.x] = dl;
        __syncthreads();
        if (qt + 1 < nq) {
            tq = load_tile(p.q, w.b, w.h, i0 + TS, p.L);
            tg = load_tile(p.dout, w.b, w.h, i0 + TS, p.L);
            load_stat(i0 + TS, ls, dl);
        }
        if (j0 >= p.L) continue;
        f32x4 s[2][4], dp[2][4];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            s[0][qb] = s[1][qb] = dp[0][qb] = dp[1][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 aq = frag_rows(sQ, qb, ks, l16, quad), ag = frag_rows(sG, qb, ks, l16, quad);
                mma_row<DT>(aq, kf[0][ks], s[0][qb]);
                mma_row<DT>(aq, kf[1][ks], s[1][qb]);
                mma_row<DT>(ag, vf[0][ks], dp[0][qb]);
                mma_row<DT>(ag, vf[1][ks], dp[1][qb]);
            }
        }
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const float4 l4 = *reinterpret_cast<const float4*>(sL + 16 * qb + 4 * quad);
            const float4 d4 = *reinterpret_cast<const float4*>(sD + 16 * qb + 4 * quad);
            const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pr = exp2_raw(__fmul_rn(s[cb][qb][r], c) - lr[r]);      // the forward's product
                    s[cb][qb][r] = pr;
                    dp[cb][qb][r] = pr * (dp[cb][qb][r] - dr[r]);
                }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 p0 = pack_acc<BF>(s[0][2 * kk], s[0][2 * kk + 1]), p1 = pack_acc<BF>(s[1][2 * kk], s[1][2 * kk + 1]);
            const uint4 d0 = pack_acc<BF>(dp[0][2 * kk], dp[0][2 * kk + 1]), d1 = pack_acc<BF>(dp[1][2 * kk], dp[1][2 * kk + 1]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const uint4 ag = frag_cols(sGt, db, kk, l16, quad), aq = frag_cols(sQt, db, kk, l16, quad);
                mma_row<DT>(ag, p0, dv[0][db]);
                mma_row<DT>(ag, p1, dv[1][db]);
                mma_row<DT>(aq, d0, dk[0][db]);
                mma_row<DT>(aq, d1, dk[1][db]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int t = j0 + 16 * cb + l16;
        if (t >= p.L) continue;
        uint16_t* pk = row_ptr(p.dk, w.b, t, w.h);
        uint16_t* pv = row_ptr(p.dv, w.b, t, w.h);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            store_acc<BF>(pk, db, quad, dk[cb][db], p.scale);
            store_acc<BF>(pv, db, quad, dv[cb][db], 1.f);
        }
    }
}

// query-stationary: dQ of 128 queries, swept over the key tiles
template <bool BF>
__global__ __launch_bounds__(TBLOCK) void attn_tiled_bwd_q_kernel(const TiledP p) {
    constexpr int DT = BF ? GDR_BF16 : GDR_F16;
    __shared__ __attribute__((aligned(16))) uint16_t sK[TS * RP];
    __shared__ __attribute__((aligned(16))) uint16_t sV[TS * RP];
    __shared__ __attribute__((aligned(16))) uint16_t sKt[TD * CP];
    const Where w = where(p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, quad = lane >> 4;
    const int q0 = w.tile * TQ + wave * TW;
    const int64_t stat = ((int64_t)w.b * p.H + w.h) * p.L;
    uint4 qf[2][2], gf[2][2];
    float ls[2], dl[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int t = q0 + 16 * cb + l16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[cb][ks] = frag_global(p.q, w.b, w.h, t, p.L, ks, quad);
            gf[cb][ks] = frag_global(p.dout, w.b, w.h, t, p.L, ks, quad);
        }
        ls[cb] = t < p.L ? (float)((double)p.lse[stat + t] * p.to_log2) : INFINITY;      // a row at or beyond L: P = 0
        dl[cb] = t < p.L ? p.delta[stat + t] : 0.f;
    }
    f32x4 dq[2][4];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int db = 0; db < 4; ++db) dq[cb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float c = p.c;
    const int nk = (p.L + TS - 1) / TS;
    Tile tk = load_tile(p.k, w.b, w.h, 0, p.L), tv = load_tile(p.v, w.b, w.h, 0, p.L);
    for (int kt = 0; kt < nk; ++kt) {
        const int k0 = kt * TS;
        __syncthreads();
        put_tile<true, true>(tk, sK, sKt);
        put_tile<true, false>(tv, sV, nullptr);
        __syncthreads();
        if (kt + 1 < nk) {
            tk = load_tile(p.k, w.b, w.h, k0 + TS, p.L);
            tv = load_tile(p.v, w.b, w.h, k0 + TS, p.L);
        }
        if (q0 >= p.L) continue;
        f32x4 s[2][4], dp[2][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            s[0][kb] = s[1][kb] = dp[0][kb] = dp[1][kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 ak = frag_rows(sK, kb, ks, l16, quad), av = frag_rows(sV, kb, ks, l16, quad);
                mma_row<DT>(ak, qf[0][ks], s[0][kb]);
                mma_row<DT>(ak, qf[1][ks], s[1][kb]);
                mma_row<DT>(av, gf[0][ks], dp[0][kb]);
                mma_row<DT>(av, gf[1][ks], dp[1][kb]);
            }
        }
        const bool tail = k0 + TS > p.L;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pr = exp2_raw(__fmul_rn(s[cb][kb][r], c) - ls[cb]);      // the forward's product
                    if (tail && k0 + 16 * kb + 4 * quad + r >= p.L) pr = 0.f;     // (its K and V rows are zeros: dS = 0 too)
                    s[cb][kb][r] = pr * (dp[cb][kb][r] - dl[cb]);
                }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 d0 = pack_acc<BF>(s[0][2 * kk], s[0][2 * kk + 1]), d1 = pack_acc<BF>(s[1][2 * kk], s[1][2 * kk + 1]);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const uint4 a = frag_cols(sKt, db, kk, l16, quad);
                mma_row<DT>(a, d0, dq[0][db]);
                mma_row<DT>(a, d1, dq[1][db]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int t = q0 + 16 * cb + l16;
        if (t >= p.L) continue;
        uint16_t* dst = row_ptr(p.dq, w.b, t, w.h);
#pragma unroll
        for (int db = 0; db < 4; ++db) store_acc<BF>(dst, db, quad, dq[cb][db], p.scale);
    }
}

// NULL if the arguments are inside the envelope
const char* tiled_check(const gdr_attn_tiled_args* a) {
    if (!a) return "attn_tiled: NULL arguments";
    if (a->dtype != GDR_F16 && a->dtype != GDR_BF16) return "attn_tiled: dtype must be GDR_F16 or GDR_BF16";
    if (a->D != TD) return "attn_tiled: head dimension D must be 64";
    if (a->B < 1) return "attn_tiled: B must be >= 1";
    if (a->H < 1) return "attn_tiled: H must be >= 1";
    if (a->L < 1 || a->L > GDR_ATTN_TILED_MAX_SEQLEN) return "attn_tiled: L must be in 1..16384";
    if ((int64_t)a->B * a->H * a->L >= INT64_C(0x80000000)) return "attn_tiled: B * H * L must be below 2^31";
    if (!(a->scale == a->scale) || a->scale - a->scale != 0.f) return "attn_tiled: softmax scale is not finite";
    return nullptr;
}

// rows of 64 16-bit words through (batch, token, head, channel) strides: channel stride 1, everything else a multiple of 8
// from a 16-byte aligned base
const char* tiled_rows(const void* ptr, const int64_t* s, Rows& r) {
    if (!ptr || !s) return "NULL";
    if (s[3] != 1) return "channel stride must be 1";
    if (misaligned(ptr, 15) || s[0] % 8 || s[1] % 8 || s[2] % 8) return "rows must be 16-byte aligned";
    r.p = (uint16_t*)ptr; r.sb = s[0]; r.st = s[1]; r.sh = s[2];
    return nullptr;
}

int tiled_refuse(const char* fn, const char* name, const char* why) {
    char text[160];
    snprintf(text, sizeof text, "%s: %s: %s", fn, name, why);     // (set_error copies)
    return invalid_arg(text);
}

void tiled_scale(const gdr_attn_tiled_args* a, TiledP& p) {
    p.scale = a->scale;
    p.c = a->scale * LOG2E;
    p.to_nat = p.c != 0.f ? (double)a->scale / (double)p.c : 0.0;
    p.to_log2 = p.c != 0.f ? (double)p.c / (double)a->scale : (double)LOG2E;
}

int tiled_blocks(const gdr_attn_tiled_args* a) { return a->B * a->H * ((a->L + TQ - 1) / TQ); }

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_attn_tiled_scratch_bytes(const gdr_attn_tiled_args* a) {
    if (const char* why = tiled_check(a)) { invalid_arg(why); return 0; }
    return (size_t)a->B * (size_t)a->H * (size_t)a->L * sizeof(float);
}

int gdr_attn_tiled_forward(const gdr_attn_tiled_args* a, const void* q, const int64_t* q_strides, const void* k,
                           const int64_t* k_strides, const void* v, const int64_t* v_strides, void* out, void* out_lo,
                           float* lse, void* stream) {
    static const char* fn = "attn_tiled_forward";
    if (const char* why = tiled_check(a)) return invalid_arg(why);
    TiledP p = {};
    if (const char* why = tiled_rows(q, q_strides, p.q)) return tiled_refuse(fn, "q", why);
    if (const char* why = tiled_rows(k, k_strides, p.k)) return tiled_refuse(fn, "k", why);
    if (const char* why = tiled_rows(v, v_strides, p.v)) return tiled_refuse(fn, "v", why);
    if (!out || !lse) return tiled_refuse(fn, "out / lse", "NULL");
    if (misaligned(out, 15) || misaligned(out_lo, 15) || misaligned(lse, 3)) return tiled_refuse(fn, "out / out_lo / lse", "unaligned buffer");
    p.out = (uint16_t*)out; p.out_lo = (uint16_t*)out_lo; p.lse = lse;
    p.B = a->B; p.L = a->L; p.H = a->H;
    tiled_scale(a, p);
    const hipStream_t st = (hipStream_t)stream;
    if (a->dtype == GDR_BF16) hipLaunchKernelGGL(attn_tiled_fwd_kernel<true>, dim3(tiled_blocks(a)), dim3(TBLOCK), 0, st, p);
    else hipLaunchKernelGGL(attn_tiled_fwd_kernel<false>, dim3(tiled_blocks(a)), dim3(TBLOCK), 0, st, p);
    return launch_status("attn_tiled_fwd_kernel");
}

int gdr_attn_tiled_backward(const gdr_attn_tiled_args* a, const void* dout, const int64_t* dout_strides, const void* q,
                            const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                            const int64_t* v_strides, const void* out, const void* out_lo, const float* lse, void* dq,
                            const int64_t* dq_strides, void* dk, const int64_t* dk_strides, void* dv, const int64_t* dv_strides,
                            void* scratch, void* stream) {
    static const char* fn = "attn_tiled_backward";
    if (const char* why = tiled_check(a)) return invalid_arg(why);
    TiledP p = {};
    if (const char* why = tiled_rows(dout, dout_strides, p.dout)) return tiled_refuse(fn, "dout", why);
    if (const char* why = tiled_rows(q, q_strides, p.q)) return tiled_refuse(fn, "q", why);
    if (const char* why = tiled_rows(k, k_strides, p.k)) return tiled_refuse(fn, "k", why);
    if (const char* why = tiled_rows(v, v_strides, p.v)) return tiled_refuse(fn, "v", why);
    if (const char* why = tiled_rows(dq, dq_strides, p.dq)) return tiled_refuse(fn, "dq", why);
    if (const char* why = tiled_rows(dk, dk_strides, p.dk)) return tiled_refuse(fn, "dk", why);
    if (const char* why = tiled_rows(dv, dv_strides, p.dv)) return tiled_refuse(fn, "dv", why);
    if (!out || !lse || !scratch) return tiled_refuse(fn, "out / lse / scratch", "NULL");
    if (misaligned(out, 15) || misaligned(out_lo, 15) || misaligned(lse, 3) || misaligned(scratch, 3))
        return tiled_refuse(fn, "out / out_lo / lse / scratch", "unaligned buffer");
    p.out = (uint16_t*)out; p.out_lo = (uint16_t*)out_lo; p.lse = (float*)lse; p.delta = (float*)scratch;
    p.B = a->B; p.L = a->L; p.H = a->H;
    tiled_scale(a, p);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 dgrid(a->B * a->H * ((a->L + TS - 1) / TS)), grid(tiled_blocks(a)), block(TBLOCK);
    if (a->dtype == GDR_BF16) {
        hipLaunchKernelGGL(attn_tiled_delta_kernel<true>, dgrid, block, 0, st, p);
        hipLaunchKernelGGL(attn_tiled_bwd_kv_kernel<true>, grid, block, 0, st, p);
        hipLaunchKernelGGL(attn_tiled_bwd_q_kernel<true>, grid, block, 0, st, p);
    } else {
        hipLaunchKernelGGL(attn_tiled_delta_kernel<false>, dgrid, block, 0, st, p);
        hipLaunchKernelGGL(attn_tiled_bwd_kv_kernel<false>, grid, block, 0, st, p);
        hipLaunchKernelGGL(attn_tiled_bwd_q_kernel<false>, grid, block, 0, st, p);
    }
    return launch_status("attn_tiled_bwd kernels");
}

}  // extern "C"

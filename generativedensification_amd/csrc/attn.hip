// attn.hip — variable-length packed-QKV attention for short sequences (gfx950), forward and backward: the one entry
// point of flash_attn the reference's point decoder calls (lightning/point_decoder/autoencoder.py SerializedAttention,
// flash_attn_varlen_qkvpacked_func with dropout 0, no mask).  Public ABI: include/gdr.h gdr_attn_*.
//
// Semantics, restated (tests/attn_ref.py is the f64 statement of the same):
//   qkv (total, 3, H, D) fp16 or bf16, cu_seqlens (batch + 1) int32.  For sequence b = rows [cu[b], cu[b+1]) and head h:
//     S = scale * Q K^T (L x L),  P = softmax over the key axis of S,  O = P V,  lse_i = log sum_j exp(S_ij)
//   out (total, H, D) in the input dtype, lse (H, total) f32.  Rows at or beyond cu[batch] are zero in out, lse and dqkv.
//   backward, with delta_i = sum_d dO_id O_id:  dV = P^T dO,  dS = P o (dO V^T - delta),  dQ = scale dS K,  dK = scale dS^T Q.
//
// Structure.  The shapes that matter are tiny (L = 48 keys, D = 8: a 48 x 48 x 8 problem per sequence and head) and the call
// moves about as many bytes as it does FLOPs, so the kernels are built around bytes and launches, not around a matrix tile:
//   - one launch forward, one backward; a 256-thread workgroup owns one sequence and G = 256 / RP heads of it, RP = 64, 128
//     or 256 rows (the smallest that holds max_seqlen), so every wave works on ONE head and a thread is ONE query row;
//   - the workgroup's K and V rows go to LDS once (f32 for D <= 16, the 16-bit input words for D >= 32: 64 KiB at D = 64);
//     every lane of a wave then reads the same key row — an LDS broadcast, no bank conflicts — and keeps its query row, its
//     running max / sum and its D output accumulators in registers (online softmax over blocks of 8 keys, all f32, P is
//     never rounded to 16 bits);
//   - backward runs two sweeps in the same workgroup: thread = query row (dQ, K and V in LDS), then thread = key row (dK,
//     dV, with Q, dO, lse and delta in LDS).  P is recomputed from lse in both.  A (sequence, head) problem never leaves its
//     workgroup: no atomics, no cross-workgroup reduction, two runs are bitwise equal;
//   - the score s_ij is the same fma chain over d in all three places it is computed, so forward and backward agree on P.
// DESIGN.md §13 has the instruction counts behind VALU-not-MFMA at D = 8, L = 48 and the LDS budget.
//
// The gather form (GA = true, gdr_attn_gather_*) is the same two kernels with the row order as a parameter: slot p of a
// sequence reads row order[p] of a dense (N, 3, H, D) qkv of any of three dtypes (rounded to fp16 on load; BF = false), and
// only the slot that is its row's own (inverse[order[p]] == p) stores, straight to that row.  The reference's padding puts a
// row's second slot one sequence later at the same position; the backward workgroup of the own slot loads that next
// sequence's Q, dO, lse and delta into the LDS it has, runs the key-row sweep over its real query rows too and adds into the
// same f32 dK / dV registers before the one rounding.  No scratch, no atomics on memory; DESIGN.md §28.
//
// Memory safety does not depend on cu_seqlens being well formed (it lives on the device and is never read by the host):
// boundaries are clamped to [0, total] and a sequence longer than RP is cut at RP rows.  Nor on order / inverse: a slot
// index is below total = Tp by that clamp, an entry of order outside [0, N) makes its slot a row of zeros that stores nothing,
// inverse is read only at such a checked row and only compared.
#include <math.h>

#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"

namespace gdr {
namespace {

constexpr int AT_BLOCK = GDR_BLOCK;   // 256 threads: G heads x RP rows
constexpr int AT_KB = 8;              // keys per online-softmax block

struct AttnP {
    const uint16_t* qkv;     // (total, 3, H, D) through q0 (token), q1 (q/k/v), q2 (head), q3 (channel) element strides
    const int32_t* cu;       // batch + 1 boundaries, or NULL: sequence b = rows [b * fixed_len, (b + 1) * fixed_len)
    uint16_t* out;           // (total, H, D) dense            (backward: read)
    float* lse;              // (H, total) dense               (backward: read)
    const uint16_t* dout;    // backward: (total, H, D) through d0, d1, d2
    uint16_t* dqkv;          // backward: (total, 3, H, D) dense
    const int64_t* order;    // gather form: (total) the row of the dense (N, 3, H, D) qkv that each slot holds
    const int64_t* inverse;  // gather form: (N) the slot that is each row's own
    float* out_full;         // gather form, forward: NULL or (N, H, D) f32, the result before any rounding
    int64_t q0, q1, q2, q3, d0, d1, d2;
    int32_t total, batch, H, fixed_len;
    int32_t N, io_dtype, out_dtype;   // gather form: rows, the dtype of qkv / out / dout / dqkv, the dtype backward reads out in
    int32_t qkv_vec, dout_vec;   // rows are unit-stride and 16-byte aligned: 128-bit loads
    float scale;
};

using gdr::load_row;    // row_io.h's rows of a run-time dtype, beside the <D, BF> rows of the dense kernels below
using gdr::store_row;

// one row of D 16-bit words from global memory, as f32
template <int D, bool BF>
__device__ __forceinline__ void load_row(const uint16_t* p, int64_t sd, int vec, float (&x)[D]) {
    if (vec) {
#pragma unroll
        for (int c = 0; c < D / 8; ++c) unpack8<BF>(reinterpret_cast<const uint4*>(p)[c], x + 8 * c);
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = up16<BF>(p[d * sd]);
    }
}

// one dense, 16-byte aligned row of D 16-bit words to global memory
template <int D, bool BF>
__device__ __forceinline__ void store_row(uint16_t* p, const float (&x)[D]) {
#pragma unroll
    for (int c = 0; c < D / 8; ++c) reinterpret_cast<uint4*>(p)[c] = pack8<BF>(x + 8 * c);
}

template <int D>
__device__ __forceinline__ void zero_row(uint16_t* p) {
#pragma unroll
    for (int c = 0; c < D / 8; ++c) reinterpret_cast<uint4*>(p)[c] = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ float as_half(float x) { return up16<false>(down16<false>(x)); }   // what .half() keeps of x

// gather form: one dense, 16-byte aligned row of D elements of the run-time dtype `dt` at element `at`, as f32, each rounded
// to fp16 first
template <int D>
__device__ __forceinline__ void load_row_half(const void* base, int64_t at, int dt, float (&x)[D]) {
    load_row<D>(base, at, dt, x);
    if (dt != GDR_ATTN_F16) {
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = as_half(x[d]);
    }
}

// gather form: x rounded to fp16 and then to `dt`, to one dense, 16-byte aligned row at element `at`
template <int D>
__device__ __forceinline__ void store_row_half(void* base, int64_t at, int dt, const float (&x)[D]) {
    if (dt == GDR_ATTN_F16) {      // (the dense kernels' own store: the composition over them is matched bit for bit)
        store_row<D, false>(static_cast<uint16_t*>(base) + at, x);
        return;
    }
    float y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = as_half(x[d]);
    store_row<D>(base, at, dt, y);
}

// LDS rows: f32 while they are small, the 16-bit input words from D = 32 on (exact either way)
template <int D> struct Store { using type = typename std::conditional<(D <= 16), float, uint16_t>::type; };

template <int D, bool BF, typename S>
__device__ __forceinline__ void lds_put(S* row, const float (&x)[D]) {
    if constexpr (std::is_same<S, float>::value) {
#pragma unroll
        for (int c = 0; c < D / 4; ++c)
            reinterpret_cast<float4*>(row)[c] = make_float4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < D / 8; ++c) reinterpret_cast<uint4*>(row)[c] = pack8<BF>(x + 8 * c);   // exact: x came from 16 bits
    }
}

// 8 consecutive channels (chunk c) of an LDS row, as f32
template <bool BF, typename S>
__device__ __forceinline__ void lds_get8(const S* row, int c, float* x) {
    if constexpr (std::is_same<S, float>::value) {
        const float4 a = reinterpret_cast<const float4*>(row)[2 * c], b = reinterpret_cast<const float4*>(row)[2 * c + 1];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
        unpack8<BF>(reinterpret_cast<const uint4*>(row)[c], x);
    }
}

// sum_d a[d] * row[d]: ONE fma chain over d, the same wherever a score is formed
template <int D, bool BF, typename S>
__device__ __forceinline__ float lds_dot(const float (&a)[D], const S* row) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D / 8; ++c) {
        float t[8];
        lds_get8<BF>(row, c, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(a[8 * c + e], t[e], acc);
    }
    return acc;
}

// acc[d] += w * row[d]
template <int D, bool BF, typename S>
__device__ __forceinline__ void lds_axpy(float w, const S* row, float (&acc)[D]) {
#pragma unroll
    for (int c = 0; c < D / 8; ++c) {
        float t[8];
        lds_get8<BF>(row, c, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[8 * c + e] = fmaf(w, t[e], acc[8 * c + e]);
    }
}

// rows [start, start + L) of sequence `seq` (L <= RP), or the tail [cu[batch], total) for seq == batch (L unclamped)
template <int RP>
__device__ __forceinline__ void seq_range(const AttnP& p, int seq, int& start, int& L) {
    const bool tail = seq == p.batch;
    int64_t a = p.cu ? (int64_t)p.cu[seq] : (int64_t)seq * p.fixed_len;
    int64_t b = tail ? (int64_t)p.total : (p.cu ? (int64_t)p.cu[seq + 1] : a + p.fixed_len);
    a = a < 0 ? 0 : (a > p.total ? p.total : a);
    b = b < a ? a : (b > p.total ? p.total : b);
    start = (int)a;
    L = (int)(b - a);
    if (!tail && L > RP) L = RP;
}

// gather form: the row slot `tok` (< total) holds, or -1 for an entry outside the table's range
__device__ __forceinline__ int64_t gather_row(const AttnP& p, int64_t tok) {
    const int64_t v = p.order[tok];
    return (v >= 0 && v < p.N) ? v : -1;
}

// Q (w = 0), K (1) or V (2) of head h: of token `row` through the strides, or (GA) of row `row` of the dense qkv, zeros for -1
template <int D, bool BF, bool GA>
__device__ __forceinline__ void load_qkv(const AttnP& p, int64_t row, int h, int w, float (&x)[D]) {
    if constexpr (GA) {
        if (row >= 0) {
            load_row_half<D>(p.qkv, ((row * 3 + w) * p.H + h) * D, p.io_dtype, x);
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = 0.f;
        }
    } else {
        load_row<D, BF>(p.qkv + row * p.q0 + w * p.q1 + (int64_t)h * p.q2, p.q3, p.qkv_vec, x);
    }
}

__device__ __forceinline__ float exp_nat(float x) { return __expf(x); }   // v_exp_f32 of x * log2(e); exp(-inf) = 0

// thread = key row j (k, v) against the n query rows in LDS (Q, dO, lse, delta): dv += sum_i P_ij dO_i and
// dk += sum_i P_ij (dO_i . V_j - delta_i) Q_i, dk without the softmax scale
template <int D, bool BF, typename S>
__device__ __forceinline__ void key_sweep(const float (&k)[D], const float (&v)[D], const S* Q, const S* G, const float* lse,
                                          const float* del, int n, float scale, float (&dk)[D], float (&dv)[D]) {
    for (int i = 0; i < n; ++i) {
        const S* Qi = Q + (size_t)i * D;
        const S* Gi = G + (size_t)i * D;
        const float s = lds_dot<D, BF>(k, Qi) * scale;
        const float pi = exp_nat(s - lse[i]);
        const float dp = lds_dot<D, BF>(v, Gi);
        lds_axpy<D, BF>(pi, Gi, dv);
        lds_axpy<D, BF>(pi * (dp - del[i]), Qi, dk);
    }
}

template <int D, int RP, bool BF, bool GA>
__global__ __launch_bounds__(AT_BLOCK) void attn_fwd_kernel(const AttnP p) {
    using S = typename Store<D>::type;
    constexpr int G = AT_BLOCK / RP;
    __shared__ __attribute__((aligned(16))) S sK[AT_BLOCK * D];
    __shared__ __attribute__((aligned(16))) S sV[AT_BLOCK * D];
    const int HG = (p.H + G - 1) / G;
    const int seq = blockIdx.x / HG, hg = blockIdx.x % HG;
    const int g = threadIdx.x / RP, r = threadIdx.x % RP;
    const int h = hg * G + g;
    int start, L;
    seq_range<RP>(p, seq, start, L);
    if constexpr (!GA) {
        if (seq == p.batch) {   // rows no sequence owns: defined as zero
            if (h < p.H)
                for (int row = start + r; row < start + L; row += RP) {
                    zero_row<D>(p.out + ((int64_t)row * p.H + h) * D);
                    p.lse[(int64_t)h * p.total + row] = 0.f;
                }
            return;
        }
    }
    if (L == 0) return;
    const bool live = r < L && h < p.H;
    const int64_t tok = start + r;
    int64_t row = tok;      // GA: the row this slot holds, and whether the slot is that row's own
    bool own = true;
    if constexpr (GA) {
        row = live ? gather_row(p, tok) : -1;
        own = row >= 0 && p.inverse[row] == tok;
    }
    float q[D], t[D];
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = 0.f, t[d] = 0.f;
    S* myK = sK + (size_t)(g * RP + r) * D;
    S* myV = sV + (size_t)(g * RP + r) * D;
    if (live) {
        load_qkv<D, BF, GA>(p, row, h, 0, q);
        load_qkv<D, BF, GA>(p, row, h, 1, t);
        lds_put<D, BF>(myK, t);
        load_qkv<D, BF, GA>(p, row, h, 2, t);
        lds_put<D, BF>(myV, t);
    } else {   // rows past the sequence are read by the last key block: zeros, weighted by exp(-inf) = 0
        lds_put<D, BF>(myK, t);
        lds_put<D, BF>(myV, t);
    }
    __syncthreads();
    if (!live) return;
    if constexpr (GA) {
        if (!own && !p.lse) return;   // a copy slot: nothing of it is stored
    }
    const S* Kg = sK + (size_t)g * RP * D;
    const S* Vg = sV + (size_t)g * RP * D;
    float m = -INFINITY, l = 0.f, acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.f;
    for (int j0 = 0; j0 < L; j0 += AT_KB) {
        float s[AT_KB], mb = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < AT_KB; ++jj) {
            const float dot = lds_dot<D, BF>(q, Kg + (size_t)(j0 + jj) * D);
            s[jj] = (j0 + jj < L) ? dot * p.scale : -INFINITY;
            mb = fmaxf(mb, s[jj]);
        }
        const float mn = fmaxf(m, mb);          // finite: key j0 < L is in the block
        const float alpha = exp_nat(m - mn);    // first block: exp(-inf) = 0 on zeros
        l *= alpha;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] *= alpha;
#pragma unroll
        for (int jj = 0; jj < AT_KB; ++jj) {
            const float pj = exp_nat(s[jj] - mn);
            l += pj;
            lds_axpy<D, BF>(pj, Vg + (size_t)(j0 + jj) * D, acc);
        }
        m = mn;
    }
    const float inv = 1.f / l;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] *= inv;
    if constexpr (GA) {
        if (own) {
            store_row_half<D>(p.out, (row * p.H + h) * D, p.io_dtype, acc);
            if (p.out_full) {
                float4* f = reinterpret_cast<float4*>(p.out_full + (row * p.H + h) * D);
#pragma unroll
                for (int c = 0; c < D / 4; ++c) f[c] = make_float4(acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]);
            }
        }
        if (p.lse) p.lse[(int64_t)h * p.total + tok] = m + logf(l);
    } else {
        store_row<D, BF>(p.out + (tok * p.H + h) * D, acc);
        p.lse[(int64_t)h * p.total + tok] = m + logf(l);
    }
}

template <int D, int RP, bool BF, bool GA>
__global__ __launch_bounds__(AT_BLOCK) void attn_bwd_kernel(const AttnP p) {
    using S = typename Store<D>::type;
    constexpr int G = AT_BLOCK / RP;
    __shared__ __attribute__((aligned(16))) S sA[AT_BLOCK * D];   // sweep 1: K rows; sweep 2: Q rows
    __shared__ __attribute__((aligned(16))) S sB[AT_BLOCK * D];   // sweep 1: V rows; sweep 2: dO rows
    __shared__ float sLse[AT_BLOCK], sDel[AT_BLOCK];
    __shared__ int sReal;                                          // GA: the real query rows of the next sequence
    const int HG = (p.H + G - 1) / G;
    const int seq = blockIdx.x / HG, hg = blockIdx.x % HG;
    const int g = threadIdx.x / RP, r = threadIdx.x % RP;
    const int h = hg * G + g;
    int start, L;
    seq_range<RP>(p, seq, start, L);
    if constexpr (!GA) {
        if (seq == p.batch) {
            if (h < p.H)
                for (int row = start + r; row < start + L; row += RP)
#pragma unroll
                    for (int w = 0; w < 3; ++w) zero_row<D>(p.dqkv + (((int64_t)row * 3 + w) * p.H + h) * D);
            return;
        }
    }
    if (L == 0) return;
    const bool live = r < L && h < p.H;
    const int64_t tok = start + r;
    int64_t row = tok;      // GA: the row this slot holds, and whether the slot is that row's own
    bool own = true;
    if constexpr (GA) {
        row = live ? gather_row(p, tok) : -1;
        own = row >= 0 && p.inverse[row] == tok;
        if (threadIdx.x == 0) sReal = 0;
    }
    S* myA = sA + (size_t)(g * RP + r) * D;
    S* myB = sB + (size_t)(g * RP + r) * D;
    const S* Ag = sA + (size_t)g * RP * D;
    const S* Bg = sB + (size_t)g * RP * D;
    float q[D], go[D], t[D];
    float lse_i = 0.f, delta = 0.f;
    if (live) {
        load_qkv<D, BF, GA>(p, row, h, 1, t);
        lds_put<D, BF>(myA, t);
        load_qkv<D, BF, GA>(p, row, h, 2, t);
        lds_put<D, BF>(myB, t);
        load_qkv<D, BF, GA>(p, row, h, 0, q);
        if constexpr (GA) {
            if (own) {
                load_row_half<D>(p.dout, (row * p.H + h) * D, p.io_dtype, go);
                load_row<D>(p.out, (row * p.H + h) * D, p.out_dtype, t);
            } else {   // a copy slot's upstream gradient is zero, and delta with it
#pragma unroll
                for (int d = 0; d < D; ++d) go[d] = 0.f, t[d] = 0.f;
            }
        } else {
            load_row<D, BF>(p.dout + tok * p.d0 + (int64_t)h * p.d1, p.d2, p.dout_vec, go);
            load_row<D, BF>(p.out + (tok * p.H + h) * D, 1, 1, t);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) delta = fmaf(go[d], t[d], delta);
        lse_i = p.lse[(int64_t)h * p.total + tok];
    }
    __syncthreads();
    // sweep 1, thread = query row i: dQ_i = scale sum_j P_ij (dO_i . V_j - delta_i) K_j
    if (live && own) {
        float dq[D];
#pragma unroll
        for (int d = 0; d < D; ++d) dq[d] = 0.f;
        for (int j = 0; j < L; ++j) {
            const float s = lds_dot<D, BF>(q, Ag + (size_t)j * D) * p.scale;
            const float pj = exp_nat(s - lse_i);
            const float dp = lds_dot<D, BF>(go, Bg + (size_t)j * D);
            lds_axpy<D, BF>(pj * (dp - delta), Ag + (size_t)j * D, dq);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) dq[d] *= p.scale;
        if constexpr (GA) store_row_half<D>(p.dqkv, ((row * 3 + 0) * p.H + h) * D, p.io_dtype, dq);
        else store_row<D, BF>(p.dqkv + ((tok * 3 + 0) * p.H + h) * D, dq);
    }
    __syncthreads();
    if (live) {
        lds_put<D, BF>(myA, q);
        lds_put<D, BF>(myB, go);
        sLse[g * RP + r] = lse_i;
        sDel[g * RP + r] = delta;
    }
    __syncthreads();
    if constexpr (!GA) {
        if (!live) return;
    }
    // sweep 2, thread = key row j: dV_j = sum_i P_ij dO_i, dK_j = scale sum_i P_ij (dO_i . V_j - delta_i) Q_i
    float (&k)[D] = q;     // the registers of q and dO now hold this thread's own key and value rows (L2 hits)
    float (&v)[D] = go;
    float dk[D], dv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) dk[d] = 0.f, dv[d] = 0.f;
    const bool mine = live && own;   // (GA: a copy slot's dK and dV are formed by the workgroup of the row's own slot, below)
    if (mine) {
        load_qkv<D, BF, GA>(p, row, h, 1, k);
        load_qkv<D, BF, GA>(p, row, h, 2, v);
        key_sweep<D, BF>(k, v, Ag, Bg, sLse + g * RP, sDel + g * RP, L, p.scale, dk, dv);
    }
    if constexpr (GA) {
        // the reference's padding repeats the tail of a segment's last full sequence in the next one, at the same position:
        // its real queries attend to those keys, and their dK / dV belong to this thread's row
        int start2 = 0, L2 = 0;
        if (seq + 1 < p.batch) seq_range<RP>(p, seq + 1, start2, L2);
        const int64_t tok2 = (int64_t)start2 + r;
        const bool copy = mine && r < L2 && tok2 != tok && gather_row(p, tok2) == row;
        if (__syncthreads_or(copy)) {   // (the barrier: sweep 2 has read the LDS rows that are replaced now)
            if (r < L2 && h < p.H) {
                const int64_t row2 = gather_row(p, tok2);
                const bool own2 = row2 >= 0 && p.inverse[row2] == tok2;
                float d2 = 0.f;
                load_qkv<D, BF, GA>(p, row2, h, 0, t);
                lds_put<D, BF>(myA, t);
                if (own2) load_row_half<D>(p.dout, (row2 * p.H + h) * D, p.io_dtype, t);
                else
#pragma unroll
                    for (int d = 0; d < D; ++d) t[d] = 0.f;
                lds_put<D, BF>(myB, t);
                if (own2) {
                    float o[D];
                    load_row<D>(p.out, (row2 * p.H + h) * D, p.out_dtype, o);
#pragma unroll
                    for (int d = 0; d < D; ++d) d2 = fmaf(t[d], o[d], d2);
                    atomicMax(&sReal, r + 1);
                }
                sLse[g * RP + r] = p.lse[(int64_t)h * p.total + tok2];
                sDel[g * RP + r] = d2;
            }
            __syncthreads();
            // rows from sReal on are copies themselves (dO = 0, delta = 0: no contribution); so is any copy before it
            if (copy) key_sweep<D, BF>(k, v, Ag, Bg, sLse + g * RP, sDel + g * RP, sReal, p.scale, dk, dv);
        }
    }
    if (!mine) return;
#pragma unroll
    for (int d = 0; d < D; ++d) dk[d] *= p.scale;
    if constexpr (GA) {
        store_row_half<D>(p.dqkv, ((row * 3 + 1) * p.H + h) * D, p.io_dtype, dk);
        store_row_half<D>(p.dqkv, ((row * 3 + 2) * p.H + h) * D, p.io_dtype, dv);
    } else {
        store_row<D, BF>(p.dqkv + ((tok * 3 + 1) * p.H + h) * D, dk);
        store_row<D, BF>(p.dqkv + ((tok * 3 + 2) * p.H + h) * D, dv);
    }
}

// NULL if the arguments are inside the envelope
const char* attn_check(const gdr_attn_args* a) {
    if (!a) return "attn: NULL arguments";
    if (a->dtype != GDR_ATTN_F16 && a->dtype != GDR_ATTN_BF16) return "attn: dtype must be GDR_ATTN_F16 or GDR_ATTN_BF16";
    if (a->D != 8 && a->D != 16 && a->D != 32 && a->D != 64) return "attn: head dimension D must be 8, 16, 32 or 64";
    if (a->H < 1) return "attn: H must be >= 1";
    if (a->total < 0 || a->batch < 0) return "attn: negative total or batch";
    if (a->max_seqlen < 1 || a->max_seqlen > GDR_ATTN_MAX_SEQLEN) return "attn: max_seqlen must be in 1..256";
    if (!(a->scale == a->scale) || a->scale - a->scale != 0.f) return "attn: softmax scale is not finite";
    if (((int64_t)a->batch + 1) * a->H > INT64_C(0x7fffffff)) return "attn: batch * H exceeds the launch grid";
    return nullptr;
}

const char* attn_check_fixed(const gdr_attn_args* a, const int32_t* cu) {
    if (cu) return nullptr;
    if (a->fixed_len < 0 || a->fixed_len > a->max_seqlen) return "attn: fixed_len must be in 0..max_seqlen without cu_seqlens";
    if ((int64_t)a->batch * a->fixed_len > a->total) return "attn: batch * fixed_len exceeds total";
    return nullptr;
}

int row_vec(const void* ptr, const int64_t* strides, int n) {   // unit-stride, 16-byte aligned rows of 16-bit words
    if (((uintptr_t)ptr & 15u) || strides[n - 1] != 1) return 0;
    for (int i = 0; i + 1 < n; ++i)
        if (strides[i] % 8) return 0;
    return 1;
}

template <bool BWD, int D, int RP, bool BF, bool GA>
void attn_launch1(const AttnP& p, int blocks, hipStream_t st) {
    if (BWD) hipLaunchKernelGGL((attn_bwd_kernel<D, RP, BF, GA>), dim3(blocks), dim3(AT_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((attn_fwd_kernel<D, RP, BF, GA>), dim3(blocks), dim3(AT_BLOCK), 0, st, p);
}

template <bool BWD, int D, bool BF, bool GA>
void attn_launch_rp(const AttnP& p, int rp, int batch, hipStream_t st) {
    const int G = AT_BLOCK / rp;
    const int blocks = (batch + (GA ? 0 : 1)) * ((p.H + G - 1) / G);   // (the gather form has no rows behind the last sequence)
    if (rp == 64) attn_launch1<BWD, D, 64, BF, GA>(p, blocks, st);
    else if (rp == 128) attn_launch1<BWD, D, 128, BF, GA>(p, blocks, st);
    else attn_launch1<BWD, D, 256, BF, GA>(p, blocks, st);
}

// dtype < 0: the gather form (fp16 arithmetic)
template <bool BWD>
int attn_launch(int D, int max_seqlen, int batch, int dtype, const AttnP& p, hipStream_t st) {
    const int rp = max_seqlen <= 64 ? 64 : (max_seqlen <= 128 ? 128 : 256);
#define GDR_ATTN_D(DD)                                                                       \
    if (dtype < 0) attn_launch_rp<BWD, DD, false, true>(p, rp, batch, st);                   \
    else if (dtype == GDR_ATTN_BF16) attn_launch_rp<BWD, DD, true, false>(p, rp, batch, st); \
    else attn_launch_rp<BWD, DD, false, false>(p, rp, batch, st)
    switch (D) {
        case 8: GDR_ATTN_D(8); break;
        case 16: GDR_ATTN_D(16); break;
        case 32: GDR_ATTN_D(32); break;
        default: GDR_ATTN_D(64); break;
    }
#undef GDR_ATTN_D
    return launch_status(BWD ? "attn_bwd_kernel" : "attn_fwd_kernel");
}

// NULL if the arguments of the gather form are inside the envelope
const char* attn_gather_check(const gdr_attn_gather_args* a) {
    if (!a) return "attn_gather: NULL arguments";
    if (a->dtype != GDR_ATTN_F16 && a->dtype != GDR_ATTN_BF16 && a->dtype != GDR_ATTN_F32)
        return "attn_gather: dtype must be GDR_ATTN_F16, GDR_ATTN_BF16 or GDR_ATTN_F32";
    if (a->D != 8 && a->D != 16 && a->D != 32 && a->D != 64) return "attn_gather: head dimension D must be 8, 16, 32 or 64";
    if (a->H < 1) return "attn_gather: H must be >= 1";
    if (a->N < 0 || a->Tp < 0 || a->batch < 0) return "attn_gather: negative N, Tp or batch";
    if (a->max_seqlen < 1 || a->max_seqlen > GDR_ATTN_MAX_SEQLEN) return "attn_gather: max_seqlen must be in 1..256";
    if (!(a->scale == a->scale) || a->scale - a->scale != 0.f) return "attn_gather: softmax scale is not finite";
    if (((int64_t)a->batch + 1) * a->H > INT64_C(0x7fffffff)) return "attn_gather: batch * H exceeds the launch grid";
    return nullptr;
}

AttnP attn_gather_params(const gdr_attn_gather_args* a, const void* qkv, const int64_t* order, const int64_t* inverse,
                         const int32_t* cu_seqlens) {
    AttnP p = {};
    p.qkv = (const uint16_t*)qkv; p.cu = cu_seqlens; p.order = order; p.inverse = inverse;
    p.total = a->Tp; p.batch = a->batch; p.H = a->H; p.N = a->N; p.io_dtype = a->dtype;
    p.scale = a->scale;
    return p;
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_attn_lse_bytes(const gdr_attn_args* a) {
    if (const char* why = attn_check(a)) { invalid_arg(why); return 0; }
    return (size_t)a->H * (size_t)a->total * sizeof(float);
}

int gdr_attn_forward(const gdr_attn_args* a, const void* qkv, const int64_t* qkv_strides, const int32_t* cu_seqlens,
                     void* out, float* lse, void* stream) {
    if (const char* why = attn_check(a)) return invalid_arg(why);
    if (const char* why = attn_check_fixed(a, cu_seqlens)) return invalid_arg(why);
    if (!qkv_strides) return invalid_arg("attn_forward: NULL strides");
    if (a->total == 0) return GDR_OK;
    if (!qkv || !out || !lse) return invalid_arg("attn_forward: NULL argument");
    if (misaligned(out, 15) || misaligned(lse, 3) || misaligned(qkv, 1)) return invalid_arg("attn_forward: unaligned buffer");
    AttnP p = {};
    p.qkv = (const uint16_t*)qkv; p.cu = cu_seqlens; p.out = (uint16_t*)out; p.lse = lse;
    p.q0 = qkv_strides[0]; p.q1 = qkv_strides[1]; p.q2 = qkv_strides[2]; p.q3 = qkv_strides[3];
    p.total = a->total; p.batch = a->batch; p.H = a->H; p.fixed_len = a->fixed_len;
    p.qkv_vec = row_vec(qkv, qkv_strides, 4);
    p.scale = a->scale;
    return attn_launch<false>(a->D, a->max_seqlen, a->batch, a->dtype, p, (hipStream_t)stream);
}

int gdr_attn_backward(const gdr_attn_args* a, const void* dout, const int64_t* dout_strides, const void* qkv,
                      const int64_t* qkv_strides, const int32_t* cu_seqlens, const void* out, const float* lse, void* dqkv,
                      void* stream) {
    if (const char* why = attn_check(a)) return invalid_arg(why);
    if (const char* why = attn_check_fixed(a, cu_seqlens)) return invalid_arg(why);
    if (!qkv_strides || !dout_strides) return invalid_arg("attn_backward: NULL strides");
    if (a->total == 0) return GDR_OK;
    if (!dout || !qkv || !out || !lse || !dqkv) return invalid_arg("attn_backward: NULL argument");
    if (misaligned(out, 15) || misaligned(dqkv, 15) || misaligned(lse, 3) || misaligned(qkv, 1) || misaligned(dout, 1))
        return invalid_arg("attn_backward: unaligned buffer");
    AttnP p = {};
    p.qkv = (const uint16_t*)qkv; p.cu = cu_seqlens; p.out = (uint16_t*)out; p.lse = (float*)lse;
    p.dout = (const uint16_t*)dout; p.dqkv = (uint16_t*)dqkv;
    p.q0 = qkv_strides[0]; p.q1 = qkv_strides[1]; p.q2 = qkv_strides[2]; p.q3 = qkv_strides[3];
    p.d0 = dout_strides[0]; p.d1 = dout_strides[1]; p.d2 = dout_strides[2];
    p.total = a->total; p.batch = a->batch; p.H = a->H; p.fixed_len = a->fixed_len;
    p.qkv_vec = row_vec(qkv, qkv_strides, 4);
    p.dout_vec = row_vec(dout, dout_strides, 3);
    p.scale = a->scale;
    return attn_launch<true>(a->D, a->max_seqlen, a->batch, a->dtype, p, (hipStream_t)stream);
}

int gdr_attn_gather_forward(const gdr_attn_gather_args* a, const void* qkv, const int64_t* order, const int64_t* inverse,
                            const int32_t* cu_seqlens, void* out, float* out_full, float* lse, void* stream) {
    if (const char* why = attn_gather_check(a)) return invalid_arg(why);
    if (a->N == 0 || a->Tp == 0 || a->batch == 0) return GDR_OK;
    if (!qkv || !order || !inverse || !cu_seqlens || !out) return invalid_arg("attn_gather_forward: NULL argument");
    if (misaligned(qkv, 15) || misaligned(out, 15) || misaligned(out_full, 15) || misaligned(lse, 3) || misaligned(order, 7) ||
        misaligned(inverse, 7) || misaligned(cu_seqlens, 3))
        return invalid_arg("attn_gather_forward: unaligned buffer");
    AttnP p = attn_gather_params(a, qkv, order, inverse, cu_seqlens);
    p.out = (uint16_t*)out; p.out_full = out_full; p.lse = lse;
    return attn_launch<false>(a->D, a->max_seqlen, a->batch, -1, p, (hipStream_t)stream);
}

int gdr_attn_gather_backward(const gdr_attn_gather_args* a, const void* dout, const void* qkv, const int64_t* order,
                             const int64_t* inverse, const int32_t* cu_seqlens, const void* out, int32_t out_dtype,
                             const float* lse, void* dqkv, void* stream) {
    if (const char* why = attn_gather_check(a)) return invalid_arg(why);
    if (out_dtype != GDR_ATTN_F16 && out_dtype != GDR_ATTN_BF16 && out_dtype != GDR_ATTN_F32)
        return invalid_arg("attn_gather_backward: out_dtype must be GDR_ATTN_F16, GDR_ATTN_BF16 or GDR_ATTN_F32");
    if (a->N == 0 || a->Tp == 0 || a->batch == 0) return GDR_OK;
    if (!dout || !qkv || !order || !inverse || !cu_seqlens || !out || !lse || !dqkv)
        return invalid_arg("attn_gather_backward: NULL argument");
    if (misaligned(qkv, 15) || misaligned(out, 15) || misaligned(dout, 15) || misaligned(dqkv, 15) || misaligned(lse, 3) ||
        misaligned(order, 7) || misaligned(inverse, 7) || misaligned(cu_seqlens, 3))
        return invalid_arg("attn_gather_backward: unaligned buffer");
    AttnP p = attn_gather_params(a, qkv, order, inverse, cu_seqlens);
    p.out = (uint16_t*)out; p.out_dtype = out_dtype; p.lse = (float*)lse;
    p.dout = (const uint16_t*)dout; p.dqkv = (uint16_t*)dqkv;
    return attn_launch<true>(a->D, a->max_seqlen, a->batch, -1, p, (hipStream_t)stream);
}

}  // extern "C"

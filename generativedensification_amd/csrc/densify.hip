// densify.hip — the densification masks of the point decoder (include/gdr.h gdr_densify_*): what the reference's MaskModule /
// MaskResModule do between scoring the points and handing them to the next upscale stage.
//
//   select   per segment b (rows ends[b - 1] .. ends[b] - 1, ends = the offsets clamped to [previous end, N]) the rows are
//            ranked by descending value: NaN above every number, -0 = +0, equal values by ascending row.
//              top-k  rank < k_b, k_b = ceil(round_any(ratio * round_any(n_b))) in f32 (the reference's
//                     (float(ratio) * num_nodes.to(x.dtype)).ceil()); k_b > n_b or not finite selects the whole segment
//              top-p  round_any(prefix_j) <= threshold, prefix_j the inclusive f32 sum of the segment's values in ranked order
//            Rows at or behind ends[B - 1] are never selected.  new_offset = the cumulative number selected per segment.
//   gate     forward out = feat (no mask) or feat * mask; backward dfeat = prob * g, dprob[i] = sum_c feat[i, c] * g[i, c] in f32.
//   split    dest[i] = the number of rows before i on i's side of the mask; row i of coord / feat goes to row dest[i] of the
//            selected or of the remaining output; the backward gathers through the same table (a permutation: no atomics).
//
// Route of select: a 64-bit key per row, (segment << 32) | ~orderable(x) with orderable = the sign-flip transform of the f32
// bits (negative: all bits flipped, else the sign bit set; -0 first canonicalised to +0; NaN -> 0xffffffff), rows behind the
// last end in segment B.  The f32 form of a bf16 (f16) value has 16 (13) zero bits at its low end, so only the v = 16 (19) high
// bits of ~orderable enter its key: (segment << v) | (~orderable >> (32 - v)).  gdr_serial_sort (stable, least significant
// digit first) on v + bits(B) bits then gives every row its position in the ranking with ties by ascending row; because
// segments are contiguous both in row order and in sorted order, rank = position - ends[b - 1].
//
// The scan of top-p has one fixed tree.  The operands are pairs (f, v): f = "a segment starts inside the span", v = the sum
// from the last such start (or the span's start) to its end; (a . b) = (a.f | b.f, b.f ? b.v : a.v + b.v).
//   chunk   DN_CHUNK = 1024 sorted positions per workgroup: a thread folds its 4 positions in order (3 additions), the 256
//           thread totals are scanned by Hillis-Steele steps (8), the exclusive thread prefix joins the thread's own (1)
//   level 1 the chunk totals in groups of DN_FAN = 1024, Hillis-Steele (10);  level 2 the group totals, at most 1024 (10)
//   result  prefix_j = (level 2 . level 1) . in-chunk (2)
// so no path holds more than 34 f32 additions, whatever N.  No atomics anywhere: two runs are bitwise equal.
//
// Bounds: ends are clamped on the device before anything reads them; every row, position, chunk and group index is checked
// against its count; the split kernels bound every store by the capacities they are passed.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"

namespace gdr {
namespace {

constexpr int DN_BLOCK = 256;
constexpr int DN_ITEMS = 4;
constexpr int DN_CHUNK = DN_BLOCK * DN_ITEMS;   // rows / sorted positions per workgroup of the scans
constexpr int DN_FAN = 1024;                    // entries per workgroup of a carry level, and the workgroup of the segment tables
constexpr int64_t DN_MAX_ROWS = GDR_SERIAL_MAX_POINTS;

struct FV { int f; float v; };
__device__ __forceinline__ FV join(FV a, FV b) { return FV{a.f | b.f, b.f ? b.v : a.v + b.v}; }

// inclusive scan of one FV per thread over the NT threads of the workgroup (sf, sv: NT entries of LDS each)
template <int NT>
__device__ __forceinline__ FV block_scan(FV x, int* sf, float* sv) {
    const int t = threadIdx.x;
    sf[t] = x.f; sv[t] = x.v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        FV a = {0, 0.f};
        const bool has = t >= d;
        if (has) { a.f = sf[t - d]; a.v = sv[t - d]; }
        __syncthreads();
        if (has) { x = join(a, x); sf[t] = x.f; sv[t] = x.v; }
        __syncthreads();
    }
    return x;
}

// inclusive scan of one int64 per thread over the DN_FAN threads of the workgroup; MAX: running maximum, else running sum
template <bool MAX>
__device__ __forceinline__ int64_t block_scan_i64(int64_t x, int64_t* sh) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int d = 1; d < DN_FAN; d <<= 1) {
        const bool has = t >= d;
        const int64_t a = has ? sh[t - d] : 0;
        __syncthreads();
        if (has) { x = MAX ? (a > x ? a : x) : a + x; sh[t] = x; }
        __syncthreads();
    }
    return x;
}

struct SelP {
    const void* x; const int64_t* offset; const int64_t* order; const int64_t* inverse;
    int64_t* starts;      // B + 2: 0, the B clamped ends, N
    int64_t* kcap;        // B: min(k_b, n_b) (top-k)
    int64_t* cnt;         // B: rows selected per segment (top-p)
    int64_t* keys; uint8_t* mask; int64_t* new_offset;
    int* c_f; float* c_v;      // chunk totals
    int* e1_f; float* e1_v;    // exclusive prefix of a chunk inside its group
    int* g_f; float* g_v;      // group totals
    int* e2_f; float* e2_v;    // exclusive prefix of a group
    int* t_f; float* t_v;      // the total of level 2 (unused)
    int64_t N;
    int32_t B, x_dt, mode, nchunks, ngroups;
    float ratio, threshold;
};

// the high bits of the orderable value that can differ: the f32 form of a bf16 has 16 zero bits below them, that of an f16 13
__host__ __device__ __forceinline__ int value_bits(int dt) { return dt == GDR_NORM_F32 ? 32 : (dt == GDR_NORM_BF16 ? 16 : 19); }

// the number of segment ends <= pos: the segment of row / sorted position pos, B behind the last end (starts non-decreasing)
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ starts, int B, int64_t pos) {
    int lo = 0, hi = B;
    for (int k = 0; k < 16 && lo < hi; ++k) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid + 1] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one workgroup of DN_FAN threads: the clamped ends, k_b and (top-k) new_offset
__global__ __launch_bounds__(DN_FAN) void dn_segments_kernel(const SelP p) {
    __shared__ int64_t sh[DN_FAN];
    const int t = threadIdx.x;
    int64_t v = 0;
    if (t < p.B) { v = p.offset[t]; v = v < 0 ? 0 : (v > p.N ? p.N : v); }
    const int64_t end = block_scan_i64<true>(v, sh);
    __syncthreads();
    sh[t] = end;
    __syncthreads();
    const int64_t start = t ? sh[t - 1] : 0;
    __syncthreads();
    int64_t kk = 0;
    if (t < p.B) {
        const int64_t n = end - start;
        const float nr = round_any((float)n, p.x_dt);
        const float k = ceilf(round_any(p.ratio * nr, p.x_dt));
        kk = (k >= 0.f && k < 4.0e18f) ? (int64_t)k : n;       // (inf and NaN: the whole segment, as k > n)
        if (kk > n) kk = n;
        p.starts[t + 1] = end;
        p.kcap[t] = kk;
        if (t == p.B - 1) p.starts[p.B + 1] = p.N;
    }
    if (t == 0) p.starts[0] = 0;
    const int64_t total = block_scan_i64<false>(kk, sh);
    if (t < p.B && p.mode == GDR_DENSIFY_TOP_K) p.new_offset[t] = total;
}

__global__ __launch_bounds__(DN_BLOCK) void dn_encode_kernel(const SelP p) {
    const int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= p.N) return;
    uint32_t u = __float_as_uint(load1(p.x, i, p.x_dt));
    uint32_t ord;
    if ((u & 0x7fffffffu) > 0x7f800000u) ord = 0xffffffffu;
    else {
        if ((u << 1) == 0u) u = 0u;
        ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    const uint64_t seg = (uint64_t)seg_of(p.starts, p.B, i);
    const int vb = value_bits(p.x_dt);
    p.keys[i] = (int64_t)((seg << vb) | (uint64_t)(~ord >> (32 - vb)));
}

__global__ __launch_bounds__(DN_BLOCK) void dn_topk_mask_kernel(const SelP p) {
    const int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= p.N) return;
    const int b = seg_of(p.starts, p.B, i);
    p.mask[i] = (b < p.B && p.inverse[i] - p.starts[b] < p.kcap[b]) ? 1 : 0;
}

// the in-chunk part of the top-p scan: the thread's DN_ITEMS inclusive prefixes inside the chunk, and the chunk total
struct ChunkScan { FV incl[DN_ITEMS]; int64_t row[DN_ITEMS]; int seg[DN_ITEMS]; FV total; };

__device__ __forceinline__ void chunk_scan(const SelP& p, int* sf, float* sv, ChunkScan& c) {
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * DN_CHUNK + (int64_t)t * DN_ITEMS;
    FV run = {0, 0.f};
#pragma unroll
    for (int q = 0; q < DN_ITEMS; ++q) {
        const int64_t j = j0 + q;
        FV e = {0, 0.f};
        c.row[q] = -1; c.seg[q] = p.B;
        if (j < p.N) {
            int64_t r = p.order[j];
            r = r < 0 ? 0 : (r >= p.N ? p.N - 1 : r);
            const int b = seg_of(p.starts, p.B, j);
            c.row[q] = r; c.seg[q] = b;
            e.f = p.starts[b] == j;
            e.v = load1(p.x, r, p.x_dt);
        }
        run = q ? join(run, e) : e;
        c.incl[q] = run;
    }
    const FV inc = block_scan<DN_BLOCK>(run, sf, sv);
    FV ex = {0, 0.f};
    if (t) { ex.f = sf[t - 1]; ex.v = sv[t - 1]; }
    c.total.f = sf[DN_BLOCK - 1]; c.total.v = sv[DN_BLOCK - 1];
    (void)inc;
    if (t) {
#pragma unroll
        for (int q = 0; q < DN_ITEMS; ++q) c.incl[q] = join(ex, c.incl[q]);
    }
}

__global__ __launch_bounds__(DN_BLOCK) void dn_chunk_total_kernel(const SelP p) {
    __shared__ int sf[DN_BLOCK];
    __shared__ float sv[DN_BLOCK];
    ChunkScan c;
    chunk_scan(p, sf, sv, c);
    if (threadIdx.x == 0) { p.c_f[blockIdx.x] = c.total.f; p.c_v[blockIdx.x] = c.total.v; }
}

// one carry level: the m entries (in_f, in_v) in groups of DN_FAN -> the exclusive prefix of every entry inside its group and
// the total of every group
__global__ __launch_bounds__(DN_FAN) void dn_level_kernel(const int* __restrict__ in_f, const float* __restrict__ in_v, int m,
                                                          int* __restrict__ ex_f, float* __restrict__ ex_v,
                                                          int* __restrict__ tot_f, float* __restrict__ tot_v) {
    __shared__ int sf[DN_FAN];
    __shared__ float sv[DN_FAN];
    const int t = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * DN_FAN + t;
    FV x = {0, 0.f};
    if (e < m) { x.f = in_f[e]; x.v = in_v[e]; }
    block_scan<DN_FAN>(x, sf, sv);
    if (e < m) {
        ex_f[e] = t ? sf[t - 1] : 0;
        ex_v[e] = t ? sv[t - 1] : 0.f;
    }
    if (t == DN_FAN - 1) { tot_f[blockIdx.x] = sf[t]; tot_v[blockIdx.x] = sv[t]; }
}

__global__ __launch_bounds__(DN_BLOCK) void dn_topp_mask_kernel(const SelP p) {
    __shared__ int sf[DN_BLOCK];
    __shared__ float sv[DN_BLOCK];
    ChunkScan c;
    chunk_scan(p, sf, sv, c);
    const int ch = blockIdx.x, g = ch / DN_FAN;
    const FV carry = join(FV{p.e2_f[g], p.e2_v[g]}, FV{p.e1_f[ch], p.e1_v[ch]});
#pragma unroll
    for (int q = 0; q < DN_ITEMS; ++q) {
        if (c.row[q] < 0) continue;
        const FV pre = join(carry, c.incl[q]);
        p.mask[c.row[q]] = (c.seg[q] < p.B && round_any(pre.v, p.x_dt) <= p.threshold) ? 1 : 0;
    }
}

// rows selected in segment blockIdx.x
__global__ __launch_bounds__(DN_BLOCK) void dn_count_kernel(const SelP p) {
    __shared__ int64_t sh[DN_BLOCK];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t a = p.starts[b], e = p.starts[b + 1];
    int64_t n = 0;
    for (int64_t i = a + t; i < e; i += DN_BLOCK) n += p.mask[i] ? 1 : 0;
    sh[t] = n;
    __syncthreads();
    for (int d = DN_BLOCK / 2; d > 0; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    if (t == 0) p.cnt[b] = sh[0];
}

__global__ __launch_bounds__(DN_FAN) void dn_offset_kernel(const SelP p) {
    __shared__ int64_t sh[DN_FAN];
    const int t = threadIdx.x;
    const int64_t total = block_scan_i64<false>(t < p.B ? p.cnt[t] : 0, sh);
    if (t < p.B) p.new_offset[t] = total;
}

// ---- gate and split ------------------------------------------------------------------------------------------------------------
struct RowP {
    const uint8_t* mask; const int64_t* dest;     // dest NULL: every row stays where it is (the gate)
    const void* feat; const void* prob; const void* g_sel; const void* g_rest;
    const void* coord; const void* gc_sel; const void* gc_rest;
    void* out_sel; void* out_rest; void* coord_sel; void* coord_rest;
    void* dfeat; void* dprob; void* dcoord;
    int64_t N, n_sel, n_rest, feat_stride, g_stride;
    int32_t C, lc_shift, feat_dt, prob_dt, out_dt, D, es;
};

__device__ __forceinline__ void copy_elem(void* dst, int64_t di, const void* src, int64_t si, int es) {
    if (es == 4) ((uint32_t*)dst)[di] = ((const uint32_t*)src)[si];
    else if (es == 8) ((uint64_t*)dst)[di] = ((const uint64_t*)src)[si];
    else if (es == 2) ((uint16_t*)dst)[di] = ((const uint16_t*)src)[si];
    else ((uint8_t*)dst)[di] = ((const uint8_t*)src)[si];
}
__device__ __forceinline__ void zero_elem(void* dst, int64_t di, int es) {
    if (es == 4) ((uint32_t*)dst)[di] = 0u;
    else if (es == 8) ((uint64_t*)dst)[di] = 0ull;
    else if (es == 2) ((uint16_t*)dst)[di] = 0;
    else ((uint8_t*)dst)[di] = 0;
}

// gate forward: out[row] = feat[row], or zero where the mask is false
template <int K>
__global__ __launch_bounds__(DN_BLOCK) void dn_gate_fwd_kernel(const RowP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (DN_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N) return;
    const bool keep = !p.mask || p.mask[row];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (l + k * lc) * 8;
        if (c0 >= p.C) continue;
        float x[8];
        if (keep) load8(p.feat, row * p.feat_stride + c0, p.feat_dt, x);
        else {
#pragma unroll
            for (int v = 0; v < 8; ++v) x[v] = 0.f;
        }
        store8(p.out_sel, row * p.C + c0, p.out_dt, x);
    }
}

// split forward: row -> row dest[row] of its side, if that lies inside the side's capacity
template <int K>
__global__ __launch_bounds__(DN_BLOCK) void dn_split_fwd_kernel(const RowP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (DN_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N) return;
    const bool sel = p.mask[row] != 0;
    const int64_t d = p.dest[row], cap = sel ? p.n_sel : p.n_rest;
    if (d < 0 || d >= cap) return;
    void* out = sel ? p.out_sel : p.out_rest;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (l + k * lc) * 8;
        if (c0 >= p.C) continue;
        float x[8];
        load8(p.feat, row * p.feat_stride + c0, p.feat_dt, x);
        store8(out, d * p.C + c0, p.out_dt, x);
    }
    void* cout = sel ? p.coord_sel : p.coord_rest;
    for (int e = l; e < p.D; e += lc) copy_elem(cout, d * p.D + e, p.coord, row * p.D + e, p.es);
}

// the backward of the gate and of the split: g = the gradient row of `row` (its own row, or row dest[row] of its side; zero
// if that lies outside the capacity); dfeat = prob * g (g without prob), dprob = sum_c feat * g, dcoord = the coord gradient row
template <int K>
__global__ __launch_bounds__(DN_BLOCK) void dn_rows_bwd_kernel(const RowP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (DN_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N) return;                        // (whole groups leave: the butterflies stay inside a group)
    bool sel = true, live = true;
    int64_t d = row;
    if (p.dest) {
        sel = p.mask[row] != 0;
        d = p.dest[row];
        live = d >= 0 && d < (sel ? p.n_sel : p.n_rest);
    }
    const void* g = sel ? p.g_sel : p.g_rest;
    const float pr = p.prob ? load1(p.prob, row, p.prob_dt) : 1.0f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (l + k * lc) * 8;
        if (c0 >= p.C) continue;
        float gv[8];
        if (live) load8(g, d * p.g_stride + c0, p.out_dt, gv);
        else {
#pragma unroll
            for (int v = 0; v < 8; ++v) gv[v] = 0.f;
        }
        if (p.dprob) {
            float f[8];
            load8(p.feat, row * p.feat_stride + c0, p.feat_dt, f);
#pragma unroll
            for (int v = 0; v < 8; ++v) s += f[v] * gv[v];
        }
        if (p.dfeat) {
            if (p.prob) {
#pragma unroll
                for (int v = 0; v < 8; ++v) gv[v] *= pr;
            }
            store8(p.dfeat, row * p.C + c0, p.feat_dt, gv);
        }
    }
    if (p.dprob) {
        s = group_sum(s, lc);
        if (l == 0) store1(p.dprob, row, p.prob_dt, s);
    }
    if (p.dcoord) {
        const void* gc = sel ? p.gc_sel : p.gc_rest;
        for (int e = l; e < p.D; e += lc) {
            if (live) copy_elem(p.dcoord, row * p.D + e, gc, d * p.D + e, p.es);
            else zero_elem(p.dcoord, row * p.D + e, p.es);
        }
    }
}

// the scan of the mask: rows selected per chunk; their exclusive prefix and the total; the destination of every row
__global__ __launch_bounds__(DN_BLOCK) void dn_mask_count_kernel(const uint8_t* __restrict__ mask, int64_t N, int32_t* __restrict__ cc) {
    __shared__ int sh[DN_BLOCK];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * DN_CHUNK + (int64_t)t * DN_ITEMS;
    int n = 0;
#pragma unroll
    for (int q = 0; q < DN_ITEMS; ++q)
        if (i0 + q < N) n += mask[i0 + q] ? 1 : 0;
    sh[t] = n;
    __syncthreads();
    for (int d = DN_BLOCK / 2; d > 0; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    if (t == 0) cc[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(DN_FAN) void dn_mask_base_kernel(const int32_t* __restrict__ cc, int nchunks, int64_t* __restrict__ cbase,
                                                              int64_t* __restrict__ count) {
    __shared__ int64_t sh[DN_FAN];
    const int t = threadIdx.x;
    int64_t carry = 0;
    for (int base = 0; base < nchunks; base += DN_FAN) {
        const int c = base + t;
        const int64_t v = c < nchunks ? cc[c] : 0;
        const int64_t inc = block_scan_i64<false>(v, sh);
        if (c < nchunks) cbase[c] = carry + inc - v;
        carry += sh[DN_FAN - 1];
        __syncthreads();
    }
    if (t == 0) *count = carry;
}

__global__ __launch_bounds__(DN_BLOCK) void dn_mask_dest_kernel(const uint8_t* __restrict__ mask, int64_t N,
                                                                const int64_t* __restrict__ cbase, int64_t* __restrict__ dest) {
    __shared__ int sh[DN_BLOCK];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * DN_CHUNK + (int64_t)t * DN_ITEMS;
    bool m[DN_ITEMS];
    int n = 0;
#pragma unroll
    for (int q = 0; q < DN_ITEMS; ++q) {
        m[q] = i0 + q < N && mask[i0 + q];
        n += m[q] ? 1 : 0;
    }
    int x = n;
    sh[t] = x;
    __syncthreads();
    for (int d = 1; d < DN_BLOCK; d <<= 1) {
        const int a = t >= d ? sh[t - d] : 0;
        __syncthreads();
        x += a;
        sh[t] = x;
        __syncthreads();
    }
    int64_t before = cbase[blockIdx.x] + (x - n);      // selected rows before row i0
#pragma unroll
    for (int q = 0; q < DN_ITEMS; ++q) {
        const int64_t i = i0 + q;
        if (i < N) dest[i] = m[q] ? before : i - before;
        before += m[q] ? 1 : 0;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int check_rows(int64_t N, int64_t C) {
    if (N < 0) return invalid_arg("densify: N must be >= 0");
    if (N > DN_MAX_ROWS) return unsupported("densify: N must be at most 2^30");
    if (C < 8 || C > GDR_DENSIFY_MAX_CHANNELS || C % 8) return unsupported("densify: C must be a multiple of 8 in 8..GDR_DENSIFY_MAX_CHANNELS");
    return GDR_OK;
}

int check_select(int64_t N, int64_t B) {
    if (N < 0 || B < 1) return invalid_arg("densify_select: N must be >= 0 and B >= 1");
    if (N > DN_MAX_ROWS) return unsupported("densify_select: N must be at most 2^30");
    if (B > GDR_DENSIFY_MAX_SEGMENTS) return unsupported("densify_select: B must be at most GDR_DENSIFY_MAX_SEGMENTS");
    return GDR_OK;
}

struct SelWs { size_t starts, kcap, cnt, keys, order, inverse, sort, sort_bytes, c_f, c_v, e1_f, e1_v, g_f, g_v, e2_f, e2_v, t_f, t_v, bytes; };

SelWs select_workspace(int64_t N, int64_t B) {
    SelWs w;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t here = at; at += align_up(n); return here; };
    const size_t nchunks = (size_t)div_up(N, DN_CHUNK), ngroups = (size_t)div_up((int64_t)nchunks, DN_FAN);
    w.starts = take((size_t)(B + 2) * 8); w.kcap = take((size_t)B * 8); w.cnt = take((size_t)B * 8);
    w.keys = take((size_t)N * 8); w.order = take((size_t)N * 8); w.inverse = take((size_t)N * 8);
    w.sort_bytes = gdr_serial_sort_bytes(1, N);
    w.sort = take(w.sort_bytes);
    w.c_f = take(nchunks * 4); w.c_v = take(nchunks * 4); w.e1_f = take(nchunks * 4); w.e1_v = take(nchunks * 4);
    w.g_f = take(ngroups * 4); w.g_v = take(ngroups * 4); w.e2_f = take(ngroups * 4); w.e2_v = take(ngroups * 4);
    w.t_f = take(4); w.t_v = take(4);
    w.bytes = at;
    return w;
}

struct SplitWs { size_t cc, cbase, bytes; };

SplitWs split_workspace(int64_t N) {
    SplitWs w;
    const size_t nchunks = (size_t)div_up(N, DN_CHUNK);
    w.cc = 0;
    w.cbase = align_up(nchunks * 4);
    w.bytes = w.cbase + align_up(nchunks * 8);
    return w;
}

bool bad_elem(int32_t es) { return es != 1 && es != 2 && es != 4 && es != 8; }

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_densify_select_bytes(int64_t N, int32_t B) {
    if (check_select(N, B)) return 0;
    return select_workspace(N, B).bytes + 256;     // (never 0 for valid arguments)
}

int gdr_densify_select(const void* x, int32_t x_dtype, const int64_t* offset, int64_t N, int32_t B, int32_t mode, float ratio,
                       float threshold, void* workspace, size_t workspace_bytes, uint8_t* mask, int64_t* new_offset, void* stream) {
    if (const int rc = check_select(N, B)) return rc;
    if (bad_dtype(x_dtype)) return invalid_arg("densify_select: unknown dtype");
    if (mode != GDR_DENSIFY_TOP_K && mode != GDR_DENSIFY_TOP_P) return invalid_arg("densify_select: unknown mode");
    if (!(ratio > 0.f && ratio < 1.f)) return invalid_arg("densify_select: ratio must lie in (0, 1)");
    if (!(threshold >= 0.f && threshold <= 1.f)) return invalid_arg("densify_select: threshold must lie in [0, 1]");
    if (!offset || !new_offset || !workspace || (N && (!x || !mask))) return invalid_arg("densify_select: NULL argument");
    if (misaligned(x, esize(x_dtype) - 1) || misaligned(offset, 7) || misaligned(new_offset, 7) || misaligned(workspace, 255))
        return invalid_arg("densify_select: unaligned buffer");
    const SelWs ws = select_workspace(N, B);
    if (workspace_bytes < ws.bytes) return workspace_too_small("densify_select: workspace smaller than gdr_densify_select_bytes");
    char* base = (char*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    SelP p = {};
    p.x = x; p.offset = offset; p.mask = mask; p.new_offset = new_offset;
    p.starts = (int64_t*)(base + ws.starts); p.kcap = (int64_t*)(base + ws.kcap); p.cnt = (int64_t*)(base + ws.cnt);
    p.keys = (int64_t*)(base + ws.keys);
    int64_t* order = (int64_t*)(base + ws.order);
    int64_t* inverse = (int64_t*)(base + ws.inverse);
    p.order = order; p.inverse = inverse;
    p.c_f = (int*)(base + ws.c_f); p.c_v = (float*)(base + ws.c_v); p.e1_f = (int*)(base + ws.e1_f); p.e1_v = (float*)(base + ws.e1_v);
    p.g_f = (int*)(base + ws.g_f); p.g_v = (float*)(base + ws.g_v); p.e2_f = (int*)(base + ws.e2_f); p.e2_v = (float*)(base + ws.e2_v);
    p.t_f = (int*)(base + ws.t_f); p.t_v = (float*)(base + ws.t_v);
    p.N = N; p.B = B; p.x_dt = x_dtype; p.mode = mode; p.ratio = ratio; p.threshold = threshold;
    p.nchunks = div_up(N, DN_CHUNK); p.ngroups = div_up(p.nchunks, DN_FAN);
    hipLaunchKernelGGL(dn_segments_kernel, dim3(1), dim3(DN_FAN), 0, st, p);
    if (N == 0) {
        if (mode == GDR_DENSIFY_TOP_P) {
            if (hipMemsetAsync(new_offset, 0, (size_t)B * 8, st) != hipSuccess) return launch_status("densify_select memset");
        }
        return launch_status("densify dn_segments_kernel");
    }
    const dim3 rows((uint32_t)div_up(N, DN_BLOCK));
    hipLaunchKernelGGL(dn_encode_kernel, rows, dim3(DN_BLOCK), 0, st, p);
    if (const int rc = launch_status("densify dn_encode_kernel")) return rc;
    int seg_bits = 0;
    while ((1 << seg_bits) <= B) ++seg_bits;       // segments 0 .. B
    if (const int rc = gdr_serial_sort(p.keys, 1, N, value_bits(x_dtype) + seg_bits, base + ws.sort, ws.sort_bytes, order, inverse, stream)) return rc;
    if (mode == GDR_DENSIFY_TOP_K) {
        hipLaunchKernelGGL(dn_topk_mask_kernel, rows, dim3(DN_BLOCK), 0, st, p);
        return launch_status("densify dn_topk_mask_kernel");
    }
    const dim3 chunks((uint32_t)p.nchunks);
    hipLaunchKernelGGL(dn_chunk_total_kernel, chunks, dim3(DN_BLOCK), 0, st, p);
    hipLaunchKernelGGL(dn_level_kernel, dim3((uint32_t)p.ngroups), dim3(DN_FAN), 0, st, p.c_f, p.c_v, p.nchunks, p.e1_f, p.e1_v, p.g_f,
                       p.g_v);
    hipLaunchKernelGGL(dn_level_kernel, dim3(1), dim3(DN_FAN), 0, st, p.g_f, p.g_v, p.ngroups, p.e2_f, p.e2_v, p.t_f, p.t_v);
    hipLaunchKernelGGL(dn_topp_mask_kernel, chunks, dim3(DN_BLOCK), 0, st, p);
    hipLaunchKernelGGL(dn_count_kernel, dim3((uint32_t)B), dim3(DN_BLOCK), 0, st, p);
    hipLaunchKernelGGL(dn_offset_kernel, dim3(1), dim3(DN_FAN), 0, st, p);
    return launch_status("densify top-p kernels");
}

int gdr_densify_gate_forward(const void* feat, int64_t feat_stride, int32_t feat_dtype, const uint8_t* mask, int64_t N, int32_t C,
                             void* out, int32_t out_dtype, void* stream) {
    if (const int rc = check_rows(N, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(out_dtype)) return invalid_arg("densify_gate_forward: unknown dtype");
    if (N == 0) return GDR_OK;
    if (!feat || !out) return invalid_arg("densify_gate_forward: NULL argument");
    if (bad_rows(feat, feat_stride, C) || misaligned(out, 15))
        return invalid_arg("densify_gate_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    RowP p = {};
    p.mask = mask; p.feat = feat; p.out_sel = out; p.N = N; p.feat_stride = feat_stride; p.C = C; p.feat_dt = feat_dtype;
    p.out_dt = out_dtype;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = DN_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((N + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    if (K == 1) hipLaunchKernelGGL(dn_gate_fwd_kernel<1>, grid, dim3(DN_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(dn_gate_fwd_kernel<2>, grid, dim3(DN_BLOCK), 0, st, p);
    return launch_status("densify dn_gate_fwd_kernel");
}

size_t gdr_densify_split_bytes(int64_t N) {
    if (N < 0 || N > DN_MAX_ROWS) {
        invalid_arg("densify_split_bytes: N outside the envelope");
        return 0;
    }
    return split_workspace(N).bytes + 256;         // (never 0 for valid arguments)
}

int gdr_densify_split_scan(const uint8_t* mask, int64_t N, void* workspace, size_t workspace_bytes, int64_t* dest, int64_t* count,
                           void* stream) {
    if (N < 0) return invalid_arg("densify_split_scan: N must be >= 0");
    if (N > DN_MAX_ROWS) return unsupported("densify_split_scan: N must be at most 2^30");
    if (!count || !workspace || (N && (!mask || !dest))) return invalid_arg("densify_split_scan: NULL argument");
    if (misaligned(dest, 7) || misaligned(count, 7) || misaligned(workspace, 255)) return invalid_arg("densify_split_scan: unaligned buffer");
    const SplitWs ws = split_workspace(N);
    if (workspace_bytes < ws.bytes) return workspace_too_small("densify_split_scan: workspace smaller than gdr_densify_split_bytes");
    int32_t* cc = (int32_t*)((char*)workspace + ws.cc);
    int64_t* cbase = (int64_t*)((char*)workspace + ws.cbase);
    const hipStream_t st = (hipStream_t)stream;
    const int nchunks = div_up(N, DN_CHUNK);
    if (nchunks) hipLaunchKernelGGL(dn_mask_count_kernel, dim3((uint32_t)nchunks), dim3(DN_BLOCK), 0, st, mask, N, cc);
    hipLaunchKernelGGL(dn_mask_base_kernel, dim3(1), dim3(DN_FAN), 0, st, cc, nchunks, cbase, count);
    if (nchunks) hipLaunchKernelGGL(dn_mask_dest_kernel, dim3((uint32_t)nchunks), dim3(DN_BLOCK), 0, st, mask, N, cbase, dest);
    return launch_status("densify split scan kernels");
}

int gdr_densify_split_forward(const uint8_t* mask, const int64_t* dest, int64_t N, int32_t C, const void* feat, int64_t feat_stride,
                              int32_t feat_dtype, const void* coord, int32_t coord_elems, int32_t coord_elem_bytes, int64_t n_sel,
                              int64_t n_rest, void* feat_sel, void* feat_rest, int32_t out_dtype, void* coord_sel, void* coord_rest,
                              void* stream) {
    if (const int rc = check_rows(N, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(out_dtype)) return invalid_arg("densify_split_forward: unknown dtype");
    if (n_sel < 0 || n_rest < 0 || coord_elems < 0 || bad_elem(coord_elem_bytes))
        return invalid_arg("densify_split_forward: capacities and coord_elems must be >= 0, coord_elem_bytes 1, 2, 4 or 8");
    if (N == 0) return GDR_OK;
    if (!mask || !dest || !feat || (n_sel && !feat_sel) || (n_rest && !feat_rest) ||
        (coord_elems && (!coord || (n_sel && !coord_sel) || (n_rest && !coord_rest))))
        return invalid_arg("densify_split_forward: NULL argument");
    const unsigned cm = (unsigned)coord_elem_bytes - 1;
    if (bad_rows(feat, feat_stride, C) || misaligned(feat_sel, 15) || misaligned(feat_rest, 15) || misaligned(dest, 7) ||
        misaligned(coord, cm) || misaligned(coord_sel, cm) || misaligned(coord_rest, cm))
        return invalid_arg("densify_split_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    RowP p = {};
    p.mask = mask; p.dest = dest; p.feat = feat; p.coord = coord; p.out_sel = feat_sel; p.out_rest = feat_rest;
    p.coord_sel = coord_sel; p.coord_rest = coord_rest;
    p.N = N; p.n_sel = n_sel; p.n_rest = n_rest; p.feat_stride = feat_stride; p.C = C; p.feat_dt = feat_dtype; p.out_dt = out_dtype;
    p.D = coord_elems; p.es = coord_elem_bytes;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = DN_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((N + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    if (K == 1) hipLaunchKernelGGL(dn_split_fwd_kernel<1>, grid, dim3(DN_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(dn_split_fwd_kernel<2>, grid, dim3(DN_BLOCK), 0, st, p);
    return launch_status("densify dn_split_fwd_kernel");
}

int gdr_densify_rows_backward(const uint8_t* mask, const int64_t* dest, int64_t N, int32_t C, const void* grad_sel, const void* grad_rest,
                              int64_t grad_stride, int32_t grad_dtype, int64_t n_sel, int64_t n_rest, const void* feat,
                              int64_t feat_stride, int32_t feat_dtype, const void* prob, int32_t prob_dtype, const void* gcoord_sel,
                              const void* gcoord_rest, int32_t coord_elems, int32_t coord_elem_bytes, void* grad_feat, void* grad_prob,
                              void* grad_coord, void* stream) {
    if (const int rc = check_rows(N, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(grad_dtype) || (prob && bad_dtype(prob_dtype))) return invalid_arg("densify_rows_backward: unknown dtype");
    if (n_sel < 0 || n_rest < 0 || coord_elems < 0 || bad_elem(coord_elem_bytes))
        return invalid_arg("densify_rows_backward: capacities and coord_elems must be >= 0, coord_elem_bytes 1, 2, 4 or 8");
    if (N == 0) return GDR_OK;
    if (!dest) { n_sel = N; n_rest = 0; }
    if ((dest && !mask) || (n_sel && !grad_sel) || (dest && n_rest && !grad_rest) || (grad_prob && (!prob || !feat)) ||
        (grad_coord && ((n_sel && !gcoord_sel) || (dest && n_rest && !gcoord_rest))))
        return invalid_arg("densify_rows_backward: NULL argument");
    const unsigned cm = (unsigned)coord_elem_bytes - 1;
    if ((feat && bad_rows(feat, feat_stride, C)) || bad_rows(grad_sel, grad_stride, C) || bad_rows(grad_rest, grad_stride, C) ||
        misaligned(grad_feat, 15) || misaligned(dest, 7) || misaligned(prob, prob ? esize(prob_dtype) - 1 : 0) ||
        misaligned(grad_prob, prob ? esize(prob_dtype) - 1 : 0) || misaligned(gcoord_sel, cm) || misaligned(gcoord_rest, cm) ||
        misaligned(grad_coord, cm))
        return invalid_arg("densify_rows_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    RowP p = {};
    p.mask = mask; p.dest = dest; p.feat = feat; p.prob = prob; p.g_sel = grad_sel; p.g_rest = grad_rest; p.gc_sel = gcoord_sel;
    p.gc_rest = gcoord_rest; p.dfeat = grad_feat; p.dprob = grad_prob; p.dcoord = grad_coord;
    p.N = N; p.n_sel = n_sel; p.n_rest = n_rest; p.feat_stride = feat_stride; p.g_stride = grad_stride; p.C = C;
    p.feat_dt = feat_dtype; p.prob_dt = prob_dtype; p.out_dt = grad_dtype; p.D = grad_coord ? coord_elems : 0; p.es = coord_elem_bytes;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = DN_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((N + groups - 1) / groups));
    const hipStream_t st = (hipStream_t)stream;
    if (K == 1) hipLaunchKernelGGL(dn_rows_bwd_kernel<1>, grid, dim3(DN_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(dn_rows_bwd_kernel<2>, grid, dim3(DN_BLOCK), 0, st, p);
    return launch_status("densify dn_rows_bwd_kernel");
}

}  // extern "C"

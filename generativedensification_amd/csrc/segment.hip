// segment.hip — CSR segment reductions for the point decoder (include/gdr.h gdr_seg_*): what the reference takes from
// torch_scatter (segment_csr, gather_csr, scatter_*) and torch_geometric.utils (scatter, softmax) in every stage of
// lightning/point_decoder.  Semantics, restated from those packages' documentation:
//   reduce   out[s, :] = op over the rows indptr[s] .. indptr[s + 1] - 1 of src, op in {sum, mean, min, max}; an empty
//            segment gives 0 (and arg = N); mean divides by max(count, 1); min / max report in arg the row that won, the
//            lowest row on ties.  With perm, logical row r reads src[perm[r]] and arg reports perm[r].
//   gather   out[r, :] = src[seg(r), :] (optionally / max(count, 1)) for the rows r that lie in a segment
//   route    grad_src = 0; grad_src[arg[s, c], c] = grad_out[s, c] where arg < N
//   ptr      indptr[s] = the first position whose (sorted) index is >= s
//
// No atomics anywhere: every output element has one writer and every sum a fixed order, so two runs are bitwise equal.
//
// Mapping (reduce and gather): the rows are cut into fixed runs of GDR_SEG_ROWS consecutive rows, the channels into tiles of
// LC lanes times one 16-byte vector (V = 4 f32, 8 f16 / bf16, 2 int64; V = 1 where C, the row stride or a pointer rule out
// 16-byte accesses).  LC is the power of two that covers ceil(C / V), at most 64, so a wave holds 64 / LC runs.  The LC lanes
// of a (run, tile) unit walk the run's rows in ascending order: the segment of the first row comes from one binary search over
// indptr, the following ones from looking at the next pointer (a new search only behind empty segments).  A segment that lies
// inside the run is finished there.  A segment that crosses a run border leaves at most two partials per run in the
// workspace: slot 0 for the piece of a segment that began in an earlier run (the head of the run), slot 1 for the piece of a
// segment that begins here and ends later (the tail).  The second launch folds them: the workgroup of run j takes the
// segment whose tail the run holds, its 16 lane rows fold contiguous blocks of the partials in ascending run order, and
// lane row 0 folds those 16 in ascending order and writes the result.  The same launch writes the empty segments.
// So thousands of 1..8-row segments finish in the first launch, and one 48 000-row segment is 1500 independent runs plus a
// fold of 1500 partials by 16 lanes per channel.
//
// Bounds: every indptr value is clamped to [0, N] where it is read and a segment with end < start is empty; every perm / arg
// value is clamped or compared to N before it addresses anything; the binary searches stop after 64 steps and every other
// loop has a trip count of at most GDR_SEG_ROWS, C, or the number of runs.  A malformed pointer array gives unspecified
// values in out, and can never address outside src, out, arg or the workspace.
#include "gdr_common.h"
#include "host_util.h"
#include "half_bits.h"

namespace gdr {
namespace {

constexpr int SG_BLOCK = 256;
constexpr int SG_R = GDR_SEG_ROWS;
constexpr int SG_FOLD_LANES = 16;      // lane rows of a fold workgroup
constexpr int SG_FOLD_CH = SG_BLOCK / SG_FOLD_LANES;   // channels of a fold workgroup
constexpr uint32_t SG_NONE = 0xffffffffu;

template <int KIND> struct Tr;
template <> struct Tr<GDR_SEG_F16>  { using Elem = uint16_t; using Acc = float;   static constexpr int VFULL = 8; };
template <> struct Tr<GDR_SEG_BF16> { using Elem = uint16_t; using Acc = float;   static constexpr int VFULL = 8; };
template <> struct Tr<GDR_SEG_F32>  { using Elem = float;    using Acc = float;   static constexpr int VFULL = 4; };
template <> struct Tr<GDR_SEG_I64>  { using Elem = int64_t;  using Acc = int64_t; static constexpr int VFULL = 2; };

// half_bits.h's conversions, and an i64 as it is
template <int KIND>
__device__ __forceinline__ typename Tr<KIND>::Acc up(typename Tr<KIND>::Elem e) {
    if constexpr (KIND == GDR_SEG_I64) return e;
    else return gdr::up<KIND>(e);
}
template <int KIND>
__device__ __forceinline__ typename Tr<KIND>::Elem down(typename Tr<KIND>::Acc a) {
    if constexpr (KIND == GDR_SEG_I64) return a;
    else return gdr::down<KIND>(a);
}

// V elements at p: one 16-byte access when V is the full vector, one element when V = 1
template <int KIND, int V>
__device__ __forceinline__ void load_vec(const typename Tr<KIND>::Elem* p, typename Tr<KIND>::Acc (&x)[V]) {
    if constexpr (V == 1) {
        x[0] = up<KIND>(p[0]);
    } else {
        static_assert(V * sizeof(typename Tr<KIND>::Elem) == 16, "a full vector is 16 bytes");
        union { uint4 raw; typename Tr<KIND>::Elem e[V]; } u;
        u.raw = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = up<KIND>(u.e[v]);
    }
}
template <int KIND, int V>
__device__ __forceinline__ void store_vec(typename Tr<KIND>::Elem* p, const typename Tr<KIND>::Acc (&x)[V]) {
    if constexpr (V == 1) {
        p[0] = down<KIND>(x[0]);
    } else {
        union { uint4 raw; typename Tr<KIND>::Elem e[V]; } u;
#pragma unroll
        for (int v = 0; v < V; ++v) u.e[v] = down<KIND>(x[v]);
        *reinterpret_cast<uint4*>(p) = u.raw;
    }
}

__device__ __forceinline__ int64_t clamp_ptr(const int64_t* __restrict__ indptr, int64_t i, int64_t N) {
    const int64_t v = indptr[i];
    return v < 0 ? 0 : (v > N ? N : v);
}

// the last i in [0, S] with indptr[i] <= row, -1 if none (indptr non-decreasing): the segment that holds `row` when i < S
__device__ __forceinline__ int64_t seg_of(const int64_t* __restrict__ indptr, int64_t S, int64_t N, int64_t row) {
    int64_t lo = 0, hi = S + 1;
    for (int k = 0; k < 64 && lo < hi; ++k) {
        const int64_t mid = (lo + hi) >> 1;
        if (clamp_ptr(indptr, mid, N) <= row) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// Walks the rows [a, b) of one run (b - a <= GDR_SEG_ROWS) in ascending order and calls piece(s, st, en, r0, r1) for every
// maximal range [r0, r1) of them that lies in segment s = [st, en), and piece(-1, 0, 0, r0, r1) for ranges in no segment.
// Every call consumes at least one row, so there are at most GDR_SEG_ROWS of them.
template <typename F>
__device__ __forceinline__ void walk_run(const int64_t* __restrict__ indptr, int64_t S, int64_t N, int64_t a, int64_t b, F&& piece) {
    int64_t row = a, s = -1;
    bool guess = false;      // s is the segment behind the one just finished: try it before searching
    for (int it = 0; it < SG_R && row < b; ++it) {
        int64_t st = 0, en = 0;
        bool ok = false;
        if (guess && s < S) {
            st = clamp_ptr(indptr, s, N); en = clamp_ptr(indptr, s + 1, N);
            ok = st <= row && row < en;
        }
        if (!ok) {
            s = seg_of(indptr, S, N, row);
            if (s >= S) { piece((int64_t)-1, (int64_t)0, (int64_t)0, row, b); return; }     // behind the last segment
            if (s >= 0) {
                st = clamp_ptr(indptr, s, N); en = clamp_ptr(indptr, s + 1, N);
                ok = st <= row && row < en;
            }
        }
        if (!ok) {   // before the first segment (jump to it), or a pointer array that is not monotone (one row on)
            int64_t nx = row + 1;
            if (s < 0) { const int64_t p0 = clamp_ptr(indptr, 0, N); nx = p0 > nx ? (p0 < b ? p0 : b) : nx; }
            piece((int64_t)-1, (int64_t)0, (int64_t)0, row, nx);
            row = nx; guess = false;
            continue;
        }
        const int64_t r1 = en < b ? en : b;
        piece(s, st, en, row, r1);
        row = r1; s += 1; guess = true;
    }
}

struct SegP {
    const void* src; const int64_t* perm; const int64_t* indptr;
    void* out; int64_t* arg; void* ws_val; uint32_t* ws_arg;
    int64_t stride, N, S, nruns;
    int32_t C, op, lc_shift, fill_outside;
};

__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ perm, int64_t r, int64_t N) {
    if (!perm) return r;
    const int64_t v = perm[r];
    return v < 0 ? 0 : (v >= N ? N - 1 : v);
}

template <int KIND, bool MM>
__device__ __forceinline__ typename Tr<KIND>::Acc finish(typename Tr<KIND>::Acc acc, int32_t op, int64_t count) {
    if constexpr (KIND != GDR_SEG_I64 && !MM) {
        if (op == GDR_SEG_MEAN) return acc / (float)(count > 1 ? count : 1);
    }
    return acc;
}

// first launch: one (run, channel tile) unit per group of LC lanes
template <int KIND, int V, bool MM>
__global__ __launch_bounds__(SG_BLOCK) void seg_reduce_kernel(const SegP p) {
    using Elem = typename Tr<KIND>::Elem;
    using Acc = typename Tr<KIND>::Acc;
    const int tid = threadIdx.x, LC = 1 << p.lc_shift;
    const int64_t j = (int64_t)blockIdx.x * (SG_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    const int64_t c0 = ((int64_t)blockIdx.y * LC + (tid & (LC - 1))) * V;
    if (j >= p.nruns || c0 >= p.C) return;
    const int64_t N = p.N, C = p.C, a = j * SG_R, b = a + SG_R < N ? a + SG_R : N;
    const Elem* __restrict__ src = (const Elem*)p.src;
    const int64_t* __restrict__ perm = p.perm;
    const bool is_max = p.op == GDR_SEG_MAX;
    walk_run(p.indptr, p.S, N, a, b, [&](int64_t s, int64_t st, int64_t en, int64_t r0, int64_t r1) {
        if (s < 0) return;
        Acc acc[V];
        uint32_t best[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { acc[v] = 0; best[v] = SG_NONE; }
#pragma unroll 4
        for (int64_t r = r0; r < r1; ++r) {       // at most GDR_SEG_ROWS rows
            const int64_t pr = row_of(perm, r, N);
            Acc x[V];
            load_vec<KIND, V>(src + pr * p.stride + c0, x);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if constexpr (MM) {
                    const bool take = best[v] == SG_NONE || (is_max ? x[v] > acc[v] : x[v] < acc[v]);   // strict: the lowest row keeps a tie
                    if (take) { acc[v] = x[v]; best[v] = (uint32_t)pr; }
                } else {
                    acc[v] += x[v];
                }
            }
        }
        if (st >= a && en <= b) {                  // the whole segment lies in this run
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = finish<KIND, MM>(acc[v], p.op, en - st);
            store_vec<KIND, V>((Elem*)p.out + s * C + c0, acc);
            if constexpr (MM) {
#pragma unroll
                for (int v = 0; v < V; ++v) p.arg[s * C + c0 + v] = best[v];
            }
        } else {                                   // head (slot 0) or tail (slot 1) partial of the run
            const int64_t at = (j * 2 + (st < a ? 0 : 1)) * C + c0;
#pragma unroll
            for (int v = 0; v < V; ++v) ((Acc*)p.ws_val)[at + v] = acc[v];
            if constexpr (MM) {
#pragma unroll
                for (int v = 0; v < V; ++v) p.ws_arg[at + v] = best[v];
            }
        }
    });
}

// second launch.  Workgroups [0, fold_blocks): run j = blockIdx / ctiles, 16 channels; folds the segment whose tail run j
// holds.  The workgroups behind them: one thread per segment, writes the empty ones.
template <int KIND, bool MM>
__global__ __launch_bounds__(SG_BLOCK) void seg_fold_kernel(const SegP p, uint32_t fold_blocks, uint32_t ctiles) {
    using Elem = typename Tr<KIND>::Elem;
    using Acc = typename Tr<KIND>::Acc;
    __shared__ Acc sh_val[SG_FOLD_LANES][SG_FOLD_CH];
    __shared__ uint32_t sh_arg[SG_FOLD_LANES][SG_FOLD_CH];
    const int tid = threadIdx.x;
    const int64_t N = p.N, S = p.S, C = p.C;
    if (blockIdx.x >= fold_blocks) {
        const int64_t s = (int64_t)(blockIdx.x - fold_blocks) * SG_BLOCK + tid;
        if (s >= S) return;
        if (clamp_ptr(p.indptr, s + 1, N) > clamp_ptr(p.indptr, s, N)) return;
        for (int64_t c = 0; c < C; ++c) {          // an empty segment: 0 and arg = N
            ((Elem*)p.out)[s * C + c] = down<KIND>((Acc)0);
            if constexpr (MM) p.arg[s * C + c] = N;
        }
        return;
    }
    // (everything up to the barrier is the same in all threads of the workgroup)
    const int64_t j = blockIdx.x / ctiles, a = j * SG_R, b = a + SG_R;
    if (b >= N) return;                            // no row behind the run: nothing crosses its end
    const int64_t s = seg_of(p.indptr, S, N, b - 1);
    if (s < 0 || s >= S) return;
    const int64_t st = clamp_ptr(p.indptr, s, N), en = clamp_ptr(p.indptr, s + 1, N);
    if (!(st >= a && st < b && en > b)) return;    // the segment of the run's last row does not begin here or ends here
    const int64_t T = (en - 1) / SG_R - j + 1;     // partials: the tail of run j, then the heads of runs j + 1 .. j + T - 1
    const int64_t per = (T + SG_FOLD_LANES - 1) / SG_FOLD_LANES;
    const int ch = tid & (SG_FOLD_CH - 1), fl = tid / SG_FOLD_CH;
    const int64_t c = (int64_t)(blockIdx.x % ctiles) * SG_FOLD_CH + ch;
    const bool is_max = p.op == GDR_SEG_MAX;
    Acc acc = 0;
    uint32_t best = SG_NONE;
    if (c < C) {
        const int64_t t0 = fl * per, t1 = t0 + per < T ? t0 + per : T;
#pragma unroll 4
        for (int64_t t = t0; t < t1; ++t) {        // at most nruns / 16 + 1 partials, in ascending run order
            const int64_t at = ((j + t) * 2 + (t == 0 ? 1 : 0)) * C + c;
            const Acc x = ((const Acc*)p.ws_val)[at];
            if constexpr (MM) {
                const uint32_t xa = p.ws_arg[at];
                const bool take = xa != SG_NONE && (best == SG_NONE || (is_max ? x > acc : x < acc));
                if (take) { acc = x; best = xa; }
            } else {
                acc += x;
            }
        }
    }
    sh_val[fl][ch] = acc;
    sh_arg[fl][ch] = best;
    __syncthreads();
    if (fl != 0 || c >= C) return;
    for (int l = 1; l < SG_FOLD_LANES; ++l) {
        const Acc x = sh_val[l][ch];
        if constexpr (MM) {
            const uint32_t xa = sh_arg[l][ch];
            const bool take = xa != SG_NONE && (best == SG_NONE || (is_max ? x > acc : x < acc));
            if (take) { acc = x; best = xa; }
        } else {
            acc += x;
        }
    }
    ((Elem*)p.out)[s * C + c] = down<KIND>(finish<KIND, MM>(acc, p.op, en - st));
    if constexpr (MM) p.arg[s * C + c] = best == SG_NONE || best >= N ? N : (int64_t)best;
}

// gather: the unit mapping of the reduce; src is (S, C), out (N, C).  Rows in no segment are zero-filled or left alone.
template <int KIND, int V>
__global__ __launch_bounds__(SG_BLOCK) void seg_gather_kernel(const SegP p, int inv_count) {
    using Elem = typename Tr<KIND>::Elem;
    using Acc = typename Tr<KIND>::Acc;
    const int tid = threadIdx.x, LC = 1 << p.lc_shift;
    const int64_t j = (int64_t)blockIdx.x * (SG_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    const int64_t c0 = ((int64_t)blockIdx.y * LC + (tid & (LC - 1))) * V;
    if (j >= p.nruns || c0 >= p.C) return;
    const int64_t N = p.N, C = p.C, a = j * SG_R, b = a + SG_R < N ? a + SG_R : N;
    const Elem* __restrict__ src = (const Elem*)p.src;
    const int64_t* __restrict__ perm = p.perm;
    walk_run(p.indptr, p.S, N, a, b, [&](int64_t s, int64_t st, int64_t en, int64_t r0, int64_t r1) {
        Acc x[V];
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = 0;
        if (s < 0) {
            if (!p.fill_outside) return;
        } else {
            load_vec<KIND, V>(src + s * p.stride + c0, x);
            if constexpr (KIND != GDR_SEG_I64) {
                if (inv_count) {
                    const float n = (float)(en - st > 1 ? en - st : 1);
#pragma unroll
                    for (int v = 0; v < V; ++v) x[v] = x[v] / n;
                }
            }
        }
        for (int64_t r = r0; r < r1; ++r)          // at most GDR_SEG_ROWS rows
            store_vec<KIND, V>((Elem*)p.out + row_of(perm, r, N) * C + c0, x);
    });
}

// route: grad_src (zero-filled by the launch before) [arg[s, c], c] = grad_out[s, c]; W = the element's storage word
template <typename W>
__global__ __launch_bounds__(SG_BLOCK) void seg_route_kernel(const W* __restrict__ grad_out, const int64_t* __restrict__ arg,
                                                             int64_t N, int64_t total, int32_t C, W* __restrict__ grad_src) {
    const int64_t i = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int64_t r = arg[i];
    if (r < 0 || r >= N) return;
    grad_src[r * C + i % C] = grad_out[i];
}

__global__ __launch_bounds__(SG_BLOCK) void seg_ptr_kernel(const int64_t* __restrict__ index, const int64_t* __restrict__ perm,
                                                           int64_t N, int64_t S, int64_t* __restrict__ indptr) {
    const int64_t s = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
    if (s > S) return;
    int64_t lo = 0, hi = N;                        // the first position whose index is >= s
    for (int k = 0; k < 64 && lo < hi; ++k) {
        const int64_t mid = (lo + hi) >> 1;
        if (index[row_of(perm, mid, N)] < s) lo = mid + 1; else hi = mid;
    }
    indptr[s] = lo;
}

constexpr int64_t SG_MAX = INT64_C(0x7ffffffe);    // rows and segments: row numbers travel as 32-bit words, 0xffffffff = none

const char* seg_check(int64_t N, int64_t S, int64_t C, int32_t dtype) {
    if (N < 0 || N > SG_MAX || S < 0 || S > SG_MAX) return "seg: N and S must be in 0..2^31-2";
    if (C < 1 || C > GDR_SEG_MAX_CHANNELS) return "seg: C must be in 1..GDR_SEG_MAX_CHANNELS";
    if (dtype < GDR_SEG_F16 || dtype > GDR_SEG_I64) return "seg: unknown dtype";
    return nullptr;
}

struct SegWs { size_t val, arg, bytes; };

SegWs seg_workspace(int64_t N, int64_t C) {
    SegWs w;
    const size_t slots = (size_t)((N + SG_R - 1) / SG_R) * 2 * (size_t)C;
    w.val = 0;
    w.arg = align_up(slots * 8);
    w.bytes = w.arg + align_up(slots * 4);
    return w;
}

int elem_bytes(int32_t dtype) { return dtype == GDR_SEG_F32 ? 4 : (dtype == GDR_SEG_I64 ? 8 : 2); }

// 16-byte accesses need whole vectors per row, rows that start on a vector, and aligned bases
bool can_vector(int32_t dtype, int64_t C, int64_t stride, const void* a, const void* b) {
    const int v = 16 / elem_bytes(dtype);
    return C % v == 0 && stride % v == 0 && !misaligned(a, 15) && !misaligned(b, 15);
}

// lanes per unit (as a shift) and channel tiles for C channels in vectors of v
void unit_shape(int64_t C, int v, int32_t* lc_shift, uint32_t* tiles) {
    const int64_t vecs = (C + v - 1) / v;
    int sh = 0;
    while (sh < 6 && (INT64_C(1) << sh) < vecs) ++sh;
    *lc_shift = sh;
    *tiles = (uint32_t)((vecs + (INT64_C(1) << sh) - 1) >> sh);
}

template <int KIND, bool MM>
void launch_reduce(const SegP& p, bool vec, dim3 grid1, uint32_t grid2, uint32_t fold_blocks, uint32_t ctiles, hipStream_t st) {
    if (grid1.x) {
        if (vec) hipLaunchKernelGGL((seg_reduce_kernel<KIND, Tr<KIND>::VFULL, MM>), grid1, dim3(SG_BLOCK), 0, st, p);
        else hipLaunchKernelGGL((seg_reduce_kernel<KIND, 1, MM>), grid1, dim3(SG_BLOCK), 0, st, p);
    }
    hipLaunchKernelGGL((seg_fold_kernel<KIND, MM>), dim3(grid2), dim3(SG_BLOCK), 0, st, p, fold_blocks, ctiles);
}

template <int KIND>
void launch_gather(const SegP& p, bool vec, dim3 grid, int inv_count, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((seg_gather_kernel<KIND, Tr<KIND>::VFULL>), grid, dim3(SG_BLOCK), 0, st, p, inv_count);
    else hipLaunchKernelGGL((seg_gather_kernel<KIND, 1>), grid, dim3(SG_BLOCK), 0, st, p, inv_count);
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_seg_reduce_bytes(int64_t N, int64_t S, int32_t C) {
    if (const char* why = seg_check(N, S, C, GDR_SEG_F32)) { invalid_arg(why); return 0; }
    return seg_workspace(N, C).bytes + 256;        // (never 0 for valid arguments)
}

int gdr_seg_reduce(const void* src, int64_t src_stride, const int64_t* perm, const int64_t* indptr, int64_t N, int64_t S,
                   int32_t C, int32_t dtype, int32_t op, void* workspace, size_t workspace_bytes, void* out, int64_t* arg,
                   void* stream) {
    if (const char* why = seg_check(N, S, C, dtype)) return invalid_arg(why);
    if (op < GDR_SEG_SUM || op > GDR_SEG_MAX) return invalid_arg("seg_reduce: unknown op");
    if (dtype == GDR_SEG_I64 && op != GDR_SEG_SUM) return invalid_arg("seg_reduce: int64 is supported for sum only");
    const bool mm = op == GDR_SEG_MIN || op == GDR_SEG_MAX;
    if (S == 0) return GDR_OK;
    if (!indptr || !out || !workspace || (N && !src) || (mm && !arg)) return invalid_arg("seg_reduce: NULL argument");
    if (src_stride < C) return invalid_arg("seg_reduce: the row stride must be at least C");
    const unsigned emask = elem_bytes(dtype) - 1;
    if (misaligned(src, emask) || misaligned(out, 15) || misaligned(perm, 7) || misaligned(indptr, 7) || misaligned(arg, 7) ||
        misaligned(workspace, 255))
        return invalid_arg("seg_reduce: unaligned buffer");
    const SegWs ws = seg_workspace(N, C);
    if (workspace_bytes < ws.bytes) return workspace_too_small("seg_reduce: workspace smaller than gdr_seg_reduce_bytes");
    SegP p = {};
    p.src = src; p.perm = perm; p.indptr = indptr; p.out = out; p.arg = arg;
    p.ws_val = (char*)workspace + ws.val; p.ws_arg = (uint32_t*)((char*)workspace + ws.arg);
    p.stride = src_stride; p.N = N; p.S = S; p.nruns = (N + SG_R - 1) / SG_R; p.C = C; p.op = op;
    const bool vec = can_vector(dtype, C, src_stride, src, out);
    uint32_t tiles;
    unit_shape(C, vec ? 16 / elem_bytes(dtype) : 1, &p.lc_shift, &tiles);
    const int64_t units = SG_BLOCK >> p.lc_shift;
    const dim3 grid1((uint32_t)((p.nruns + units - 1) / units), tiles);
    const int64_t ctiles = (C + SG_FOLD_CH - 1) / SG_FOLD_CH;
    const int64_t fold_blocks = (p.nruns > 1 ? p.nruns - 1 : 0) * ctiles, grid2 = fold_blocks + (S + SG_BLOCK - 1) / SG_BLOCK;
    if (grid2 > INT64_C(0x7fffffff) || tiles > 65535) return invalid_arg("seg_reduce: N * C is beyond the launch grid");
    const hipStream_t st = (hipStream_t)stream;
#define GDR_SEG_GO(KIND) (mm ? launch_reduce<KIND, true>(p, vec, grid1, (uint32_t)grid2, (uint32_t)fold_blocks, (uint32_t)ctiles, st) \
                             : launch_reduce<KIND, false>(p, vec, grid1, (uint32_t)grid2, (uint32_t)fold_blocks, (uint32_t)ctiles, st))
    if (dtype == GDR_SEG_F16) GDR_SEG_GO(GDR_SEG_F16);
    else if (dtype == GDR_SEG_BF16) GDR_SEG_GO(GDR_SEG_BF16);
    else if (dtype == GDR_SEG_F32) GDR_SEG_GO(GDR_SEG_F32);
    else launch_reduce<GDR_SEG_I64, false>(p, vec, grid1, (uint32_t)grid2, (uint32_t)fold_blocks, (uint32_t)ctiles, st);
#undef GDR_SEG_GO
    return launch_status("seg_reduce kernels");
}

int gdr_seg_gather(const void* src, int64_t src_stride, const int64_t* indptr, const int64_t* perm, int64_t N, int64_t S,
                   int32_t C, int32_t dtype, int32_t inv_count, int32_t fill_outside, void* out, void* stream) {
    if (const char* why = seg_check(N, S, C, dtype)) return invalid_arg(why);
    if (dtype == GDR_SEG_I64 && inv_count) return invalid_arg("seg_gather: int64 cannot be divided by the count");
    if (N == 0) return GDR_OK;
    if (!indptr || !out || (S && !src)) return invalid_arg("seg_gather: NULL argument");
    if (src_stride < C) return invalid_arg("seg_gather: the row stride must be at least C");
    const unsigned emask = elem_bytes(dtype) - 1;
    if (misaligned(src, emask) || misaligned(out, 15) || misaligned(perm, 7) || misaligned(indptr, 7))
        return invalid_arg("seg_gather: unaligned buffer");
    SegP p = {};
    p.src = src; p.perm = perm; p.indptr = indptr; p.out = out;
    p.stride = src_stride; p.N = N; p.S = S; p.nruns = (N + SG_R - 1) / SG_R; p.C = C; p.fill_outside = fill_outside ? 1 : 0;
    const bool vec = can_vector(dtype, C, src_stride, src, out);
    uint32_t tiles;
    unit_shape(C, vec ? 16 / elem_bytes(dtype) : 1, &p.lc_shift, &tiles);
    if (tiles > 65535) return invalid_arg("seg_gather: C is beyond the launch grid");
    const int64_t units = SG_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((p.nruns + units - 1) / units), tiles);
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == GDR_SEG_F16) launch_gather<GDR_SEG_F16>(p, vec, grid, inv_count, st);
    else if (dtype == GDR_SEG_BF16) launch_gather<GDR_SEG_BF16>(p, vec, grid, inv_count, st);
    else if (dtype == GDR_SEG_F32) launch_gather<GDR_SEG_F32>(p, vec, grid, inv_count, st);
    else launch_gather<GDR_SEG_I64>(p, vec, grid, 0, st);
    return launch_status("seg_gather_kernel");
}

int gdr_seg_route(const void* grad_out, const int64_t* arg, int64_t N, int64_t S, int32_t C, int32_t dtype, void* grad_src,
                  void* stream) {
    if (const char* why = seg_check(N, S, C, dtype)) return invalid_arg(why);
    if (dtype == GDR_SEG_I64) return invalid_arg("seg_route: floating dtypes only");
    if (N == 0) return GDR_OK;
    if (!grad_src || (S && (!grad_out || !arg))) return invalid_arg("seg_route: NULL argument");
    const unsigned emask = elem_bytes(dtype) - 1;
    if (misaligned(grad_out, emask) || misaligned(grad_src, emask) || misaligned(arg, 7))
        return invalid_arg("seg_route: unaligned buffer");
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(grad_src, 0, (size_t)N * C * elem_bytes(dtype), st);
    if (e != hipSuccess) { set_error("seg_route: hipMemsetAsync", e); return GDR_ERR_HIP; }
    const int64_t total = S * C, blocks = (total + SG_BLOCK - 1) / SG_BLOCK;
    if (blocks > INT64_C(0x7fffffff)) return invalid_arg("seg_route: S * C is beyond the launch grid");
    if (blocks) {
        if (dtype == GDR_SEG_F32)
            hipLaunchKernelGGL(seg_route_kernel<uint32_t>, dim3((uint32_t)blocks), dim3(SG_BLOCK), 0, st, (const uint32_t*)grad_out,
                               arg, N, total, C, (uint32_t*)grad_src);
        else
            hipLaunchKernelGGL(seg_route_kernel<uint16_t>, dim3((uint32_t)blocks), dim3(SG_BLOCK), 0, st, (const uint16_t*)grad_out,
                               arg, N, total, C, (uint16_t*)grad_src);
    }
    return launch_status("seg_route_kernel");
}

int gdr_seg_ptr_from_sorted(const int64_t* index, const int64_t* perm, int64_t N, int64_t S, int64_t* indptr, void* stream) {
    if (N < 0 || N > SG_MAX || S < 0 || S > SG_MAX) return invalid_arg("seg_ptr_from_sorted: N and S must be in 0..2^31-2");
    if (!indptr || (N && !index)) return invalid_arg("seg_ptr_from_sorted: NULL argument");
    if (misaligned(index, 7) || misaligned(perm, 7) || misaligned(indptr, 7))
        return invalid_arg("seg_ptr_from_sorted: unaligned buffer");
    hipLaunchKernelGGL(seg_ptr_kernel, dim3((uint32_t)((S + 1 + SG_BLOCK - 1) / SG_BLOCK)), dim3(SG_BLOCK), 0, (hipStream_t)stream,
                       index, perm, N, S, indptr);
    return launch_status("seg_ptr_kernel");
}

}  // extern "C"

// head_rows.h — what the two Gaussian heads (coarsehead.hip, finehead.hip) share (internal): a row MLP whose workgroup of
// 4 waves owns 64 rows, reads its operand rows from LDS and its weights from a packed buffer, and whose backward keeps
// 16 x 16 tiles of the weight gradients in registers over a slab of rows and leaves one partial set per slab for a fold.
// Device side: the geometry, the tile product, the x-row staging, the grad_x product, the weight-gradient tile bookkeeping and
// the fold kernel.  Host side: the backward's LDS carve, the slab count, the dtype dispatch and the fold's launch.
// What differs between the heads stays in their files: the layer count and the activations, the packed and partial layouts,
// the epilogues, the backward's step sequence.  Nothing here asks which head is calling.
// Include after gdr_common.h, host_util.h, row_io.h and mfma_rows.h.
#pragma once
#include <stdio.h>

namespace gdr {
namespace {      // the including file's own names: the fold kernel is then one kernel of each code object, not one shared symbol

constexpr int HEAD_BLOCK = GDR_BLOCK;
constexpr int HEAD_ROWS = GDR_COARSEHEAD_TILE_ROWS;      // rows of one workgroup of a forward
constexpr int HEAD_TPW = 16;                             // weight-gradient tiles a wave accumulates
constexpr int HEAD_FOLD = 16;                            // fold: elements per block, and segments of the slabs per element
constexpr size_t HEAD_LDS_MAX = 160 * 1024;
constexpr size_t HEAD_LDS_PREFER = 80 * 1024;            // two workgroups per CU
static_assert(GDR_COARSEHEAD_TILE_ROWS == GDR_FINEHEAD_TILE_ROWS, "the heads share one row tile");
static_assert(HEAD_FOLD * HEAD_FOLD == HEAD_BLOCK, "the fold's threads are (segment, element)");
static_assert(HEAD_ROWS == 64 && HEAD_BLOCK == 256, "4 waves, 4 row tiles of 16");

template <int DT> using Sc = typename std::conditional<DT == GDR_NORM_F32, double, float>::type;      // the accumulator's element

__host__ __device__ inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// D += A B over kpad sum elements: A points at the tile's first A row (row stride lda), B at its first B row (the D column),
// both 16-byte aligned with strides of whole vectors.  Lane (l16, quad) ends with D rows 4 quad .. + 3 of D column l16.
// kpad is at least one chunk (Cpad, Opad and the step all are), and the loop says so: with a `for`, the compiler guards the loop
// with a branch round it, the accumulator reads of the epilogue land in the block where the two paths join, and the first two
// of them are issued without the wait states an MFMA result needs (seen in the fine head's forward, last layer: columns 4 q
// and 4 q + 1 came out as the bias alone).  A loop that always runs once leaves the epilogue one predecessor, and the reads get
// their nops.
template <int DT>
__device__ __forceinline__ void tile_mma(const typename El<DT>::type* A, int lda, const typename El<DT>::type* B, int ldb, int kpad, int l16,
                                         int quad, typename El<DT>::acc& acc) {
    constexpr int VE = El<DT>::VE, KC = El<DT>::KC;
    const typename El<DT>::type* a = A + (int64_t)a_row<DT>(l16) * lda + quad * VE;
    const typename El<DT>::type* b = B + (int64_t)l16 * ldb + quad * VE;
    int k = 0;
    do {
        mma_row<DT>(*reinterpret_cast<const uint4*>(a + k), *reinterpret_cast<const uint4*>(b + k), acc);
        k += KC;
    } while (k < kpad);
}

// a bias as the forward adds it: rounded to the compute dtype; 0 beyond its n entries
template <int DT> __device__ __forceinline__ Sc<DT> bias_at(const void* b, int dt, int c, int n) {
    return c < n ? (Sc<DT>)up<DT>(down<DT>(load1(b, c, dt))) : (Sc<DT>)0;
}

// 4 consecutive elements of an LDS / global row
template <int DT> __device__ __forceinline__ void store4(typename El<DT>::type* dst, const typename El<DT>::type (&v)[4]) {
    if constexpr (DT == GDR_NORM_F32) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
}

// rows r0 .. r0 + rows - 1 of the dense (., C) matrix X -> dst[row][lda], zeros from row `end` on and in columns C .. Cpad - 1;
// transposed: dstT[column][ldt] as well
template <int DT>
__device__ __forceinline__ void stage_rows(const typename El<DT>::type* X, int64_t r0, int64_t end, int rows, int C, int Cpad,
                                           typename El<DT>::type* dst, int lda, bool transposed, typename El<DT>::type* dstT, int ldt, int tid) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE;
    const int vpr = Cpad / VE;
    for (int v = tid; v < rows * vpr; v += HEAD_BLOCK) {
        const int r = v / vpr, c = (v - r * vpr) * VE;
        union { uint4 v; E e[VE]; } u;
        u.v = make_uint4(0, 0, 0, 0);
        if (r0 + r < end && c < C) u.v = *reinterpret_cast<const uint4*>(X + (r0 + r) * C + c);
        *reinterpret_cast<uint4*>(dst + r * lda + c) = u.v;
        if (transposed)
#pragma unroll
            for (int e = 0; e < VE; ++e) dstT[(c + e) * ldt + r] = u.e[e];
    }
}

// grad_x of the step's rows r0 .. = rd(dz1 W1): Z holds the rt row tiles of dz1 (row stride lda), W1t is the packed [in][out] W1;
// the (row tile, channel tile) pairs are dealt round to the 4 waves
template <int DT>
__device__ __forceinline__ void grad_x_tiles(const typename El<DT>::type* W1t, const typename El<DT>::type* Z, int lda, void* grad_x, int64_t r0,
                                             int64_t r_end, int rt, int C, int C16, int Cpad, int wave, int l16, int quad) {
    using E = typename El<DT>::type;
    for (int pr = wave; pr < (C16 / 16) * rt; pr += 4) {
        const int ti = pr % rt, jt = pr / rt, ch = 16 * jt + 4 * quad;
        const int64_t row = r0 + 16 * ti + l16;
        typename El<DT>::acc acc = {0, 0, 0, 0};
        tile_mma<DT>(W1t + (int64_t)16 * jt * Cpad, Cpad, Z + 16 * ti * lda, lda, Cpad, l16, quad, acc);
        if (row < r_end && ch < C) {          // C is a multiple of 8: the 4 channels are in or out together
            E d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = down<DT>((float)acc[e]);
            store4<DT>((E*)grad_x + row * C + ch, d);
        }
    }
}

// The weight-gradient tiles of a backward: the 16 x 16 tiles of its grad_W sections laid end to end, (out tile, in tile)
// row-major within a section.  Section grad_W = A^T B over the rows, A and B transposed ([channel][row]) in LDS; every section
// has C in channels.  A kernel fills the sections it has; wave w of tile group blockIdx.y owns tiles t_first .. + HEAD_TPW - 1.
template <int DT> struct WgSection {
    const typename El<DT>::type* A;      // [out channel][row]
    const typename El<DT>::type* B;      // [in channel][row]
    int first;                           // its first tile
    int outs;                            // its out channels
    int64_t base;                        // where it starts in a partial set
};
template <int DT> struct WgTiles {
    int n, ntiles;                       // sections in use (at most 3), and their tiles
    int C, c16;                          // in channels, and in tiles per out tile
    WgSection<DT> s[3];
};

template <int DT> __device__ __forceinline__ WgSection<DT> section_of(const WgTiles<DT>& w, int t) {
    WgSection<DT> s = w.s[0];
#pragma unroll
    for (int j = 1; j < 3; ++j)
        if (j < w.n && t >= w.s[j].first) s = w.s[j];
    return s;
}

// one step's rows into this wave's tiles
template <int DT>
__device__ __forceinline__ void wgrad_step(const WgTiles<DT>& w, int t_first, int ldt, int step, int l16, int quad,
                                           typename El<DT>::acc (&accW)[HEAD_TPW]) {
#pragma unroll
    for (int i = 0; i < HEAD_TPW; ++i) {
        if (t_first + i >= w.ntiles) continue;            // (uniform over the wave)
        const WgSection<DT> s = section_of(w, t_first + i);
        const int t = t_first + i - s.first;
        tile_mma<DT>(s.A + 16 * (t / w.c16) * ldt, ldt, s.B + 16 * (t % w.c16) * ldt, ldt, step, l16, quad, accW[i]);
    }
}

// the end of the slab: this wave's tiles into the slab's partial set
template <int DT>
__device__ __forceinline__ void wgrad_store(const WgTiles<DT>& w, int t_first, Sc<DT>* part, int l16, int quad,
                                            const typename El<DT>::acc (&accW)[HEAD_TPW]) {
#pragma unroll
    for (int i = 0; i < HEAD_TPW; ++i) {
        if (t_first + i >= w.ntiles) continue;
        const WgSection<DT> s = section_of(w, t_first + i);
        const int t = t_first + i - s.first, in = 16 * (t % w.c16) + l16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = 16 * (t / w.c16) + 4 * quad + e;
            if (o < s.outs && in < w.C) part[s.base + (int64_t)o * w.C + in] = accW[i][e];
        }
    }
}

// the parameter gradients = the slabs' partial sets added in slab order, each rounded once to its dtype
struct FoldP {
    const void* part;
    void* out[6];              // in the order of a partial set; any may be NULL
    int32_t out_dtype[6];
    int64_t size[6];
    int64_t total;
    int32_t slabs, count;      // count: the outputs in use
};

// a block owns HEAD_FOLD elements; 16 threads per element add one segment of the slabs each, in slab order, then the first
// adds the 16 segment sums in segment order
template <typename T>
__global__ __launch_bounds__(HEAD_BLOCK) void head_fold_kernel(const FoldP p) {
    __shared__ T sSeg[HEAD_FOLD][HEAD_FOLD];
    const int el = threadIdx.x % HEAD_FOLD, seg = threadIdx.x / HEAD_FOLD;
    int64_t i = (int64_t)blockIdx.x * HEAD_FOLD + el;
    const int per = (p.slabs + HEAD_FOLD - 1) / HEAD_FOLD, b0 = seg * per, b1 = b0 + per < p.slabs ? b0 + per : p.slabs;
    T s = 0;
    if (i < p.total)
        for (int b = b0; b < b1; ++b) s += ((const T*)p.part)[(int64_t)b * p.total + i];
    sSeg[seg][el] = s;
    __syncthreads();
    if (seg != 0 || i >= p.total) return;
    T sum = 0;
    for (int k = 0; k < HEAD_FOLD; ++k) sum += sSeg[k][el];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k >= p.count) return;
        if (i < p.size[k]) {
            if (p.out[k]) store1(p.out[k], i, p.out_dtype[k], (float)sum);
            return;
        }
        i -= p.size[k];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the LDS of a backward step: two Cpad-wide and one Opad-wide row buffers, then `nt` transposed buffers of Cpad channels and
// one of Opad
struct BwdLds { int step, lda, ldz, ldt; size_t total; };
size_t bwd_bytes(int dtype, int Cpad, int Opad, int nt, int step, BwdLds* l) {
    const int ve = dtype == GDR_NORM_F32 ? 4 : 8;
    l->step = step; l->lda = Cpad + ve; l->ldz = Opad + ve; l->ldt = step + ve;
    l->total = esize(dtype) * ((size_t)2 * step * l->lda + (size_t)step * l->ldz + (size_t)(nt * Cpad + Opad) * l->ldt);
    return l->total;
}
// the rows per step: the most that leave room for two workgroups per CU, or else the fewest
BwdLds bwd_lds(int dtype, int Cpad, int Opad, int nt) {
    BwdLds l;
    const int least = dtype == GDR_NORM_F32 ? 16 : 32;
    for (int step = 64; step > least; step /= 2)
        if (bwd_bytes(dtype, Cpad, Opad, nt, step, &l) <= HEAD_LDS_PREFER) return l;
    bwd_bytes(dtype, Cpad, Opad, nt, least, &l);
    return l;
}

template <typename K> hipError_t allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// KERNEL<dtype> on GRID x HEAD_BLOCK with LDS bytes of dynamic LDS; `dtype` is the caller's variable
#define GDR_HEAD_DT(KERNEL, GRID, LDS, ST, P)                                                                              \
    do {                                                                                                                   \
        hipError_t e_;                                                                                                     \
        if (dtype == GDR_NORM_F16) {                                                                                       \
            if ((e_ = allow_lds(KERNEL<GDR_NORM_F16>, LDS)) != hipSuccess) { set_error(#KERNEL, e_); return GDR_ERR_HIP; } \
            hipLaunchKernelGGL(KERNEL<GDR_NORM_F16>, GRID, dim3(HEAD_BLOCK), LDS, ST, P);                                  \
        } else if (dtype == GDR_NORM_BF16) {                                                                               \
            if ((e_ = allow_lds(KERNEL<GDR_NORM_BF16>, LDS)) != hipSuccess) { set_error(#KERNEL, e_); return GDR_ERR_HIP; } \
            hipLaunchKernelGGL(KERNEL<GDR_NORM_BF16>, GRID, dim3(HEAD_BLOCK), LDS, ST, P);                                 \
        } else {                                                                                                           \
            if ((e_ = allow_lds(KERNEL<GDR_NORM_F32>, LDS)) != hipSuccess) { set_error(#KERNEL, e_); return GDR_ERR_HIP; } \
            hipLaunchKernelGGL(KERNEL<GDR_NORM_F32>, GRID, dim3(HEAD_BLOCK), LDS, ST, P);                                  \
        }                                                                                                                  \
    } while (0)

// a fold's unknown dtype: the compute dtype's, or that of a gradient asked for (the first check of an entry point, before
// its shape's)
bool fold_bad_dtype(int32_t dtype, const FoldP& p) {
    if (bad_dtype(dtype)) return true;
    for (int k = 0; k < p.count; ++k)
        if (p.out[k] && bad_dtype(p.out_dtype[k])) return true;
    return false;
}

// the rest of a fold once the entry point has checked the shape and filled p's outputs, sizes and slabs: the workspace and
// alignment checks and the launch.  `who` is "coarsehead" or "finehead" in the error text; need: the bytes of the partial sets.
int head_fold(const char* who, const void* workspace, size_t workspace_bytes, size_t need, int32_t dtype, FoldP& p, void* stream) {
    char msg[128];
    auto say = [&](const char* what) { snprintf(msg, sizeof(msg), "%s_fold: %s", who, what); return msg; };
    if (!workspace) return invalid_arg(say("NULL workspace"));
    if (misaligned(workspace, 255)) return unsupported(say("the workspace must start on 256 bytes"));
    for (int k = 0; k < p.count; ++k)
        if (p.out[k] && misaligned(p.out[k], esize(p.out_dtype[k]) - 1)) return unsupported(say("a gradient must be aligned to its element"));
    if (workspace_bytes < need) {
        snprintf(msg, sizeof(msg), "%s_fold: workspace smaller than gdr_%s_workspace_bytes", who, who);
        return workspace_too_small(msg);
    }
    p.part = workspace;
    p.total = 0;
    for (int k = 0; k < p.count; ++k) p.total += p.size[k];
    const dim3 grid((uint32_t)div_up(p.total, (int64_t)HEAD_FOLD));
    if (dtype == GDR_NORM_F32) hipLaunchKernelGGL(head_fold_kernel<double>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(head_fold_kernel<float>, grid, dim3(HEAD_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("head_fold_kernel");
}

}  // namespace
}  // namespace gdr

// ln_rows.h — what the three LayerNorms over a row held by a lane group share (norm_rows.h ada for norm.hip and upscale.hip, groupattn.hip rowmap,
// volcond.hip modln; internal): the pieces a lane holds, the zero-filled load of a row, the tail of the backward behind the
// caller's element loop, the sum of the groups' register sums through LDS into a partial row (chain or pairwise), the fold
// of (slabs, 2, C) partials into dweight / dbias with its launch, and the dispatch on the pieces per lane.
// What differs between the norms stays in their files: how a row is addressed, the element loop that forms dxh and the
// parameter-gradient sums (m2 is (g * xh) * sc in ada and rowmap, (dy * w) * xh in modln: they round differently), the
// forward epilogues, the host checks.  Nothing here asks which norm is calling.
// Include after gdr_common.h, host_util.h and row_io.h.
#pragma once

namespace gdr {
namespace {      // the including file's own names: the fold kernel is then one kernel of each code object, not one shared symbol

constexpr int LN_BLOCK = 256;
constexpr int LN_FOLD_LANES = 16;
constexpr int LN_FOLD_CH = LN_BLOCK / LN_FOLD_LANES;

// lane l of a group of lc lanes holds, as piece k, the 8 channels behind piece_c0; on[k] says whether the row has them
__device__ __forceinline__ int piece_c0(int l, int lc, int k) { return (l + k * lc) * 8; }

template <int K>
__device__ __forceinline__ void pieces_on(int l, int lc, int C, bool (&on)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) on[k] = piece_c0(l, lc, k) < C;
}

template <int K>
__device__ __forceinline__ void fill_row(float (&x)[K][8], float val) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < 8; ++v) x[k][v] = val;
}

using gdr::load_row;    // (row_io.h's row of one lane stays visible beside this one)

// the lane's pieces of the row that starts at element `off` of base (a multiple of 8); pieces that are off hold zeros
template <int K>
__device__ __forceinline__ void load_row(const void* base, int64_t off, int dt, const bool (&on)[K], int l, int lc, float (&x)[K][8]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int v = 0; v < 8; ++v) x[k][v] = 0.f;
        if (on[k]) load8(base, off + piece_c0(l, lc, k), dt, x[k]);
    }
}

// the tail of a backward: dxh -> dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)) in place, m1 and m2 the lane's shares of
// the sums of dxh and of dxh * xh over the row
template <int K>
__device__ __forceinline__ void ln_dx(float (&dxh)[K][8], const float (&xh)[K][8], const bool (&on)[K], float m1, float m2, int lc,
                                      float inv_c, float rstd) {
    {   // the means are rounded before they are subtracted: these two products must not fuse into the subtractions below (the
        // compiler did that in some instantiations and not in others); everything else contracts as the build's mode allows
#pragma clang fp contract(off)
        m1 = group_sum(m1, lc) * inv_c;
        m2 = group_sum(m2, lc) * inv_c;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) {
#pragma unroll
            for (int v = 0; v < 8; ++v) dxh[k][v] = rstd * (dxh[k][v] - m1 - xh[k][v] * m2);
        }
}

// the sum of v[0], v[stride], ... (n <= 32 values), pairwise in a fixed order: a chain of 32 additions carries several times
// the rounding of five levels
__device__ __forceinline__ float tree_sum(const float* v, int stride, int n) {
    float a[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) a[i] = i < n ? v[i * stride] : 0.f;
#pragma unroll
    for (int w = 16; w > 0; w >>= 1) {
#pragma unroll
        for (int i = 0; i < w; ++i) a[i] += a[i + w];
    }
    return a[0];
}

// The groups' register sums -> one partial row.  Every group puts its sums of one vector of C channels at `row` = its own LDS
// row + the vector's offset (put_sums, once per vector); then sum_groups adds the G rows of `width` = vectors * C floats
// column by column in group order, as a chain or pairwise, into dst.  One barrier for all vectors; a caller that uses the
// LDS again puts a barrier behind.
template <int K>
__device__ __forceinline__ void put_sums(float* row, const float (&acc)[K][8], const bool (&on)[K], int l, int lc) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) {
#pragma unroll
            for (int v = 0; v < 8; ++v) row[piece_c0(l, lc, k) + v] = acc[k][v];
        }
}

template <bool TREE>
__device__ __forceinline__ void sum_groups(const float* sh, int width, int G, float* dst) {
    __syncthreads();
    for (int c = threadIdx.x; c < width; c += LN_BLOCK) {
        if constexpr (TREE) dst[c] = tree_sum(sh + c, width, G);
        else {
            float s = 0.f;
            for (int g = 0; g < G; ++g) s += sh[g * width + c];
            dst[c] = s;
        }
    }
}

// dweight[c] = sum_t part[t, 0, c], dbias[c] = sum_t part[t, 1, c] over the T slabs in ascending order: 16 contiguous ranges
// per column, then those 16 in order (chain) or pairwise (TREE).  One workgroup per 16 of the 2 C columns.
template <bool TREE>
__global__ __launch_bounds__(LN_BLOCK) void ln_fold_kernel(const float* __restrict__ part, int64_t T, int C, void* dweight, int w_dt,
                                                           void* dbias, int b_dt) {
    __shared__ float sh[LN_FOLD_LANES][LN_FOLD_CH];
    const int tid = threadIdx.x, ch = tid & (LN_FOLD_CH - 1), fl = tid / LN_FOLD_CH;
    const int col = blockIdx.x * LN_FOLD_CH + ch;
    float acc = 0.f;
    if (col < 2 * C) {
        const int64_t per = (T + LN_FOLD_LANES - 1) / LN_FOLD_LANES;
        const int64_t t0 = fl * per, t1 = t0 + per < T ? t0 + per : T;
#pragma unroll 4
        for (int64_t t = t0; t < t1; ++t) acc += part[t * 2 * C + col];
    }
    sh[fl][ch] = acc;
    __syncthreads();
    if (fl != 0 || col >= 2 * C) return;
    if constexpr (TREE) acc = tree_sum(&sh[0][ch], LN_FOLD_CH, LN_FOLD_LANES);
    else
        for (int i = 1; i < LN_FOLD_LANES; ++i) acc += sh[i][ch];
    if (col < C) {
        if (dweight) store1(dweight, col, w_dt, acc);
    } else if (dbias) {
        store1(dbias, col - C, b_dt, acc);
    }
}

template <bool TREE>
void launch_ln_fold(const float* part, int64_t T, int C, void* dweight, int w_dt, void* dbias, int b_dt, hipStream_t st) {
    hipLaunchKernelGGL(ln_fold_kernel<TREE>, dim3((uint32_t)((2 * C + LN_FOLD_CH - 1) / LN_FOLD_CH)), dim3(LN_BLOCK), 0, st, part, T, C,
                       dweight, w_dt, dbias, b_dt);
}

// KERNEL<1> or KERNEL<2> by the pieces per lane K (row_io.h row_shape), 256 threads
#define LN_LAUNCH_K(KERNEL, K, GRID, ST, P)                                                                                      \
    do {                                                                                                                         \
        if ((K) == 1) hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(LN_BLOCK), 0, ST, P);                                             \
        else hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(LN_BLOCK), 0, ST, P);                                                      \
    } while (0)

}  // namespace
}  // namespace gdr

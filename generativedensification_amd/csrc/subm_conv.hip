// subm_conv.hip — submanifold sparse 3-D convolution (gfx950), neighbour table, forward and backward: the one spconv layer
// the reference's point decoder builds (lightning/point_decoder/autoencoder.py, spconv.SubMConv3d(C, C, kernel_size=3) at the
// head of every Block).  Public ABI: include/gdr.h gdr_subm_*.
//
// Semantics, restated (tests/subm_ref.py holds two f64 statements of the same):
//   indices (N, 4) int32 (batch, c0, c1, c2); K = k0 k1 k2 taps, tap k = (t0 k1 + t1) k2 + t2, offset_k = t - ksize / 2.
//   nbr[k, i] = the site at coord_i + offset_k in site i's batch, or -1;  out[i] = bias + sum_k feat[nbr[k, i]] @ W[k],
//   W[k][ci][co] = weight[co, t0, t1, t2, ci] (spconv 2.x's parameter layout) — cross-correlation, as F.conv3d on the grid.
//   Sites that share a voxel: a lookup resolves to the LOWEST point index with that key (rep[i] for site i's own key), so
//   the sites of one voxel get identical output rows.  A site outside the grid is never found and has no taps.
//   backward: G = the sum of grad_out over each voxel's sites, stored at the representative (zero rows elsewhere);
//     grad_feat[j] = sum_k G[nbr[K-1-k, j]] @ W[k]^T for representatives (zero rows elsewhere),
//     grad_weight[k] = sum_r feat[nbr[k, r]]^T @ G[r],   grad_bias = column sums of grad_out.
//
// Structure.
//   table: one launch forms the int64 key ((b S0 + c0) S1 + c1) S2 + c2 per site (R = B S0 S1 S2 for a site outside the
//     grid), gdr_serial_sort orders the sites by key (stable), one launch runs a lower-bound binary search per (site, tap)
//     with ceil(log2 N) + 1 steps — a trip count the host knows.  The neighbour coordinate is checked per axis against
//     [0, S) BEFORE the key is formed, so a step off a face never aliases into the next row or batch.
//   product kernel (forward and grad_feat): output-stationary.  A 256-thread workgroup owns 64 sites x 64 output channels;
//     per tap it stages the 64 gathered rows (zeros for -1) and the 64 x 32 slice of W[k] in LDS, 32 input channels at a
//     time, and every wave accumulates its 32 x 32 quarter in f32 MFMA registers (16x16x32 f16 / bf16, 16x16x4 f32).  A tap
//     with no neighbour in the tile is skipped by the whole workgroup.  One store per output element, no atomics.
//     grad_feat is the same kernel on G with the weight transposed and tap-mirrored by one small launch.
//   grad_weight: one workgroup per (tap, 64 input channels, 64 output channels) walks all N rows 64 at a time, transposing
//     the gathered feature rows and the G rows into LDS so that the row index is the MFMA's sum index; no atomics, no
//     partial buffers.
//   G is kept in `planes` words of the operand type whose sum is the f32 sum (1 for f32, 2 for f16, 3 for bf16): with one
//     site per voxel the further planes are zero, with several the 16-bit MFMA still sees the f32 sum.
// Tile sizes are an unmeasured choice.
#include "gdr_common.h"
#include "half_bits.h"
#include "host_util.h"

namespace gdr {
namespace {

constexpr int SC_BLOCK = GDR_BLOCK;
constexpr int SC_TM = 64;      // sites per workgroup
constexpr int SC_TN = 64;      // output channels per workgroup
constexpr int SC_KC = 32;      // reduction elements staged per step
constexpr int SC_RC = 64;      // rows per step of grad_weight
constexpr int SC_BIAS_BLOCKS = 256;

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// DT: GDR_SUBM_F16, GDR_SUBM_BF16, GDR_SUBM_F32
template <int DT> struct El : Stored<DT> {
    static constexpr int PLANES = DT == GDR_SUBM_F32 ? 1 : (DT == GDR_SUBM_F16 ? 2 : 3);
};

// VE elements from global memory as one 16-byte vector (vec) or one by one
template <int DT> __device__ __forceinline__ uint4 load_vec(const typename El<DT>::type* p, int vec) {
    if (vec) return *reinterpret_cast<const uint4*>(p);
    using E = typename El<DT>::type;
    union { uint4 v; E e[El<DT>::VE]; } u;
#pragma unroll
    for (int i = 0; i < El<DT>::VE; ++i) u.e[i] = p[i];
    return u.v;
}

// D += A B for one 16 x 16 tile over `SC_KC` (half types: one 16x16x32 step; f32: 8 steps of 16x16x4).  ra / rb: the LDS rows
// of this lane's A row and B column, both contiguous along the sum index.
template <int DT> __device__ __forceinline__ void mma_kc(const typename El<DT>::type* ra, const typename El<DT>::type* rb, int quad,
                                                         f32x4& acc) {
    if constexpr (DT == GDR_SUBM_F32) {
#pragma unroll
        for (int s = 0; s < SC_KC / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[4 * s + quad], rb[4 * s + quad], acc, 0, 0, 0);
    } else {
        const uint4 a = *reinterpret_cast<const uint4*>(ra + 8 * quad), b = *reinterpret_cast<const uint4*>(rb + 8 * quad);
        if constexpr (DT == GDR_SUBM_F16)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
        else
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
}

// ---- neighbour table ------------------------------------------------------------------------------------------------
struct TableP {
    const int32_t* idx;      // (N, 4)
    int64_t* key;            // N
    const int64_t* order;    // N, sites in key order (from gdr_serial_sort)
    int32_t* nbr;            // (K, N)
    int32_t* rep;            // N
    int32_t* order32;        // N
    int64_t R;               // B S0 S1 S2: the key of a site outside the grid
    int32_t n, B, S0, S1, S2, k0, k1, k2, steps;
};

__device__ __forceinline__ bool site_in_grid(const TableP& p, int b, int c0, int c1, int c2) {
    return (uint32_t)b < (uint32_t)p.B && (uint32_t)c0 < (uint32_t)p.S0 && (uint32_t)c1 < (uint32_t)p.S1 && (uint32_t)c2 < (uint32_t)p.S2;
}

__device__ __forceinline__ int64_t site_key(const TableP& p, int b, int c0, int c1, int c2) {
    return (((int64_t)b * p.S0 + c0) * p.S1 + c1) * p.S2 + c2;
}

__global__ __launch_bounds__(SC_BLOCK) void subm_key_kernel(const TableP p) {
    const int64_t i = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    const int4 v = reinterpret_cast<const int4*>(p.idx)[i];
    p.key[i] = site_in_grid(p, v.x, v.y, v.z, v.w) ? site_key(p, v.x, v.y, v.z, v.w) : p.R;
}

// blockIdx.y = tap
__global__ __launch_bounds__(SC_BLOCK) void subm_lookup_kernel(const TableP p) {
    const int64_t i = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    const int k = blockIdx.y, K = p.k0 * p.k1 * p.k2;
    const int t2 = k % p.k2, t1 = (k / p.k2) % p.k1, t0 = k / (p.k2 * p.k1);
    const bool centre = k == K / 2;
    if (centre) {   // the sort's int64 order as the int32 run table of the backward
        const int64_t o = p.order[i];
        p.order32[i] = (uint64_t)o < (uint64_t)p.n ? (int32_t)o : 0;
    }
    const int4 v = reinterpret_cast<const int4*>(p.idx)[i];
    int found = -1;
    if (site_in_grid(p, v.x, v.y, v.z, v.w)) {
        // (64-bit sums: a coordinate near INT_MAX cannot wrap; an in-grid one is far below it anyway)
        const int64_t n0 = (int64_t)v.y + t0 - p.k0 / 2, n1 = (int64_t)v.z + t1 - p.k1 / 2, n2 = (int64_t)v.w + t2 - p.k2 / 2;
        if (n0 >= 0 && n0 < p.S0 && n1 >= 0 && n1 < p.S1 && n2 >= 0 && n2 < p.S2) {
            const int64_t q = site_key(p, v.x, (int)n0, (int)n1, (int)n2);
            int lo = 0, hi = p.n;
            for (int s = 0; s < p.steps; ++s) {      // lower bound: ceil(log2 N) + 1 steps always suffice
                if (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    const uint64_t o = (uint64_t)p.order[mid];
                    const int64_t km = o < (uint64_t)p.n ? p.key[o] : p.R;
                    if (km < q) lo = mid + 1; else hi = mid;
                }
            }
            if (lo < p.n) {
                const uint64_t o = (uint64_t)p.order[lo];
                if (o < (uint64_t)p.n && p.key[o] == q) found = (int)o;
            }
        }
    }
    p.nbr[(int64_t)k * p.n + i] = found;
    if (centre) p.rep[i] = found >= 0 ? found : (int)i;
}

// ---- the product kernel: out (N, CB) = [bias] + sum_k sum_planes A[plane][nbr[k, .]] (., CA) @ W[., k, .]^T, W (CB, K, CA) ------
struct ConvP {
    const void* a;           // (planes, N, CA): rows through a_stride, planes through a_plane (elements)
    const void* w;           // (CB, K, CA) dense
    const void* bias;        // CB or NULL
    const int32_t* nbr;      // (K, N)
    const int32_t* only_rep; // NULL, or rep: a site with rep[i] != i gets a zero row
    void* out;               // (N, CB) dense
    int64_t a_stride, a_plane;
    int32_t n, CA, CB, K, planes, a_vec;
};

template <int DT>
__global__ __launch_bounds__(SC_BLOCK) void subm_product_kernel(const ConvP p) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE, LDW = SC_KC + VE, VPR = SC_KC / VE;
    __shared__ __attribute__((aligned(16))) E sA[SC_TM * LDW];
    __shared__ __attribute__((aligned(16))) E sW[SC_TN * LDW];
    __shared__ int32_t sNbr[SC_TM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * SC_TM;
    const int col0 = blockIdx.y * SC_TN;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const E* A = (const E*)p.a;
    const E* W = (const E*)p.w;
    f32x4 acc[2][2];      // [channel tile][site tile]: D rows = output channels, D columns = sites
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < p.K; ++k) {
        int nb = -1;
        if (tid < SC_TM) {
            const int64_t r = row0 + tid;
            if (r < p.n) {
                nb = p.nbr[(int64_t)k * p.n + r];
                if ((uint32_t)nb >= (uint32_t)p.n) nb = -1;
            }
            sNbr[tid] = nb;
        }
        if (!__syncthreads_or(nb >= 0)) continue;      // no neighbour in the tile under this tap (uniform over the workgroup)
        // f32: a tap's CA products are summed on their own and the tap sums added up, so that no fma chain is longer than
        // CA + K terms (one chain over K * CA = 4320 terms at C = 160 loses ~sqrt(K CA) eps, visible at fp32 rounding)
        f32x4 part[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) part[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int pl = 0; pl < p.planes; ++pl) {
            const E* Ap = A + (int64_t)pl * p.a_plane;
            for (int c0 = 0; c0 < p.CA; c0 += SC_KC) {
                for (int v = tid; v < SC_TM * VPR; v += SC_BLOCK) {
                    const int r = v / VPR, c = c0 + (v % VPR) * VE, src = sNbr[r];
                    uint4 val = make_uint4(0, 0, 0, 0);
                    if (src >= 0 && c < p.CA) val = load_vec<DT>(Ap + (int64_t)src * p.a_stride + c, p.a_vec);
                    *reinterpret_cast<uint4*>(sA + r * LDW + (v % VPR) * VE) = val;
                }
                for (int v = tid; v < SC_TN * VPR; v += SC_BLOCK) {
                    const int r = v / VPR, c = c0 + (v % VPR) * VE, co = col0 + r;
                    uint4 val = make_uint4(0, 0, 0, 0);
                    if (co < p.CB && c < p.CA) val = *reinterpret_cast<const uint4*>(W + ((int64_t)co * p.K + k) * p.CA + c);
                    *reinterpret_cast<uint4*>(sW + r * LDW + (v % VPR) * VE) = val;
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        mma_kc<DT>(sW + (wn + 16 * j + l16) * LDW, sA + (wm + 16 * i + l16) * LDW, quad,
                                   DT == GDR_SUBM_F32 ? part[j][i] : acc[j][i]);
                __syncthreads();
            }
        }
        if constexpr (DT == GDR_SUBM_F32) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[j][i] += part[j][i];
        }
    }
    // D: column = lane & 15 (site), rows 4 * quad .. + 3 (output channels): one packed store of 4 channels per tile
    E* out = (E*)p.out;
    const E* bias = (const E*)p.bias;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t site = row0 + wm + 16 * i + l16;
        if (site >= p.n) continue;
        const bool zero = p.only_rep && p.only_rep[site] != (int32_t)site;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int co = col0 + wn + 16 * j + 4 * quad;
            if (co >= p.CB) continue;       // CB is a multiple of 8: the 4 channels are in or out together
            E o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x = acc[j][i][e];
                if (bias) x += up<DT>(bias[co + e]);
                o[e] = down<DT>(zero ? 0.f : x);
            }
            E* dst = out + site * p.CB + co;
            if constexpr (DT == GDR_SUBM_F32) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            else *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
        }
    }
}

// ---- backward helpers -----------------------------------------------------------------------------------------------
// wt[ci][K-1-k][co] = w[co][k][ci]
template <typename E>
__global__ __launch_bounds__(SC_BLOCK) void subm_wt_kernel(const E* w, E* wt, int CI, int CO, int K, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int co = (int)(t % CO), k = (int)((t / CO) % K), ci = (int)(t / ((int64_t)CO * K));
    wt[t] = w[((int64_t)co * K + (K - 1 - k)) * CI + ci];
}

// G planes: thread = (position j in key order, chunk of 4 channels).  The site at j sums its voxel's run if it is the
// representative (the first of the run: the sort is stable) and gets zero rows otherwise.
template <int DT>
__global__ __launch_bounds__(SC_BLOCK) void subm_g_kernel(const void* go_, const int32_t* order, const int32_t* rep, void* G_, int n, int C) {
    using E = typename El<DT>::type;
    constexpr int P = El<DT>::PLANES;
    const E* go = (const E*)go_;
    E* G = (E*)G_;
    const int cpr = C / 4;
    const int64_t t = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (t >= (int64_t)n * cpr) return;
    const int j = (int)(t / cpr), c = (int)(t % cpr) * 4;
    const int32_t site = order[j];
    if ((uint32_t)site >= (uint32_t)n) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (rep[site] == site) {
        for (int jj = j; jj < n; ++jj) {          // the run is contiguous in key order, members in ascending point index
            const int32_t m = order[jj];
            if ((uint32_t)m >= (uint32_t)n || (jj > j && rep[m] != site)) break;
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += up<DT>(go[(int64_t)m * C + c + e]);
        }
    }
#pragma unroll
    for (int pl = 0; pl < P; ++pl)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const E q = down<DT>(s[e]);
            G[((int64_t)pl * n + site) * C + c + e] = q;
            s[e] -= up<DT>(q);
        }
}

// grad_bias: per-block column sums of 4-row strides, then one block adds the partials in order
template <int DT>
__global__ __launch_bounds__(SC_BLOCK) void subm_bias_part_kernel(const void* go_, float* part, int n, int C) {
    const typename El<DT>::type* go = (const typename El<DT>::type*)go_;
    const int64_t rows = ((int64_t)n + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * rows;
    const int64_t r1 = r0 + rows < n ? r0 + rows : n;
    for (int c = threadIdx.x; c < C; c += SC_BLOCK) {
        float s = 0.f;
        for (int64_t r = r0; r < r1; ++r) s += up<DT>(go[r * C + c]);
        part[(int64_t)blockIdx.x * C + c] = s;
    }
}

__global__ __launch_bounds__(SC_BLOCK) void subm_bias_sum_kernel(const float* part, float* out, int blocks, int C) {
    const int c = blockIdx.x * SC_BLOCK + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int b = 0; b < blocks; ++b) s += part[(int64_t)b * C + c];
    out[c] = s;
}

// grad_weight[co][k][ci] = sum_r sum_planes G[plane][r][co] feat[nbr[k, r]][ci]; blockIdx = (tap, ci tile, co tile)
struct GwP {
    const void* feat; const void* G; const int32_t* nbr; float* gw;
    int64_t f_stride, g_plane;
    int32_t n, CI, CO, K, planes, f_vec;
};

template <int DT>
__global__ __launch_bounds__(SC_BLOCK) void subm_gw_kernel(const GwP p) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE, LDW = SC_RC + VE, VPR = 64 / VE;
    __shared__ __attribute__((aligned(16))) E sF[64 * LDW];     // [ci][row]
    __shared__ __attribute__((aligned(16))) E sG[64 * LDW];     // [co][row]
    __shared__ int32_t sNbr[SC_RC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int k = blockIdx.x, ci0 = blockIdx.y * 64, co0 = blockIdx.z * 64;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const E* F = (const E*)p.feat;
    const E* G = (const E*)p.G;
    f32x4 acc[2][2];      // [ci tile][co tile]: D rows = input channels, D columns = output channels
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t r0 = 0; r0 < p.n; r0 += SC_RC) {
        int nb = -1;
        if (tid < SC_RC) {
            const int64_t r = r0 + tid;
            if (r < p.n) {
                nb = p.nbr[(int64_t)k * p.n + r];
                if ((uint32_t)nb >= (uint32_t)p.n) nb = -1;
            }
            sNbr[tid] = nb;
        }
        if (!__syncthreads_or(nb >= 0)) continue;
        f32x4 part[2][2];     // f32: the 64 rows of a step are summed on their own (no fma chain over all N rows)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) part[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int v = tid; v < SC_RC * VPR; v += SC_BLOCK) {
            const int r = v / VPR, cl = (v % VPR) * VE, src = sNbr[r];
            union { uint4 v; E e[VE]; } u;
            u.v = make_uint4(0, 0, 0, 0);
            if (src >= 0 && ci0 + cl < p.CI) u.v = load_vec<DT>(F + (int64_t)src * p.f_stride + ci0 + cl, p.f_vec);
#pragma unroll
            for (int e = 0; e < VE; ++e) sF[(cl + e) * LDW + r] = u.e[e];
        }
        for (int pl = 0; pl < p.planes; ++pl) {
            for (int v = tid; v < SC_RC * VPR; v += SC_BLOCK) {
                const int r = v / VPR, cl = (v % VPR) * VE;
                union { uint4 v; E e[VE]; } u;
                u.v = make_uint4(0, 0, 0, 0);
                if (sNbr[r] >= 0 && co0 + cl < p.CO)
                    u.v = *reinterpret_cast<const uint4*>(G + (int64_t)pl * p.g_plane + (r0 + r) * p.CO + co0 + cl);
#pragma unroll
                for (int e = 0; e < VE; ++e) sG[(cl + e) * LDW + r] = u.e[e];
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SC_RC / SC_KC; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        mma_kc<DT>(sF + (wm + 16 * i + l16) * LDW + s * SC_KC, sG + (wn + 16 * j + l16) * LDW + s * SC_KC, quad,
                                   DT == GDR_SUBM_F32 ? part[i][j] : acc[i][j]);
            __syncthreads();
        }
        if constexpr (DT == GDR_SUBM_F32) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];
        }
    }
    // D: column = lane & 15 (co), rows 4 * quad .. + 3 (ci): one float4 per tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = co0 + wn + 16 * j + l16;
        if (co >= p.CO) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ci = ci0 + wm + 16 * i + 4 * quad;
            if (ci >= p.CI) continue;
            *reinterpret_cast<float4*>(p.gw + ((int64_t)co * p.K + k) * p.CI + ci) =
                make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
const char* subm_check(const gdr_subm_args* a) {
    if (!a) return "subm: NULL arguments";
    if (a->dtype != GDR_SUBM_F16 && a->dtype != GDR_SUBM_BF16 && a->dtype != GDR_SUBM_F32) return "subm: unknown dtype";
    if (a->N < 0 || a->N > GDR_SUBM_MAX_POINTS) return "subm: N must be in 0..GDR_SUBM_MAX_POINTS";
    if (a->Cin < 8 || a->Cin > GDR_SUBM_MAX_CHANNELS || a->Cin % 8 || a->Cout < 8 || a->Cout > GDR_SUBM_MAX_CHANNELS || a->Cout % 8)
        return "subm: Cin and Cout must be multiples of 8 in 8..512";
    if (a->K < 1 || a->K > GDR_SUBM_MAX_TAPS) return "subm: K must be in 1..125";
    return nullptr;
}

int planes_of(int dtype) { return dtype == GDR_SUBM_F32 ? 1 : (dtype == GDR_SUBM_F16 ? 2 : 3); }

struct BwdWs { size_t G, wt, part, bytes; };

BwdWs bwd_workspace(const gdr_subm_args* a) {
    BwdWs w;
    size_t at = 0;
    w.G = at; at += align_up((size_t)planes_of(a->dtype) * (size_t)a->N * a->Cout * esize(a->dtype));
    w.wt = at; at += align_up((size_t)a->K * a->Cin * a->Cout * esize(a->dtype));
    w.part = at; at += align_up((size_t)SC_BIAS_BLOCKS * a->Cout * sizeof(float));
    w.bytes = at;
    return w;
}

int row_vec(const void* ptr, int64_t stride, int dtype) {
    return !((uintptr_t)ptr & 15u) && (stride * (int64_t)esize(dtype)) % 16 == 0;
}

#define GDR_SUBM_DT(KERNEL, ...)                                                                          \
    do {                                                                                                  \
        if (dtype == GDR_SUBM_F16) hipLaunchKernelGGL(KERNEL<GDR_SUBM_F16>, __VA_ARGS__);              \
        else if (dtype == GDR_SUBM_BF16) hipLaunchKernelGGL(KERNEL<GDR_SUBM_BF16>, __VA_ARGS__);       \
        else hipLaunchKernelGGL(KERNEL<GDR_SUBM_F32>, __VA_ARGS__);                                       \
    } while (0)

void launch_product(int dtype, const ConvP& p, hipStream_t st) {
    const dim3 grid(div_up(p.n, SC_TM), div_up(p.CB, SC_TN));
    GDR_SUBM_DT(subm_product_kernel, grid, dim3(SC_BLOCK), 0, st, p);
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_subm_table_bytes(int64_t N) {
    if (N < 0 || N > GDR_SUBM_MAX_POINTS) {
        invalid_arg("subm_table_bytes: N must be in 0..GDR_SUBM_MAX_POINTS");
        return 0;
    }
    const size_t sort = gdr_serial_sort_bytes(1, N);
    if (!sort) return 0;
    return 3 * align_up((size_t)N * 8) + align_up(sort) + 256;      // keys, order, inverse, the sort's own
}

int gdr_subm_build_table(const int32_t* indices, int64_t N, const int32_t* spatial_shape, int32_t batch_size, const int32_t* ksize,
                         void* workspace, size_t workspace_bytes, int32_t* nbr, int32_t* rep, int32_t* order, void* stream) {
    if (N < 0 || N > GDR_SUBM_MAX_POINTS) return invalid_arg("subm_build_table: N must be in 0..GDR_SUBM_MAX_POINTS");
    if (!spatial_shape || !ksize) return invalid_arg("subm_build_table: NULL spatial_shape or kernel size");
    if (batch_size < 1) return invalid_arg("subm_build_table: batch_size must be >= 1");
    int64_t R = batch_size;
    for (int d = 0; d < 3; ++d) {
        if (ksize[d] != 1 && ksize[d] != 3 && ksize[d] != 5)
            return invalid_arg("subm_build_table: kernel size must be 1, 3 or 5 per axis");
        if (spatial_shape[d] < 1) return invalid_arg("subm_build_table: spatial_shape must be >= 1 per axis");
        if (R > (INT64_C(1) << 61) / spatial_shape[d])
            return invalid_arg("subm_build_table: batch_size * spatial_shape exceeds 2^61 keys");
        R *= spatial_shape[d];
    }
    if (N == 0) return GDR_OK;
    if (!indices || !workspace || !nbr || !rep || !order) return invalid_arg("subm_build_table: NULL argument");
    if (misaligned(indices, 15) || misaligned(workspace, 255) || misaligned(nbr, 3) || misaligned(rep, 3) ||
        misaligned(order, 3))
        return invalid_arg("subm_build_table: unaligned buffer");
    const size_t need = gdr_subm_table_bytes(N);
    if (!need || workspace_bytes < need - 256)
        return workspace_too_small("subm_build_table: workspace smaller than gdr_subm_table_bytes");
    char* base = (char*)workspace;
    const size_t col = align_up((size_t)N * 8);
    int64_t* key = (int64_t*)base;
    int64_t* ord = (int64_t*)(base + col);
    int64_t* inv = (int64_t*)(base + 2 * col);
    void* sort_ws = base + 3 * col;
    int bits = 1;
    while (bits < 63 && (INT64_C(1) << bits) <= R) ++bits;      // keys 0..R
    int steps = 1;
    while ((INT64_C(1) << (steps - 1)) < N) ++steps;             // ceil(log2 N) + 1
    TableP p = {};
    p.idx = indices; p.key = key; p.order = ord; p.nbr = nbr; p.rep = rep; p.order32 = order; p.R = R;
    p.n = (int32_t)N; p.B = batch_size; p.S0 = spatial_shape[0]; p.S1 = spatial_shape[1]; p.S2 = spatial_shape[2];
    p.k0 = ksize[0]; p.k1 = ksize[1]; p.k2 = ksize[2]; p.steps = steps;
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = div_up(N, SC_BLOCK);
    hipLaunchKernelGGL(subm_key_kernel, dim3(blocks), dim3(SC_BLOCK), 0, st, p);
    if (const int rc = launch_status("subm_key_kernel")) return rc;
    if (const int rc = gdr_serial_sort(key, 1, N, bits, sort_ws, workspace_bytes - 3 * col, ord, inv, stream)) return rc;
    hipLaunchKernelGGL(subm_lookup_kernel, dim3(blocks, p.k0 * p.k1 * p.k2), dim3(SC_BLOCK), 0, st, p);
    return launch_status("subm_lookup_kernel");
}

int gdr_subm_conv_forward(const gdr_subm_args* a, const void* feat, int64_t feat_stride, const int32_t* nbr, const void* weight,
                          const void* bias, void* out, void* stream) {
    if (const char* why = subm_check(a)) return invalid_arg(why);
    if (a->N == 0) return GDR_OK;
    if (!feat || !nbr || !weight || !out) return invalid_arg("subm_conv_forward: NULL argument");
    if (feat_stride < a->Cin) return invalid_arg("subm_conv_forward: feature row stride smaller than Cin");
    const size_t es = esize(a->dtype);
    if (misaligned(feat, es - 1) || misaligned(bias, es - 1) || misaligned(weight, 15) || misaligned(out, 15) ||
        misaligned(nbr, 3))
        return invalid_arg("subm_conv_forward: unaligned buffer");
    ConvP p = {};
    p.a = feat; p.w = weight; p.bias = bias; p.nbr = nbr; p.only_rep = nullptr; p.out = out;
    p.a_stride = feat_stride; p.a_plane = 0; p.n = a->N; p.CA = a->Cin; p.CB = a->Cout; p.K = a->K; p.planes = 1;
    p.a_vec = row_vec(feat, feat_stride, a->dtype);
    launch_product(a->dtype, p, (hipStream_t)stream);
    return launch_status("subm_product_kernel");
}

size_t gdr_subm_backward_bytes(const gdr_subm_args* a) {
    if (const char* why = subm_check(a)) { invalid_arg(why); return 0; }
    return bwd_workspace(a).bytes + 256;
}

int gdr_subm_conv_backward(const gdr_subm_args* a, const void* grad_out, const void* feat, int64_t feat_stride, const int32_t* nbr,
                           const int32_t* rep, const int32_t* order, const void* weight, void* workspace, size_t workspace_bytes,
                           void* grad_feat, float* grad_weight, float* grad_bias, void* stream) {
    if (const char* why = subm_check(a)) return invalid_arg(why);
    if (a->N == 0) return GDR_OK;
    if (!grad_feat && !grad_weight && !grad_bias) return GDR_OK;
    const size_t es = esize(a->dtype);
    if (!grad_out || misaligned(grad_out, 15)) return invalid_arg("subm_conv_backward: grad_out NULL or unaligned");
    const hipStream_t st = (hipStream_t)stream;
    const BwdWs ws = bwd_workspace(a);
    char* base = (char*)workspace;
    const int N = a->N, P = planes_of(a->dtype), dtype = a->dtype;
    if (grad_feat || grad_weight) {
        if (!nbr || !rep || !order || !workspace) return invalid_arg("subm_conv_backward: NULL table or workspace");
        if (misaligned(workspace, 255) || misaligned(nbr, 3) || misaligned(rep, 3) || misaligned(order, 3))
            return invalid_arg("subm_conv_backward: unaligned buffer");
        if (grad_feat && (!weight || misaligned(weight, 15) || misaligned(grad_feat, 15)))
            return invalid_arg("subm_conv_backward: weight / grad_feat NULL or unaligned");
        if (grad_weight && (!feat || misaligned(feat, es - 1) || feat_stride < a->Cin || misaligned(grad_weight, 15)))
            return invalid_arg("subm_conv_backward: feat / grad_weight NULL, unaligned or row stride smaller than Cin");
    } else if (!workspace || misaligned(workspace, 255)) {
        return invalid_arg("subm_conv_backward: workspace NULL or unaligned");
    }
    if (workspace_bytes < ws.bytes)
        return workspace_too_small("subm_conv_backward: workspace smaller than gdr_subm_backward_bytes");
    if (grad_bias) {
        int blocks = div_up(N, 64);
        if (blocks > SC_BIAS_BLOCKS) blocks = SC_BIAS_BLOCKS;
        float* part = (float*)(base + ws.part);
        GDR_SUBM_DT(subm_bias_part_kernel, dim3(blocks), dim3(SC_BLOCK), 0, st, grad_out, part, N, a->Cout);
        hipLaunchKernelGGL(subm_bias_sum_kernel, dim3(div_up(a->Cout, SC_BLOCK)), dim3(SC_BLOCK), 0, st, (const float*)part, grad_bias, blocks,
                           a->Cout);
    }
    if (grad_feat || grad_weight) {
        void* G = base + ws.G;
        const int gblocks = div_up((int64_t)N * (a->Cout / 4), SC_BLOCK);
        GDR_SUBM_DT(subm_g_kernel, dim3(gblocks), dim3(SC_BLOCK), 0, st, grad_out, order, rep, G, N, a->Cout);
        if (grad_feat) {
            void* wt = base + ws.wt;
            const int64_t total = (int64_t)a->K * a->Cin * a->Cout;
            if (es == 4)
                hipLaunchKernelGGL(subm_wt_kernel<float>, dim3(div_up(total, SC_BLOCK)), dim3(SC_BLOCK), 0, st, (const float*)weight, (float*)wt,
                                   a->Cin, a->Cout, a->K, total);
            else
                hipLaunchKernelGGL(subm_wt_kernel<uint16_t>, dim3(div_up(total, SC_BLOCK)), dim3(SC_BLOCK), 0, st, (const uint16_t*)weight,
                                   (uint16_t*)wt, a->Cin, a->Cout, a->K, total);
            ConvP p = {};
            p.a = G; p.w = wt; p.bias = nullptr; p.nbr = nbr; p.only_rep = rep; p.out = grad_feat;
            p.a_stride = a->Cout; p.a_plane = (int64_t)N * a->Cout; p.n = N; p.CA = a->Cout; p.CB = a->Cin; p.K = a->K; p.planes = P;
            p.a_vec = 1;
            launch_product(a->dtype, p, st);
        }
        if (grad_weight) {
            GwP p = {};
            p.feat = feat; p.G = G; p.nbr = nbr; p.gw = grad_weight; p.f_stride = feat_stride; p.g_plane = (int64_t)N * a->Cout;
            p.n = N; p.CI = a->Cin; p.CO = a->Cout; p.K = a->K; p.planes = P; p.f_vec = row_vec(feat, feat_stride, a->dtype);
            const dim3 grid(a->K, div_up(a->Cin, 64), div_up(a->Cout, 64));
            GDR_SUBM_DT(subm_gw_kernel, grid, dim3(SC_BLOCK), 0, st, p);
        }
    }
    return launch_status("subm backward kernels");
}

}  // extern "C"

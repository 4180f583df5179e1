// deconv3d.hip — [LayerNorm +] 2x transposed convolution of channels-last volumes (gfx950), forward and every gradient: the
// nn.LayerNorm(embed_dim) and nn.ConvTranspose3d(embed_dim, out_dim, kernel_size=2, stride=2) at the tail of the reference's
// VolTransformer (lightning/network.py), from the (B, D, H, W, Cin) rows the bound blocks hand on to the (B, 2D, 2H, 2W, Cout)
// rows every later step reads.  Public ABI: include/gdr.h gdr_deconv3d_*.
//
// Semantics, restated (tests/deconv3d_ref.py holds the f64 statement):
//   x (B, D, H, W, Cin) rows, weight (Cin, Cout, 8) as nn.ConvTranspose3d stores it, tap t = (i 2 + j) 2 + k.
//   n[p][c]   = x[p][c]                                                      without the norm
//             = (x[p][c] - mean_p) rstd_p gamma[c] + beta[c]                  with it (biased variance over the Cin channels of row p)
//   out[child(p, t)][co] = bias[co] + sum_c n[p][c] weight[c][co][t],   child((b, d, h, w), (i, j, k)) = (b, 2d + i, 2h + j, 2w + k):
//   kernel 2, stride 2: every child voxel has exactly one parent and one tap, so the layer is ONE GEMM, (B D H W) x Cin times
//   Cin x (8 Cout), with no halo and no zero fill.
//   g_n[p][c] = sum_t sum_co g[child(p, t)][co] weight[c][co][t];  grad_x = g_n, or the LayerNorm's
//               rstd (gamma g_n - mean_c(gamma g_n) - xhat mean_c(gamma g_n xhat)) with xhat = (x - mean) rstd
//   grad_weight[c][co][t] = sum_p n[p][c] g[child(p, t)][co]  (n rounded as the forward's operand was)
//   grad_bias = column sums of g;  grad_gamma[c] = sum_p g_n[p][c] xhat[p][c];  grad_beta[c] = sum_p g_n[p][c]
//
// Structure (256 threads = 4 waves everywhere; D rows are channels, D columns voxels, as in conv3d.hip).
//   pack: one launch rounds the weight to the compute dtype and lays it out [t][Cout][Cin] (forward) or [t][Cin][Cout]
//     (transposed, for g_n): contiguous along the sum index.
//   forward: a workgroup owns DC_ROWS = 64 consecutive parent rows times one tile of output channels (64; 32 for f32).  It
//     first takes mean and rstd of its rows (one pass over the row, sum and sum of squares in f64), then walks Cin in chunks of 64 bytes: the
//     chunk of the 64 rows is normalised, affine-applied, rounded ONCE to the compute dtype (f32 operands: kept in f64) and
//     staged in LDS once, next to the chunk of all 8 taps' weights; wave w owns the taps (i, j) = (w / 2, w % 2), k = 0, 1,
//     so all 8 taps reuse the one A image, and the two child rows a wave writes per parent are adjacent in memory
//     (2 Cout elements).  Epilogue: bias joins the accumulator, one rounding, packed stores of 4 channels.
//   grad_input: the same shape with the 8 child rows gathered as one K = 8 Cout row and the transposed weight; a workgroup
//     owns WHOLE rows (all Cin channels of 16 VT rows, VT = 4 / 2 / 1 for Cin <= 256 / 512 / 1024, every wave 16 tiles) because
//     the LayerNorm backward in its epilogue needs two row-wide sums; it also leaves its partial column sums for grad_gamma
//     and grad_beta.
//   grad_weight: a workgroup owns (tap, 64 input channels, 64 output channels, slab of parent rows); it walks the slab 64
//     rows at a time, transposing the normalised x rows and the gathered grad_out rows into LDS so that the voxel is the
//     MFMA's sum index, and writes a partial tile; one fold launch adds the slabs in order and writes the module's layout.
//   column sums (grad_bias; grad_gamma / grad_beta from the partials): per-block partials in f64, one fold launch in block order.
// No atomics.  Tile sizes are an unmeasured choice.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "mfma_rows.h"

namespace gdr {
namespace {

constexpr int DC_BLOCK = GDR_BLOCK;
constexpr int DC_ROWS = GDR_DECONV3D_TILE_ROWS;   // parent rows per workgroup of the forward
constexpr int DC_TAPS = 8;
constexpr int DC_ROWV = 5;                        // 16-byte vectors per LDS row of 64 bytes: 4 of data, 1 of padding
constexpr int DC_GROUP = 256;                     // grad_input: channels staged per pass, 64 per wave
constexpr int DC_GT = 64;                         // grad_weight: channels per tile side, parent rows per step
constexpr int DC_MAX_SLABS = 8;
constexpr int DC_SLAB_MIN = GDR_DECONV3D_SLAB_MIN;      // parent rows per slab below which no further slab is cut
constexpr int DC_SUM_BLOCKS = 1024;
constexpr int DC_FOLD = 16;                       // fold: channels per block, and segments of the partials per channel
static_assert(DC_ROWS == 64 && DC_BLOCK == 256, "4 waves, 4 voxel tiles of 16 rows, 4 threads per row");

// the forward's normalised operand: the compute dtype, or f64 for f32 rows (fed to the f64 MFMA unrounded)
template <int DT> struct Op {
    using type = typename std::conditional<DT == GDR_NORM_F32, double, uint16_t>::type;
    static constexpr int V = El<DT>::KC * (int)sizeof(type) / 16;        // 16-byte vectors per LDS row of one chunk
    static constexpr int CT = DT == GDR_NORM_F32 ? 32 : 64;               // output channels per workgroup of the forward
    using scalar = typename std::conditional<DT == GDR_NORM_F32, double, float>::type;      // the accumulator's element
};

// the normalised operand of one MFMA tile column: 16 bytes of the compute dtype, or 4 doubles
template <int DT> struct Frag { uint4 v[Op<DT>::V / 4]; };

template <int DT> __device__ __forceinline__ void mma_op(const uint4& w, const Frag<DT>& n, typename El<DT>::acc& acc) {
    if constexpr (DT == GDR_NORM_F32) {
        const f32x4 fw = __builtin_bit_cast(f32x4, w);
        const double2 lo = __builtin_bit_cast(double2, n.v[0]), hi = __builtin_bit_cast(double2, n.v[1]);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fw[0], lo.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fw[1], lo.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fw[2], hi.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fw[3], hi.y, acc, 0, 0, 0);
    } else {
        mma_row<DT>(w, n.v[0], acc);
    }
}

// (b, d, h, w) of parent row r of a (B, D, H, W) volume; the caller has checked r < B D H W, so b < B
struct Vox { int64_t b; int d, h, w; };
__device__ __forceinline__ Vox vox_of(int64_t r, int D, int H, int W) {
    const uint32_t u = (uint32_t)r;
    Vox v;
    v.w = u % W; v.h = (u / W) % H; v.d = (u / W / H) % D; v.b = u / W / H / D;
    return v;
}

// the child row of tap t = (i 2 + j) 2 + k: every axis from its own coordinate
__device__ __forceinline__ int64_t child_of(const Vox& v, int t, int D, int H, int W) {
    return ((v.b * (2 * D) + 2 * v.d + (t >> 2)) * (2 * H) + 2 * v.h + ((t >> 1) & 1)) * (int64_t)(2 * W) + 2 * v.w + (t & 1);
}

// the normalised 16-byte vector of row values at channels c .. c + VE - 1
template <int DT>
__device__ __forceinline__ void normalise(const uint4& raw, int c, double mean, double rstd, const void* ln_w, int ln_w_dtype,
                                          const void* ln_b, int ln_b_dtype, typename Op<DT>::type* dst) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE;
    union { uint4 v; E e[VE]; } u;
    u.v = raw;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        if constexpr (DT == GDR_NORM_F32) {
            double y = ((double)u.e[e] - mean) * rstd;
            if (ln_w) y *= (double)load1(ln_w, c + e, ln_w_dtype);
            if (ln_b) y += (double)load1(ln_b, c + e, ln_b_dtype);
            dst[e] = y;
        } else {
            float y = (up<DT>(u.e[e]) - (float)mean) * (float)rstd;
            if (ln_w) y *= load1(ln_w, c + e, ln_w_dtype);
            if (ln_b) y += load1(ln_b, c + e, ln_b_dtype);
            dst[e] = down<DT>(y);
        }
    }
}

// ---- pack: packed of the compute dtype from weight (Cin, Cout, 8) -----------------------------------------------------------------
// forward: packed[t][co][ci].  transposed: packed[t][ci][co].
template <int DT>
__global__ __launch_bounds__(DC_BLOCK) void deconv3d_pack_kernel(const void* w, int w_dtype, void* packed_, int Cin, int Cout, int transposed,
                                                                 int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int CA = transposed ? Cout : Cin, CB = transposed ? Cin : Cout;
    const int ca = (int)(i % CA), cb = (int)((i / CA) % CB), t = (int)(i / ((int64_t)CA * CB));
    const int ci = transposed ? cb : ca, co = transposed ? ca : cb;
    ((typename El<DT>::type*)packed_)[i] = down<DT>(load1(w, ((int64_t)ci * Cout + co) * DC_TAPS + t, w_dtype));
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
struct FwdP {
    const void* x;           // (B, D, H, W, CI) dense rows
    const void* w;           // packed (8, CO, CI)
    const void* bias;        // CO values of bias_dtype, or NULL
    const void* ln_w;        // CI values, or NULL
    const void* ln_b;
    void* out;               // (B, 2D, 2H, 2W, CO) dense rows
    double* stats;           // (rows, 2): mean and rstd of every parent row, or NULL
    int64_t n;               // parent rows
    double eps;
    int32_t bias_dtype, ln_w_dtype, ln_b_dtype, has_norm, D, H, W, CI, CO;
};

template <int DT>
__global__ __launch_bounds__(DC_BLOCK, 2) void deconv3d_forward_kernel(const FwdP p) {
    using E = typename El<DT>::type;
    using O = typename Op<DT>::type;
    constexpr int VE = El<DT>::VE, KC = El<DT>::KC, CT = Op<DT>::CT, NJ = CT / 16, AV = Op<DT>::V, AROWV = AV + 1;
    __shared__ uint4 sA[DC_ROWS * AROWV];                      // the normalised chunk of the 64 rows
    __shared__ uint4 sW[DC_TAPS * CT * DC_ROWV];               // [tap][output channel], KC per row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * DC_ROWS;
    const int col0 = blockIdx.y * CT;
    const E* X = (const E*)p.x;
    const E* Wp = (const E*)p.w;

    // this thread's staging item: row sr, vector sq of the chunk; 4 threads share a row
    const int sr = tid >> 2, sq = tid & 3;
    const int64_t srow = row0 + sr;
    const bool svalid = srow < p.n;
    double mean = 0.0, rstd = 0.0;
    if (p.has_norm) {
        // one pass, both sums in f64: a value of 24 bits squares exactly, and the difference below loses 53 - 24 bits at most
        // before it would show in an f32 result
        const int nv = p.CI / VE;
        double s = 0.0, q = 0.0;
        if (svalid)
            for (int v = sq; v < nv; v += 4) {
                union { uint4 v; E e[VE]; } u;
                u.v = *reinterpret_cast<const uint4*>(X + srow * p.CI + v * VE);
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const double d = (double)up<DT>(u.e[e]);
                    s += d;
                    q += d * d;
                }
            }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        q += __shfl_xor(q, 1);
        q += __shfl_xor(q, 2);
        mean = s / p.CI;
        const double var = q / p.CI - mean * mean;
        rstd = svalid ? 1.0 / sqrt((var > 0.0 ? var : 0.0) + p.eps) : 0.0;
        if (sq == 0 && svalid && p.stats && blockIdx.y == 0) {
            p.stats[2 * srow] = mean;
            p.stats[2 * srow + 1] = rstd;
        }
    }

    typename El<DT>::acc acc[2][NJ][4];      // [k][channel tile][voxel tile]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][j][i] = typename El<DT>::acc{0, 0, 0, 0};

    for (int c0 = 0; c0 < p.CI; c0 += KC) {
        {
            const int c = c0 + sq * VE;
            union { uint4 v[AV / 4]; O e[VE]; } o;
#pragma unroll
            for (int k = 0; k < AV / 4; ++k) o.v[k] = make_uint4(0, 0, 0, 0);
            if (svalid && c < p.CI) {
                const uint4 raw = *reinterpret_cast<const uint4*>(X + srow * p.CI + c);
                if (p.has_norm) {
                    normalise<DT>(raw, c, mean, rstd, p.ln_w, p.ln_w_dtype, p.ln_b, p.ln_b_dtype, o.e);
                } else if constexpr (DT == GDR_NORM_F32) {
                    const f32x4 f = __builtin_bit_cast(f32x4, raw);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o.e[e] = (double)f[e];
                } else {
                    o.v[0] = raw;
                }
            }
#pragma unroll
            for (int k = 0; k < AV / 4; ++k) sA[sr * AROWV + sq * (AV / 4) + k] = o.v[k];
        }
        for (int v = tid; v < DC_TAPS * CT * 4; v += DC_BLOCK) {
            const int t = v / (CT * 4), r = (v >> 2) % CT, q = v & 3, co = col0 + r, c = c0 + q * VE;
            uint4 val = make_uint4(0, 0, 0, 0);
            if (co < p.CO && c < p.CI) val = *reinterpret_cast<const uint4*>(Wp + ((int64_t)t * p.CO + co) * p.CI + c);
            sW[(t * CT + r) * DC_ROWV + q] = val;
        }
        __syncthreads();
        Frag<DT> fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < AV / 4; ++k) fb[i].v[k] = sA[(16 * i + l16) * AROWV + quad * (AV / 4) + k];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (col0 + 16 * j >= p.CO) continue;      // (uniform over the workgroup)
                const uint4 fa = sW[((2 * wave + t) * CT + 16 * j + a_row<DT>(l16)) * DC_ROWV + quad];
#pragma unroll
                for (int i = 0; i < 4; ++i) mma_op<DT>(fa, fb[i], acc[t][j][i]);
            }
        __syncthreads();
    }

    // D: column = lane & 15 (parent row), rows 4 quad .. + 3 (output channels).  This wave's taps are (i, j) = (wave / 2, wave % 2)
    // with k = 0 and 1: the two child rows of a parent are adjacent, 2 CO elements
    E* out = (E*)p.out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + 16 * i + l16;
        if (row >= p.n) continue;
        const Vox vx = vox_of(row, p.D, p.H, p.W);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t child = child_of(vx, 2 * wave + t, p.D, p.H, p.W);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int co = col0 + 16 * j + 4 * quad;
                if (co >= p.CO) continue;       // CO is a multiple of 8: the 4 channels are in or out together
                typename El<DT>::acc sum = acc[t][j][i];
                if (p.bias) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[e] += up<DT>(down<DT>(load1(p.bias, co + e, p.bias_dtype)));
                }
                float r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = (float)sum[e];
                E* dst = out + child * p.CO + co;
                if constexpr (DT == GDR_NORM_F32) {
                    *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
                } else {
                    const uint32_t lo = (uint32_t)down<DT>(r[0]) | ((uint32_t)down<DT>(r[1]) << 16);
                    const uint32_t hi = (uint32_t)down<DT>(r[2]) | ((uint32_t)down<DT>(r[3]) << 16);
                    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
                }
            }
        }
    }
}

// ---- grad_input: g_n and the LayerNorm backward ---------------------------------------------------------------------------------
struct GinP {
    const void* g;           // (B, 2D, 2H, 2W, CO) dense rows
    const void* w;           // packed (8, CI, CO)
    const void* x;           // (B, D, H, W, CI) dense rows (read with the norm only)
    const double* stats;     // (rows, 2), with the norm
    const void* ln_w;        // CI values, or NULL
    void* grad_x;            // (B, D, H, W, CI) dense rows, or NULL
    double* part;            // [block][2][CI]: this block's column sums of g_n xhat and of g_n, or NULL
    int64_t n;
    int32_t ln_w_dtype, has_norm, D, H, W, CI, CO;
};

template <int DT, int VT>
__global__ __launch_bounds__(DC_BLOCK) void deconv3d_grad_input_kernel(const GinP p) {
    using E = typename El<DT>::type;
    using T = typename Op<DT>::scalar;
    constexpr int VE = El<DT>::VE, KC = El<DT>::KC, R = 16 * VT, NG = 4 / VT;
    __shared__ uint4 sG[R * DC_ROWV];                    // the gathered chunk of grad_out
    __shared__ uint4 sW[DC_GROUP * DC_ROWV];             // [input channel of the group], KC per row
    __shared__ T sRed[4 * R * 2];                        // [wave][row][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const E* G = (const E*)p.g;
    const E* Wp = (const E*)p.w;

    // this thread's staging item of the grad_out chunk (the first R 4 threads have one): the child row under tap 0
    const int sr = tid >> 2, sq = tid & 3;
    int64_t child0 = -1;
    if (tid < R * 4 && row0 + sr < p.n) child0 = child_of(vox_of(row0 + sr, p.D, p.H, p.W), 0, p.D, p.H, p.W);

    typename El<DT>::acc acc[NG][4][VT];      // [channel group][channel tile of this wave][voxel tile]
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < VT; ++i) acc[g][j][i] = typename El<DT>::acc{0, 0, 0, 0};

    for (int t = 0; t < DC_TAPS; ++t) {
        const int64_t toff = ((int64_t)(t >> 2) * (2 * p.H) + ((t >> 1) & 1)) * (2 * p.W) + (t & 1);      // child(p, t) - child(p, 0)
        for (int c0 = 0; c0 < p.CO; c0 += KC) {
            if (tid < R * 4) {
                const int co = c0 + sq * VE;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (child0 >= 0 && co < p.CO) val = *reinterpret_cast<const uint4*>(G + (child0 + toff) * p.CO + co);
                sG[sr * DC_ROWV + sq] = val;
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g * DC_GROUP >= p.CI) continue;       // (uniform over the workgroup)
                for (int v = tid; v < DC_GROUP * 4; v += DC_BLOCK) {
                    const int r = v >> 2, q = v & 3, c = g * DC_GROUP + r, co = c0 + q * VE;
                    uint4 val = make_uint4(0, 0, 0, 0);
                    if (c < p.CI && co < p.CO) val = *reinterpret_cast<const uint4*>(Wp + ((int64_t)t * p.CI + c) * p.CO + co);
                    sW[r * DC_ROWV + q] = val;
                }
                __syncthreads();
                uint4 fb[VT];
#pragma unroll
                for (int i = 0; i < VT; ++i) fb[i] = sG[(16 * i + l16) * DC_ROWV + quad];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (g * DC_GROUP + wave * 64 + 16 * j >= p.CI) continue;      // (uniform over the wave)
                    const uint4 fa = sW[(wave * 64 + 16 * j + a_row<DT>(l16)) * DC_ROWV + quad];
#pragma unroll
                    for (int i = 0; i < VT; ++i) mma_row<DT>(fa, fb[i], acc[g][j][i]);
                }
                __syncthreads();
            }
        }
    }

    // D: column = lane & 15 (parent row), rows 4 quad .. + 3 (input channels c = 256 g + 64 wave + 16 j + 4 quad + e)
    E* gx = (E*)p.grad_x;
    const E* X = (const E*)p.x;
    if (!p.has_norm) {
        if (!gx) return;
#pragma unroll
        for (int i = 0; i < VT; ++i) {
            const int64_t row = row0 + 16 * i + l16;
            if (row >= p.n) continue;
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = g * DC_GROUP + wave * 64 + 16 * j + 4 * quad;
                    if (c >= p.CI) continue;
                    E* dst = gx + row * p.CI + c;
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[e] = down<DT>((float)acc[g][j][i][e]);
                }
        }
        return;
    }

    // with the norm: s1 = sum_c gamma g_n, s2 = sum_c gamma g_n xhat of every row, and this block's column sums
    T mean[VT], rstd[VT], s1[VT], s2[VT];
    bool valid[VT];
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int64_t row = row0 + 16 * i + l16;
        valid[i] = row < p.n;
        mean[i] = valid[i] ? (T)p.stats[2 * row] : (T)0;
        rstd[i] = valid[i] ? (T)p.stats[2 * row + 1] : (T)0;
        s1[i] = s2[i] = (T)0;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = g * DC_GROUP + wave * 64 + 16 * j + 4 * quad;
            if (g * DC_GROUP + wave * 64 + 16 * j >= p.CI) continue;      // (uniform over the wave: the shuffles below are whole)
            const bool in = c < p.CI;       // CI is a multiple of 8: the 4 channels are in or out together
            T pg[4] = {0, 0, 0, 0}, pb[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < VT; ++i) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!(in && valid[i])) continue;
                    const T xh = ((T)up<DT>(X[(row0 + 16 * i + l16) * p.CI + c + e]) - mean[i]) * rstd[i];
                    const T gn = (T)acc[g][j][i][e];
                    const T a = p.ln_w ? gn * (T)load1(p.ln_w, c + e, p.ln_w_dtype) : gn;
                    s1[i] += a;
                    s2[i] += a * xh;
                    pg[e] += gn * xh;
                    pb[e] += gn;
                }
            }
            if (p.part) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int m = 1; m < 16; m <<= 1) {
                        pg[e] += __shfl_xor(pg[e], m);
                        pb[e] += __shfl_xor(pb[e], m);
                    }
                    if (l16 == 0 && in) {
                        p.part[((int64_t)blockIdx.x * 2) * p.CI + c + e] = (double)pg[e];
                        p.part[((int64_t)blockIdx.x * 2 + 1) * p.CI + c + e] = (double)pb[e];
                    }
                }
            }
        }
    if (!gx) return;
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        s1[i] += __shfl_xor(s1[i], 16);
        s1[i] += __shfl_xor(s1[i], 32);
        s2[i] += __shfl_xor(s2[i], 16);
        s2[i] += __shfl_xor(s2[i], 32);
        if (quad == 0) {
            sRed[(wave * R + 16 * i + l16) * 2] = s1[i];
            sRed[(wave * R + 16 * i + l16) * 2 + 1] = s2[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        T a1 = 0, a2 = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            a1 += sRed[(w * R + 16 * i + l16) * 2];
            a2 += sRed[(w * R + 16 * i + l16) * 2 + 1];
        }
        s1[i] = a1 / (T)p.CI;
        s2[i] = a2 / (T)p.CI;
    }
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        if (!valid[i]) continue;
        const int64_t row = row0 + 16 * i + l16;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = g * DC_GROUP + wave * 64 + 16 * j + 4 * quad;
                if (c >= p.CI) continue;
                E* dst = gx + row * p.CI + c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const T xh = ((T)up<DT>(X[row * p.CI + c + e]) - mean[i]) * rstd[i];
                    const T gn = (T)acc[g][j][i][e];
                    const T a = p.ln_w ? gn * (T)load1(p.ln_w, c + e, p.ln_w_dtype) : gn;
                    dst[e] = down<DT>((float)(rstd[i] * (a - s1[i] - xh * s2[i])));
                }
            }
    }
}

// ---- grad_weight ------------------------------------------------------------------------------------------------------------------
// part[slab][t][ci][co] = sum over the slab's parent rows r of n[r][ci] g[child(r, t)][co]; blockIdx = (tap, ci tile + tiles co tile, slab)
struct GwP {
    const void* x; const void* g; void* part;      // partials: f32, f64 for f32 operands
    const double* stats; const void* ln_w; const void* ln_b;
    int64_t n, slab_rows;      // parent rows in all, per slab (a multiple of DC_GT)
    int32_t ln_w_dtype, ln_b_dtype, has_norm, D, H, W, CI, CO, ci_tiles;
};

template <int DT>
__global__ __launch_bounds__(DC_BLOCK) void deconv3d_gw_kernel(const GwP p) {
    using E = typename El<DT>::type;
    using O = typename Op<DT>::type;
    constexpr int VE = El<DT>::VE, KC = El<DT>::KC, LDW = DC_GT + VE, VPR = DC_GT / VE;
    __shared__ __attribute__((aligned(16))) O sX[DC_GT * LDW];     // [ci][row], normalised
    __shared__ __attribute__((aligned(16))) E sG[DC_GT * LDW];     // [co][row]
    __shared__ int64_t sChild[DC_GT];                              // the child row of each parent row of the step, or -1
    __shared__ double sStat[DC_GT * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, quad = lane >> 4;
    const int t = blockIdx.x, ci0 = (blockIdx.y % p.ci_tiles) * DC_GT, co0 = (blockIdx.y / p.ci_tiles) * DC_GT;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const E* X = (const E*)p.x;
    const E* G = (const E*)p.g;
    const int64_t r_begin = (int64_t)blockIdx.z * p.slab_rows;
    const int64_t r_end = r_begin + p.slab_rows < p.n ? r_begin + p.slab_rows : p.n;
    using Acc = typename El<DT>::acc;
    Acc acc[2][2];      // [ci tile][co tile]: D rows = output channels, D columns = input channels
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Acc{0, 0, 0, 0};
    for (int64_t r0 = r_begin; r0 < r_end; r0 += DC_GT) {
        if (tid < DC_GT) {
            const int64_t r = r0 + tid;
            int64_t child = -1;
            double mean = 0.0, rstd = 0.0;
            if (r < r_end) {
                child = child_of(vox_of(r, p.D, p.H, p.W), t, p.D, p.H, p.W);
                if (p.has_norm) {
                    mean = p.stats[2 * r];
                    rstd = p.stats[2 * r + 1];
                }
            }
            sChild[tid] = child;
            sStat[2 * tid] = mean;
            sStat[2 * tid + 1] = rstd;
        }
        __syncthreads();
        for (int v = tid; v < DC_GT * VPR; v += DC_BLOCK) {
            const int r = v / VPR, cl = (v % VPR) * VE;
            const int64_t child = sChild[r];
            union { uint4 v; E e[VE]; } ug;
            O xn[VE];
            ug.v = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < VE; ++e) xn[e] = 0;
            if (child >= 0) {
                if (ci0 + cl < p.CI) {
                    const uint4 raw = *reinterpret_cast<const uint4*>(X + (r0 + r) * p.CI + ci0 + cl);
                    if (p.has_norm) {
                        normalise<DT>(raw, ci0 + cl, sStat[2 * r], sStat[2 * r + 1], p.ln_w, p.ln_w_dtype, p.ln_b, p.ln_b_dtype, xn);
                    } else {
                        union { uint4 v; E e[VE]; } ux;
                        ux.v = raw;
#pragma unroll
                        for (int e = 0; e < VE; ++e) xn[e] = (O)ux.e[e];
                    }
                }
                if (co0 + cl < p.CO) ug.v = *reinterpret_cast<const uint4*>(G + child * p.CO + co0 + cl);
            }
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                sX[(cl + e) * LDW + r] = xn[e];
                sG[(cl + e) * LDW + r] = ug.e[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < DC_GT / KC; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    Frag<DT> xn;
                    const O* src = sX + (wm + 16 * i + l16) * LDW + s * KC + quad * VE;
#pragma unroll
                    for (int k = 0; k < Op<DT>::V / 4; ++k) xn.v[k] = reinterpret_cast<const uint4*>(src)[k];
                    const uint4 gg = *reinterpret_cast<const uint4*>(sG + (wn + 16 * j + a_row<DT>(l16)) * LDW + s * KC + quad * VE);
                    mma_op<DT>(gg, xn, acc[i][j]);
                }
        __syncthreads();
    }
    // D: column = lane & 15 (ci), rows 4 quad .. + 3 (co): one vector of 4 per tile
    using P = typename Op<DT>::scalar;
    P* out = (P*)p.part + (int64_t)blockIdx.z * DC_TAPS * p.CO * p.CI;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ci = ci0 + wm + 16 * i + l16;
        if (ci >= p.CI) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int co = co0 + wn + 16 * j + 4 * quad;
            if (co >= p.CO) continue;
            *reinterpret_cast<Acc*>(out + ((int64_t)t * p.CI + ci) * p.CO + co) = acc[i][j];
        }
    }
}

// gw (Cin, Cout, 8) of gw_dtype = the slabs' partials [t][ci][co] added in slab order, rounded once
template <typename P>
__global__ __launch_bounds__(DC_BLOCK) void deconv3d_gw_fold_kernel(const P* part, void* gw, int gw_dtype, int CI, int CO, int slabs,
                                                                    int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i % CO), ci = (int)((i / CO) % CI), t = (int)(i / ((int64_t)CI * CO));
    P s = 0;
    for (int b = 0; b < slabs; ++b) s += part[(int64_t)b * total + i];
    store1(gw, ((int64_t)ci * CO + co) * DC_TAPS + t, gw_dtype, (float)s);
}

// ---- column sums: per-block partials in f64, then one launch adds the partials in block order ------------------------------------
// part[block][c] = sum over the block's rows of a[row][c]; the block's threads are (row phase, 16-byte vector of the row)
template <int DT>
__global__ __launch_bounds__(DC_BLOCK) void deconv3d_colsum_kernel(const void* a_, double* part, int64_t n, int C) {
    using E = typename El<DT>::type;
    constexpr int VE = El<DT>::VE;
    __shared__ double sSum[DC_BLOCK * VE];      // [row phase][channel]; phases CVN <= C: at most 256 / CVN * C = 256 VE values
    const E* a = (const E*)a_;
    const int cvn = C / VE, phases = DC_BLOCK / cvn, cv = threadIdx.x % cvn, ph = threadIdx.x / cvn;
    const int64_t rows = (n + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * rows;
    const int64_t r1 = r0 + rows < n ? r0 + rows : n;
    if (ph < phases) {
        double s[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) s[e] = 0.0;
        for (int64_t r = r0 + ph; r < r1; r += phases) {
            union { uint4 v; E e[VE]; } u;
            u.v = *reinterpret_cast<const uint4*>(a + r * C + cv * VE);
#pragma unroll
            for (int e = 0; e < VE; ++e) s[e] += (double)up<DT>(u.e[e]);
        }
#pragma unroll
        for (int e = 0; e < VE; ++e) sSum[ph * C + cv * VE + e] = s[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += DC_BLOCK) {
        double s = 0.0;
        for (int k = 0; k < phases; ++k) s += sSum[k * C + c];
        part[(int64_t)blockIdx.x * C + c] = s;
    }
}

// out[y][c] = sum over blocks b of part[(b ny + y) C + c], in block order: 16 segments of the blocks per channel, then their sum
struct FoldP { const double* part; void* out[2]; int32_t out_dtype[2]; int32_t blocks, C; };

__global__ __launch_bounds__(DC_BLOCK) void deconv3d_colsum_fold_kernel(const FoldP p) {
    __shared__ double sSeg[DC_FOLD][DC_FOLD];
    const int ch = threadIdx.x % DC_FOLD, seg = threadIdx.x / DC_FOLD, c = blockIdx.x * DC_FOLD + ch, y = blockIdx.y, ny = gridDim.y;
    const int per = (p.blocks + DC_FOLD - 1) / DC_FOLD, b0 = seg * per, b1 = b0 + per < p.blocks ? b0 + per : p.blocks;
    double s = 0.0;
    if (c < p.C)
        for (int b = b0; b < b1; ++b) s += p.part[((int64_t)b * ny + y) * p.C + c];
    sSeg[seg][ch] = s;
    __syncthreads();
    if (seg == 0 && c < p.C && p.out[y]) {
        double total = 0.0;
        for (int k = 0; k < DC_FOLD; ++k) total += sSeg[k][ch];
        store1(p.out[y], c, p.out_dtype[y], (float)total);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
bool bad_cin(int32_t C) { return C < 8 || C > GDR_DECONV3D_MAX_CIN || C % 8; }
bool bad_cout(int32_t C) { return C < 8 || C > GDR_DECONV3D_MAX_COUT || C % 8; }

constexpr int64_t DC_MAX_PARENT_ROWS = ((INT64_C(1) << 31) - 1) / DC_TAPS;

// parent rows of a (B, D, H, W) volume, or -1 beyond the envelope (8 times as many child rows stay below 2^31)
int64_t rows_of(int64_t B, int32_t D, int32_t H, int32_t W) {
    int64_t n = B;
    for (int32_t s : {D, H, W}) {
        if (n > DC_MAX_PARENT_ROWS / s) return -1;
        n *= s;
    }
    return n;
}

int slabs_of(int64_t n) { return gdr::slabs_of(n, DC_SLAB_MIN, DC_MAX_SLABS); }

int sum_blocks_of(int64_t rows) {
    const int64_t b = (rows + 63) / 64;
    return b < 1 ? 1 : (b > DC_SUM_BLOCKS ? DC_SUM_BLOCKS : (int)b);
}

// parent rows per workgroup of grad_input
int gin_rows_of(int32_t Cin) { return Cin <= DC_GROUP ? 64 : (Cin <= 2 * DC_GROUP ? 32 : 16); }

#define GDR_DECONV3D_DT(KERNEL, ...)                                                                     \
    do {                                                                                                 \
        if (dtype == GDR_NORM_F16) hipLaunchKernelGGL(KERNEL<GDR_NORM_F16>, __VA_ARGS__);             \
        else if (dtype == GDR_NORM_BF16) hipLaunchKernelGGL(KERNEL<GDR_NORM_BF16>, __VA_ARGS__);      \
        else hipLaunchKernelGGL(KERNEL<GDR_NORM_F32>, __VA_ARGS__);                                      \
    } while (0)

template <int VT> void launch_grad_input(int dtype, dim3 grid, hipStream_t st, const GinP& p) {
    if (dtype == GDR_NORM_F16) hipLaunchKernelGGL((deconv3d_grad_input_kernel<GDR_NORM_F16, VT>), grid, dim3(DC_BLOCK), 0, st, p);
    else if (dtype == GDR_NORM_BF16) hipLaunchKernelGGL((deconv3d_grad_input_kernel<GDR_NORM_BF16, VT>), grid, dim3(DC_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((deconv3d_grad_input_kernel<GDR_NORM_F32, VT>), grid, dim3(DC_BLOCK), 0, st, p);
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

size_t gdr_deconv3d_workspace_bytes(int32_t what, int32_t dtype, int64_t rows, int32_t Cin, int32_t Cout) {
    if (bad_dtype(dtype)) { invalid_arg("deconv3d_workspace_bytes: unknown dtype"); return 0; }
    if (rows < 0) { invalid_arg("deconv3d_workspace_bytes: rows must be >= 0"); return 0; }
    if (bad_cin(Cin) || bad_cout(Cout) || rows > DC_MAX_PARENT_ROWS) {
        unsupported("deconv3d_workspace_bytes: Cin must be a multiple of 8 in 8..GDR_DECONV3D_MAX_CIN, Cout one in 8..GDR_DECONV3D_MAX_COUT "
                    "and 8 rows below 2^31");
        return 0;
    }
    const size_t w = (size_t)DC_TAPS * Cin * Cout;
    switch (what) {
        case GDR_DECONV3D_WS_PACKED: return align_up(w * esize(dtype));
        case GDR_DECONV3D_WS_GRAD_WEIGHT: return align_up((size_t)slabs_of(rows) * w * (dtype == GDR_NORM_F32 ? sizeof(double) : sizeof(float)));
        case GDR_DECONV3D_WS_GRAD_BIAS: return align_up((size_t)sum_blocks_of(rows * DC_TAPS) * Cout * sizeof(double));
        case GDR_DECONV3D_WS_GRAD_INPUT: {
            const size_t blocks = (size_t)((rows + gin_rows_of(Cin) - 1) / gin_rows_of(Cin));
            return align_up((blocks < 1 ? 1 : blocks) * 2 * Cin * sizeof(double));
        }
        case GDR_DECONV3D_WS_STATS: return align_up((size_t)(rows < 1 ? 1 : rows) * 2 * sizeof(double));
    }
    invalid_arg("deconv3d_workspace_bytes: unknown workspace kind");
    return 0;
}

int gdr_deconv3d_pack_weight(const void* weight, int32_t weight_dtype, int32_t Cin, int32_t Cout, int32_t transposed, void* packed,
                             int32_t dtype, void* stream) {
    if (bad_dtype(weight_dtype) || bad_dtype(dtype)) return invalid_arg("deconv3d_pack_weight: unknown dtype");
    if (bad_cin(Cin) || bad_cout(Cout))
        return unsupported("deconv3d_pack_weight: Cin must be a multiple of 8 in 8..GDR_DECONV3D_MAX_CIN, Cout one in 8..GDR_DECONV3D_MAX_COUT");
    if (!weight || !packed) return invalid_arg("deconv3d_pack_weight: NULL argument");
    if (misaligned(weight, esize(weight_dtype) - 1) || misaligned(packed, 15))
        return unsupported("deconv3d_pack_weight: the weight must be aligned to its element and the packed buffer to 16 bytes");
    const int64_t total = (int64_t)DC_TAPS * Cin * Cout;
    GDR_DECONV3D_DT(deconv3d_pack_kernel, dim3(div_up(total, DC_BLOCK)), dim3(DC_BLOCK), 0, (hipStream_t)stream, weight, weight_dtype, packed,
                    Cin, Cout, transposed ? 1 : 0, total);
    return launch_status("deconv3d_pack_kernel");
}

int gdr_deconv3d_forward(const void* x, int32_t dtype, const void* packed, const void* bias, int32_t bias_dtype, int32_t has_norm,
                         const void* ln_weight, int32_t ln_weight_dtype, const void* ln_bias, int32_t ln_bias_dtype, double eps, int64_t B,
                         int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stats, void* out, void* stream) {
    if (bad_dtype(dtype) || (bias && bad_dtype(bias_dtype)) || (ln_weight && bad_dtype(ln_weight_dtype)) ||
        (ln_bias && bad_dtype(ln_bias_dtype)))
        return invalid_arg("deconv3d_forward: unknown dtype");
    if (B < 0 || D < 1 || H < 1 || W < 1) return invalid_arg("deconv3d_forward: B must be >= 0 and D, H, W >= 1");
    if (!has_norm && (ln_weight || ln_bias)) return invalid_arg("deconv3d_forward: an affine parameter without the norm");
    if (has_norm && !(eps >= 0.0)) return invalid_arg("deconv3d_forward: eps must be >= 0");
    if (bad_cin(Cin) || bad_cout(Cout))
        return unsupported("deconv3d_forward: Cin must be a multiple of 8 in 8..GDR_DECONV3D_MAX_CIN, Cout one in 8..GDR_DECONV3D_MAX_COUT");
    const int64_t n = rows_of(B, D, H, W);
    if (n < 0) return unsupported("deconv3d_forward: 8 B D H W must be below 2^31");
    if (n == 0) return GDR_OK;
    if (!x || !packed || !out) return invalid_arg("deconv3d_forward: NULL argument");
    if (misaligned(x, 15) || misaligned(packed, 15) || misaligned(out, 15) || misaligned(stats, 15) ||
        misaligned(bias, esize(bias_dtype) - 1) || misaligned(ln_weight, esize(ln_weight_dtype) - 1) ||
        misaligned(ln_bias, esize(ln_bias_dtype) - 1))
        return unsupported("deconv3d_forward: every row buffer must start on 16 bytes and a parameter on its element");
    FwdP p = {};
    p.x = x; p.w = packed; p.bias = bias; p.ln_w = ln_weight; p.ln_b = ln_bias; p.out = out; p.stats = has_norm ? (double*)stats : nullptr;
    p.n = n; p.eps = eps; p.bias_dtype = bias_dtype; p.ln_w_dtype = ln_weight_dtype; p.ln_b_dtype = ln_bias_dtype;
    p.has_norm = has_norm ? 1 : 0; p.D = D; p.H = H; p.W = W; p.CI = Cin; p.CO = Cout;
    const int ct = dtype == GDR_NORM_F32 ? Op<GDR_NORM_F32>::CT : Op<GDR_NORM_BF16>::CT;
    GDR_DECONV3D_DT(deconv3d_forward_kernel, dim3((uint32_t)div_up(n, DC_ROWS), div_up(Cout, ct)), dim3(DC_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("deconv3d_forward_kernel");
}

int gdr_deconv3d_grad_input(const void* grad_out, int32_t dtype, const void* packed_t, const void* x, const void* stats, int32_t has_norm,
                            const void* ln_weight, int32_t ln_weight_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t Cin,
                            int32_t Cout, void* workspace, size_t workspace_bytes, void* grad_x, void* grad_ln_weight,
                            int32_t grad_ln_weight_dtype, void* grad_ln_bias, int32_t grad_ln_bias_dtype, void* stream) {
    if (bad_dtype(dtype) || (ln_weight && bad_dtype(ln_weight_dtype)) || (grad_ln_weight && bad_dtype(grad_ln_weight_dtype)) ||
        (grad_ln_bias && bad_dtype(grad_ln_bias_dtype)))
        return invalid_arg("deconv3d_grad_input: unknown dtype");
    if (B < 0 || D < 1 || H < 1 || W < 1) return invalid_arg("deconv3d_grad_input: B must be >= 0 and D, H, W >= 1");
    if (!has_norm && (ln_weight || grad_ln_weight || grad_ln_bias)) return invalid_arg("deconv3d_grad_input: an affine parameter without the norm");
    if (bad_cin(Cin) || bad_cout(Cout))
        return unsupported("deconv3d_grad_input: Cin must be a multiple of 8 in 8..GDR_DECONV3D_MAX_CIN, Cout one in 8..GDR_DECONV3D_MAX_COUT");
    const int64_t n = rows_of(B, D, H, W);
    if (n < 0) return unsupported("deconv3d_grad_input: 8 B D H W must be below 2^31");
    const bool sums = grad_ln_weight || grad_ln_bias;
    if (!grad_x && !sums) return invalid_arg("deconv3d_grad_input: no gradient asked for");
    if (n && (!grad_out || !packed_t || (has_norm && (!x || !stats)))) return invalid_arg("deconv3d_grad_input: NULL argument");
    if (sums && !workspace) return invalid_arg("deconv3d_grad_input: NULL workspace");
    if (misaligned(grad_out, 15) || misaligned(packed_t, 15) || misaligned(x, 15) || misaligned(stats, 15) || misaligned(grad_x, 15) ||
        misaligned(workspace, 255) || misaligned(ln_weight, esize(ln_weight_dtype) - 1) ||
        misaligned(grad_ln_weight, esize(grad_ln_weight_dtype) - 1) || misaligned(grad_ln_bias, esize(grad_ln_bias_dtype) - 1))
        return unsupported("deconv3d_grad_input: every row buffer must start on 16 bytes, the workspace on 256 and a parameter on its element");
    if (sums && workspace_bytes < gdr_deconv3d_workspace_bytes(GDR_DECONV3D_WS_GRAD_INPUT, dtype, n, Cin, Cout))
        return workspace_too_small("deconv3d_grad_input: workspace smaller than gdr_deconv3d_workspace_bytes");
    const hipStream_t st = (hipStream_t)stream;
    const int rows = gin_rows_of(Cin);
    const int64_t blocks = div_up(n, (int64_t)rows);
    if (n) {
        GinP p = {};
        p.g = grad_out; p.w = packed_t; p.x = x; p.stats = (const double*)stats; p.ln_w = ln_weight; p.grad_x = grad_x;
        p.part = sums ? (double*)workspace : nullptr; p.n = n; p.ln_w_dtype = ln_weight_dtype; p.has_norm = has_norm ? 1 : 0;
        p.D = D; p.H = H; p.W = W; p.CI = Cin; p.CO = Cout;
        const dim3 grid((uint32_t)blocks);
        if (rows == 64) launch_grad_input<4>(dtype, grid, st, p);
        else if (rows == 32) launch_grad_input<2>(dtype, grid, st, p);
        else launch_grad_input<1>(dtype, grid, st, p);
        if (const int rc = launch_status("deconv3d_grad_input_kernel")) return rc;
    }
    if (sums) {
        FoldP f = {};
        f.part = (const double*)workspace; f.out[0] = grad_ln_weight; f.out[1] = grad_ln_bias;
        f.out_dtype[0] = grad_ln_weight_dtype; f.out_dtype[1] = grad_ln_bias_dtype; f.blocks = (int32_t)blocks; f.C = Cin;
        hipLaunchKernelGGL(deconv3d_colsum_fold_kernel, dim3(div_up(Cin, DC_FOLD), 2), dim3(DC_BLOCK), 0, st, f);
        return launch_status("deconv3d_colsum_fold_kernel");
    }
    return GDR_OK;
}

int gdr_deconv3d_grad_weight(const void* x, const void* stats, int32_t has_norm, const void* ln_weight, int32_t ln_weight_dtype,
                             const void* ln_bias, int32_t ln_bias_dtype, const void* grad_out, int32_t dtype, int64_t B, int32_t D, int32_t H,
                             int32_t W, int32_t Cin, int32_t Cout, void* workspace, size_t workspace_bytes, void* grad_weight,
                             int32_t grad_weight_dtype, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(grad_weight_dtype) || (ln_weight && bad_dtype(ln_weight_dtype)) || (ln_bias && bad_dtype(ln_bias_dtype)))
        return invalid_arg("deconv3d_grad_weight: unknown dtype");
    if (B < 0 || D < 1 || H < 1 || W < 1) return invalid_arg("deconv3d_grad_weight: B must be >= 0 and D, H, W >= 1");
    if (!has_norm && (ln_weight || ln_bias)) return invalid_arg("deconv3d_grad_weight: an affine parameter without the norm");
    if (bad_cin(Cin) || bad_cout(Cout))
        return unsupported("deconv3d_grad_weight: Cin must be a multiple of 8 in 8..GDR_DECONV3D_MAX_CIN, Cout one in 8..GDR_DECONV3D_MAX_COUT");
    const int64_t n = rows_of(B, D, H, W);
    if (n < 0) return unsupported("deconv3d_grad_weight: 8 B D H W must be below 2^31");
    if (!workspace || !grad_weight || (n && (!x || !grad_out || (has_norm && !stats)))) return invalid_arg("deconv3d_grad_weight: NULL argument");
    if (misaligned(x, 15) || misaligned(grad_out, 15) || misaligned(stats, 15) || misaligned(workspace, 255) ||
        misaligned(grad_weight, esize(grad_weight_dtype) - 1) || misaligned(ln_weight, esize(ln_weight_dtype) - 1) ||
        misaligned(ln_bias, esize(ln_bias_dtype) - 1))
        return unsupported("deconv3d_grad_weight: every row buffer must start on 16 bytes, the workspace on 256 and a parameter on its element");
    if (workspace_bytes < gdr_deconv3d_workspace_bytes(GDR_DECONV3D_WS_GRAD_WEIGHT, dtype, n, Cin, Cout))
        return workspace_too_small("deconv3d_grad_weight: workspace smaller than gdr_deconv3d_workspace_bytes");
    const hipStream_t st = (hipStream_t)stream;
    const int slabs = slabs_of(n);
    GwP p = {};
    p.x = x; p.g = grad_out; p.part = workspace; p.stats = (const double*)stats; p.ln_w = ln_weight; p.ln_b = ln_bias; p.n = n;
    p.slab_rows = (int64_t)align_up((size_t)((n + slabs - 1) / slabs), DC_GT);
    p.ln_w_dtype = ln_weight_dtype; p.ln_b_dtype = ln_bias_dtype; p.has_norm = has_norm ? 1 : 0;
    p.D = D; p.H = H; p.W = W; p.CI = Cin; p.CO = Cout; p.ci_tiles = div_up(Cin, DC_GT);
    GDR_DECONV3D_DT(deconv3d_gw_kernel, dim3(DC_TAPS, p.ci_tiles * div_up(Cout, DC_GT), slabs), dim3(DC_BLOCK), 0, st, p);
    if (const int rc = launch_status("deconv3d_gw_kernel")) return rc;
    const int64_t total = (int64_t)DC_TAPS * Cin * Cout;
    if (dtype == GDR_NORM_F32)
        hipLaunchKernelGGL(deconv3d_gw_fold_kernel<double>, dim3(div_up(total, DC_BLOCK)), dim3(DC_BLOCK), 0, st, (const double*)workspace,
                           grad_weight, grad_weight_dtype, Cin, Cout, slabs, total);
    else
        hipLaunchKernelGGL(deconv3d_gw_fold_kernel<float>, dim3(div_up(total, DC_BLOCK)), dim3(DC_BLOCK), 0, st, (const float*)workspace,
                           grad_weight, grad_weight_dtype, Cin, Cout, slabs, total);
    return launch_status("deconv3d_gw_fold_kernel");
}

int gdr_deconv3d_grad_bias(const void* grad_out, int32_t dtype, int64_t child_rows, int32_t Cout, void* workspace, size_t workspace_bytes,
                           void* grad_bias, int32_t grad_bias_dtype, void* stream) {
    if (bad_dtype(dtype) || bad_dtype(grad_bias_dtype)) return invalid_arg("deconv3d_grad_bias: unknown dtype");
    if (child_rows < 0 || child_rows % DC_TAPS) return invalid_arg("deconv3d_grad_bias: child_rows must be 8 times the parent rows");
    if (bad_cout(Cout) || child_rows / DC_TAPS > DC_MAX_PARENT_ROWS)
        return unsupported("deconv3d_grad_bias: Cout must be a multiple of 8 in 8..GDR_DECONV3D_MAX_COUT and child_rows below 2^31");
    if (!workspace || !grad_bias || (child_rows && !grad_out)) return invalid_arg("deconv3d_grad_bias: NULL argument");
    if (misaligned(grad_out, 15) || misaligned(workspace, 255) || misaligned(grad_bias, esize(grad_bias_dtype) - 1))
        return unsupported("deconv3d_grad_bias: grad_out must start on 16 bytes and the workspace on 256");
    if (workspace_bytes < gdr_deconv3d_workspace_bytes(GDR_DECONV3D_WS_GRAD_BIAS, dtype, child_rows / DC_TAPS, 8, Cout))
        return workspace_too_small("deconv3d_grad_bias: workspace smaller than gdr_deconv3d_workspace_bytes");
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = sum_blocks_of(child_rows);
    GDR_DECONV3D_DT(deconv3d_colsum_kernel, dim3(blocks), dim3(DC_BLOCK), 0, st, grad_out, (double*)workspace, child_rows, Cout);
    if (const int rc = launch_status("deconv3d_colsum_kernel")) return rc;
    FoldP f = {};
    f.part = (const double*)workspace; f.out[0] = grad_bias; f.out_dtype[0] = grad_bias_dtype; f.blocks = blocks; f.C = Cout;
    hipLaunchKernelGGL(deconv3d_colsum_fold_kernel, dim3(div_up(Cout, DC_FOLD), 1), dim3(DC_BLOCK), 0, st, f);
    return launch_status("deconv3d_colsum_fold_kernel");
}

}  // extern "C"

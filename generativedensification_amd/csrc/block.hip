// block.hip — the residual junctions of the point decoder's Block, the row-wise glue between its conv, attention and MLP, as
// one launch each way (include/gdr.h gdr_block_*; reference lightning/point_decoder/autoencoder.py, Block.forward):
//
//   forward   per row r of (N, C):
//               b0 = pre(branch[r])                     rounded to pre_out_dtype (pre none: branch[r] itself)
//               b  = keep[r] * b0                       rounded to kept_dtype (without keep: b0)
//               y  = skip[r] + b                        rounded to y_dtype, stored
//               n  = post(y)                            stored when post is not none
//             a norm is none, LN (mean / biased variance over the C channels, rstd = 1 / sqrt(var + eps), xh = (x - mean) * rstd),
//             LN with weight / bias (w * xh + bias, either may be absent) or ada (scale[seg(r)] * xh by norm.hip's ada rules:
//             rows at or behind offset[B - 1] give zeros, an empty segment is legal).  y is defined for every row.
//   backward  from grad_y and grad_n (either may be absent: zeros), recomputing b0, y and both sets of statistics:
//               dy = grad_y + post'(grad_n at y);  grad_skip = dy;  db = keep * dy;  grad_branch = pre'(db at branch)
//             with, for a norm with multiplier s (1, w or scale[b]) and incoming g:  dxh = g * s,
//               dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh));  ds = sum_rows g * xh;  dbias = sum_rows g.
//
// The statistics, the lane mapping, the backward's tail and the LDS sum of the groups are row_io.h's and ln_rows.h's; the
// segment search, ada's partial layout and its fold are norm_rows.h's, so an ada `post` fed the same y gives norm.hip's bits
// and a plain LN gives the bits of ada with a scale of ones.  norm_rows.h's ada kernels are templates over where ONE row comes
// from and where ONE gradient goes, with one statistics pass and one parameter sum per row; a junction has two statistics
// passes, two outputs and up to four parameter sums per row, which no policy of those templates can state, so its two kernels
// stand here, written in the same style over the same pieces.
//
// Mapping: as norm.hip — a row is held by a group of LC lanes, 8 channels per piece, one or two pieces per lane; the forward
// takes one row per group; the backward takes GDR_NORM_ROWS consecutive rows per workgroup and walks them by pieces that lie in
// one segment (one piece when no norm is ada), the groups take the rows of a piece in turn and keep the parameter sums of their
// rows in registers.  Behind a piece ada's sums go through LDS in group order into the segment's finished sum or its head / tail
// partial; behind the workgroup's rows the weight / bias sums go into the workgroup's partial pair.  The folds (ada's, and
// ln_rows.h's chain fold) add the partials in ascending order.  No atomics, every element has one writer: two runs are bitwise
// equal.  No entry point allocates or synchronises.
//
// Bounds: every row index is checked against N; offset values are clamped to [0, N] where they are read, the search stops after
// 16 steps and a piece consumes at least one row; keep is indexed by the row; parameter rows by a segment below B.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "ln_rows.h"
#include "norm_rows.h"

namespace gdr {
namespace {

struct JNorm {
    const void* w; const void* b; void* dw; void* db;
    float* ws_seg; float* ws_part;
    int64_t w_stride;
    int32_t kind, w_dt, b_dt;
    float eps;
};

struct JuncP {
    const void* skip; const void* branch; const void* keep; const int64_t* offset; const void* gy; const void* gn;
    void* y; void* n; void* dskip; void* dbranch;
    JNorm pre, post;
    int64_t N, skip_stride, branch_stride, gy_stride, gn_stride;
    int32_t B, C, lc_shift, skip_dt, branch_dt, keep_dt, b0_dt, kb_dt, y_dt, n_dt, gy_dt, gn_dt;
};

constexpr int JN_NONE = GDR_BLOCK_NORM_NONE, JN_LN = GDR_BLOCK_NORM_LN, JN_AFFINE = GDR_BLOCK_NORM_LN_AFFINE, JN_ADA = GDR_BLOCK_NORM_ADA;

// the multiplier row of a norm for segment b: ones (LN), the weight or ones (affine), scale[b] (ada)
template <int K>
__device__ __forceinline__ void norm_mult(const JNorm& m, int b, const bool (&on)[K], int l, int lc, float (&s)[K][8]) {
    if (m.kind == JN_ADA) load_row<K>(m.w, (int64_t)b * m.w_stride, m.w_dt, on, l, lc, s);
    else if (m.kind == JN_AFFINE && m.w) load_row<K>(m.w, 0, m.w_dt, on, l, lc, s);
    else fill_row<K>(s, 1.f);
}

// x -> the norm's result in place; xh (the normalised row) is left in `xh` when the norm is not none.  `behind`: the row lies
// at or behind the last segment end (ada: zeros).  The element expression of ada and plain LN is norm_rows.h ada_fwd_kernel's.
template <int K>
__device__ __forceinline__ void norm_apply(const JNorm& m, const float (&s)[K][8], bool behind, const bool (&on)[K], int l, int lc,
                                           float inv_c, float (&x)[K][8], float (&xh)[K][8], float& rstd) {
    if (m.kind == JN_NONE) return;
    float mean;
    row_stats<K>(x, on, lc, inv_c, m.eps, mean, rstd);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!on[k]) continue;
        float bias[8];
        if (m.kind == JN_AFFINE && m.b) load8(m.b, piece_c0(l, lc, k), m.b_dt, bias);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            xh[k][v] = (x[k][v] - mean) * rstd;
            float r = s[k][v] * xh[k][v];
            if (m.kind == JN_AFFINE && m.b) r += bias[v];
            x[k][v] = (m.kind == JN_ADA && behind) ? 0.f : r;
        }
    }
}

// the rows of the junction up to y: x holds branch[r] on entry and y on return, xh0 / rstd0 the normalised branch row and its
// rstd (pre not none).
// Rounded where torch rounds and kept from contracting: the forward and the backward's recomputation give the same y.
template <int K>
__device__ __forceinline__ void form_y(const JuncP& p, int64_t r, const float (&s0)[K][8], bool behind, const bool (&on)[K], int l,
                                       int lc, float inv_c, float kv, float (&x)[K][8], float (&xh0)[K][8], float& rstd0) {
    norm_apply<K>(p.pre, s0, behind, on, l, lc, inv_c, x, xh0, rstd0);
    float sk[K][8];
    load_row<K>(p.skip, r * p.skip_stride, p.skip_dt, on, l, lc, sk);
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    float b = p.pre.kind != JN_NONE ? round_any(x[k][v], p.b0_dt) : x[k][v];
                    if (p.keep) b = round_any(kv * b, p.kb_dt);
                    x[k][v] = round_any(sk[k][v] + b, p.y_dt);
                }
            }
    }
}

template <int K>
__global__ __launch_bounds__(NM_BLOCK) void junction_fwd_kernel(const JuncP p) {
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1);
    const int64_t row = (int64_t)blockIdx.x * (NM_BLOCK >> p.lc_shift) + (tid >> p.lc_shift);
    if (row >= p.N) return;                        // (whole groups leave: the butterflies stay inside a group)
    const float inv_c = 1.0f / (float)p.C;
    bool on[K];
    pieces_on<K>(l, lc, p.C, on);
    int b = 0;
    bool behind = false;
    if (p.offset) {
        b = seg_of_row(p.offset, p.B, p.N, row);
        behind = b >= p.B;
        if (behind) b = 0;                         // (a row that exists; its values are not used)
    }
    float x[K][8], xh[K][8], s[K][8];
    load_row<K>(p.branch, row * p.branch_stride, p.branch_dt, on, l, lc, x);
    norm_mult<K>(p.pre, b, on, l, lc, s);
    const float kv = p.keep ? load1(p.keep, row, p.keep_dt) : 1.f;
    float rstd;
    form_y<K>(p, row, s, behind, on, l, lc, inv_c, kv, x, xh, rstd);
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) store8(p.y, row * p.C + piece_c0(l, lc, k), p.y_dt, x[k]);
    if (p.post.kind == JN_NONE) return;
    norm_mult<K>(p.post, b, on, l, lc, s);
    norm_apply<K>(p.post, s, behind, on, l, lc, inv_c, x, xh, rstd);
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) store8(p.n, row * p.C + piece_c0(l, lc, k), p.n_dt, x[k]);
}

// g -> the gradient at the norm's input in place, xh the normalised input; as / ab take the row's shares of the multiplier
// and bias sums (ACC).  The element loop is norm_rows.h ada_bwd_kernel's: m2 is (g * xh) * s.
template <int K, bool ACC>
__device__ __forceinline__ void norm_back(const float (&s)[K][8], const float (&xh)[K][8], const bool (&on)[K], int lc, float inv_c,
                                          float rstd, float (&g)[K][8], float (&as)[K][8], float (&ab)[K][8]) {
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (on[k]) {
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const float gx = g[k][v] * xh[k][v];
                if constexpr (ACC) { as[k][v] += gx; ab[k][v] += g[k][v]; }
                g[k][v] *= s[k][v];
                m1 += g[k][v];
                m2 += gx * s[k][v];
            }
        }
    ln_dx<K>(g, xh, on, m1, m2, lc, inv_c, rstd);
}

// the groups' sums of one vector -> dst through LDS, in group order; the LDS is free again on return
template <int K>
__device__ __forceinline__ void groups_to(float* sh, int grp, int C, int G, const float (&acc)[K][8], const bool (&on)[K], int l, int lc,
                                          float* dst) {
    put_sums<K>(sh + grp * C, acc, on, l, lc);
    sum_groups<false>(sh, C, G, dst);
    __syncthreads();
}

// ACC: some parameter gradient is wanted
template <int K, bool ACC>
__global__ __launch_bounds__(NM_BLOCK) void junction_bwd_kernel(const JuncP p) {
    __shared__ float sh[ACC ? 2048 * K : 1];       // (256 / LC) groups x C channels: C <= 8 LC K
    const int tid = threadIdx.x, lc = 1 << p.lc_shift, l = tid & (lc - 1), grp = tid >> p.lc_shift, G = NM_BLOCK >> p.lc_shift;
    const int64_t N = p.N, j = blockIdx.x, a = j * NM_ROWS, e = a + NM_ROWS < N ? a + NM_ROWS : N;
    const int C = p.C;
    const float inv_c = 1.0f / (float)C;
    const bool pre_sums = ACC && (p.pre.dw || p.pre.db), post_sums = ACC && (p.post.dw || p.post.db);
    bool on[K];
    pieces_on<K>(l, lc, C, on);
    float as0[K][8], ab0[K][8], as1[K][8], ab1[K][8];
    fill_row<K>(as0, 0.f); fill_row<K>(ab0, 0.f); fill_row<K>(as1, 0.f); fill_row<K>(ab1, 0.f);
    int64_t row = a;
    // (everything that steers the loop is the same in all threads of the workgroup)
    for (int it = 0; it < NM_ROWS && row < e; ++it) {
        int b = 0;
        bool behind = false;
        int64_t r1 = e, st = 0, en = N;
        if (p.offset) {
            b = seg_of_row(p.offset, p.B, N, row);
            behind = b >= p.B;
            if (behind) b = 0;
            else {
                st = b ? clamp_end(p.offset, b - 1, N) : 0;
                en = clamp_end(p.offset, b, N);
                r1 = en < e ? en : e;
                if (r1 <= row) r1 = row + 1;       // (ends that are not monotone: one row on)
            }
        }
        float s0[K][8], s1[K][8];
        norm_mult<K>(p.pre, b, on, l, lc, s0);
        norm_mult<K>(p.post, b, on, l, lc, s1);
        for (int64_t r = row + grp; r < r1; r += G) {          // at most GDR_NORM_ROWS / G rows
            float x[K][8], xh0[K][8], g[K][8];
            load_row<K>(p.branch, r * p.branch_stride, p.branch_dt, on, l, lc, x);
            float rstd0 = 0.f;
            const float kv = p.keep ? load1(p.keep, r, p.keep_dt) : 1.f;
            form_y<K>(p, r, s0, behind, on, l, lc, inv_c, kv, x, xh0, rstd0);  // x = y
            // dy: grad_y and what comes back through post
            if (p.gy) load_row<K>(p.gy, r * p.gy_stride, p.gy_dt, on, l, lc, g);
            else fill_row<K>(g, 0.f);
            if (p.post.kind != JN_NONE && p.gn && !(p.post.kind == JN_ADA && behind)) {
                float gn[K][8], mean1, rstd1;
                load_row<K>(p.gn, r * p.gn_stride, p.gn_dt, on, l, lc, gn);
                row_stats<K>(x, on, lc, inv_c, p.post.eps, mean1, rstd1);
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (on[k]) {
#pragma unroll
                        for (int v = 0; v < 8; ++v) x[k][v] = (x[k][v] - mean1) * rstd1;      // xh1
                    }
                norm_back<K, ACC>(s1, x, on, lc, inv_c, rstd1, gn, as1, ab1);
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (on[k]) {
#pragma unroll
                        for (int v = 0; v < 8; ++v) g[k][v] += gn[k][v];
                    }
            }
            if (p.dskip) {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (on[k]) store8(p.dskip, r * C + piece_c0(l, lc, k), p.skip_dt, g[k]);
            }
            if (!p.dbranch && !pre_sums) continue;
            if (p.keep) {
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int v = 0; v < 8; ++v) g[k][v] *= kv;
            }
            if (p.pre.kind != JN_NONE) {
                if (p.pre.kind == JN_ADA && behind) fill_row<K>(g, 0.f);
                else norm_back<K, ACC>(s0, xh0, on, lc, inv_c, rstd0, g, as0, ab0);
            }
            if (p.dbranch) {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (on[k]) store8(p.dbranch, r * C + piece_c0(l, lc, k), p.branch_dt, g[k]);
            }
        }
        if constexpr (ACC) {
            if (p.offset && !behind) {             // ada's sums of this piece: finished, or the head / tail partial of its segment
                const int64_t slot = (st >= a && en <= e) ? -1 : (j * 2 + (st < a ? 0 : 1));
                if (p.pre.kind == JN_ADA && p.pre.dw) {
                    groups_to<K>(sh, grp, C, G, as0, on, l, lc, slot < 0 ? p.pre.ws_seg + (int64_t)b * C : p.pre.ws_part + slot * C);
                    fill_row<K>(as0, 0.f);
                }
                if (p.post.kind == JN_ADA && p.post.dw) {
                    groups_to<K>(sh, grp, C, G, as1, on, l, lc, slot < 0 ? p.post.ws_seg + (int64_t)b * C : p.post.ws_part + slot * C);
                    fill_row<K>(as1, 0.f);
                }
            }
        }
        row = r1;
    }
    if constexpr (ACC) {                           // the weight / bias sums of the workgroup's rows: its partial pair
        if (p.pre.kind == JN_AFFINE && pre_sums) {
            groups_to<K>(sh, grp, C, G, as0, on, l, lc, p.pre.ws_part + (j * 2 + 0) * C);
            groups_to<K>(sh, grp, C, G, ab0, on, l, lc, p.pre.ws_part + (j * 2 + 1) * C);
        }
        if (p.post.kind == JN_AFFINE && post_sums) {
            groups_to<K>(sh, grp, C, G, as1, on, l, lc, p.post.ws_part + (j * 2 + 0) * C);
            groups_to<K>(sh, grp, C, G, ab1, on, l, lc, p.post.ws_part + (j * 2 + 1) * C);
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
bool bad_vec(const void* ptr, int32_t dt) { return misaligned(ptr, esize(dt) - 1); }

int check_junction(int64_t N, int64_t B, int64_t C) {
    if (N < 0 || B < 1) return invalid_arg("block_junction: N must be >= 0 and B >= 1");
    if (N > NM_MAX_ROWS) return unsupported("block_junction: N must be below 2^31");
    if (B > GDR_NORM_MAX_SEGMENTS) return unsupported("block_junction: B must be at most GDR_NORM_MAX_SEGMENTS");
    if (C < 8 || C > GDR_NORM_MAX_CHANNELS || C % 8) return unsupported("block_junction: C must be a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS");
    return GDR_OK;
}

// 0, or the status with the message set; m filled from the caller's description (NULL: none)
int take_norm(const GdrBlockNorm* in, int64_t C, bool need_offset_ok, JNorm& m) {
    m = JNorm{};
    m.kind = JN_NONE;
    if (!in || in->kind == JN_NONE) return GDR_OK;
    if (in->kind < JN_NONE || in->kind > JN_ADA) return invalid_arg("block_junction: unknown norm kind");
    if (!(in->eps >= 0.f)) return invalid_arg("block_junction: eps must be >= 0");
    m.kind = in->kind; m.eps = in->eps;
    if (in->kind == JN_LN) return GDR_OK;
    if ((in->w || in->grad_w) && bad_dtype(in->w_dtype)) return invalid_arg("block_junction: unknown dtype of a norm's weight / scale");
    m.w = in->w; m.w_dt = in->w_dtype; m.dw = in->grad_w;
    if (in->kind == JN_ADA) {
        if (!need_offset_ok) return invalid_arg("block_junction: an ada norm needs offset");
        if (!in->w || bad_rows(in->w, in->w_stride, C) || misaligned(in->grad_w, 15))
            return invalid_arg("block_junction: scale rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
        m.w_stride = in->w_stride;
        return GDR_OK;
    }
    if ((in->b || in->grad_b) && bad_dtype(in->b_dtype)) return invalid_arg("block_junction: unknown dtype of a norm's bias");
    if (misaligned(in->w, 15) || misaligned(in->b, 15) || bad_vec(in->grad_w, in->w_dtype) || bad_vec(in->grad_b, in->b_dtype))
        return invalid_arg("block_junction: weight and bias must start on 16 bytes");
    m.b = in->b; m.b_dt = in->b_dtype; m.db = in->grad_b;
    return GDR_OK;
}

struct JuncWs { size_t seg[2], part[2], bytes; };

JuncWs junction_workspace(int64_t N, int64_t B, int64_t C) {
    JuncWs w;
    const size_t seg = align_up((size_t)B * (size_t)C * 4), part = align_up((size_t)((N + NM_ROWS - 1) / NM_ROWS) * 2 * (size_t)C * 4);
    w.seg[0] = 0; w.part[0] = seg; w.seg[1] = seg + part; w.part[1] = 2 * seg + part;
    w.bytes = 2 * (seg + part);
    return w;
}

// the parameter gradients of one norm from its partials
void fold_norm(const JuncP& p, const JNorm& m, hipStream_t st) {
    const int64_t chunks = (p.N + NM_ROWS - 1) / NM_ROWS;
    if (m.kind == JN_ADA && m.dw) {
        AdaP a = {};
        a.offset = p.offset; a.dscale = m.dw; a.ws_seg = m.ws_seg; a.ws_part = m.ws_part;
        a.N = p.N; a.B = p.B; a.C = p.C; a.scale_dt = m.w_dt;
        const uint32_t ctiles = (uint32_t)((p.C + LN_FOLD_CH - 1) / LN_FOLD_CH);
        hipLaunchKernelGGL(ada_fold_kernel, dim3((uint32_t)p.B * ctiles), dim3(NM_BLOCK), 0, st, a, ctiles);
    } else if (m.kind == JN_AFFINE && (m.dw || m.db)) {
        launch_ln_fold<false>(m.ws_part, chunks, p.C, m.dw, m.w_dt, m.db, m.b_dt, st);
    }
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_block_junction_forward(const void* skip, int64_t skip_stride, int32_t skip_dtype, const void* branch, int64_t branch_stride,
                               int32_t branch_dtype, const void* keep, int32_t keep_dtype, const GdrBlockNorm* pre,
                               const GdrBlockNorm* post, const int64_t* offset, int64_t N, int32_t B, int32_t C, int32_t pre_out_dtype,
                               int32_t kept_dtype, void* y, int32_t y_dtype, void* n, int32_t n_dtype, void* stream) {
    if (const int rc = check_junction(N, B, C)) return rc;
    if (bad_dtype(skip_dtype) || bad_dtype(branch_dtype) || bad_dtype(pre_out_dtype) || bad_dtype(kept_dtype) || bad_dtype(y_dtype) ||
        (keep && bad_dtype(keep_dtype)))
        return invalid_arg("block_junction_forward: unknown dtype");
    JuncP p = {};
    if (const int rc = take_norm(pre, C, offset != nullptr, p.pre)) return rc;
    if (const int rc = take_norm(post, C, offset != nullptr, p.post)) return rc;
    if (p.post.kind != JN_NONE && bad_dtype(n_dtype)) return invalid_arg("block_junction_forward: unknown dtype");
    if (N == 0) return GDR_OK;
    if (!skip || !branch || !y || (p.post.kind != JN_NONE && !n)) return invalid_arg("block_junction_forward: NULL argument");
    if (bad_rows(skip, skip_stride, C) || bad_rows(branch, branch_stride, C) || misaligned(y, 15) || misaligned(n, 15) ||
        misaligned(offset, 7) || (keep && bad_vec(keep, keep_dtype)))
        return invalid_arg("block_junction_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    const bool ada = p.pre.kind == JN_ADA || p.post.kind == JN_ADA;
    p.skip = skip; p.branch = branch; p.keep = keep; p.offset = ada ? offset : nullptr; p.y = y; p.n = n;
    p.N = N; p.skip_stride = skip_stride; p.branch_stride = branch_stride;
    p.B = B; p.C = C; p.skip_dt = skip_dtype; p.branch_dt = branch_dtype; p.keep_dt = keep ? keep_dtype : GDR_F32;
    p.b0_dt = pre_out_dtype; p.kb_dt = kept_dtype; p.y_dt = y_dtype; p.n_dt = n_dtype;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const int64_t groups = NM_BLOCK >> p.lc_shift;
    const dim3 grid((uint32_t)((N + groups - 1) / groups));
    LN_LAUNCH_K(junction_fwd_kernel, K, grid, (hipStream_t)stream, p);
    return launch_status("block junction_fwd_kernel");
}

size_t gdr_block_junction_backward_bytes(int64_t N, int32_t B, int32_t C) {
    if (check_junction(N, B, C)) return 0;
    return junction_workspace(N, B, C).bytes + 256;        // (never 0 for valid arguments)
}

int gdr_block_junction_backward(const void* grad_y, int64_t grad_y_stride, int32_t grad_y_dtype, const void* grad_n,
                                int64_t grad_n_stride, int32_t grad_n_dtype, const void* skip, int64_t skip_stride, int32_t skip_dtype,
                                const void* branch, int64_t branch_stride, int32_t branch_dtype, const void* keep, int32_t keep_dtype,
                                const GdrBlockNorm* pre, const GdrBlockNorm* post, const int64_t* offset, int64_t N, int32_t B, int32_t C,
                                int32_t pre_out_dtype, int32_t kept_dtype, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                                void* grad_skip, void* grad_branch, void* stream) {
    if (const int rc = check_junction(N, B, C)) return rc;
    if (bad_dtype(skip_dtype) || bad_dtype(branch_dtype) || bad_dtype(pre_out_dtype) || bad_dtype(kept_dtype) || bad_dtype(y_dtype) ||
        (keep && bad_dtype(keep_dtype)) || (grad_y && bad_dtype(grad_y_dtype)) || (grad_n && bad_dtype(grad_n_dtype)))
        return invalid_arg("block_junction_backward: unknown dtype");
    JuncP p = {};
    if (const int rc = take_norm(pre, C, offset != nullptr, p.pre)) return rc;
    if (const int rc = take_norm(post, C, offset != nullptr, p.post)) return rc;
    const bool sums = p.pre.dw || p.pre.db || p.post.dw || p.post.db;
    if (!grad_skip && !grad_branch && !sums) return GDR_OK;
    if (!workspace || (N && (!skip || !branch))) return invalid_arg("block_junction_backward: NULL argument");
    if ((N && (bad_rows(skip, skip_stride, C) || bad_rows(branch, branch_stride, C) || (grad_y && bad_rows(grad_y, grad_y_stride, C)) ||
               (grad_n && bad_rows(grad_n, grad_n_stride, C)))) ||
        misaligned(grad_skip, 15) || misaligned(grad_branch, 15) || misaligned(offset, 7) || misaligned(workspace, 255) ||
        (keep && bad_vec(keep, keep_dtype)))
        return invalid_arg("block_junction_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    const JuncWs ws = junction_workspace(N, B, C);
    if (workspace_bytes < ws.bytes) return workspace_too_small("block_junction_backward: workspace smaller than gdr_block_junction_backward_bytes");
    const bool ada = p.pre.kind == JN_ADA || p.post.kind == JN_ADA;
    p.skip = skip; p.branch = branch; p.keep = keep; p.offset = ada ? offset : nullptr; p.gy = grad_y;
    p.gn = p.post.kind != JN_NONE ? grad_n : nullptr;
    p.dskip = grad_skip; p.dbranch = grad_branch;
    p.pre.ws_seg = (float*)((char*)workspace + ws.seg[0]); p.pre.ws_part = (float*)((char*)workspace + ws.part[0]);
    p.post.ws_seg = (float*)((char*)workspace + ws.seg[1]); p.post.ws_part = (float*)((char*)workspace + ws.part[1]);
    p.N = N; p.skip_stride = skip_stride; p.branch_stride = branch_stride; p.gy_stride = grad_y_stride; p.gn_stride = grad_n_stride;
    p.B = B; p.C = C; p.skip_dt = skip_dtype; p.branch_dt = branch_dtype; p.keep_dt = keep ? keep_dtype : GDR_F32;
    p.b0_dt = pre_out_dtype; p.kb_dt = kept_dtype; p.y_dt = y_dtype; p.gy_dt = grad_y_dtype; p.gn_dt = grad_n_dtype;
    int K;
    row_shape(C, &p.lc_shift, &K);
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t chunks = (uint32_t)((N + NM_ROWS - 1) / NM_ROWS);
    if (chunks) {
        if (sums) {
            if (K == 1) hipLaunchKernelGGL((junction_bwd_kernel<1, true>), dim3(chunks), dim3(NM_BLOCK), 0, st, p);
            else hipLaunchKernelGGL((junction_bwd_kernel<2, true>), dim3(chunks), dim3(NM_BLOCK), 0, st, p);
        } else {
            if (K == 1) hipLaunchKernelGGL((junction_bwd_kernel<1, false>), dim3(chunks), dim3(NM_BLOCK), 0, st, p);
            else hipLaunchKernelGGL((junction_bwd_kernel<2, false>), dim3(chunks), dim3(NM_BLOCK), 0, st, p);
        }
    }
    fold_norm(p, p.pre, st);
    fold_norm(p, p.post, st);
    return launch_status("block junction_bwd kernels");
}

}  // extern "C"

// norm.hip — the two row normalisations of the point decoder that sit between its kernels (include/gdr.h gdr_norm_*):
//
//   ada    out[i] = scale[b] * (feat[i] - mean_i) * rstd_i for row i of segment b (offset[b - 1] <= i < offset[b], offset[-1] = 0),
//          mean / biased variance over the C channels, rstd = 1 / sqrt(var + eps); rows behind offset[B - 1] are zero.  The
//          reference's AdaLayerNorm: gather_csr(affine(global_feat), [0, offset]) * layer_norm(feat).
//          backward, xh the normalised row, g = grad_out, means over the C channels:
//            dxh = g * scale[b];  dfeat[i] = rstd_i * (dxh - mean(dxh) - xh * mean(dxh * xh));  dscale[b] = sum_i g[i] * xh[i]
//   pe     out[r] = layer_norm([sin(f_k x[r, j]) at 3k + j, cos(f_k x[r, j]) at 3F + 3k + j, feat[r / S]]), no affine, over the
//          W = 6F + C entries: UpscaleModule's gather_csr + positional_encoding + cat + LayerNorm.
//          backward, dz = rstd * (g - mean(g) - zh * mean(g * zh)):
//            dx[r, j] = sum_k f_k * (cos * dz_sin - sin * dz_cos);  dfeat[p] = sum over the S children of dz_feat
//
// Everything is computed in f32 whatever the storage types, and the statistics are recomputed in the backward (nothing is
// saved but the inputs).  No atomics: every output element has one writer and every sum a fixed order, so two runs are
// bitwise equal.  No entry point allocates or synchronises.
//
// Mapping: a row is held by a group of LC lanes, LC the power of two in 8..64 that covers C / 8; lane l holds the 8 channels
// behind 8 * l (and, at C > 512, the 8 behind 8 * (l + 64)): one 16-byte access per lane for 16-bit rows, two for f32 rows.  A
// workgroup of 256 threads holds 256 / LC groups.  Row sums are xor butterflies inside the group, which give every lane the
// same bits.  Mean first, then the squared deviations (two passes over registers).
//   ada forward   one row per group.
//   ada backward  a workgroup takes GDR_NORM_ROWS consecutive rows and walks them by pieces (the maximal ranges that lie in
//                 one segment, found by all threads alike); the groups take the rows of a piece in turn and keep the dscale sum
//                 of their rows in registers; behind a piece the sums of the groups are added through LDS in group order.  A
//                 segment that lies inside the workgroup's rows is finished there (f32, in the workspace), one that crosses
//                 the border leaves a head (slot 0) or a tail (slot 1) partial.  The fold launch adds the partials of every
//                 segment in ascending order (16 lane rows per channel, then those 16 in order) and writes dscale.
//   pe            one parent per group, its S children in turn: feat is read once, the trig values (lane l takes the
//                 (k, j) pairs l, l + LC, ...: one sincosf for two columns) and the normalised row go through an LDS row, so
//                 the result leaves in aligned 8-element pieces although the feat part starts at column 6F.  dfeat is summed
//                 over the children in registers; dx over k by lanes 0..2 from an LDS row, k ascending.
//
// The pieces of a lane, the zero-filled row load, the backward's tail behind the element loop and the LDS sum of the groups are
// ln_rows.h's, shared with groupattn.hip's and volcond.hip's norms.  The kernels themselves, ada's segmented fold and the
// launches are norm_rows.h's, templates over where a row comes from: this file instantiates them over rows and x in memory,
// upscale.hip over the rows UpscaleModule forms (merge, expand).
//
// Bounds: offset values are clamped to [0, N] where they are read; the searches stop after 16 steps; a piece consumes at
// least one row; every row index is checked against N or P.  A malformed offset gives unspecified values and never an access
// outside the buffers.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "ln_rows.h"
#include "norm_rows.h"

using namespace gdr;

extern "C" {

int gdr_norm_ada_forward(const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* scale, int64_t scale_stride,
                         int32_t scale_dtype, const int64_t* offset, int64_t N, int32_t B, int32_t C, float eps, void* out,
                         int32_t out_dtype, void* stream) {
    if (const int rc = check_ada(N, B, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(scale_dtype) || bad_dtype(out_dtype)) return invalid_arg("norm_ada_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_ada_forward: eps must be >= 0");
    if (N == 0) return GDR_OK;
    if (!feat || !scale || !offset || !out) return invalid_arg("norm_ada_forward: NULL argument");
    if (bad_rows(feat, feat_stride, C) || bad_rows(scale, scale_stride, C) || misaligned(out, 15) || misaligned(offset, 7))
        return invalid_arg("norm_ada_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    AdaP p = {};
    p.feat = feat; p.scale = scale; p.offset = offset; p.out = out;
    p.N = N; p.feat_stride = feat_stride; p.scale_stride = scale_stride;
    p.B = B; p.C = C; p.feat_dt = feat_dtype; p.scale_dt = scale_dtype; p.out_dt = out_dtype; p.eps = eps;
    p.S = 1;
    launch_ada_fwd<AdaPlain>(p, (hipStream_t)stream);
    return launch_status("norm ada_fwd_kernel");
}

size_t gdr_norm_ada_backward_bytes(int64_t N, int32_t B, int32_t C) {
    if (check_ada(N, B, C)) return 0;
    return ada_workspace(N, B, C).bytes + 256;     // (never 0 for valid arguments)
}

int gdr_norm_ada_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* feat, int64_t feat_stride,
                          int32_t feat_dtype, const void* scale, int64_t scale_stride, int32_t scale_dtype, const int64_t* offset,
                          int64_t N, int32_t B, int32_t C, float eps, void* workspace, size_t workspace_bytes, void* grad_feat,
                          void* grad_scale, void* stream) {
    if (const int rc = check_ada(N, B, C)) return rc;
    if (bad_dtype(feat_dtype) || bad_dtype(scale_dtype) || bad_dtype(grad_dtype)) return invalid_arg("norm_ada_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_ada_backward: eps must be >= 0");
    if (!offset || !workspace || !grad_scale || (N && (!grad_out || !feat || !scale || !grad_feat)))
        return invalid_arg("norm_ada_backward: NULL argument");
    if ((N && (bad_rows(feat, feat_stride, C) || bad_rows(scale, scale_stride, C) || bad_rows(grad_out, grad_stride, C))) ||
        misaligned(grad_feat, 15) || misaligned(grad_scale, 15) || misaligned(offset, 7) || misaligned(workspace, 255))
        return invalid_arg("norm_ada_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    const AdaWs ws = ada_workspace(N, B, C);
    if (workspace_bytes < ws.bytes) return workspace_too_small("norm_ada_backward: workspace smaller than gdr_norm_ada_backward_bytes");
    AdaP p = {};
    p.feat = feat; p.scale = scale; p.offset = offset; p.grad = grad_out; p.dfeat = grad_feat; p.dscale = grad_scale;
    p.ws_seg = (float*)((char*)workspace + ws.seg); p.ws_part = (float*)((char*)workspace + ws.part);
    p.N = N; p.feat_stride = feat_stride; p.scale_stride = scale_stride; p.grad_stride = grad_stride;
    p.B = B; p.C = C; p.feat_dt = feat_dtype; p.scale_dt = scale_dtype; p.out_dt = grad_dtype; p.eps = eps;
    p.S = 1;
    launch_ada_bwd<AdaPlain>(p, (hipStream_t)stream);
    return launch_status("norm ada_bwd kernels");
}

int gdr_norm_pe_forward(const void* x, int32_t x_dtype, const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq,
                        int32_t freq_dtype, int64_t P, int32_t S, int32_t C, int32_t F, float eps, void* out, int64_t out_stride,
                        int32_t out_dtype, void* stream) {
    if (const int rc = check_pe(P, S, C, F)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(feat_dtype) || bad_dtype(freq_dtype) || bad_dtype(out_dtype))
        return invalid_arg("norm_pe_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_pe_forward: eps must be >= 0");
    if (P == 0) return GDR_OK;
    if (!x || !feat || !freq || !out) return invalid_arg("norm_pe_forward: NULL argument");
    if (bad_rows(feat, feat_stride, C) || bad_rows(out, out_stride, 6 * F + C) || misaligned(x, esize(x_dtype) - 1) ||
        misaligned(freq, esize(freq_dtype) - 1))
        return invalid_arg("norm_pe_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    PeP p = {};
    p.x = x; p.feat = feat; p.freq = freq; p.out = out;
    p.P = P; p.feat_stride = feat_stride; p.out_stride = out_stride;
    p.S = S; p.C = C; p.F = F; p.x_dt = x_dtype; p.feat_dt = feat_dtype; p.freq_dt = freq_dtype; p.out_dt = out_dtype; p.eps = eps;
    launch_pe_fwd<PeGiven>(p, (hipStream_t)stream);
    return launch_status("norm pe_fwd_kernel");
}

int gdr_norm_pe_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* x, int32_t x_dtype,
                         const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype, int64_t P,
                         int32_t S, int32_t C, int32_t F, float eps, void* grad_x, void* grad_feat, void* stream) {
    if (const int rc = check_pe(P, S, C, F)) return rc;
    if (bad_dtype(x_dtype) || bad_dtype(feat_dtype) || bad_dtype(freq_dtype) || bad_dtype(grad_dtype))
        return invalid_arg("norm_pe_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("norm_pe_backward: eps must be >= 0");
    if (P == 0) return GDR_OK;
    if (!x || !feat || !freq || !grad_out) return invalid_arg("norm_pe_backward: NULL argument");
    const int W = 6 * F + C;
    const unsigned gmask = 2 * esize(grad_dtype) - 1;
    if (bad_rows(feat, feat_stride, C) || misaligned(grad_feat, 15) || misaligned(x, esize(x_dtype) - 1) ||
        misaligned(grad_x, esize(x_dtype) - 1) || misaligned(freq, esize(freq_dtype) - 1) || grad_stride < W ||
        grad_stride % 2 || misaligned(grad_out, gmask))
        return invalid_arg("norm_pe_backward: feat rows must start on 16 bytes with a stride that is a multiple of 8; grad_out "
                           "rows on two elements with an even stride that covers the row");
    PeP p = {};
    p.x = x; p.feat = feat; p.freq = freq; p.grad = grad_out; p.dx = grad_x; p.dfeat = grad_feat;
    p.P = P; p.feat_stride = feat_stride; p.grad_stride = grad_stride;
    p.S = S; p.C = C; p.F = F; p.x_dt = x_dtype; p.feat_dt = feat_dtype; p.freq_dt = freq_dtype; p.out_dt = grad_dtype; p.eps = eps;
    launch_pe_bwd<PeGiven>(p, grad_stride % 8 == 0 && !misaligned(grad_out, 15), (hipStream_t)stream);
    return launch_status("norm pe_bwd_kernel");
}

}  // extern "C"

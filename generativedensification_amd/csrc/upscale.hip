// upscale.hip — the torch glue of the point decoder's UpscaleModule on either side of its Linears, as one launch each
// (include/gdr.h gdr_upscale_*):
//
//   expand  from t = delta_x(in_f) (N, 3S), for parent p, child s, axis j, rd = the rounding to t's storage type:
//             u = rd(tanh(t[p, 3s + j]));  d = rd(half_grid * u);  out_x[pS + s, j] = coord[p, j] + d (rounded to out_x's type)
//             h[pS + s] = norm.hip's pe row of x = d (x = out_x as stored when absolute_pe) and feat[p]
//           backward, g = grad_out_x (or 0), dx the pe row's gradient at x (norm.hip), gd = g + dx:
//             grad_t[p, 3s + j] = gd * half_grid * (1 - u^2);  grad_coord[p, j] = sum_s (absolute_pe ? gd : g);  grad_feat: norm.hip's
//   merge   y[r] = rdy(skip[r / S] + rdb(keep[r] * branch[r])) (rdb to branch's type, rdy to the promotion of skip's and
//           branch's; without keep the product is branch[r]); out[r] = scale[b] * layer_norm(y[r]) by norm.hip's ada rules over
//           the parents' segment ends.
//           backward, dy the ada row's gradient at y: grad_branch[r] = keep[r] * dy[r];  grad_skip[p] = sum_s dy[pS + s] (child
//           order, in registers);  grad_scale through ada's partials and fold.
//
// Both are instantiations of norm_rows.h's kernels over a policy that forms the row: nothing of the statistics, the trig
// columns, the normalised row or the parameter-gradient sums is restated here, and a call that feeds ada / pe the same values
// returns the same bits.  The policies' own arithmetic is kept from contracting into FMAs: torch rounds each product.
//
// expand keeps the 3S PE arguments of a parent in LDS behind the group's row (lanes i, i + LC, ... of the group compute element
// i = 3s + j and store out_x), so the shared code reads x from memory in both instantiations.  u is recomputed in the backward.
//
// Bounds: a group touches global memory only when its parent is below N; element i is below 3S <= 48 = the LDS slots of a
// group; rows of merge are checked against N S, units against N; keep is indexed by the row, skip by the parent.
#include "gdr_common.h"
#include "host_util.h"
#include "row_io.h"
#include "ln_rows.h"
#include "norm_rows.h"

namespace gdr {
namespace {

// ---- expand ------------------------------------------------------------------------------------------------------------------
struct ExpandX {
    static constexpr int LDS = 3 * GDR_NORM_MAX_UPSCALE;
    struct State { float gc; };

    // element i = 3s + j of the parent: u, the offset d and the child coordinate as stored
    static __device__ __forceinline__ void child(const PeP& p, int64_t parent, int i, float& u, float& d, float& ox) {
#pragma clang fp contract(off)
        u = round_any(tanhf(load1(p.t, parent * (3 * p.S) + i, p.t_dt)), p.t_dt);
        d = round_any(p.half_grid * u, p.t_dt);
        ox = round_any(load1(p.coord, parent * 3 + i % 3, p.coord_dt) + d, p.ox_dt);
    }
    static __device__ __forceinline__ void prepare(const PeP& p, int64_t parent, bool active, int l, int lc, float* xs) {
        if (!active) return;
        for (int i = l; i < 3 * p.S; i += lc) {
            float u, d, ox;
            child(p, parent, i, u, d, ox);
            xs[i] = p.absolute ? ox : d;
            if (p.out_x) store1(p.out_x, parent * (3 * p.S) + i, p.ox_dt, ox);
        }
    }
    static __device__ __forceinline__ float x(const PeP&, const float* xs, int64_t, int s, int jj) { return xs[3 * s + jj]; }
    static __device__ __forceinline__ bool wants_dx(const PeP& p) { return p.dt != nullptr || p.dcoord != nullptr; }
    static __device__ __forceinline__ void put_dx(const PeP& p, const float*, State& st, int64_t r, int64_t parent, int s, int l, float dx) {
        float u, d, ox;
        child(p, parent, 3 * s + l, u, d, ox);
        const float g = p.grad_ox ? load1(p.grad_ox, r * 3 + l, p.ox_dt) : 0.f;
        const float gd = g + dx;
        st.gc += p.absolute ? gd : g;
        if (p.dt) store1(p.dt, r * 3 + l, p.t_dt, gd * p.half_grid * (1.f - u * u));
    }
    static __device__ __forceinline__ void finish(const PeP& p, const State& st, int64_t parent, int l) {
        if (p.dcoord) store1(p.dcoord, parent * 3 + l, p.coord_dt, st.gc);
    }
};

// ---- merge -------------------------------------------------------------------------------------------------------------------
struct MergeRows {
    template <int K> struct Unit { float sk[K][8], ds[K][8]; };
    static __device__ __forceinline__ int children(const AdaP& p) { return p.S; }
    static __device__ __forceinline__ int64_t unit_of(const AdaP& p, int64_t row) { return row / p.S; }

    // y[r] from the unit's skip row
    template <int K>
    static __device__ __forceinline__ void form(const AdaP& p, int64_t r, const float (&sk)[K][8], const bool (&on)[K], int l, int lc,
                                                float (&x)[K][8]) {
        load_row<K>(p.feat, r * p.feat_stride, p.feat_dt, on, l, lc, x);
        const float kv = p.keep ? load1(p.keep, r, p.keep_dt) : 1.f;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (on[k]) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        const float b = p.keep ? round_any(kv * x[k][v], p.feat_dt) : x[k][v];
                        x[k][v] = round_any(sk[k][v] + b, p.y_dt);
                    }
                }
        }
    }
    template <int K>
    static __device__ __forceinline__ void load_fwd(const AdaP& p, int64_t r, int64_t u, const bool (&on)[K], int l, int lc, float (&x)[K][8]) {
        float sk[K][8];
        load_row<K>(p.skip, u * p.skip_stride, p.skip_dt, on, l, lc, sk);
        form<K>(p, r, sk, on, l, lc, x);
    }
    template <int K>
    static __device__ __forceinline__ void begin(const AdaP& p, int64_t u, const bool (&on)[K], int l, int lc, Unit<K>& unit) {
        load_row<K>(p.skip, u * p.skip_stride, p.skip_dt, on, l, lc, unit.sk);
        fill_row<K>(unit.ds, 0.f);
    }
    template <int K>
    static __device__ __forceinline__ void load(const AdaP& p, int64_t r, const Unit<K>& unit, const bool (&on)[K], int l, int lc, float (&x)[K][8]) {
        form<K>(p, r, unit.sk, on, l, lc, x);
    }
    template <int K>
    static __device__ __forceinline__ void store(const AdaP& p, int64_t r, Unit<K>& unit, const bool (&on)[K], int l, int lc, const float (&dy)[K][8]) {
        const float kv = p.keep ? load1(p.keep, r, p.keep_dt) : 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
                float gb[8];
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    unit.ds[k][v] += dy[k][v];
                    gb[v] = p.keep ? kv * dy[k][v] : dy[k][v];
                }
                if (p.dfeat) store8(p.dfeat, r * p.C + piece_c0(l, lc, k), p.feat_dt, gb);
            }
    }
    template <int K>
    static __device__ __forceinline__ void end(const AdaP& p, int64_t u, const Unit<K>& unit, const bool (&on)[K], int l, int lc) {
        if (!p.dskip) return;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) store8(p.dskip, u * p.C + piece_c0(l, lc, k), p.skip_dt, unit.ds[k]);
    }
    template <int K>
    static __device__ __forceinline__ void zero(const AdaP& p, int64_t u, const bool (&on)[K], int l, int lc) {
        float z[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) z[v] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (on[k]) {
                const int c0 = piece_c0(l, lc, k);
                if (p.dskip) store8(p.dskip, u * p.C + c0, p.skip_dt, z);
                if (p.dfeat)
                    for (int s = 0; s < p.S; ++s) store8(p.dfeat, (u * p.S + s) * p.C + c0, p.feat_dt, z);
            }
    }
};

// ---- host --------------------------------------------------------------------------------------------------------------------
int check_merge(int64_t N, int64_t S, int64_t B, int64_t C) {
    if (S < 1 || S > GDR_NORM_MAX_UPSCALE) return unsupported("upscale_merge: S must be in 1..GDR_NORM_MAX_UPSCALE");
    if (const int rc = check_ada(N, B, C)) return rc;
    if (N > NM_MAX_ROWS / S) return unsupported("upscale_merge: N * S must be below 2^31");
    return GDR_OK;
}

int32_t promoted(int32_t a, int32_t b) { return a == b ? a : GDR_NORM_F32; }

bool bad_vec(const void* ptr, int32_t dt) { return misaligned(ptr, esize(dt) - 1); }

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_upscale_expand_forward(const void* t, int32_t t_dtype, const void* coord, int32_t coord_dtype, const void* feat,
                               int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype, int64_t N, int32_t S,
                               int32_t C, int32_t F, float half_grid, int32_t absolute_pe, float eps, void* out_x, int32_t out_x_dtype,
                               void* h, int64_t h_stride, int32_t h_dtype, void* stream) {
    if (const int rc = check_pe(N, S, C, F)) return rc;
    if (bad_dtype(t_dtype) || bad_dtype(coord_dtype) || bad_dtype(feat_dtype) || bad_dtype(freq_dtype) || bad_dtype(out_x_dtype) ||
        bad_dtype(h_dtype))
        return invalid_arg("upscale_expand_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("upscale_expand_forward: eps must be >= 0");
    if (N == 0) return GDR_OK;
    if (!t || !coord || !feat || !freq || !out_x || !h) return invalid_arg("upscale_expand_forward: NULL argument");
    if (bad_rows(feat, feat_stride, C) || bad_rows(h, h_stride, 6 * F + C) || bad_vec(t, t_dtype) || bad_vec(coord, coord_dtype) ||
        bad_vec(freq, freq_dtype) || bad_vec(out_x, out_x_dtype))
        return invalid_arg("upscale_expand_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and covers the row");
    PeP p = {};
    p.t = t; p.coord = coord; p.feat = feat; p.freq = freq; p.out_x = out_x; p.out = h;
    p.P = N; p.feat_stride = feat_stride; p.out_stride = h_stride;
    p.S = S; p.C = C; p.F = F; p.t_dt = t_dtype; p.coord_dt = coord_dtype; p.feat_dt = feat_dtype; p.freq_dt = freq_dtype;
    p.ox_dt = out_x_dtype; p.out_dt = h_dtype; p.absolute = absolute_pe != 0; p.eps = eps; p.half_grid = half_grid;
    launch_pe_fwd<ExpandX>(p, (hipStream_t)stream);
    return launch_status("upscale expand forward");
}

int gdr_upscale_expand_backward(const void* grad_h, int64_t grad_h_stride, int32_t grad_h_dtype, const void* grad_out_x,
                                int32_t out_x_dtype, const void* t, int32_t t_dtype, const void* coord, int32_t coord_dtype,
                                const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype,
                                int64_t N, int32_t S, int32_t C, int32_t F, float half_grid, int32_t absolute_pe, float eps,
                                void* grad_t, void* grad_coord, void* grad_feat, void* stream) {
    if (const int rc = check_pe(N, S, C, F)) return rc;
    if (bad_dtype(t_dtype) || bad_dtype(coord_dtype) || bad_dtype(feat_dtype) || bad_dtype(freq_dtype) || bad_dtype(out_x_dtype) ||
        bad_dtype(grad_h_dtype))
        return invalid_arg("upscale_expand_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("upscale_expand_backward: eps must be >= 0");
    if (N == 0 || (!grad_t && !grad_coord && !grad_feat)) return GDR_OK;
    if (!t || !coord || !feat || !freq) return invalid_arg("upscale_expand_backward: NULL argument");
    const int W = 6 * F + C;
    const unsigned gmask = 2 * esize(grad_h_dtype) - 1;
    if (bad_rows(feat, feat_stride, C) || misaligned(grad_feat, 15) || bad_vec(t, t_dtype) || bad_vec(grad_t, t_dtype) ||
        bad_vec(coord, coord_dtype) || bad_vec(grad_coord, coord_dtype) || bad_vec(freq, freq_dtype) ||
        bad_vec(grad_out_x, out_x_dtype) || (grad_h && (grad_h_stride < W || grad_h_stride % 2 || misaligned(grad_h, gmask))))
        return invalid_arg("upscale_expand_backward: feat rows must start on 16 bytes with a stride that is a multiple of 8; grad_h "
                           "rows on two elements with an even stride that covers the row");
    PeP p = {};
    p.t = t; p.coord = coord; p.feat = feat; p.freq = freq; p.grad = grad_h; p.grad_ox = grad_out_x;
    p.dt = grad_t; p.dcoord = grad_coord; p.dfeat = grad_feat;
    p.P = N; p.feat_stride = feat_stride; p.grad_stride = grad_h_stride;
    p.S = S; p.C = C; p.F = F; p.t_dt = t_dtype; p.coord_dt = coord_dtype; p.feat_dt = feat_dtype; p.freq_dt = freq_dtype;
    p.ox_dt = out_x_dtype; p.out_dt = grad_h_dtype; p.absolute = absolute_pe != 0; p.eps = eps; p.half_grid = half_grid;
    launch_pe_bwd<ExpandX>(p, !grad_h || (grad_h_stride % 8 == 0 && !misaligned(grad_h, 15)), (hipStream_t)stream);
    return launch_status("upscale expand backward");
}

int gdr_upscale_merge_forward(const void* skip, int64_t skip_stride, int32_t skip_dtype, const void* branch, int64_t branch_stride,
                              int32_t branch_dtype, const void* keep, int32_t keep_dtype, const void* scale, int64_t scale_stride,
                              int32_t scale_dtype, const int64_t* offset, int64_t N, int32_t S, int32_t B, int32_t C, float eps,
                              void* out, int32_t out_dtype, void* stream) {
    if (const int rc = check_merge(N, S, B, C)) return rc;
    if (bad_dtype(skip_dtype) || bad_dtype(branch_dtype) || bad_dtype(scale_dtype) || bad_dtype(out_dtype) || (keep && bad_dtype(keep_dtype)))
        return invalid_arg("upscale_merge_forward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("upscale_merge_forward: eps must be >= 0");
    if (N == 0) return GDR_OK;
    if (!skip || !branch || !scale || !offset || !out) return invalid_arg("upscale_merge_forward: NULL argument");
    if (bad_rows(skip, skip_stride, C) || bad_rows(branch, branch_stride, C) || bad_rows(scale, scale_stride, C) || misaligned(out, 15) ||
        misaligned(offset, 7) || (keep && bad_vec(keep, keep_dtype)))
        return invalid_arg("upscale_merge_forward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    AdaP p = {};
    p.feat = branch; p.skip = skip; p.keep = keep; p.scale = scale; p.offset = offset; p.out = out;
    p.N = N; p.S = S; p.feat_stride = branch_stride; p.skip_stride = skip_stride; p.scale_stride = scale_stride;
    p.B = B; p.C = C; p.feat_dt = branch_dtype; p.skip_dt = skip_dtype; p.keep_dt = keep ? keep_dtype : GDR_NORM_F32;
    p.y_dt = promoted(skip_dtype, branch_dtype); p.scale_dt = scale_dtype; p.out_dt = out_dtype; p.eps = eps;
    launch_ada_fwd<MergeRows>(p, (hipStream_t)stream);
    return launch_status("upscale merge forward");
}

size_t gdr_upscale_merge_backward_bytes(int64_t N, int32_t S, int32_t B, int32_t C) {
    if (check_merge(N, S, B, C)) return 0;
    return ada_workspace(N, B, C).bytes + 256;     // (never 0 for valid arguments)
}

int gdr_upscale_merge_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* skip, int64_t skip_stride,
                               int32_t skip_dtype, const void* branch, int64_t branch_stride, int32_t branch_dtype, const void* keep,
                               int32_t keep_dtype, const void* scale, int64_t scale_stride, int32_t scale_dtype, const int64_t* offset,
                               int64_t N, int32_t S, int32_t B, int32_t C, float eps, void* workspace, size_t workspace_bytes,
                               void* grad_skip, void* grad_branch, void* grad_scale, void* stream) {
    if (const int rc = check_merge(N, S, B, C)) return rc;
    if (bad_dtype(skip_dtype) || bad_dtype(branch_dtype) || bad_dtype(scale_dtype) || bad_dtype(grad_dtype) || (keep && bad_dtype(keep_dtype)))
        return invalid_arg("upscale_merge_backward: unknown dtype");
    if (!(eps >= 0.f)) return invalid_arg("upscale_merge_backward: eps must be >= 0");
    if (!grad_skip && !grad_branch && !grad_scale) return GDR_OK;
    if (!offset || !workspace || !scale || (N && (!grad_out || !skip || !branch)))
        return invalid_arg("upscale_merge_backward: NULL argument");
    if ((N && (bad_rows(skip, skip_stride, C) || bad_rows(branch, branch_stride, C) || bad_rows(grad_out, grad_stride, C))) ||
        bad_rows(scale, scale_stride, C) || misaligned(grad_skip, 15) || misaligned(grad_branch, 15) || misaligned(grad_scale, 15) ||
        misaligned(offset, 7) || misaligned(workspace, 255) || (keep && bad_vec(keep, keep_dtype)))
        return invalid_arg("upscale_merge_backward: rows must start on 16 bytes with a stride that is a multiple of 8 and at least C");
    const AdaWs ws = ada_workspace(N, B, C);
    if (workspace_bytes < ws.bytes) return workspace_too_small("upscale_merge_backward: workspace smaller than gdr_upscale_merge_backward_bytes");
    AdaP p = {};
    p.feat = branch; p.skip = skip; p.keep = keep; p.scale = scale; p.offset = offset; p.grad = grad_out;
    p.dfeat = grad_branch; p.dskip = grad_skip; p.dscale = grad_scale;
    p.ws_seg = (float*)((char*)workspace + ws.seg); p.ws_part = (float*)((char*)workspace + ws.part);
    p.N = N; p.S = S; p.feat_stride = branch_stride; p.skip_stride = skip_stride; p.scale_stride = scale_stride; p.grad_stride = grad_stride;
    p.B = B; p.C = C; p.feat_dt = branch_dtype; p.skip_dt = skip_dtype; p.keep_dt = keep ? keep_dtype : GDR_NORM_F32;
    p.y_dt = promoted(skip_dtype, branch_dtype); p.scale_dt = scale_dtype; p.out_dt = grad_dtype; p.eps = eps;
    launch_ada_bwd<MergeRows>(p, (hipStream_t)stream);
    return launch_status("upscale merge backward");
}

}  // extern "C"
